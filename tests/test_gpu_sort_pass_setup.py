"""The per-sort setup of the single-read radix passes (csrc/kernels_sort.hip launch_onesweep_passes, launch_radix_ghist_scan,
launch_sort_pack): the digit counts of all passes become bases in ONE launch (both words of a key beyond 64 bits), the look-back
words and tickets live in two regions that the passes use alternately -- one fill per sequence, every pass clears the region of the
next one -- and the pack kernel's grid follows the row count.  What can go wrong is state: a look-back word or a ticket left by an
earlier pass or an earlier run, a base taken from the wrong pass.  So every operator here runs twice at one size, then on fewer rows,
then on the larger input again, over composite keys of 1, 2, 4, 5, 8, 9 and 16 passes (widths chosen through the value ranges), with
heavy ties (stability), at row counts around the 6144- and 8192-record tiles; with the interpreter kernels and the generated ones.
Checker: Python's stable sort over tuples of Python integers.  The radix aggregate and the hash partition share the passes
(csrc/capi.cpp bucket_records) and are run at bucket / partition counts of one and two passes."""
import numpy as np
import pyarrow as pa
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit
from oracle import oracle_np as O
from test_gpu_operators import rand_table

pytestmark = pytest.mark.gpu

SIZES = [2049, 2 * 6144 + 1, 2 * 8192 + 1, 100_003]
N_MAX = max(SIZES)

# passes -> the value ranges (in bits) of the keys of the composite; a key of b bits takes values in [0, 2^b) shifted to be signed
WIDTHS = {1: [8], 2: [16], 4: [16, 16], 5: [17, 16], 8: [32, 32], 9: [33, 32], 16: [64, 64]}


@pytest.fixture(params=["off", "force"])
def jit_tc(tc, request):
    if request.param == "force" and not tc.ctx.jit_stats()["available"]:
        pytest.skip("no run-time compiler")
    tc.ctx.set_jit(request.param)
    yield tc
    tc.ctx.set_jit("auto")


def key_column(r, bits, n, pool):
    """n values out of `pool` distinct ones (ties), spanning exactly `bits` bits: rows 0 and 1 hold the extremes, so every prefix of at
    least two rows has the same key layout"""
    lo = -(1 << (bits - 1))
    vals = [lo + int(x) for x in r.integers(0, 1 << min(bits, 62), pool)]
    if bits > 62:
        vals = [v + (int(x) << 62) for v, x in zip(vals, r.integers(0, 1 << (bits - 62), pool))]
    out = [vals[i] for i in r.integers(0, pool, n)]
    out[0], out[1] = lo, lo + (1 << bits) - 1
    return out


def columns(passes):
    r = np.random.default_rng(passes)
    bits = WIDTHS[passes]
    # the first key repeats a lot (ties that only the later keys or the row order break), the last one less
    return [key_column(r, b, N_MAX, 37 if i + 1 < len(bits) else 5000) for i, b in enumerate(bits)]


_COLS = {}


def table_for(passes, n):
    if passes not in _COLS:
        _COLS[passes] = columns(passes)
    cols = {"rid": pa.array(np.arange(n, dtype=np.int64))}
    for i, c in enumerate(_COLS[passes]):
        cols["k%d" % i] = pa.array(c[:n], type=pa.int64())
    t = pa.table(cols)
    return t.cast(pa.schema([pa.field(f.name, f.type, nullable=False) for f in t.schema])), [c[:n] for c in _COLS[passes]]


def stable_order(keys, n):
    return np.array(sorted(range(n), key=lambda i: tuple(k[i] for k in keys)), dtype=np.int64)


def rids(p):
    return np.asarray(p.execute(0).to_arrow().column("rid"))


def smaller(n):
    return n * 2 // 3 if n * 2 // 3 > 2048 else 1500      # (1500: the one-block sort in between, then the passes again)


@pytest.mark.parametrize("passes", sorted(WIDTHS))
@pytest.mark.parametrize("n", SIZES)
def test_every_pass_count_twice_then_fewer_rows_then_more(jit_tc, n, passes):
    tc = jit_tc
    t, keys = table_for(passes, n)
    want = stable_order(keys, n)
    src = g.MemoryExec([t]); s = src.schema()
    p = g.NativePlan(g.SortExec([{"expr": col("k%d" % i, s), "asc": True, "nulls_first": False} for i in range(len(keys))], src), tc)
    assert np.array_equal(rids(p), want)
    assert np.array_equal(rids(p), want)                # (the second run is deferred: the layout of the first, checked row by row)
    m = smaller(n)
    tm, keys_m = table_for(passes, m)
    p.set_input(0, g.DeviceTable.from_arrow(tm, tc.device))
    assert np.array_equal(rids(p), stable_order(keys_m, m))
    p.set_input(0, g.DeviceTable.from_arrow(t, tc.device))
    assert np.array_equal(rids(p), want)


@pytest.mark.parametrize("n", SIZES)
def test_desc_and_nulls_first_with_ties(jit_tc, n):
    """(d DESC NULLS FIRST, a ASC): a null bit above the 12-bit field of d, 17 bits of a -- 30 bits, packed records"""
    tc = jit_tc
    r = np.random.default_rng(n)
    d = r.integers(-2000, 2000, n); d[0], d[1] = -2000, 1999
    mask = r.random(n) < 0.2; mask[:2] = False
    a = r.integers(0, 1 << 17, 50)[r.integers(0, 50, n)]; a[0], a[1] = 0, (1 << 17) - 1
    t = pa.table({"rid": pa.array(np.arange(n, dtype=np.int64)), "d": pa.array(d, type=pa.int64(), mask=mask), "a": pa.array(a, type=pa.int64())})
    dl, al, ml = d.tolist(), a.tolist(), mask.tolist()
    want = np.array(sorted(range(n), key=lambda i: (0, 0, al[i]) if ml[i] else (1, -dl[i], al[i])), dtype=np.int64)
    src = g.MemoryExec([t]); s = src.schema()
    p = g.NativePlan(g.SortExec([{"expr": col("d", s), "asc": False, "nulls_first": True}, {"expr": col("a", s), "asc": True, "nulls_first": False}], src), tc)
    for _ in range(3):
        assert np.array_equal(rids(p), want)


def test_deferred_sort_with_fewer_rows_than_the_bound(jit_tc):
    """SortExec above a filter: from the second execution on the row count is a device word below the bound the sort is launched
    with, and the positions up to the bound become padding records behind every real row (5 passes: key + id records)"""
    tc = jit_tc
    n = 2 * 6144 + 1
    t, keys = table_for(5, n)
    keep = np.arange(n) % 3 != 2
    t = t.append_column(pa.field("keep", pa.int32(), nullable=False), pa.array(keep.astype(np.int32)))
    sel = np.flatnonzero(keep).tolist()
    want = np.array(sorted(sel, key=lambda i: tuple(k[i] for k in keys)), dtype=np.int64)
    src = g.MemoryExec([t]); s = src.schema()
    f = g.FilterExec(binary(col("keep", s), Op.Eq, lit(1, "Int32")), src)
    fs = f.schema()
    p = g.NativePlan(g.SortExec([{"expr": col("k%d" % i, fs), "asc": True, "nulls_first": False} for i in range(len(keys))], f), tc)
    assert np.array_equal(rids(p), want) and not p.exec_stats()["deferred"]
    for _ in range(2):
        assert np.array_equal(rids(p), want)
        st = p.exec_stats()
        assert st["deferred"] and st["retries"] == 0, st


@pytest.mark.parametrize("n", [700, 300_000])
def test_radix_aggregate_buckets_of_one_and_two_passes(jit_tc, n):
    """strategy "radix": the rows are bucketed by key hash through the same passes -- a few buckets (one pass) at 700 rows, more than
    256 (two passes) at 300,000 distinct keys; twice on one operator"""
    tc = jit_tc
    r = np.random.default_rng(n)
    k = r.permutation(n).astype(np.int64) * 7 + 3
    v = r.integers(-10**9, 10**9, n)
    t = pa.table({"k": pa.array(k), "v": pa.array(v)})
    src = g.MemoryExec([t]); s = src.schema()
    plan = g.AggregateExec("Single", [(col("k", s), "k")], [{"fn": "SUM", "expr": col("v", s), "name": "sv"}, {"fn": "COUNT", "expr": lit(1), "name": "c"}], src,
                           strategy="radix", expected_groups=n)
    p = g.NativePlan(plan, tc)
    order = np.argsort(k)
    for _ in range(2):
        out = p.execute(0).to_arrow()
        got = np.argsort(np.asarray(out["k"]))
        assert out.num_rows == n
        assert np.array_equal(np.asarray(out["k"])[got], k[order]) and np.array_equal(np.asarray(out["sv"])[got], v[order]) and np.all(np.asarray(out["c"]) == 1)


@pytest.mark.parametrize("nparts", [16, 5000])
def test_hash_partition_of_one_and_two_passes(jit_tc, nparts):
    """the views' index vectors one after the other are the stable sort of the rows by partition; twice (the workspace is the operator's)"""
    import torch
    tc = jit_tc
    t = rand_table(56, 20_000, 0.1)
    ot = O.Table.from_arrow(t)
    src = g.MemoryExec([t])
    keys = [col("k64", src.schema())]
    pid = np.asarray(O.hash_partition(ot, keys, nparts), dtype=np.int64)
    plan = g.RepartitionExec(src, keys, nparts)
    for _ in range(2):
        views = plan.execute_all(0, tc)
        assert np.array_equal(np.array([v.num_rows for v in views], dtype=np.int64), np.bincount(pid, minlength=nparts))
        order = torch.cat([v.via[0][:v.num_rows] for v in views]).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        assert np.array_equal(order, np.argsort(pid, kind="stable"))
