"""Aggregate over key-clustered input by runs (csrc/kernels_hash.hip k_agg_runs_count / k_agg_runs_order / k_agg_runs_write; the
fourth aggregate path, csrc/capi.cpp): input whose packed key arrives in runs of equal values with strictly increasing heads needs no
hash table -- every group is one run and the result is one row per run.  strategy="runs" reaches the path at any size; "auto" tries it
from 2^20 rows on where the global table would be next.  Input that is not so clustered falls to the table inside the same call (no
retry is booked); a deferred execution that meets such input is redone once and the operator keeps to the table from then on.

Every case is checked against the oracle's aggregate over SUM + COUNT, with BIT_OR per group by numpy next to it as in
test_gpu_bitwise.py (the oracle has no bitwise functions), and numpy alone for the 2^20-row case; the operator's
"agg_path" (NativePlan.profile_all) says which way the last run took.  The path needs a key that packs into the table's state word
(csrc/agg_compile.cpp: 62 bits), so an Int32 key takes it and an Int64 key -- run through the same cases -- must come out right by the
table: `expect_runs` states that per key type.  Keys are non-negative: the packed form of a signed key orders as its unsigned
pattern."""
import numpy as np
import pyarrow as pa
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit
from oracle import oracle_np as O
from test_gpu_agg_by_build_row import by_build_row, native_rows
from test_gpu_operators import close_rows, norm, ora_rows

pytestmark = pytest.mark.gpu

KEY_TYPES = {"int32": (np.int32, pa.int32()), "int64": (np.int64, pa.int64())}


def agg_path(p):
    aggs = [o for o in p.profile_all() if o["op"] == "aggregate"]
    assert len(aggs) == 1
    return aggs[0]["agg_path"]


def expect_runs(key_type):
    return key_type == "int32"


def table(keys, key_type="int32", seed=0, key_mask=None, value_nulls=0.0, extra=None):
    r = np.random.default_rng(seed)
    n = len(keys)
    npt, pat = KEY_TYPES[key_type]
    vmask = (r.random(n) < value_nulls) if value_nulls > 0 else None
    cols = {"k": pa.array(np.asarray(keys, dtype=npt), type=pat, mask=key_mask),
            "v": pa.array(r.integers(-10**12, 10**12, n), type=pa.int64(), mask=vmask),
            "b": pa.array(r.integers(0, 2**40, n), type=pa.int64())}
    cols.update(extra or {})
    fields = [pa.field(name, a.type, nullable=a.null_count > 0 or (name == "k" and key_mask is not None)) for name, a in cols.items()]
    return pa.Table.from_arrays(list(cols.values()), schema=pa.schema(fields))


def aggs_of(s):
    return [{"fn": "SUM", "expr": col("v", s), "name": "sv"}, {"fn": "COUNT", "expr": lit(1), "name": "c"}, {"fn": "COUNT", "expr": col("v", s), "name": "cv"},
            {"fn": "BIT_OR", "expr": col("b", s), "name": "bo"}]


def with_bit_or(rows, keys, bits, n_keys=1):
    """oracle rows (keys..., sums and counts) + BIT_OR of `bits` per key tuple (rows of `keys`: one tuple per input row that counts)"""
    acc = {}
    for k, x in zip(keys, bits):
        acc[k] = acc.get(k, 0) | int(x)
    return [tuple(r) + (acc[tuple(r[:n_keys])],) for r in rows]


def expected_rows(t, s, pred=None, keep=None):
    """`keep`: the predicate's outcome per row, by numpy"""
    rows = ora_rows(O.aggregate(O.Table.from_arrow(t), [(col("k", s), "k")], aggs_of(s)[:3], "Single", predicate=pred))
    sel = np.arange(t.num_rows) if keep is None else np.flatnonzero(keep)
    k, b = t["k"].to_pylist(), t["b"].to_numpy()
    return norm(with_bit_or(rows, [(k[i],) for i in sel], b[sel]))


def check(tc, t, strategy="runs", pred_of=None, keep=None):
    """(NativePlan after one execution that equals the oracle, the expected rows)"""
    src = g.MemoryExec([t])
    s = src.schema()
    groups = [(col("k", s), "k")]
    pred = pred_of(s) if pred_of else None
    plan = g.AggregateExec("Single", groups, aggs_of(s), g.FilterExec(pred, src) if pred is not None else src, strategy=strategy)
    exp = expected_rows(t, s, pred, keep)
    p = g.NativePlan(plan, tc)
    close_rows(norm(native_rows(p)), exp)
    assert p.exec_stats()["retries"] == 0
    return p, exp


@pytest.mark.parametrize("key_type", ["int32", "int64"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4 * 256 * 3 + 1])
def test_row_counts_all_keys_distinct(tc, n, key_type):
    p, exp = check(tc, table(np.arange(n) * 3 + 1, key_type, seed=n), "runs")
    assert len(exp) == n
    assert (agg_path(p) == "runs") == expect_runs(key_type), agg_path(p)


@pytest.mark.parametrize("key_type", ["int32", "int64"])
def test_one_run(tc, key_type):
    p, exp = check(tc, table(np.full(1000, 77), key_type, seed=1), "runs")
    assert len(exp) == 1
    assert (agg_path(p) == "runs") == expect_runs(key_type)


@pytest.mark.parametrize("key_type", ["int32", "int64"])
@pytest.mark.parametrize("n,a,b", [(300, 60, 70), (600, 250, 260), (600, 30, 229)], ids=["wave_boundary", "block_boundary", "whole_words_inside"])
def test_runs_crossing_boundaries(tc, n, a, b, key_type):
    keys = np.arange(n) * 3 + 1
    keys[a:b + 1] = keys[a]
    p, exp = check(tc, table(keys, key_type, seed=2), "runs")
    assert len(exp) == n - (b - a)
    assert (agg_path(p) == "runs") == expect_runs(key_type)


def heavy_keys(n, longest=7):
    """runs of length 1..longest, keys ascending with gaps"""
    lens = np.arange(n) % longest + 1
    keys = np.repeat(np.arange(n) * 5 + 2, lens)
    return keys[:n]


@pytest.mark.parametrize("key_type", ["int32", "int64"])
def test_heavy_runs(tc, key_type):
    p, exp = check(tc, table(heavy_keys(50_000), key_type, seed=3), "runs")
    assert len(exp) > 12_000
    assert (agg_path(p) == "runs") == expect_runs(key_type)


UNORDERED = {"descending": np.arange(2000)[::-1] + 5, "p121": np.array([1, 2, 1]), "p3311": np.array([3, 3, 1, 1]),
             "p121_runs_far_apart": np.repeat([1, 2, 1], [100, 300, 100]), "one_step_back_late": np.concatenate([np.arange(5000) * 2, [9001], np.arange(5000, 6000) * 2])}


@pytest.mark.parametrize("key_type", ["int32", "int64"])
@pytest.mark.parametrize("name", sorted(UNORDERED))
def test_keys_out_of_order_fall_back_in_the_same_call(tc, name, key_type):
    p, _ = check(tc, table(UNORDERED[name], key_type, seed=4), "runs")      # (check: the result is right and no retry was booked)
    assert agg_path(p) == "table"
    for _ in range(2):
        p.execute(0)
        assert p.exec_stats()["retries"] == 0 and agg_path(p) == "table"


# The order test across segments (k_agg_runs_order) is a one-block running maximum over the segments (csrc/gpuq_dev.h block_walk_scan):
# every wave owns ((segments + 15) / 16 rounded up to 64) of them and walks them 64 at a time.  A segment is one wave's two 64-row words
# (csrc/kernels_hash.hip agg_runs_geometry, while the input has at most 2 * 32 words per compute unit), so `segs` segments are
# 128 * segs rows less a ragged tail.  Only a segment's FIRST head is left to that kernel (the count kernel has tested the others inside
# the segment), so the out-of-order key goes to the first row of a segment.
def seg_keys(tc, segs, bad_seg=None):
    import torch
    n = 128 * segs - 5
    assert (n + 63) // 64 <= torch.cuda.get_device_properties(tc.device).multi_processor_count * 32 * 2
    keys = np.arange(n) * 3 + 1
    if bad_seg is not None:
        keys[128 * bad_seg] = keys[128 * bad_seg - 2] + 1      # a key of its own, below the last key of the segment before
    return keys


def wave_range_start(segs):
    """the first segment of a wave's range, the middle one of the ranges that start inside (0, segs); None when wave 0 owns them all"""
    per = ((segs + 15) // 16 + 63) & ~63
    starts = list(range(per, segs, per))
    return starts[len(starts) // 2] if starts else None


@pytest.mark.parametrize("segs", [64, 65, 1024, 1025])
def test_segment_counts_at_the_order_scan_edges_in_order(tc, segs):
    p, exp = check(tc, table(seg_keys(tc, segs), seed=segs), "runs")
    assert len(exp) == 128 * segs - 5 and agg_path(p) == "runs"


@pytest.mark.parametrize("where", ["first_of_a_wave_range", "last_segment"])
@pytest.mark.parametrize("segs", [64, 65, 1024, 1025])
def test_one_head_out_of_order_at_the_order_scan_edges(tc, segs, where):
    """the flag is raised and the table takes over inside the same call (check: the result equals the oracle's, no retry booked).
    64 segments are wave 0's alone: no other wave range starts there, so that case puts the head into the last segment of the
    one 64-item step both times."""
    bad = wave_range_start(segs) if where == "first_of_a_wave_range" else segs - 1
    assert (bad is None) == (segs == 64 and where == "first_of_a_wave_range")
    p, exp = check(tc, table(seg_keys(tc, segs, segs - 1 if bad is None else bad), seed=segs), "runs")
    assert len(exp) == 128 * segs - 5 and agg_path(p) == "table"


def test_null_arguments_and_a_null_key_run(tc):
    """NULL arguments inside runs (SUM and COUNT(v) skip them; a run of only NULLs sums to NULL); a nullable key with one NULL run -- its
    packed form lies above every value, so as the last run it keeps the order and in the middle it breaks it: right either way."""
    keys = heavy_keys(20_000)
    p, exp = check(tc, table(keys, seed=5, value_nulls=0.4), "runs")
    assert agg_path(p) == "runs" and any(r[1] is None for r in exp) and any(r[3] not in (0, r[2]) for r in exp)
    for lo, hi in ((len(keys) - 40, len(keys)), (7000, 7100)):
        mask = np.zeros(len(keys), dtype=bool); mask[lo:hi] = True
        p, exp = check(tc, table(keys, seed=6, key_mask=mask, value_nulls=0.2), "runs")
        assert sum(r[0] is None for r in exp) == 1
        assert agg_path(p) == ("runs" if hi == len(keys) else "table")


def test_predicate_drops_a_row_inside_a_run(tc):
    """the rows around the dropped one are two runs of one key: out of order by the path's rule, so the table takes it"""
    keys = np.repeat(np.arange(4000) * 2 + 1, 5)
    drop = np.zeros(len(keys), dtype=np.int32); drop[[502, 7777]] = 1      # third row of a run of five
    t = table(keys, seed=7, extra={"drop": pa.array(drop)})
    p, exp = check(tc, t, "runs", pred_of=lambda s: binary(col("drop", s), Op.Eq, lit(0, "Int32")), keep=drop == 0)
    assert len(exp) == 4000 and agg_path(p) == "table"


def test_predicate_drops_whole_runs(tc):
    keys = np.repeat(np.arange(4000) * 2 + 1, 5)
    drop = ((keys // 2) % 3 == 1).astype(np.int32)
    drop[:300] = 1      # ... among them the first words of the input
    t = table(keys, seed=8, extra={"drop": pa.array(drop)})
    p, exp = check(tc, t, "runs", pred_of=lambda s: binary(col("drop", s), Op.Eq, lit(0, "Int32")), keep=drop == 0)
    assert 2000 < len(exp) < 4000 and agg_path(p) == "runs"


def test_deferred_runs_then_shuffled_input_is_redone_once(tc):
    """2^20 + 5 ordered rows under "auto": the first execution tries runs, the next ones replay them deferred.  The same rows shuffled
    under the plan raise the order bit at the settle: one retry, redone through the table, which the operator then keeps to.
    (Runs of 1..3 rows: the first run's key sample then sees most keys once and sends the input to the global table, where runs are
    tried; with every key seen several times it would go to the radix path, as before.)"""
    n = (1 << 20) + 5
    r = np.random.default_rng(9)
    keys = heavy_keys(n, 3).astype(np.int32)
    v = r.integers(-10**9, 10**9, n)

    def tab(perm=None):
        k, vv = (keys, v) if perm is None else (keys[perm], v[perm])
        return pa.table({"k": pa.array(k, pa.int32()), "v": pa.array(vv, pa.int64())})
    u, inv = np.unique(keys, return_inverse=True)
    sv = np.zeros(len(u), dtype=np.int64)
    np.add.at(sv, inv, v)
    exp = sorted(zip(u.tolist(), sv.tolist(), np.bincount(inv).tolist()))
    src = g.MemoryExec([tab()])
    s = src.schema()
    p = g.NativePlan(g.AggregateExec("Single", [(col("k", s), "k")], [{"fn": "SUM", "expr": col("v", s), "name": "sv"}, {"fn": "COUNT", "expr": lit(1), "name": "c"}], src), tc)

    def run():
        t = p.execute(0).to_arrow()
        return sorted(zip(t["k"].to_pylist(), t["sv"].to_pylist(), t["c"].to_pylist()))
    assert run() == exp and agg_path(p) == "runs" and not p.exec_stats()["deferred"]
    for _ in range(3):
        assert run() == exp
        st = p.exec_stats()
        assert st["deferred"] and st["retries"] == 0 and agg_path(p) == "runs", st
    p.set_input(0, g.DeviceTable.from_arrow(tab(r.permutation(n)), tc.device))
    assert run() == exp
    st = p.exec_stats()
    assert not st["deferred"] and st["retries"] == 1, st
    for _ in range(2):
        assert run() == exp
        st = p.exec_stats()
        assert st["deferred"] and st["retries"] == 1 and agg_path(p) == "table", st


# ------------------------------------------------------------------------------------ the join shape: group by the build row
def join_agg(bt, pt):
    L, R = g.MemoryExec([bt]), g.MemoryExec([pt])
    ls, rs = L.schema(), R.schema()
    on = [(col("bk", ls), col("pk", rs))]
    j = g.HashJoinExec(L, R, on, None, "Inner", "CollectLeft", False)
    js = j.schema()
    groups = [(col(n, js), n) for n in ("pk", "bd")]
    aggs = [{"fn": "SUM", "expr": col("pv", js), "name": "sv"}, {"fn": "COUNT", "expr": lit(1), "name": "c"}, {"fn": "BIT_OR", "expr": col("pb", js), "name": "bo"}]
    plan = g.AggregateExec("Single", groups, aggs, j, strategy="runs")
    ol, orr = O.Table.from_arrow(bt), O.Table.from_arrow(pt)
    pairs = O.hash_join(ol, orr, on, "Inner")
    lj, rj = ol.take([i for i, _ in pairs]), orr.take([k for _, k in pairs])
    joined = O.Table(lj.names + rj.names, lj.types + rj.types, lj.cols + rj.cols)
    rows = [tuple(r) for r in O.aggregate(joined, groups, aggs[:2], "Single").rows()]
    jc = {n: c for n, c in zip(joined.names, joined.cols)}
    return plan, norm(with_bit_or(rows, list(zip(jc["pk"], jc["bd"])), jc["pb"], n_keys=2))


def join_tables(permute_build):
    r = np.random.default_rng(10)
    nb, npr = 3000, 30_000
    bk = np.arange(nb, dtype=np.int64) * 3 + 7
    if permute_build:
        bk = bk[r.permutation(nb)]
    bt = pa.table({"bk": pa.array(bk), "bd": pa.array(r.integers(9000, 9400, nb).astype(np.int32)).cast(pa.date32())})
    pk = np.sort(np.where(r.random(npr) < 0.7, (r.integers(0, nb, npr) * 3 + 7), -5 - r.integers(0, 1000, npr)))
    pt = pa.table({"pk": pa.array(pk.astype(np.int64)), "pv": pa.array(r.integers(-10**6, 10**6, npr)), "pb": pa.array(r.integers(0, 2**30, npr))})
    return bt, pt


@pytest.mark.parametrize("permute_build", [False, True], ids=["build_in_key_order", "build_permuted"])
def test_join_shape_groups_by_the_build_row(tc, permute_build):
    """the aggregate above a unique-key join groups by the build row; the pair list comes in probe order, so with the probe sorted and the
    build side stored in key order the build rows arrive in increasing runs -- and with the build side permuted they do not"""
    plan, exp = join_agg(*join_tables(permute_build))
    assert len(exp) > 1000
    p = g.NativePlan(plan, tc)
    for k in range(3):
        close_rows(norm(native_rows(p)), exp)
        assert p.exec_stats()["retries"] == 0 and p.exec_stats()["deferred"] == (k > 0)
        assert agg_path(p) == ("table" if permute_build else "runs")
    assert by_build_row(p)
