"""Hash aggregate whose whole key fits the slot's state word (csrc/kernels_hash.hip ht_state_find_or_insert, KeySpec::state_key): one
compare-and-swap claims a slot and publishes the key, the groups are extracted straight into the result columns.  AggregateExec("Single",
strategy="hash") against the oracle over narrow keys of every eligible type (values 0, the type's minimum and maximum, NULL), every
accumulator kind, a fused predicate, the row counts around a wave, and the shapes that stress the slot protocol: one key for all rows,
all keys distinct, runs of equal keys with and without their order, a table that fills up and is regrown.  Keys that are not eligible
(Int64, three columns) keep the key-word protocol and are checked the same way."""
import numpy as np
import pyarrow as pa
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit
from oracle import oracle_np as O
from test_gpu_operators import agg_cases, close_rows, dev_rows, native_rows_of, norm, ora_rows, rand_table

pytestmark = pytest.mark.gpu

EXTREMES = {"u32": (0, 2**32 - 1, np.uint32, pa.uint32()), "i32": (-2**31, 2**31 - 1, np.int32, pa.int32()), "d32": (-2**31, 2**31 - 1, np.int32, pa.date32()),
            "i16": (-2**15, 2**15 - 1, np.int16, pa.int16()), "i8": (-2**7, 2**7 - 1, np.int8, pa.int8())}
KEY_SHAPES = [["u32"], ["i32"], ["d32"], ["i16", "i8"]]


def key_column(r, name, n, nullable, domain):
    """n values of the type: 0, its minimum and maximum among `domain` other values; NULLs when nullable"""
    lo, hi, npt, pat = EXTREMES[name]
    pool = np.concatenate([np.array([0, lo, hi], dtype=np.int64), r.integers(max(lo, -10**6), min(hi, 10**6) + 1, max(domain - 3, 1))])
    vals = pool[r.integers(0, len(pool), n)]
    if n >= 3:
        vals[:3] = [0, lo, hi]
    mask = (r.random(n) < 0.1) if nullable else None
    if nullable and n >= 4:
        mask[:3] = False; mask[3] = True
    a = pa.array(vals.astype(npt), mask=mask)
    return a.cast(pat) if pat != a.type else a


def table_with_keys(seed, n, nullable, domain=300):
    r = np.random.default_rng(seed)
    t = rand_table(seed, n, 0.15 if nullable else 0.0)
    for name in EXTREMES:
        dom = 7 if name == "i8" else domain
        t = t.append_column(pa.field(name, EXTREMES[name][3], nullable=nullable), key_column(r, name, n, nullable, dom))
    return t


def acc_lists(s):
    """the two lists of agg_cases that between them hold every accumulator kind (the second one's MIN over a float keeps rows unfolded)"""
    c = agg_cases(s)
    return [c[0][1], c[1][1]]


def check(tc, t, key_names, aggs_of, pred_of=None, **kw):
    src = g.MemoryExec([t])
    s = src.schema()
    ot = O.Table.from_arrow(t)
    groups = [(col(k, s), k) for k in key_names]
    pred = pred_of(s) if pred_of else None
    for aggs in aggs_of(s):
        plan = g.AggregateExec("Single", groups, aggs, g.FilterExec(pred, src) if pred is not None else src, strategy="hash", **kw)
        exp = norm(ora_rows(O.aggregate(ot, groups, aggs, "Single", predicate=pred)))
        close_rows(norm(dev_rows(tc, plan.execute(0, tc))), exp)
    return plan, exp


PRED = lambda s: binary(col("k32", s), Op.Gt, lit(-30, "Int32"))      # noqa: E731


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 5000, 60_000])
def test_state_key_grid(tc, n, nullable):
    t = table_with_keys(900 + n, n, nullable)
    for keys in KEY_SHAPES:
        check(tc, t, keys, acc_lists, PRED)


SUMS = lambda s: [[{"fn": "SUM", "expr": col("k64", s), "name": "sk"}, {"fn": "COUNT", "expr": lit(1), "name": "c"}, {"fn": "MAX", "expr": col("k32", s), "name": "mx"}]]      # noqa: E731


def with_key(n, keys, seed=1):
    t = rand_table(seed, n)
    return t.append_column("u32", pa.array(np.asarray(keys, dtype=np.uint32)))


def test_every_row_one_key(tc):
    """every lane of every wave contends for one slot"""
    for n in (65, 60_000):
        _, exp = check(tc, with_key(n, np.full(n, 4_000_000_000)), ["u32"], SUMS)
        assert len(exp) == 1
        _, exp = check(tc, with_key(n, np.full(n, 4_000_000_000)), ["u32"], lambda s: [agg_cases(s)[1][1]])      # (unfolded: MIN over a float)
        assert len(exp) == 1


def test_all_keys_distinct_in_random_order(tc):
    n = 60_000
    keys = np.random.default_rng(2).permutation(n).astype(np.int64) * 71_000 % (2**32)
    assert len(set(keys.tolist())) == n
    _, exp = check(tc, with_key(n, keys), ["u32"], SUMS)
    assert len(exp) == n


def test_runs_of_equal_keys_then_shuffled(tc):
    """keys in runs of 2-5 (folded inside the wave), then the same rows shuffled (hardly a run left): the same groups"""
    r = np.random.default_rng(3)
    keys = np.repeat(r.permutation(20_000) * 9 + 1, r.integers(2, 6, 20_000))
    n = len(keys)
    t = with_key(n, keys)
    _, exp_runs = check(tc, t, ["u32"], SUMS)
    _, exp_shuf = check(tc, t.take(pa.array(r.permutation(n))), ["u32"], SUMS)
    assert exp_runs == exp_shuf and len(exp_runs) == 20_000


def test_table_full_then_regrown(tc):
    n = 5000
    _, exp = check(tc, with_key(n, np.arange(n) * 3), ["u32"], SUMS, expected_groups=1)
    assert len(exp) == n


def test_ineligible_keys_keep_the_key_words(tc):
    t = table_with_keys(77, 20_000, True)
    check(tc, t, ["k64"], acc_lists, PRED)                       # Int64: 64 bits
    check(tc, t, ["k64", "d", "k32"], acc_lists, PRED)           # three columns, beyond 62 bits


def state_key_of(p):
    """state_key of the aggregate operator a NativePlan compiled, from the operator's own description"""
    import json
    aggs = [json.loads(o["desc"]) for o in p.profile_all() if o["op"] == "aggregate"]
    assert len(aggs) == 1
    return g.compile_check(aggs[0])["state_key"]


def test_large_input_counting_pass_and_regrown_result(tc):
    """More than 2^20 rows: the group count is not bounded by a small input, so the first run counts the groups before it extracts
    them, later runs size the result from the last count -- and an input with many more groups overflows that and is extracted again
    into re-laid columns.  UInt32 state-word key; expected sums by numpy."""
    n = (1 << 20) + 70_001
    r = np.random.default_rng(9)

    def table(ngroups):
        return pa.table({"u32": pa.array((r.integers(0, ngroups, n) * 4099 % (2**32)).astype(np.uint32)), "v": pa.array(r.integers(-10**9, 10**9, n))})

    def expected(t):
        k, v = t["u32"].to_numpy().astype(np.int64), t["v"].to_numpy()
        u, inv = np.unique(k, return_inverse=True)
        sv = np.zeros(len(u), dtype=np.int64)
        np.add.at(sv, inv, v)
        return sorted(zip(u.tolist(), np.bincount(inv).tolist(), sv.tolist()))
    small, big = table(50_000), table(400_000)
    src = g.MemoryExec([small])
    s = src.schema()
    p = g.NativePlan(g.AggregateExec("Single", [(col("u32", s), "u32")], [{"fn": "COUNT", "expr": lit(1), "name": "c"}, {"fn": "SUM", "expr": col("v", s), "name": "sv"}], src, strategy="hash"), tc)

    def run():
        t = p.execute(0).to_arrow()
        return sorted(zip(t["u32"].to_pylist(), t["c"].to_pylist(), t["sv"].to_pylist()))
    assert run() == expected(small)                     # counting pass, then the extract
    assert state_key_of(p) is True
    assert run() == expected(small) and p.exec_stats()["deferred"]
    p.set_input(0, g.DeviceTable.from_arrow(big, tc.device))
    assert run() == expected(big)                       # 8 x the groups: the deferred run does not hold, the synchronous one outgrows the remembered count
    assert p.exec_stats()["retries"] == 1
    assert run() == expected(big)


def test_native_plan_three_executions(tc):
    """one handle, three executions: the first synchronous, the others deferred (nothing read back before the settle)"""
    t = table_with_keys(78, 40_000, True)
    src = g.MemoryExec([t])
    s = src.schema()
    ot = O.Table.from_arrow(t)
    for keys in (["u32"], ["i16", "i8"]):
        groups = [(col(k, s), k) for k in keys]
        aggs = agg_cases(s)[0][1]
        plan = g.AggregateExec("Single", groups, aggs, g.FilterExec(PRED(s), src), strategy="hash")
        exp = norm(ora_rows(O.aggregate(ot, groups, aggs, "Single", predicate=PRED(s))))
        p = g.NativePlan(plan, tc)
        for k in range(3):
            tb = p.execute(0).to_arrow()
            cols = []
            for f, c in zip(tb.schema, tb.columns):
                if pa.types.is_decimal128(f.type):
                    cols.append([None if v is None else int(v.scaleb(f.type.scale)) for v in c.to_pylist()])
                elif pa.types.is_date32(f.type):
                    cols.append(c.cast(pa.int32()).to_pylist())
                else:
                    cols.append(c.to_pylist())
            close_rows(norm(list(zip(*cols))), exp)
            assert p.exec_stats()["deferred"] == (k > 0), (k, p.exec_stats())
        assert state_key_of(p) is True                  # the operator that ran is one whose key lives in the state word ...
    p = g.NativePlan(g.AggregateExec("Single", [(col("k64", s), "k64")], agg_cases(s)[0][1], src, strategy="hash"), tc)
    p.execute(0)
    assert state_key_of(p) is False                     # ... and an Int64 key is not
