"""AggregateExec directly above an Inner HashJoinExec over unique build keys (csrc/plan_exec.cpp, BuildRows): when the group
columns are the join keys plus build-side columns, two joined rows are in one group exactly when they came from one build row,
and the native executor groups by that row (one UInt32) instead of by the declared columns -- the operator's descriptor then
says "group_by":"build_row".  Every case runs through NativePlan and is checked against the oracle's join + aggregate; the cases
that must NOT be rewritten (duplicate build keys, no join key among the groups, a probe-side group column, an outer join) assert
that too."""
import json

import numpy as np
import pyarrow as pa
import pytest

import arrow_ballista_amd as g
import tpch_util as T
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit
from oracle import oracle_np as O
from test_gpu_native_plan import arrow_rows
from test_gpu_operators import close_rows, norm

pytestmark = pytest.mark.gpu


def by_build_row(plan):
    """Did the plan's aggregate group by the build row?"""
    aggs = [json.loads(o["desc"]) for o in plan.profile_all() if o["op"] == "aggregate"]
    assert aggs, "the plan compiled no aggregate operator"
    return any(d.get("group_by") == "build_row" for d in aggs)


def native_rows(p):
    t = p.execute(0).to_arrow()
    cols = []
    for f, c in zip(t.schema, t.columns):
        if pa.types.is_decimal128(f.type):
            cols.append([None if v is None else int(v.scaleb(f.type.scale)) for v in c.to_pylist()])
        elif pa.types.is_date32(f.type):
            cols.append(c.cast(pa.int32()).to_pylist())
        else:
            cols.append(c.to_pylist())
    return list(zip(*cols)) if cols else []


def build_table(seed, n, dup=False, nulls=0.0, key_stride=3):
    r = np.random.default_rng(seed)
    keys = np.arange(n, dtype=np.int64) * key_stride + 7
    if dup:
        keys[n // 2:] = keys[:n - n // 2]            # every key of the first half occurs twice
    keys = keys[r.permutation(n)]
    mask = (lambda: r.random(n) < nulls) if nulls > 0 else (lambda: None)
    return pa.table({"bk": pa.array(keys), "bk2": pa.array((keys % 5).astype(np.int32)),
                     "bd": pa.array(r.integers(9000, 9400, n).astype(np.int32), mask=mask()).cast(pa.date32()),
                     "bp": pa.array(r.integers(-3, 4, n).astype(np.int32), mask=mask()),
                     "b64": pa.array(r.integers(-2**40, 2**40, n), mask=mask())})


def probe_table(seed, n, build, hit=0.7, in_order=True):
    r = np.random.default_rng(seed)
    bk = build.column("bk").to_numpy()
    keys = np.where(r.random(n) < hit, bk[r.integers(0, len(bk), n)], -5 - r.integers(0, 1000, n))
    if in_order:
        keys = np.sort(keys)
    return pa.table({"pk": pa.array(keys.astype(np.int64)), "pk2": pa.array((keys % 5).astype(np.int32)),
                     "pv": pa.array(r.integers(-10**6, 10**6, n)), "pg": pa.array(r.integers(0, 3, n).astype(np.int32)),
                     "pd": pa.array(r.integers(9000, 9400, n).astype(np.int32)).cast(pa.date32())})


AGGS = lambda s: [{"fn": "SUM", "expr": col("pv", s), "name": "sv"}, {"fn": "COUNT", "expr": lit(1), "name": "c"},      # noqa: E731
                  {"fn": "MIN", "expr": col("pv", s), "name": "mn"}, {"fn": "MAX", "expr": col("pd", s), "name": "mx"}]


def join_agg(bt, pt, on_names, group_names, jt="Inner", probe_pred=None):
    """(plan, oracle rows) of AggregateExec(Single, group_names) over HashJoinExec(bt, pt) on on_names = [(build, probe)]."""
    L, R = g.MemoryExec([bt]), g.MemoryExec([pt])
    ls, rs = L.schema(), R.schema()
    on = [(col(a, ls), col(b, rs)) for a, b in on_names]
    right = g.CoalesceBatchesExec(g.FilterExec(probe_pred(rs), R)) if probe_pred else R
    j = g.HashJoinExec(L, right, on, None, jt, "CollectLeft", False)
    js = j.schema()
    groups = [(col(n, js), n) for n in group_names]
    plan = g.AggregateExec("Single", groups, AGGS(js), j)
    ol, orr = O.Table.from_arrow(bt), O.Table.from_arrow(pt)
    pairs = O.hash_join(ol, orr, on, jt, right_pred=probe_pred(rs) if probe_pred else None)
    lj, rj = ol.take([i for i, _ in pairs]), orr.take([k for _, k in pairs])
    joined = O.Table(lj.names + rj.names, lj.types + rj.types, lj.cols + rj.cols)
    exp = norm([tuple(r) for r in O.aggregate(joined, groups, AGGS(js), "Single").rows()])
    return plan, exp


def check(tc, plan, exp, rewritten, runs=1):
    p = g.NativePlan(plan, tc)
    for k in range(runs):
        close_rows(norm(native_rows(p)), exp)
        if k > 0:
            assert p.exec_stats()["deferred"], p.exec_stats()
    assert by_build_row(p) == rewritten
    return p


# ------------------------------------------------------------------------------------ q3's own shape
def _q3_tables(tc, n_li, n_cust):
    cols = ("l_orderkey", "l_suppkey", "l_extendedprice", "l_discount", "l_shipdate")
    li = T.gen_lineitem_device(tc, n_li, n_supp=100, columns=cols)
    od = T.gen_orders_device(tc, (n_li + 3) // 4, n_cust)
    cu = T.gen_customer_device(tc, n_cust)
    hl = T.lineitem_host_to_arrow(T.gen_lineitem_host(n_li, n_supp=100), n_li)
    ho, hc, _ = T.gen_other_tables_host((n_li + 3) // 4, n_cust, 100)
    return (li, od, cu), (hl, ho, hc)


def _check_q3(got, exp):
    assert len(got) == len(exp) and len(exp) > 0
    assert [(r[1], r[2]) for r in got] == [(r[1], r[2]) for r in exp]      # the ORDER BY columns, in order
    assert sorted(got) == sorted(exp)


@pytest.fixture(scope="module")
def q3(tc):
    dev, host = _q3_tables(tc, 80_000, 1500)
    return dev, host, T.q3_oracle(host[2], host[1], host[0])


def test_q3_groups_by_the_orders_row(tc, q3):
    (li, od, cu), _, exp = q3
    p = g.NativePlan(T.q3_plan(g.MemoryExec([cu]), g.MemoryExec([od]), g.MemoryExec([li])), tc)
    _check_q3(arrow_rows(p.execute(0).to_arrow()), exp)
    assert by_build_row(p)
    assert [n for n, _, _ in p.schema()] == ["l_orderkey", "revenue", "o_orderdate", "o_shippriority"]
    got = p.execute(0).to_arrow()
    assert p.exec_stats()["deferred"] and p.exec_stats()["retries"] == 0
    assert got.schema.names == ["l_orderkey", "revenue", "o_orderdate", "o_shippriority"]
    _check_q3(arrow_rows(got), exp)


def test_q3_probe_side_shuffled(tc, q3):
    """The rewrite needs no row order: lineitem shuffled, the same groups."""
    (_, od, cu), (hl, _, _), exp = q3
    perm = np.random.default_rng(5).permutation(hl.num_rows)
    li = hl.take(pa.array(perm))
    p = g.NativePlan(T.q3_plan(g.MemoryExec([cu]), g.MemoryExec([od]), g.MemoryExec([li])), tc)
    for _ in range(2):
        _check_q3(arrow_rows(p.execute(0).to_arrow()), exp)
    assert by_build_row(p)


# ------------------------------------------------------------------------------------ where the rewrite applies
def test_group_by_probe_key_and_build_columns(tc):
    bt = build_table(1, 5000); pt = probe_table(2, 40_000, bt)
    plan, exp = join_agg(bt, pt, [("bk", "pk")], ["pk", "bd", "bp"])
    assert len(exp) > 1000
    check(tc, plan, exp, True, runs=3)


def test_group_by_build_key(tc):
    bt = build_table(3, 2000); pt = probe_table(4, 20_000, bt, in_order=False)
    plan, exp = join_agg(bt, pt, [("bk", "pk")], ["bd", "bk"])
    check(tc, plan, exp, True, runs=2)


def test_build_side_group_columns_with_nulls(tc):
    bt = build_table(5, 3000, nulls=0.3); pt = probe_table(6, 30_000, bt)
    plan, exp = join_agg(bt, pt, [("bk", "pk")], ["pk", "bd", "bp", "b64"], probe_pred=lambda rs: binary(col("pg", rs), Op.Gt, lit(0, "Int32")))
    assert any(r[1] is None for r in exp) and any(r[3] is None for r in exp)
    check(tc, plan, exp, True, runs=2)


def test_two_key_join_both_keys_grouped(tc):
    bt = build_table(7, 4000); pt = probe_table(8, 30_000, bt)
    plan, exp = join_agg(bt, pt, [("bk", "pk"), ("bk2", "pk2")], ["pk", "pk2", "bd"])
    assert len(exp) > 1000
    check(tc, plan, exp, True, runs=2)


def test_empty_join_result(tc):
    bt = build_table(9, 2000); pt = probe_table(10, 20_000, bt, hit=0.0)
    plan, exp = join_agg(bt, pt, [("bk", "pk")], ["pk", "bd"])
    assert exp == []
    check(tc, plan, exp, True, runs=2)


# ------------------------------------------------------------------------------------ where it must not
def test_duplicate_build_keys_are_not_rewritten(tc):
    bt = build_table(11, 4000, dup=True); pt = probe_table(12, 20_000, bt)
    plan, exp = join_agg(bt, pt, [("bk", "pk")], ["pk", "bd", "bp"])
    check(tc, plan, exp, False, runs=2)


def test_group_list_without_the_join_key_is_not_rewritten(tc):
    bt = build_table(13, 2000); pt = probe_table(14, 20_000, bt)
    plan, exp = join_agg(bt, pt, [("bk", "pk")], ["bd", "bp"])
    check(tc, plan, exp, False, runs=2)


def test_probe_side_group_column_is_not_rewritten(tc):
    bt = build_table(15, 2000); pt = probe_table(16, 20_000, bt)
    plan, exp = join_agg(bt, pt, [("bk", "pk")], ["pk", "bd", "pg"])
    check(tc, plan, exp, False, runs=2)


def test_left_join_is_not_rewritten(tc):
    bt = build_table(17, 2000); pt = probe_table(18, 20_000, bt, hit=0.3)
    plan, exp = join_agg(bt, pt, [("bk", "pk")], ["bk", "bd"], jt="Left")
    assert any(r[2] is None for r in exp)          # build rows without a match: one group each, no probe values
    check(tc, plan, exp, False, runs=2)


# ------------------------------------------------------------------------------------ the build side changes under the handle
def test_build_side_gets_duplicate_keys_under_the_plan(tc):
    """Three executions over unique build keys (synchronous, then deferred), then the build input is replaced by one WITH duplicate
    keys: the deferred run's remembered "unique" no longer holds, the execution is redone synchronously -- over the declared group
    columns -- and equals the oracle; back on unique keys it groups by the build row again."""
    bt = build_table(19, 6000); pt = probe_table(20, 40_000, bt)
    plan, exp = join_agg(bt, pt, [("bk", "pk")], ["pk", "bd", "bp"])
    p = check(tc, plan, exp, True, runs=3)
    bt2 = build_table(19, 6000, dup=True)
    _, exp2 = join_agg(bt2, pt, [("bk", "pk")], ["pk", "bd", "bp"])
    assert exp2 != exp
    p.set_input(0, g.DeviceTable.from_arrow(bt2, tc.device))
    close_rows(norm(native_rows(p)), exp2)
    st = p.exec_stats()
    assert not st["deferred"] and st["retries"] == 1, st
    close_rows(norm(native_rows(p)), exp2)
    p.set_input(0, g.DeviceTable.from_arrow(bt, tc.device))
    close_rows(norm(native_rows(p)), exp)


def test_offset_between_join_and_aggregate_is_not_rewritten(tc):
    """GlobalLimitExec(skip > 0) between the join and the aggregate moves the rows but not the join's pair list: the aggregate must not
    take the join's word for its input.  Expected: the limit's own output rows, grouped on the host."""
    bt = build_table(21, 3000); pt = probe_table(22, 30_000, bt)
    L, R = g.MemoryExec([bt]), g.MemoryExec([pt])
    j = g.HashJoinExec(L, R, [(col("bk", L.schema()), col("pk", R.schema()))], None, "Inner", "CollectLeft", False)
    js = j.schema()
    lim = g.GlobalLimitExec(j, skip=1234, fetch=15_000)
    rows = native_rows(g.NativePlan(g.ProjectionExec([(col(n, js), n) for n in ("pk", "bd", "bp", "pv", "pd")], lim), tc))
    assert len(rows) == 15_000
    groups = {}
    for pk, bd, bp, pv, pd_ in rows:
        s, c, mn, mx = groups.get((pk, bd, bp), (0, 0, pv, pd_))
        groups[(pk, bd, bp)] = (s + pv, c + 1, min(mn, pv), max(mx, pd_))
    exp = norm([k + v for k, v in groups.items()])
    plan = g.AggregateExec("Single", [(col(n, js), n) for n in ("pk", "bd", "bp")], AGGS(js), lim)
    check(tc, plan, exp, False, runs=2)
    # ... and without the offset the same plan shape is rewritten and agrees with the oracle
    plan0, exp0 = join_agg(bt, pt, [("bk", "pk")], ["pk", "bd", "bp"])
    check(tc, plan0, exp0, True)
