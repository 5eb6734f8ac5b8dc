"""The float aggregates on the device against exact rationals (tests/float_agg_exact.py: the references, the bounds and why they are
what they are, the data families).  VARIANCE / VAR_POP / STDDEV / STDDEV_POP / SUM / AVG over x and COVAR / COVAR_POP / CORR over
(x, y) run over every family -- data far from zero, where sums of x itself lose the variance in the subtraction Sxx - Sx^2/n -- by
every strategy, grouped and ungrouped, with and without NULLs, with a predicate fused into the aggregate, through the Python mirror of
the executor and through NativePlan (executed twice: the second execution is the deferred replay), and as Partial ->
FinalPartitioned over three partitions whose state columns are themselves checked against the exact per-partition values.

strategy="runs" is asked for the way tests/test_gpu_agg_runs.py reaches that path (an Int32 key, rows clustered on it): a float sum is
not among the accumulators the path folds, so the operator answers by the table, and the answer is held to the same bounds.  The way
every native execution took is asserted (`agg_path`, AGG_PATH below): a strategy that quietly fell to another would otherwise pass.

Run once against the library of the commit before the origins (power sums of x itself): 16 cases passed -- every f64_n1e3 case and the
Single cases of group_offsets, whose bound is loose -- and every m2 / VAR / STDDEV / COVAR / CORR comparison of the other families
failed, the SUM / AVG comparisons before them passing: VARIANCE over the 5000-row group of f64_1e9 came out as 629.27 for an exact
0.98525, of f64_1e6 as 5.6e-3 for 8.5e-6, of ts_us as 0.0 for 8.29e10 (profiles/r14_moment_origins.json)."""
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit
from oracle import oracle_np as O

import float_agg_exact as X
from test_gpu_agg_by_build_row import native_rows
from test_gpu_operators import dev_rows, norm, ora_rows

pytestmark = pytest.mark.gpu

FAMILY_NAMES = sorted(X.FAMILIES)
STRATEGIES = ["tiny", "hash", "lds", "radix", "auto", "runs"]
ONE = ["VARIANCE", "VAR_POP", "STDDEV", "STDDEV_POP", "SUM", "AVG"]
TWO = ["COVAR", "COVAR_POP", "CORR"]
PRED_LT = 7      # the fused predicate: p < 7 keeps ~70 % of the rows
# the way a grouped execution of 7198 rows takes, as NativePlan.profile_all reports it: "lds" is the global table filled through the
# blocks' LDS tables, "auto" takes the table for an input this small, "runs" does not fold float sums and goes on to the table
AGG_PATH = {"tiny": "tiny", "hash": "table", "lds": "table", "radix": "radix", "auto": "table", "runs": "table"}


def agg_path(p):
    aggs = [o for o in p.profile_all() if o["op"] == "aggregate"]
    assert len(aggs) == 1
    return aggs[0]["agg_path"]


def table_of(name, nulls, strategy):
    t = X.family(name, 0, nulls)
    t = t.append_column(pa.field("g32", pa.int32(), nullable=False), t["g"].cast(pa.int32()))
    if strategy == "runs":      # clustered on the key, the rows of a group in their table order (the reference does not depend on the order)
        t = t.take(pc.sort_indices(t, sort_keys=[("g", "ascending")]))
    return t


def aggs_of(s, fns):
    return [dict({"fn": fn, "expr": col("x", s), "name": fn}, **({"expr2": col("y", s)} if fn in TWO else {})) for fn in fns]


def plan_of(t, fns, strategy, grouped, pred, mode="Single"):
    src = g.MemoryExec([t])
    s = src.schema()
    inp = g.FilterExec(binary(col("p", s), Op.Lt, lit(PRED_LT, "Int32")), src) if pred else src
    groups = [(col("g32", s), "g")] if grouped else []
    return g.AggregateExec(mode, groups, aggs_of(s, fns), inp, strategy=strategy if grouped else "auto", expected_groups=len(X.SIZES) if strategy == "radix" else 0)


def wrap64(v):
    return (int(v) + 2 ** 63) % 2 ** 64 - 2 ** 63


def check_values(rows, ref, grouped, fns, int_sum, what):
    """rows: (group?, one value per function) against the exact values: the same rows, NULL where the exact value is, within the bound elsewhere."""
    nk = 1 if grouped else 0
    got = {tuple(r[:nk]): r[nk:] for r in rows}
    assert sorted(got) == sorted(ref) and len(rows) == len(ref), (what, sorted(got), sorted(ref))
    for key, (st, tol) in ref.items():
        exact = st.values()
        for fn, v in zip(fns, got[key]):
            e = exact[fn]
            if e is None:
                assert v is None, (what, key, fn, st.n, v)
                continue
            assert v is not None, (what, key, fn, st.n)
            if fn == "SUM" and int_sum:
                assert isinstance(v, int) and v == wrap64(e), (what, key, fn, v, int(e))      # an integer SUM is Int64 and exact (it wraps)
                continue
            err, bound = abs(Fraction(v) - e), tol.of(fn)
            print("%s %s %s n=%d: error %.3e, bound %.3e" % (what, key, fn, st.n, float(err), float(bound)))
            assert err <= bound, (what, key, fn, st.n, v, float(e), float(err), float(bound))


def run_single(tc, monkeypatch, name, strategy, nulls, grouped, pred, layers=("mirror", "native")):
    t = table_of(name, nulls, strategy)
    ref = X.reference(name, 0, nulls, PRED_LT if pred else None, grouped)
    int_sum = pa.types.is_integer(t["x"].type)
    for fns, which in ((ONE, "x"), (TWO, "xy")):
        plan = plan_of(t, fns, strategy, grouped, pred)
        what = "%s/%s/nulls=%s/%s%s" % (name, strategy, nulls, "grouped" if grouped else "ungrouped", "/pred" if pred else "")
        if "mirror" in layers:
            with monkeypatch.context() as m:
                m.setenv("GPUQ_PLAN_LAYER", "mirror")
                check_values(dev_rows(tc, plan.execute(0, tc)), ref[which], grouped, fns, int_sum, what + "/mirror")
        if "native" in layers:
            p = g.NativePlan(plan, tc)
            for run in (1, 2):      # the second execution replays the first one's decisions, deferred
                check_values(native_rows(p), ref[which], grouped, fns, int_sum, what + "/native%d" % run)
                assert agg_path(p) == (AGG_PATH[strategy] if grouped else "tiny"), (what, run, agg_path(p))


# 11 families x 6 strategies; per case 2 NULL fractions x 2 operators x (mirror + native twice) over 7198 rows
@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_single_grouped(tc, monkeypatch, name, strategy):
    for nulls in (0.0, 0.2):
        run_single(tc, monkeypatch, name, strategy, nulls, True, False)


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_single_ungrouped(tc, monkeypatch, name):
    for nulls in (0.0, 0.2):
        run_single(tc, monkeypatch, name, "auto", nulls, False, False)
    run_single(tc, monkeypatch, name, "auto", 0.2, False, True, layers=("native",))


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_single_with_a_fused_predicate(tc, monkeypatch, strategy):
    """Once per strategy, over the families in turn: the predicate drops rows whose values must not reach the origin or the sums."""
    for name in (FAMILY_NAMES[STRATEGIES.index(strategy) % len(FAMILY_NAMES)], "ts_us"):
        run_single(tc, monkeypatch, name, strategy, 0.2, True, True)


def test_the_origin_skips_leading_rows_that_do_not_take_part(tc, monkeypatch):
    """The first rows of the table are NULL or fail the predicate and hold huge values under their validity bits: an origin taken from
    one of them (1e300: d^2 overflows) would make every result inf or NaN."""
    base = X.family("f64_1e9", 0, 0.0)
    n, lead = base.num_rows, 300      # more than one step of the pick kernel's walk
    x, p = base["x"].to_numpy().copy(), base["p"].to_numpy().copy()
    y = base["y"].to_numpy().copy()
    x[:lead] = 1e300
    y[:lead] = -1e300
    p[lead // 2:lead] = 9      # the second half of the leading rows is valid and filtered; the first half is NULL
    mask = np.arange(n) < lead // 2
    t = pa.table({"g": base["g"], "x": pa.array(x, mask=mask), "y": pa.array(y, mask=mask), "p": pa.array(p), "g32": base["g"].cast(pa.int32())})
    keep = [i >= lead and p[i] < PRED_LT for i in range(n)]
    gl, xs, ys = t["g"].to_pylist(), x.tolist(), y.tolist()
    part = [i for i in range(n) if keep[i]]
    rx = Fraction(max(xs[i] for i in part)) - Fraction(min(xs[i] for i in part))
    ry = Fraction(max(ys[i] for i in part)) - Fraction(min(ys[i] for i in part))
    for fns, pair in ((ONE, False), (TWO, True)):
        ref = {}
        for k in sorted(set(gl[i] for i in range(n) if p[i] < PRED_LT)):      # (a group whose kept rows are all NULL still has a row)
            idx = [i for i in part if gl[i] == k]
            st = X.Stats([xs[i] for i in idx], [ys[i] for i in idx] if pair else None)
            ref[(k,)] = (st, X.Tolerances(st, rx, ry if pair else None))
        for strategy in ("hash", "tiny"):
            plan = plan_of(t, fns, strategy, True, True)
            check_values(native_rows(g.NativePlan(plan, tc)), ref, True, fns, False, "leading/" + strategy)


@pytest.mark.parametrize("strategy", ["tiny", "hash", "lds"])
def test_the_deferred_replay_reads_nothing_back(tc, strategy):
    """The origins are picked and handed over on the device: from its second execution on the plan is queued without a host read."""
    t = table_of("ts_us", 0.2, strategy)
    p = g.NativePlan(plan_of(t, ONE + ["CORR"], strategy, True, True), tc)
    first = native_rows(p)
    for _ in range(2):
        assert len(native_rows(p)) == len(first) >= len(X.SIZES) - 1      # (the predicate may drop the group of one row)
        st = p.exec_stats()
        assert st["deferred"] and st["settles"] == 1 and st["host_syncs"] == 0 and st["retries"] == 0, st


# ------------------------------------------------------------------------------------ Partial -> FinalPartitioned
STATE_NAMES = {"VARIANCE": ["count", "mean", "m2"], "CORR": ["count", "mean1", "m2_1", "mean2", "m2_2", "algoConst"], "COVAR": ["count", "mean1", "mean2", "algoConst"]}


def check_states(rows, ref, fn, what):
    got = {tuple(r[:1]): r[1:] for r in rows}
    assert sorted(got) == sorted(ref), (what, sorted(got), sorted(ref))
    for key, (st, tol) in ref.items():
        v = got[key]
        assert v[0] == st.n, (what, key, v[0], st.n)
        if fn == "VARIANCE":
            pairs = [(v[1], st.mean_x, tol.mean_x, "mean"), (v[2], st.m2_x, tol.m2_x, "m2")]
        elif fn == "CORR":
            pairs = [(v[1], st.mean_x, tol.mean_x, "mean1"), (v[2], st.m2_x, tol.m2_x, "m2_1"), (v[3], st.mean_y, tol.mean_y, "mean2"),
                     (v[4], st.m2_y, tol.m2_y, "m2_2"), (v[5], st.c_xy, tol.c_xy, "algoConst")]
        else:
            pairs = [(v[1], st.mean_x, tol.mean_x, "mean1"), (v[2], st.mean_y, tol.mean_y, "mean2"), (v[3], st.c_xy, tol.c_xy, "algoConst")]
        for dev, exact, bound, nm in pairs:
            if st.n == 0:
                assert dev == 0.0, (what, key, nm, dev)      # the state columns of an empty group are 0
                continue
            err = abs(Fraction(dev) - exact)
            print("%s %s %s n=%d: error %.3e, bound %.3e" % (what, key, nm, st.n, float(err), float(bound)))
            assert err <= bound, (what, key, nm, st.n, dev, float(exact), float(err), float(bound))


@pytest.mark.parametrize("nulls", [0.0, 0.2])
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_partial_states_and_final_partitioned(tc, name, nulls):
    """Three partitions by the terciles of x.  The Partial's state columns (names and order the reference's) are held to the mean and m2
    bounds against each partition's exact values, the FinalPartitioned over them to the bounds of the whole table: its origin is a state
    mean, and the terms n_i (mean_i - K)^2 it adds are of the data's range like the rows' own."""
    t = X.family(name, 0, nulls)
    t = t.append_column(pa.field("g32", pa.int32(), nullable=False), t["g"].cast(pa.int32()))
    pid = X.partition_of(t)
    parts = [t.take([i for i in range(t.num_rows) if pid[i] == k]) for k in range(3)]
    whole = X.reference(name, 0, nulls)
    src = g.MemoryExec(parts)
    s = src.schema()
    for fn, which, finals in (("VARIANCE", "x", ["VARIANCE", "VAR_POP", "STDDEV", "STDDEV_POP"]), ("CORR", "xy", ["CORR"]), ("COVAR", "xy", ["COVAR", "COVAR_POP"])):
        what = "%s/nulls=%s/%s" % (name, nulls, fn)
        partial = g.AggregateExec("Partial", [(col("g32", s), "g")], aggs_of(s, [fn]), src)
        states = [g.plan.materialize(tc, partial.execute(k, tc)).to_arrow(tc.ctx) for k in range(3)]
        for k in range(3):
            assert states[k].schema.names == ["g"] + ["%s[%s]" % (fn, nm) for nm in STATE_NAMES[fn]], states[k].schema.names
            assert [str(f.type) for f in states[k].schema][1:] == ["uint64"] + ["double"] * (len(STATE_NAMES[fn]) - 1)
            check_states([tuple(r.values()) for r in states[k].to_pylist()], X.reference(name, 0, nulls, None, True, k)[which], fn, what + "/partition%d" % k)
        merged = g.MemoryExec([pa.concat_tables(states)])
        fs = merged.schema()
        for ffn in finals:      # every function of a layout reads the same states
            final = g.AggregateExec("FinalPartitioned", [(col("g", fs), "g")], [{"fn": ffn, "name": ffn}], merged)
            p = g.NativePlan(final, tc)
            for run in (1, 2):
                check_values(native_rows(p), whole[which], True, [ffn], False, what + "/final%d/%s" % (run, ffn))


# ------------------------------------------------------------------------------------ NULL and non-NULL status
@pytest.mark.parametrize("strategy", ["tiny", "hash", "lds", "auto"])
def test_null_status_equals_the_oracle(tc, strategy):
    """n = 0 (a group of NULLs), n = 1 (the sample forms are NULL, the population forms 0), CORR over a zero variance (0, not NULL and
    not NaN), far from zero; grouped and ungrouped over no rows at all."""
    b = 2.0 ** 30 + 0.5      # (every value and every intermediate of the grouped cases is exact in f64, by Welford and by power sums alike)
    t = pa.table({"g": pa.array([1, 2, 2, 3, 3, 3, 4, 4], pa.int32()), "x": pa.array([b, None, None, b, b, b, b, b + 1], pa.float64()),
                  "y": pa.array([b, 1.0, None, b + 1, b + 2, b + 4, None, 2.0], pa.float64())})
    fns = ["VARIANCE", "VAR_POP", "STDDEV", "STDDEV_POP", "COVAR", "COVAR_POP", "CORR"]
    for tab in (t, t.slice(0, 0)):
        src = g.MemoryExec([tab])
        s = src.schema()
        for groups in ([(col("g", s), "g")], []):
            aggs = aggs_of(s, fns)
            exp = norm(ora_rows(O.aggregate(O.Table.from_arrow(tab), groups, aggs, "Single")))
            got = norm(dev_rows(tc, g.AggregateExec("Single", groups, aggs, src, strategy=strategy if groups else "auto").execute(0, tc)))
            assert [[v is None for v in r] for r in got] == [[v is None for v in r] for r in exp], (got, exp)
            if groups:
                assert got == exp, (got, exp)      # 0, 1/2, 1, sqrt(1/2), ...
    if strategy == "hash":
        assert exp == [(None,) * 7]      # ungrouped over no rows: one row of NULLs
