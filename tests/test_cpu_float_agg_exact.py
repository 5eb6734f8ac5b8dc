"""CPU: the bounds of tests/float_agg_exact.py have teeth without a device.  For every data family and every group of it
  - the oracle's Welford recurrence over the table's own row order stays within the tolerance max(F, 16 W);
  - sequential f64 power sums about an origin taken from the data (the first row, the smallest, the largest, the middle one --
    what csrc/agg_compile.cpp accumulates, Moments) stay within F ALONE, in the table's order and in a shuffled one;
  - power sums about 0 (what the aggregate compile accumulated before) miss the tolerance by a factor of 1000 and more on the
    ill-conditioned families, in their group of 5000 rows.
The aggregate compile's side is pinned too: the moment aggregates read their origins from immediate slots no literal shares, the
program the origins are picked with holds the predicate and the raw arguments, and no other function's programs know of either."""
from fractions import Fraction

import numpy as np
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit

import float_agg_exact as X

FAMILY_NAMES = sorted(X.FAMILIES)


def _errors(st, got):
    """|got - exact| of (m2_x, m2_y, algo, mean_x, mean_y); the pair's entries None for a one-argument group"""
    e = [abs(Fraction(got[0]) - st.m2_x), None, None, abs(Fraction(got[3]) - st.mean_x), None]
    if st.ys is not None:
        e[1] = abs(Fraction(got[1]) - st.m2_y); e[2] = abs(Fraction(got[2]) - st.c_xy); e[4] = abs(Fraction(got[4]) - st.mean_y)
    return e


def _bounds(tol, f_alone):
    pair = tol.st.ys is not None
    if f_alone:
        return [tol.f_x, tol.f_y if pair else None, tol.f_c if pair else None, tol.mean_x, tol.mean_y if pair else None]
    return [tol.m2_x, tol.m2_y if pair else None, tol.c_xy if pair else None, tol.mean_x, tol.mean_y if pair else None]


def _groups(name, nulls):
    ref = X.reference(name, 0, nulls)
    for which in ("x", "xy"):
        for key, (st, tol) in sorted(ref[which].items()):
            yield which, key, st, tol


@pytest.mark.parametrize("nulls", [0.0, 0.2])
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_welford_in_table_order_is_within_the_tolerance(name, nulls):
    for which, key, st, tol in _groups(name, nulls):
        for err, bound, what in zip(_errors(st, X.welford(st.xs, st.ys)), _bounds(tol, False), ("m2_x", "m2_y", "algo")):
            if err is not None:
                assert err <= bound, (name, which, key, st.n, what, float(err), float(bound))


@pytest.mark.parametrize("nulls", [0.0, 0.2])
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_power_sums_about_a_data_value_are_within_f_alone(name, nulls):
    """The origin the device picks is the first row of the OPERATOR that takes part, not of the group: every origin tried here is a value
    of the whole table."""
    ref = X.reference(name, 0, nulls)
    allx = sorted(v for st, _ in ref["x"].values() for v in st.xs)
    ally = sorted(v for st, _ in ref["xy"].values() for v in st.ys)
    t = X.family(name, 0, nulls)
    first_x = next(v for v in X.f64_column(t, "x") if v is not None)
    origins = [(first_x, ally[0]), (allx[0], ally[-1]), (allx[-1], ally[len(ally) // 2]), (allx[len(allx) // 2], ally[0])]
    r = np.random.default_rng(7)
    for which, key, st, tol in _groups(name, nulls):
        o = r.permutation(st.n)
        orders = [(st.xs, st.ys), ([st.xs[i] for i in o], [st.ys[i] for i in o] if st.ys is not None else None)]
        for kx, ky in origins:
            for xs, ys in orders:
                got = X.power_sums(xs, ys, kx, ky)
                for err, bound, what in zip(_errors(st, got), _bounds(tol, True), ("m2_x", "m2_y", "algo", "mean_x", "mean_y")):
                    if err is not None:
                        assert err <= bound, (name, which, key, st.n, what, kx, ky, float(err), float(bound))


@pytest.mark.parametrize("name", X.ILL_CONDITIONED)
def test_raw_power_sums_miss_the_tolerance_by_1000x(name):
    ref = X.reference(name, 0, 0.0)
    for which, what in (("x", 0), ("xy", 2)):
        st, tol = ref[which][(len(X.SIZES) - 1,)]
        assert st.n == 5000
        err = _errors(st, X.power_sums(st.xs, st.ys, 0.0, 0.0))[what]
        bound = _bounds(tol, False)[what]
        assert err >= 1000 * bound, (name, which, float(err), float(bound), float(err / bound))
        shifted = _errors(st, X.power_sums(st.xs, st.ys, st.xs[0], st.ys[0] if st.ys is not None else 0.0))[what]
        assert shifted <= bound, (name, which, float(shifted), float(bound))


def test_values_and_statuses_of_the_exact_reference():
    st = X.Stats([1.0, 2.0, 4.0], [2.0, 4.0, 8.0])
    v = st.values()
    assert v["SUM"] == 7 and v["AVG"] == Fraction(7, 3) and v["VAR_POP"] == Fraction(14, 9) and v["VARIANCE"] == Fraction(7, 3)
    assert v["COVAR_POP"] == Fraction(28, 9) and v["COVAR"] == Fraction(14, 3)
    assert abs(v["CORR"] - 1) < Fraction(1, 10 ** 70) and abs(v["STDDEV"] ** 2 - v["VARIANCE"]) < Fraction(1, 10 ** 70)
    one = X.Stats([5.0], [5.0]).values()
    assert one["VARIANCE"] is None and one["STDDEV"] is None and one["COVAR"] is None and one["VAR_POP"] == 0 and one["CORR"] == 0
    none = X.Stats([], []).values()
    assert all(x is None for x in none.values())
    assert X.Stats([3.0, 3.0], [1.0, 2.0]).values()["CORR"] == 0      # a zero variance: 0, as the oracle says


# ------------------------------------------------------------------------------------ the aggregate compile
FIELDS = [{"name": "g", "type": "Int64", "nullable": False}, {"name": "x", "type": "Float64", "nullable": True},
          {"name": "y", "type": "Float64", "nullable": True}, {"name": "p", "type": "Int32", "nullable": False}]


def _desc(aggs, mode="Single", pred=False, fields=FIELDS):
    d = {"op": "aggregate", "mode": mode, "input": {"fields": fields}, "group_expr": [{"expr": col("g", fields), "name": "g"}], "aggr_expr": aggs}
    if pred:
        d["predicate"] = binary(col("p", fields), Op.Lt, lit(7, "Int32"))
    return d


def _imm_reads(prog):
    return [int(i.split("#")[1]) for i in prog["insns"] if i.startswith("IMM ")]


def test_origins_have_immediate_slots_of_their_own_and_a_pick_program():
    aggs = [{"fn": "VARIANCE", "expr": col("x", FIELDS), "name": "v"}, {"fn": "CORR", "expr": col("x", FIELDS), "expr2": col("y", FIELDS), "name": "c"},
            {"fn": "SUM", "expr": binary(col("x", FIELDS), Op.Plus, lit(0.0)), "name": "s"}]      # (a literal 0.0: the value a parameter slot is uploaded with)
    d = g.compile_check(_desc(aggs, pred=True))
    # VARIANCE(x) reads x where x is valid, CORR(x, y) where both are: two arguments of their own, then y
    assert [k for k, _ in d["origin_imm"]] == [0, 1, 2]
    slots = [slot for _, slot in d["origin_imm"]]
    assert len(set(slots)) == 3
    reads = _imm_reads(d["program"])
    assert all(reads.count(s) == 1 for s in slots)                       # ... each read by the one instruction of its parameter
    assert len(reads) > len(slots)                                       # ... and the literals (0.0, 7) read other slots
    # the pick program: the predicate, the three arguments, and no parameter of its own (it does not even hold a subtraction)
    assert d["pick"]["pred_reg"] >= 0 and len(d["pick"]["out_reg"]) == 3 and set(d["pick"]["columns"]) == {"x", "y", "p"}
    assert not any(i.startswith("FSUB ") for i in d["pick"]["insns"]) and sum(i.startswith("FSUB ") for i in d["program"]["insns"]) == 3


def test_a_final_picks_its_origins_from_the_state_means():
    aggs = [{"fn": "STDDEV", "expr": col("x", FIELDS), "name": "sd"}]
    partial = g.compile_check(_desc(aggs, "Partial"))
    assert [o["name"] for o in partial["outputs"]] == ["g", "sd[count]", "sd[mean]", "sd[m2]"]
    assert [o["type"] for o in partial["outputs"]] == ["Int64", "UInt64", "Float64", "Float64"]
    fields = [{"name": o["name"], "type": o["type"], "nullable": bool(o["nullable"])} for o in partial["outputs"]]
    final = g.compile_check(_desc([{"fn": "STDDEV", "name": "sd"}], "FinalPartitioned", fields=fields))
    assert set(final["pick"]["columns"]) == {"sd[count]", "sd[mean]"} and len(final["origin_imm"]) == 1


@pytest.mark.parametrize("fn", ["SUM", "AVG", "MIN", "MAX", "COUNT"])
def test_other_functions_have_no_origin(fn):
    d = g.compile_check(_desc([{"fn": fn, "expr": col("x", FIELDS), "name": "a"}], pred=True))
    assert "pick" not in d and "origin_imm" not in d
