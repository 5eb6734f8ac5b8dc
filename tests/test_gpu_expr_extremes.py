"""Expression arithmetic at its magnitude bounds against exact integers (tests/expr_exact.py; the tables and expression lists are in
tests/expr_extreme_cases.py and are checked against their own conditions on the CPU by test_cpu_expr_exact.py).

Every expression runs through three consumers -- a ProjectionExec (the value is stored), a FilterExec (the expression is an intermediate
of the predicate; the surviving row ids are compared) and an ungrouped and a grouped SUM / COUNT (the fused-argument path) -- under both
evaluators (the interpreter, set_jit("off"), and the generated code, set_jit("force")), each plan twice so that the deferred replay
runs too.  Integers, decimals, booleans, strings and validity are compared exactly, Float64 bit for bit (NaN matches NaN): every
float here is one conversion, or one conversion and one division, of an exact integer, and the reference does the same IEEE operations.
Where the reference says OVERFLOW the execution has to raise; those plans are separate, so that they cannot hide an exact row.

What the bounds decide on the device (|value| < 2^bits from the declared types): 64- or 128-bit arithmetic in generated code, OP_MULW
or OP_MUL, whether a Decimal128 column is read from its low 8 bytes only.  What this file found, by the case that shows it:
  test_decimal_overflow_raises[*]                        a rescale / product / sum beyond 127 bits or 38 digits returned a wrapped value, status 0
  test_projection[*-dec:1] (mul_f64), [*-dec38:6] (a_f64)  i128 -> f64 through two halves rounded twice (2^64 * h + 2^63 + 2^11 + 1)
  test_filter[*-int:Int32] (mul_gt_b), test_aggregate[*-int:Int32-*] (add)
                                                         an integer node held the unwrapped value as an intermediate
  test_projection[*-int:UInt64] (div)                    a UInt64 of 2^63 or more was read as a negative number
  test_projection[force-int:Int8], [force-int:Int16]     the generated code did not compile for Int8 / Int16 columns (no int8_t under hiprtc)
  test_substr[*-prefix-3-len1]                           a two-byte character in the skipped prefix: substr('éabc', 3, 1) gave 'a', no flag

Documented refusals (the only ones a case may meet; each is matched by its message):
  "longer than 15 bytes reached"       a string result beyond 15 bytes, or a substr that cannot count bytes for characters (non-ASCII)
  "MIN/MAX over a value outside"       MIN / MAX over values outside the int64 range (FLAG_WIDE_MINMAX), under every strategy
  (ILIKE is refused when the plan is built; no expression here uses it)
"""
import decimal

import pyarrow as pa
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit, substr

import expr_exact as X
import expr_extreme_cases as K

pytestmark = pytest.mark.gpu
PACKED15 = "longer than 15 bytes reached"
WIDE_MINMAX = "MIN/MAX over a value outside the int64 range"
_CTX = decimal.Context(prec=80)
_PA = {"Int8": pa.int8(), "Int16": pa.int16(), "Int32": pa.int32(), "Int64": pa.int64(), "UInt8": pa.uint8(), "UInt16": pa.uint16(), "UInt32": pa.uint32(),
       "UInt64": pa.uint64(), "Float64": pa.float64(), "Utf8": pa.string(), "Date32": pa.date32(), "Boolean": pa.bool_()}


@pytest.fixture(params=["off", "force"])
def ev(tc, request):
    """The TaskContext with one evaluator pinned: the interpreter, or the generated (hiprtc) code for every sink."""
    if request.param == "force" and not tc.ctx.jit_stats()["available"]:
        pytest.skip("hiprtc not available")
    tc.ctx.set_jit(request.param)
    before = tc.ctx.jit_stats()["launches"]
    yield tc
    tc.ctx.set_jit("auto")
    assert (tc.ctx.jit_stats()["launches"] > before) == (request.param == "force")


def pa_type(t):
    return pa.decimal128(*t["Decimal128"]) if X.is_dec(t) else _PA[t]


def values(column, t):
    """A result column as the reference writes values: unscaled ints for decimals, days for dates, the bit pattern for floats."""
    v = column.combine_chunks() if isinstance(column, pa.ChunkedArray) else column
    assert v.type == pa_type(t), (v.type, t)
    if X.is_dec(t):
        return [None if x is None else int(x.scaleb(t["Decimal128"][1], context=_CTX)) for x in v.to_pylist()]
    if t == "Date32":
        return v.cast(pa.int32()).to_pylist()
    if t == "Float64":
        return [fkey(x) for x in v.to_pylist()]
    return v.to_pylist()


def fkey(x):
    return None if x is None else ("nan" if x != x else X.f64_bits(x))


def expected(t, vals):
    assert not any(v is X.OVERFLOW for v in vals)
    return [fkey(v) for v in vals] if t == "Float64" else list(vals)


def run(tc, plan):
    p = g.NativePlan(plan, tc)
    first = p.execute(0).to_arrow()
    again = p.execute(0).to_arrow()          # deferred from the second execution on
    return first, again


_SRC = {}


def source(t):
    if t.name not in _SRC:
        _SRC[t.name] = g.MemoryExec([t.arrow()])
    return _SRC[t.name]


def predicate_over(e, t):
    """The expression as an intermediate of a predicate: itself when Boolean, else compared with a literal of its own kind."""
    if t == "Boolean":
        return e
    if t == "Float64":
        return binary(e, Op.Gt, lit(0.5))
    if t == "Utf8":
        return binary(e, Op.GtEq, lit("b"))
    if X.is_dec(t):
        return binary(e, Op.Gt, lit(5, ("Decimal128", 1, 0)))
    return binary(e, Op.Gt, lit(1, t))


def predicate_rows(e, t, schema, cols):
    pt, pv = X.evaluate(predicate_over(e, t), schema, cols)
    assert pt == "Boolean" and not any(v is X.OVERFLOW for v in pv)
    return [i for i, v in enumerate(pv) if v is True]


def chunks(xs, k):
    return [xs[i:i + k] for i in range(0, len(xs), k)]


# ------------------------------------------------------------------------------------------------ the three consumers
@pytest.mark.parametrize("name", K.TABLES)
def test_projection(ev, name):
    t, exprs = K.table_and_exprs(name)
    ref = K.reference(name)
    src = source(t)
    for part in chunks(exprs, 4):
        for out in run(ev, g.ProjectionExec([(e, n) for n, e in part] + [(col("id", t.schema), "id")], src)):
            assert out["id"].to_pylist() == t.cols["id"]
            for n, _ in part:
                rt, rv = ref[n]
                assert values(out[n], rt) == expected(rt, rv), (name, n)


@pytest.mark.parametrize("name", K.TABLES)
def test_filter(ev, name):
    t, exprs = K.table_and_exprs(name)
    ref = K.reference(name)
    src = source(t)
    dropped = 0
    for n, e in exprs:
        want = predicate_rows(e, ref[n][0], t.schema, t.cols)
        for out in run(ev, g.FilterExec(predicate_over(e, ref[n][0]), src)):
            assert out["id"].to_pylist() == want, (name, n)
        dropped += sum(v is X.OVERFLOW for v in ref[n][1])
    assert dropped == 0


def sum_type(t):
    """SUM's declared type (DataFusion: Decimal(min(38, p + 10), s), Int64 / UInt64 for integers), or None where the type has no exact
    SUM (Float64 sums depend on the order of the adds; Boolean, Utf8, Date32)."""
    if X.is_dec(t):
        p, s = t["Decimal128"]
        return {"Decimal128": [min(38, p + 10), s]}
    if X.is_int(t):
        return "Int64" if X._INT[t][1] else "UInt64"
    return None


def aggregate_rows(rt, rv, groups):
    """({group: (exact SUM or None, COUNT)}, whether SUM is asked for).  Integer sums wrap at 64 bits.  A decimal SUM is asked for
    wherever every group's exact total fits the declared SUM type (a value condition, worked out here on the CPU: a total beyond it is an
    overflow of SUM itself, which arrow wraps and nothing defines)."""
    st = sum_type(rt)
    out, fits = {}, st is not None
    for k in sorted(set(groups)):
        vs = [v for v, gk in zip(rv, groups) if gk == k and v is not None]
        total = None
        if st is not None and vs:
            total = sum(vs)
            if X.is_int(st):
                total = X.wrap(total, st)
            elif abs(total) >= 10 ** st["Decimal128"][0]:
                fits = False
        out[k] = (total, len(vs))
    return out, fits


@pytest.mark.parametrize("grouped", [False, True], ids=["ungrouped", "grouped"])
@pytest.mark.parametrize("name", K.TABLES)
def test_aggregate(ev, name, grouped):
    t, exprs = K.table_and_exprs(name)
    ref = K.reference(name)
    src = source(t)
    groups = t.cols["g"] if grouped else [0] * t.n
    want = {n: aggregate_rows(ref[n][0], ref[n][1], groups) for n, _ in exprs}
    if name.startswith("dec:") and not grouped:
        assert want["mul"][1] and want["add"][1]          # the SUM of the wide products is compared by value
    for part in chunks(exprs, 3):
        aggs = []
        for n, e in part:
            if want[n][1]:
                aggs.append({"fn": "SUM", "expr": e, "name": "s_" + n})
            aggs.append({"fn": "COUNT", "expr": e, "name": "c_" + n})
        plan = g.AggregateExec("Single", [(col("g", t.schema), "g")] if grouped else [], aggs, src)
        for out in run(ev, plan):
            keys = out["g"].to_pylist() if grouped else [0]
            assert sorted(keys) == sorted(set(groups))
            for n, _ in part:
                rows, with_sum = want[n]
                counts = dict(zip(keys, out["c_" + n].to_pylist()))
                assert out["c_" + n].type == pa.int64() and counts == {k: c for k, (_, c) in rows.items()}, (name, n)
                if with_sum:
                    sums = dict(zip(keys, values(out["s_" + n], sum_type(ref[n][0]))))
                    assert sums == {k: s for k, (s, _) in rows.items()}, (name, n)


# ------------------------------------------------------------------------------------------------ OVERFLOW has to raise
@pytest.mark.parametrize("consumer", ["projection", "filter", "aggregate"])
@pytest.mark.parametrize("case", [n for n, _, _ in K.overflow_cases()])
def test_decimal_overflow_raises(ev, case, consumer):
    """Every non-NULL row of these plans is OVERFLOW in the reference (arrow-arith raises): the device must raise, never answer."""
    t, e = {n: (t, e) for n, t, e in K.overflow_cases()}[case]
    rt, rv = X.evaluate(e, t.schema, t.cols)
    assert all(v is X.OVERFLOW or v is None for v in rv) and sum(v is X.OVERFLOW for v in rv) >= t.n - 2
    src = source(t)
    if consumer == "projection":
        plan = g.ProjectionExec([(e, "x"), (col("id", t.schema), "id")], src)
    elif consumer == "filter":
        plan = g.FilterExec(predicate_over(e, rt), src)
    else:
        plan = g.AggregateExec("Single", [(col("g", t.schema), "g")], [{"fn": "COUNT", "expr": e, "name": "c"}], src)
    p = g.NativePlan(plan, ev)
    for _ in range(2):
        with pytest.raises(g.GpuqError, match="overflow"):
            p.execute(0).to_arrow()


def test_bounds_beyond_127_bits_with_small_values_still_run(ev):
    """The bound comes from the declared types; the check is on the values: q14's Decimal(38,6) / Decimal(38,4) over small numbers."""
    n = 131
    a = [(i - 60) * 10**6 + 1 for i in range(n)]
    b = [((i % 9) - 4) * 10**4 for i in range(n)]
    a[7] = None
    cols = {"id": list(range(n)), "g": [i % 7 for i in range(n)], "a": a, "b": b, "f": [None] * n}
    t = K.Table("small38", [("id", "Int32"), ("g", "Int32"), ("a", K.D(38, 6)), ("b", K.D(38, 4)), ("f", "Float64")], cols)
    s = t.schema
    exprs = [("div", binary(col("a", s), Op.Divide, col("b", s))), ("mul", binary(col("a", s), Op.Multiply, col("b", s))), ("lt", binary(col("a", s), Op.Lt, col("b", s)))]
    for out in run(ev, g.ProjectionExec([(e, nm) for nm, e in exprs], source(t))):
        for nm, e in exprs:
            rt, rv = X.evaluate(e, s, cols)
            assert values(out[nm], rt) == expected(rt, rv), nm


# ------------------------------------------------------------------------------------------------ aggregates at the bounds
def _agg_table(name, ty, vals):
    n = len(vals)
    cols = {"id": list(range(n)), "g": [i % 7 for i in range(n)], "a": vals, "b": vals, "f": [None] * n}
    return K.Table(name, [("id", "Int32"), ("g", "Int32"), ("a", ty), ("b", ty), ("f", "Float64")], cols)


STRATEGIES = ["tiny", "lds", "hash", "radix", "auto"]


def strategy_args(strategy, groups):
    """AggregateExec keywords that force one strategy; the radix path is sized by the expected number of groups."""
    return {"strategy": strategy, "expected_groups": groups} if strategy == "radix" else {"strategy": strategy}


@pytest.mark.parametrize("grouped,strategy", [(False, "auto")] + [(True, s) for s in STRATEGIES], ids=lambda v: v if isinstance(v, str) else ("grouped" if v else "ungrouped"))
def test_sum_beyond_64_bits_and_of_mixed_sign_extremes(ev, grouped, strategy):
    """The carry across 2^64 and the mixed-sign 128-bit sums through every strategy's fold and combine (7 groups x 2 accumulators fit the
    tiny path; an aggregate without keys has one strategy)."""
    near = [10**18 - 1 - i for i in range(190)] + [None, -(10**18 - 1), 10**17]               # total ~ 1.9e20 > 2^64; per group > 2^64 too
    assert sum(v for v in near if v is not None) > 2**64 * 7
    mixed38 = ([10**38 - 1, -(10**38 - 1), 2**64 + K.PATTERN, -(2**64) - 1, 2**126, -(2**126) + 5, None, 1] * 7 * 3 + [10**37, -3])      # period 8: every group meets every value
    mixed64 = [-2**63, 2**63 - 1, 2**63 - 1, -2**63, -1, 2**62, 2**62, 2**62, None] * 7 * 3 + [5, -2**63]
    for name, ty, vals in (("sum18", K.D(18, 0), near), ("sum38", K.D(38, 0), mixed38), ("sum64", "Int64", mixed64)):
        t = _agg_table(name, ty, vals)
        rt = X._type(ty)
        st = {"Decimal128": [min(38, rt["Decimal128"][0] + 10), 0]} if X.is_dec(rt) else "Int64"
        groups = t.cols["g"] if grouped else [0] * t.n
        want = {}
        for k in set(groups):
            vs = [v for v, gk in zip(t.cols["a"], groups) if gk == k and v is not None]
            want[k] = X.wrap(sum(vs), "Int64") if st == "Int64" else sum(vs)
            assert st == "Int64" or abs(want[k]) < 10**38
        aggs = [{"fn": "SUM", "expr": col("a", t.schema), "name": "s"}, {"fn": "COUNT", "expr": col("a", t.schema), "name": "c"}]
        for out in run(ev, g.AggregateExec("Single", [(col("g", t.schema), "g")] if grouped else [], aggs, source(t), **strategy_args(strategy, 7))):
            keys = out["g"].to_pylist() if grouped else [0]
            assert dict(zip(keys, values(out["s"], st))) == want, name


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("order", ["clustered", "shuffled"])
def test_float_accumulators_under_every_strategy(ev, order, strategy):
    """Every accumulator kind over K.float_acc_table under every strategy, bit for bit: MIN / MAX of Float64 specials by the IEEE total
    order (zeros of both signs, infinities, the subnormal, +-max, NaN, an all-NULL group), a float SUM whose every partial sum is exact,
    MIN / MAX / COUNT of Int64 at its bounds, COUNT(*).  Clustered keys run through the wave scan of the hash kernel with runs that start,
    end and span the 64-lane boundary; shuffled keys make every row its own run.  Three plans of three device accumulators each."""
    t = K.float_acc_table(order)
    want = K.float_acc_reference(t)
    s = t.schema
    plans = [[("MIN", "fx", "min_fx", "Float64"), ("MAX", "fx", "max_fx", "Float64")],
             [("SUM", "fs", "sum_fs", "Float64"), ("COUNT", "fs", "cnt_fs", "Int64"), ("COUNT", None, "cnt_all", "Int64")],
             [("MIN", "i", "min_i", "Int64"), ("MAX", "i", "max_i", "Int64"), ("COUNT", "i", "cnt_i", "Int64")]]
    for accs in plans:
        aggs = [{"fn": fn, "expr": lit(1) if c is None else col(c, s), "name": n} for fn, c, n, _ in accs]
        for out in run(ev, g.AggregateExec("Single", [(col("g", s), "g")], aggs, source(t), **strategy_args(strategy, len(want)))):
            keys = out["g"].to_pylist()
            assert sorted(keys) == sorted(want)
            for _, _, n, ty in accs:
                assert dict(zip(keys, values(out[n], ty))) == {k: (fkey(r[n]) if ty == "Float64" else r[n]) for k, r in want.items()}, (n, strategy, order)


@pytest.mark.parametrize("strategy", ["tiny", "lds", "hash", "radix", "auto"])
@pytest.mark.parametrize("fn", ["MIN", "MAX"])
def test_min_max_outside_int64_is_refused_under_every_strategy(ev, fn, strategy):
    vals = [1, -1, 2**63, -(2**63) - 1, 2**64 + 1, None, 10**19, 5] * 19 + [0] * 7
    t = _agg_table("wide_minmax", K.D(20, 0), vals)
    plan = g.AggregateExec("Single", [(col("g", t.schema), "g")], [{"fn": fn, "expr": col("a", t.schema), "name": "m"}], source(t), strategy=strategy)
    p = g.NativePlan(plan, ev)
    for _ in range(2):
        with pytest.raises(g.GpuqError, match=WIDE_MINMAX) as ei:
            p.execute(0).to_arrow()
        assert ei.value.status == 3          # Unsupported


# ------------------------------------------------------------------------------------------------ substr counts characters
@pytest.mark.parametrize("length", [0, 1, None], ids=["len0", "len1", "rest"])
@pytest.mark.parametrize("start", [1, 2, 3])
@pytest.mark.parametrize("table", [n for n, _ in K.utf8_tables()])
def test_substr(ev, table, start, length):
    """substr(s, start [, length]) as a value, inside a predicate and as an aggregate argument.  The device counts bytes: it is exact when
    every character up to the end of the kept part is ASCII and that end lies inside the 15 packed bytes; otherwise it has to refuse
    (the documented PACKED15 refusal), in particular for a multi-byte character in the SKIPPED prefix: substr('éabc', 3, 1) is 'b'."""
    vals = dict(K.utf8_tables())[table]
    n = len(vals)
    schema = [{"name": "id", "type": "Int32", "nullable": False}, {"name": "s", "type": "Utf8", "nullable": True}]
    cols = {"id": list(range(n)), "s": vals}
    key = "utf8:" + table
    if key not in _SRC:
        _SRC[key] = g.MemoryExec([pa.table({"id": pa.array(cols["id"], pa.int32()), "s": pa.array(vals, pa.string())})])
    src = _SRC[key]
    e = substr(col("s", schema), start, length)
    rt, rv = X.evaluate(e, schema, cols)
    plans = [g.ProjectionExec([(e, "x"), (col("id", schema), "id")], src), g.FilterExec(predicate_over(e, "Utf8"), src),
             g.AggregateExec("Single", [], [{"fn": "COUNT", "expr": e, "name": "c"}], src)]
    if not K.substr_is_exact(vals, start, length):
        for plan in plans:
            p = g.NativePlan(plan, ev)
            for _ in range(2):
                with pytest.raises(g.GpuqError, match=PACKED15):
                    p.execute(0).to_arrow()
        return
    for out in run(ev, plans[0]):
        assert values(out["x"], "Utf8") == rv and out["id"].to_pylist() == cols["id"]
    for out in run(ev, plans[1]):
        assert out["id"].to_pylist() == predicate_rows(e, "Utf8", schema, cols)
    for out in run(ev, plans[2]):
        assert out["c"].to_pylist() == [sum(v is not None for v in rv)]
