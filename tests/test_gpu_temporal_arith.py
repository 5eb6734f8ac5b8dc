"""Interval and Duration arithmetic on the device: `date / timestamp +- interval`, `timestamp - timestamp`, `timestamp +- duration`
through ProjectionExec, as FilterExec predicates, as group key and MIN / MAX argument, a Duration as sort key and as a column in
and out; in the interpreter and, for the 4097-row case, in the run-time compiled evaluator.

Expected values are the restatement's (tests/temporal_exact.py: datetime.date, dateutil and Python ints), exactly; `timestamp - timestamp`
and `timestamp +- duration` are compared with pyarrow.compute as well.

Rows: 0, 1, 63, 64, 65 (the wave boundaries) and 4097 (one block tail).  Every column exists required and with ~20 % NULLs.  The
dates are the month ends of 2023, 2024, 1900, 2000 and 2100, and 0101-01-01 / 9899-12-31 (the ends of what datetime.date holds, moved
in by the largest shift, 1200 months); the Nanosecond column keeps to the years an int64 of nanoseconds reaches.  Every timestamp has
a non-zero time of day, so the instants before 1970 have a negative count that is not a whole number of days."""
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd import expr as E
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_exact as X      # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 4097]
UNITS = X.UNITS
PA_UNIT = {"Second": "s", "Millisecond": "ms", "Microsecond": "us", "Nanosecond": "ns"}
COLUMNS = ["d"] + ["ts_" + PA_UNIT[u] for u in UNITS]
UNIT_OF = {"ts_" + PA_UNIT[u]: u for u in UNITS}

MONTHS = [-25, -12, -1, 0, 1, 11, 12, 13, 1200]
INTERVALS = [("ym%d" % k, E.interval_year_month(k), X.year_month(k)) for k in MONTHS] + [
    ("dt+1d", E.interval_day_time(1, 0), X.day_time(1, 0)), ("dt-1d", E.interval_day_time(-1, 0), X.day_time(-1, 0)),
    ("dt+1500", E.interval_day_time(0, 1500), X.day_time(0, 1500)), ("dt-1500", E.interval_day_time(0, -1500), X.day_time(0, -1500)),
    ("dt1day_ms", E.interval_day_time(0, 86400000), X.day_time(0, 86400000)),
    ("mdn", E.interval_month_day_nano(-13, 3, -90000000001501), X.month_day_nano(-13, 3, -90000000001501)),
    ("null", E.interval_year_month(None), None)]
# the run-time compiled evaluator: one projection per column
JIT_SUBSET = ["ym-25", "ym1200", "dt-1500", "mdn", "null"]


def month_ends(years):
    out = []
    for y in years:
        for m in range(1, 13):
            out.append(X.days_of(y + (m == 12), m % 12 + 1, 1) - 1)
    return out


WIDE_DAYS = month_ends([2023, 2024, 1900, 2000, 2100]) + [X.days_of(101, 1, 1), X.days_of(9899, 12, 31), X.days_of(1969, 12, 31), X.days_of(1970, 1, 1), X.days_of(1600, 2, 29)]
NS_DAYS = month_ends([2023, 2024, 1900, 2000, 2100]) + [X.days_of(1800, 1, 31), X.days_of(2150, 12, 31), X.days_of(1969, 12, 31), X.days_of(1970, 1, 1)]

_TABLES = {}


def data(n):
    """{column: [int]} and {column: validity} for n rows: drawn once per size and shared, never changed."""
    if n in _TABLES:
        return _TABLES[n]
    r = np.random.default_rng(1000 + n)
    vals, valid = {}, {}

    def days_for(pool):
        extra = [int(x) for x in r.integers(min(pool), max(pool), 40)]
        p = pool + extra
        return [p[i % len(p)] if i < len(p) else p[int(r.integers(0, len(p)))] for i in range(n)]
    vals["d"] = days_for(WIDE_DAYS)
    for u in UNITS:
        per = X.PER_SECOND[u]
        for name in ("ts_" + PA_UNIT[u], "tb_" + PA_UNIT[u]):
            days = days_for(NS_DAYS if u == "Nanosecond" else WIDE_DAYS)
            tod = r.integers(1, 86400 * per, n)      # never midnight
            vals[name] = [int(d) * 86400 * per + int(t) for d, t in zip(days, tod)]
        # the second column stays close to the first on most rows, so that differences repeat (group keys) and are small (durations)
        vals["tb_" + PA_UNIT[u]] = [a - int(k) * per if i % 4 else b for i, (a, b, k) in enumerate(zip(vals["ts_" + PA_UNIT[u]], vals["tb_" + PA_UNIT[u]], r.integers(-3, 4, n)))]
        vals["du_" + PA_UNIT[u]] = [int(x) for x in r.integers(-10 ** 6, 10 ** 6, n) * per]
    # rows whose 64-bit difference and sum wrap (in the columns no interval is added to: that would leave int64 and fail the run)
    if n > 2:
        vals["tb_us"][1], vals["du_us"][1] = -2 ** 63 + 5, 2 ** 63 - 1
        vals["tb_us"][2], vals["du_us"][2] = 2 ** 63 - 1, -2 ** 63
    for name in vals:
        valid[name] = r.random(n) >= 0.2
    _TABLES[n] = (vals, valid)
    return _TABLES[n]


def arrow_type(name):
    if name == "d":
        return pa.date32()
    return pa.duration(name[3:]) if name.startswith("du_") else pa.timestamp(name[3:])


def arrow_of(values, t):
    """[int or None] -> an array of a date / timestamp / duration type."""
    store = pa.int32() if t == pa.date32() else pa.int64()
    return pa.array(values, type=store).cast(t)


def table(n, nullable, names):
    vals, valid = data(n)
    arrays = [arrow_of([v if (ok or not nullable) else None for v, ok in zip(vals[c], valid[c])], arrow_type(c)) for c in names]
    return pa.Table.from_arrays(arrays, schema=pa.schema([pa.field(c, arrow_type(c), nullable=nullable) for c in names]))


def column(n, nullable, name):
    vals, valid = data(n)
    return [v if (ok or not nullable) else None for v, ok in zip(vals[name], valid[name])]


def ints(a):
    a = a.combine_chunks() if isinstance(a, pa.ChunkedArray) else a
    return a.cast(pa.int32() if a.type == pa.date32() else pa.int64()).to_pylist()


def run(tc, node, runs=2):
    p = g.NativePlan(node, tc)
    first = p.execute(0).to_arrow()
    for again in range(1, runs):      # deferred from the second execution on
        t = p.execute(0).to_arrow()
        assert t.schema == first.schema and t.equals(first), ("execution", again)
    return first


def projected(tc, t, named, chunk=4):
    src = g.MemoryExec([t])
    exprs = named(src.schema())
    out = {}
    for i in range(0, len(exprs), chunk):
        got = run(tc, g.ProjectionExec(exprs[i:i + chunk], src))
        assert got.num_rows == t.num_rows
        out.update({n: got[n] for n in got.column_names})
    return out


def evaluators(tc, n):
    """The interpreter, and for the 4097-row case the run-time compiled evaluator as well (a launch of it is asserted)."""
    yield "auto"
    if n == max(SIZES) and tc.ctx.jit_stats()["available"]:
        before = tc.ctx.jit_stats()["launches"]
        tc.ctx.set_jit("force")
        try:
            yield "force"
        finally:
            tc.ctx.set_jit("auto")
        assert tc.ctx.jit_stats()["launches"] > before, "no JIT launch happened"


_SHIFT = {}


def expected_add(name, values, interval, sign):
    """The restatement over a column; the month shifts are memoised by day."""
    key = (name, id(values), interval, sign)
    if key not in _SHIFT:
        if name == "d":
            _SHIFT[key] = [X.date32_add(v, interval, sign) for v in values]
        else:
            _SHIFT[key] = [X.timestamp_add(v, UNIT_OF[name], interval, sign) for v in values]
    return _SHIFT[key]


_COLS = {}


def shared_column(n, nullable, name):
    if (n, nullable, name) not in _COLS:
        _COLS[(n, nullable, name)] = column(n, nullable, name)
    return _COLS[(n, nullable, name)]


# ------------------------------------------------------------------------------------ date / timestamp +- interval
@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("name", COLUMNS)
def test_intervals_through_projection(tc, name, nullable):
    for n in SIZES:
        t = table(n, nullable, [name])
        values = shared_column(n, nullable, name)
        for mode in evaluators(tc, n):
            chosen = [iv for iv in INTERVALS if mode == "auto" or iv[0] in JIT_SUBSET]

            def named(s):
                x = col(name, s)
                out = []
                for tag, e, _ in chosen:
                    out += [(binary(x, Op.Plus, e), tag + "|+"), (binary(x, Op.Minus, e), tag + "|-")]
                    if mode == "auto":
                        out.append((binary(e, Op.Plus, x), tag + "|c"))
                return out
            got = projected(tc, t, named, chunk=5 if mode == "force" else 4)
            for tag, _, iv in chosen:
                for form, sign in (("+", 1), ("-", -1), ("c", 1)):
                    if tag + "|" + form not in got:
                        continue
                    out = got[tag + "|" + form]
                    assert out.type == arrow_type(name), (name, n, mode, tag, form, out.type)
                    assert ints(out) == expected_add(name, values, iv, sign), (name, n, mode, tag, form)


# ------------------------------------------------------------------------------------ timestamp - timestamp, +- duration
@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("unit", UNITS)
def test_differences_and_durations(tc, unit, nullable):
    a, b, d = ("%s_%s" % (p, PA_UNIT[unit]) for p in ("ts", "tb", "du"))
    T, D = pa.timestamp(PA_UNIT[unit]), pa.duration(PA_UNIT[unit])
    for n in SIZES:
        t = table(n, nullable, [a, b, d])
        va, vb, vd = (shared_column(n, nullable, c) for c in (a, b, d))
        want = {"a-b": (D, [X.sub64(x, y) for x, y in zip(va, vb)], pc.subtract(t[a], t[b])),
                "a+d": (T, [X.add64(x, y) for x, y in zip(va, vd)], pc.add(t[a], t[d])),
                "d+a": (T, [X.add64(x, y) for x, y in zip(va, vd)], pc.add(t[d], t[a])),
                "a-d": (T, [X.sub64(x, y) for x, y in zip(va, vd)], pc.subtract(t[a], t[d])),
                "d+d": (D, [X.add64(x, x) for x in vd], None),
                "(a-b)-d": (D, [X.sub64(X.sub64(x, y), z) for x, y, z in zip(va, vb, vd)], None),
                "-d": (D, [X.sub64(0, x) for x in vd], None),
                "a+lit": (T, [X.add64(x, 3600 * X.PER_SECOND[unit]) for x in va], None),
                "a+null": (T, [None] * n, None),
                "d": (D, vd, t[d]),
                "d as i64": (pa.int64(), vd, None)}
        if unit == "Microsecond" and n > 2 and not nullable:      # the wrapping rows
            assert any(not -2 ** 63 <= x - y < 2 ** 63 for x, y in zip(va, vb)) and any(not -2 ** 63 <= x + y < 2 ** 63 for x, y in zip(va, vd))
            assert any(not -2 ** 63 <= x - y < 2 ** 63 for x, y in zip(va, vd))
        for mode in evaluators(tc, n):
            def named(s):
                ca, cb, cd = col(a, s), col(b, s), col(d, s)
                return [(binary(ca, Op.Minus, cb), "a-b"), (binary(ca, Op.Plus, cd), "a+d"), (binary(cd, Op.Plus, ca), "d+a"), (binary(ca, Op.Minus, cd), "a-d"),
                        (binary(cd, Op.Plus, cd), "d+d"), (binary(binary(ca, Op.Minus, cb), Op.Minus, cd), "(a-b)-d"), (E.negative(cd), "-d"),
                        (binary(ca, Op.Plus, E.duration(3600 * X.PER_SECOND[unit], unit)), "a+lit"), (binary(ca, Op.Plus, E.duration(None, unit)), "a+null"), (cd, "d"),
                        (E.cast(cd, "Int64"), "d as i64")]
            got = projected(tc, t, named, chunk=6)
            for key, (ty, exact, arrow) in want.items():
                assert got[key].type == ty, (unit, n, mode, key, got[key].type)
                assert ints(got[key]) == exact, (unit, n, mode, key)
                if arrow is not None:
                    assert got[key].combine_chunks().equals(arrow.combine_chunks()), (unit, n, mode, key, "pyarrow")


# ------------------------------------------------------------------------------------ predicates
@pytest.mark.parametrize("nullable", [False, True])
def test_filter_predicates(tc, nullable):
    a, b = "ts_s", "tb_s"
    iv, xiv = E.interval_month_day_nano(0, 0, 1500000000), X.month_day_nano(0, 0, 1500000000)
    for n in SIZES:
        t = table(n, nullable, [a, b, "d"])
        va, vb, vd = (shared_column(n, nullable, c) for c in (a, b, "d"))
        keep1 = [x is not None and y is not None and x < X.timestamp_add(y, "Second", xiv) for x, y in zip(va, vb)]
        keep2 = [x is not None and y is not None and X.sub64(x, y) > 1 for x, y in zip(va, vb)]
        keep3 = [x is not None and x >= X.date32_add(X.days_of(2024, 3, 31), X.year_month(1), -1) for x in vd]
        if n == max(SIZES):
            assert 0 < sum(keep1) < n and 0 < sum(keep2) < n and 0 < sum(keep3) < n
        for mode in evaluators(tc, n):
            src = g.MemoryExec([t])
            s = src.schema()
            for pred, keep in ((binary(col(a, s), Op.Lt, binary(col(b, s), Op.Plus, iv)), keep1),
                               (binary(binary(col(a, s), Op.Minus, col(b, s)), Op.Gt, E.duration(1, "Second")), keep2),
                               (binary(col("d", s), Op.GtEq, binary(lit(X.days_of(2024, 3, 31), "Date32"), Op.Minus, E.interval_year_month(1))), keep3)):
                got = run(tc, g.FilterExec(pred, src))
                want = t.filter(pa.array(keep, pa.bool_()))
                assert got.column_names == want.column_names and got.num_rows == want.num_rows, (n, mode)
                for c in want.column_names:      # (the result's schema does not say "not null": column by column)
                    assert got[c].combine_chunks().equals(want[c].combine_chunks()), (n, mode, c)


# ------------------------------------------------------------------------------------ group key, MIN / MAX, sort key
@pytest.mark.parametrize("nullable", [False, True])
def test_difference_as_group_key_and_min_max_argument(tc, nullable):
    a, b, d = "ts_ms", "tb_ms", "du_ms"
    D = pa.duration("ms")
    for n in SIZES:
        t = table(n, nullable, [a, b, d])
        va, vb, vd = (shared_column(n, nullable, c) for c in (a, b, d))
        want = {}
        for x, y, z in zip(va, vb, vd):
            k = X.sub64(x, y)
            lo, hi, nz = want.get(k, (None, None, 0))
            diff = X.sub64(y, x)
            want[k] = (diff if lo is None or (diff is not None and diff < lo) else lo, z if hi is None or (z is not None and z > hi) else hi, nz + (z is not None))
        for mode in evaluators(tc, n):
            src = g.MemoryExec([t])
            s = src.schema()
            aggs = [{"fn": "MIN", "expr": binary(col(b, s), Op.Minus, col(a, s)), "name": "lo"},
                    {"fn": "MAX", "expr": col(d, s), "name": "hi"}, {"fn": "COUNT", "expr": col(d, s), "name": "nz"}]
            plan = g.NativePlan(g.AggregateExec("Single", [(binary(col(a, s), Op.Minus, col(b, s)), "gap")], aggs, src), tc)
            for again in range(2):      # the second execution is deferred; groups come in no particular order
                out = plan.execute(0).to_arrow()
                assert [c.type for c in out.columns] == [D, D, D, pa.int64()], (n, mode, again)
                got = {row[0]: row[1:] for row in zip(*[ints(c) for c in out.columns])}
                assert got == want, (n, mode, again)


@pytest.mark.parametrize("nullable", [False, True])
def test_duration_sort_key(tc, nullable):
    d = "du_s"
    for n in SIZES:
        t = table(n, nullable, [d, "d"])
        vd = shared_column(n, nullable, d)
        order = sorted(range(n), key=lambda i: (vd[i] is None, vd[i] if vd[i] is not None else 0, i))      # ascending, NULLs last; ties keep their order
        for mode in evaluators(tc, n):
            src = g.MemoryExec([t])
            got = run(tc, g.SortExec([E.sort_expr(col(d, src.schema()), asc=True, nulls_first=False)], src))
            assert got[d].type == pa.duration("s")
            assert ints(got[d]) == [vd[i] for i in order], (n, mode)
            # rows with equal keys may come in any order: compare the other column as a multiset per key
            pairs = sorted(zip([(x is None, x or 0) for x in ints(got[d])], [(x is None, x or 0) for x in ints(got["d"])]))
            want_d = ints(t["d"])
            assert pairs == sorted(((vd[i] is None, vd[i] or 0), (want_d[i] is None, want_d[i] or 0)) for i in range(n)), (n, mode)


def test_a_duration_column_in_and_out_keeps_its_arrow_type(tc):
    for unit in UNITS:
        t = table(65, True, ["du_" + PA_UNIT[unit]])
        got = run(tc, g.ProjectionExec([(col("du_" + PA_UNIT[unit], g.MemoryExec([t]).schema()), "x")], g.MemoryExec([t])))
        assert got.schema.field("x").type == pa.duration(PA_UNIT[unit]) and got["x"].combine_chunks().equals(t["du_" + PA_UNIT[unit]].combine_chunks()), unit


# ------------------------------------------------------------------------------------ out of range
def test_a_result_out_of_range_is_an_error_of_the_run(tc):
    """Date32 2,147,483,000 + 1,200 months is beyond int32 days: the run fails and names the expression; the context goes on."""
    bad = pa.Table.from_arrays([arrow_of([19000, 2147483000, None, 19001], pa.date32())], names=["d"])
    src = g.MemoryExec([bad])
    e = binary(col("d", src.schema()), Op.Plus, E.interval_year_month(1200))
    for mode in ("auto", "force") if tc.ctx.jit_stats()["available"] else ("auto",):
        tc.ctx.set_jit(mode)
        try:
            with pytest.raises(g.GpuqError, match="out of range.*Date32 \\+ Interval\\(YearMonth\\)"):
                g.NativePlan(g.ProjectionExec([(e, "x")], src), tc).execute(0).to_arrow()
        finally:
            tc.ctx.set_jit("auto")
    assert 2147483000 + 1200 * 28 > 2 ** 31 - 1      # (datetime.date does not reach that far: 1,200 months are at least that many days)
    ok = pa.Table.from_arrays([arrow_of([19000, None, 19001], pa.date32())], names=["d"])
    src = g.MemoryExec([ok])
    got = run(tc, g.ProjectionExec([(binary(col("d", src.schema()), Op.Plus, E.interval_year_month(1200)), "x")], src))
    assert ints(got["x"]) == [X.date32_add(19000, X.year_month(1200)), None, X.date32_add(19001, X.year_month(1200))]
