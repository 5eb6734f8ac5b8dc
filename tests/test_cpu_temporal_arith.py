"""CPU: Interval and Duration arithmetic without a device.

The restatement (tests/temporal_exact.py) pinned on answers written down by hand; every row of the typing table through compile_check
(output type and nullability, required and nullable operands); every refusal by its message and status; every malformed Interval
literal; the schema of a plan that yields a Duration; the run-time sources of a projection and a filter that use every rule
cross-compile for gfx950; and csrc/date_shift_op.h as a host program of its own under AddressSanitizer / UBSan against dateutil."""
import importlib.util
import os
import subprocess
import sys

import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd import binding as B
from arrow_ballista_amd import expr as E
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, cast, col, lit

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_exact as X      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arrow-ballista_amd", "csrc")
UNITS = X.UNITS
ABBR = {"Second": "s", "Millisecond": "ms", "Microsecond": "us", "Nanosecond": "ns"}

FIELDS = []
for _n, _t in ([("d32", "Date32"), ("d64", "Date64"), ("i64", "Int64"), ("f64", "Float64")]
               + [("ts_" + ABBR[u], {"Timestamp": [u, None]}) for u in UNITS] + [("dur_" + ABBR[u], {"Duration": u}) for u in UNITS]
               + [("ts_utc", {"Timestamp": ["Microsecond", "UTC"]}), ("ts_off", {"Timestamp": ["Microsecond", "+00:00"]}),
                  ("ts_ny", {"Timestamp": ["Microsecond", "America/New_York"]})]):
    FIELDS += [{"name": _n, "type": _t, "nullable": False}, {"name": _n + "n", "type": _t, "nullable": True}]

YM, DT, MDN = E.interval_year_month(3), E.interval_day_time(1, -1500), E.interval_month_day_nano(-1, 2, 3)
INTERVALS = [("Interval(YearMonth)", YM), ("Interval(DayTime)", DT), ("Interval(MonthDayNano)", MDN)]


def c(name):
    return col(name, FIELDS)


def project(*es):
    return {"op": "project", "input": {"fields": FIELDS}, "exprs": [{"expr": e, "name": "x%d" % i} for i, e in enumerate(es)]}


def outputs(*es):
    return [(o["type"], bool(o["nullable"])) for o in g.compile_check(project(*es))["outputs"]]


def failure(desc):
    with pytest.raises(g.GpuqError) as err:
        g.compile_check(desc)
    return err.value.status, err.value.refusal, str(err.value)


def refused(e, message):
    status, refusal, text = failure(project(e) if "op" not in e else e)
    assert message in text and status == 3 and refusal == B.REFUSAL_NONE, (status, refusal, text)


# ---------------------------------------------------------------- the restatement, on answers written down by hand
def test_the_restatement_on_hand_written_answers():
    d = X.days_of
    assert X.date32_add(d(2024, 1, 31), X.year_month(1)) == d(2024, 2, 29)
    assert X.date32_add(d(2023, 1, 31), X.year_month(1)) == d(2023, 2, 28)
    assert X.date32_add(d(2024, 3, 31), X.year_month(1), -1) == d(2024, 2, 29)
    assert X.date32_add(d(2100, 1, 31), X.year_month(1)) == d(2100, 2, 28)
    # 1969-12-31T23:59:59 + 1 month = 1970-01-31T23:59:59: a pre-epoch instant keeps its time of day
    for u in UNITS:
        p = X.PER_SECOND[u]
        assert X.timestamp_add(-1 * p, u, X.year_month(1)) == (d(1970, 1, 31) * 86400 + 86399) * p, u
    # each part of an interval is added to a date as whole days, truncated toward zero
    assert X.date32_add(d(2024, 1, 31), X.day_time(0, -86399999)) == d(2024, 1, 31)
    assert X.date32_add(d(2024, 1, 31), X.day_time(0, -86400000)) == d(2024, 1, 30)
    assert X.date32_add(d(2024, 1, 31), X.day_time(0, 86399999), -1) == d(2024, 1, 31)
    assert X.date32_add(d(2024, 1, 31), X.month_day_nano(1, 1, 2 * X.DAY_NS - 1)) == d(2024, 3, 2)
    # a Second timestamp + 1,500 ms: the exact instant is floored to the unit
    assert X.timestamp_add(10, "Second", X.day_time(0, 1500)) == 11
    assert X.timestamp_add(10, "Second", X.day_time(0, 1500), -1) == 8
    assert X.timestamp_add(-10, "Second", X.day_time(0, -1500)) == -12
    assert X.timestamp_add(7, "Microsecond", X.month_day_nano(0, 0, 1)) == 7 and X.timestamp_add(7, "Microsecond", X.month_day_nano(0, 0, -1)) == 6
    assert X.timestamp_add(7, "Nanosecond", X.month_day_nano(0, 1, -1)) == 7 + X.DAY_NS - 1
    assert X.date32_add(None, X.year_month(1)) is None and X.timestamp_add(5, "Second", None) is None
    with pytest.raises(X.OutOfRange):
        X.date32_add(2 ** 31 - 1, X.day_time(1, 0))
    with pytest.raises(X.OutOfRange):
        X.timestamp_add(2 ** 63 - 1, "Second", X.day_time(0, 1000))
    assert X.sub64(2 ** 63 - 1, -1) == -2 ** 63 and X.add64(-2 ** 63, -1) == 2 ** 63 - 1 and X.sub64(None, 1) is None


# ---------------------------------------------------------------- the typing table
def test_a_date_or_timestamp_takes_an_interval_and_keeps_its_type():
    for base, shown in [("d32", "Date32")] + [("ts_" + ABBR[u], "Timestamp(%s)" % u) for u in UNITS] + [("ts_utc", "Timestamp(Microsecond)"), ("ts_off", "Timestamp(Microsecond)")]:
        for _, iv in INTERVALS:
            assert outputs(binary(c(base), Op.Plus, iv), binary(c(base), Op.Minus, iv), binary(iv, Op.Plus, c(base)),
                           binary(c(base + "n"), Op.Plus, iv), binary(c(base + "n"), Op.Minus, iv), binary(iv, Op.Plus, c(base + "n"))) == [(shown, False)] * 3 + [(shown, True)] * 3, base
        # a NULL interval makes the result NULL
        assert outputs(binary(c(base), Op.Plus, E.interval_year_month(None))) == [(shown, True)], base


def test_timestamps_and_durations():
    for u in UNITS:
        ts, dur, T, D = "ts_" + ABBR[u], "dur_" + ABBR[u], "Timestamp(%s)" % u, "Duration(%s)" % u
        for a, b, nullable in ((ts, ts, False), (ts + "n", ts, True), (ts, ts + "n", True), (ts + "n", ts + "n", True)):
            assert outputs(binary(c(a), Op.Minus, c(b))) == [(D, nullable)], u
        for a, b, nullable in ((ts, dur, False), (ts + "n", dur, True), (ts, dur + "n", True)):
            assert outputs(binary(c(a), Op.Plus, c(b)), binary(c(a), Op.Minus, c(b)), binary(c(b), Op.Plus, c(a))) == [(T, nullable)] * 3, u
        for a, b, nullable in ((dur, dur, False), (dur + "n", dur, True), (dur, dur + "n", True)):
            assert outputs(binary(c(a), Op.Plus, c(b)), binary(c(a), Op.Minus, c(b))) == [(D, nullable)] * 2, u
        assert outputs(E.negative(c(dur)), E.negative(c(dur + "n"))) == [(D, False), (D, True)], u
        assert outputs(binary(c(ts), Op.Plus, E.duration(5, u)), binary(binary(c(ts), Op.Minus, c(ts)), Op.Gt, E.duration(5, u)),
                       binary(c(dur), Op.LtEq, c(dur + "n")), binary(c(ts), Op.Plus, E.duration(None, u))) == [(T, False), ("Boolean", False), ("Boolean", True), (T, True)], u
        # the count is kept to and from Int64
        assert outputs(cast(c(dur), "Int64"), cast(c("i64n"), ("Duration", u)), c(dur + "n")) == [("Int64", False), (D, True), (D, True)], u
    # Duration arithmetic is zone-free
    assert outputs(binary(c("ts_ny"), Op.Plus, c("dur_us")), binary(c("ts_ny"), Op.Minus, c("ts_nyn"))) == [("Timestamp(Microsecond)", False), ("Duration(Microsecond)", True)]


def test_what_was_there_before_is_untouched():
    assert outputs(binary(c("d32"), Op.Plus, lit(3, "Int32")), binary(c("d32n"), Op.Minus, lit(3, "Int32")), binary(c("d32"), Op.Minus, c("d32n")),
                   binary(c("ts_us"), Op.Lt, c("ts_usn")), binary(c("ts_ny"), Op.Eq, c("ts_us")), cast(c("ts_ms"), ("Timestamp", "Second")), cast(c("ts_ns"), "Date32")) == \
        [("Date32", False), ("Date32", True), ("Int32", True), ("Boolean", True), ("Boolean", False), ("Timestamp(Second)", False), ("Date32", False)]


def test_a_duration_passes_where_a_timestamp_does():
    f = FIELDS
    d = g.compile_check({"op": "aggregate", "mode": "Single", "input": {"fields": f}, "group_expr": [{"expr": binary(c("ts_us"), Op.Minus, c("ts_usn")), "name": "k"}],
                         "aggr_expr": [{"fn": "MIN", "expr": c("dur_msn"), "name": "lo"}, {"fn": "MAX", "expr": binary(c("ts_s"), Op.Minus, c("ts_s")), "name": "hi"},
                                       {"fn": "COUNT", "expr": c("dur_nsn"), "name": "n"}]})
    assert [(o["name"], o["type"]) for o in d["outputs"]] == [("k", "Duration(Microsecond)"), ("lo", "Duration(Millisecond)"), ("hi", "Duration(Second)"), ("n", "Int64")]
    g.compile_check({"op": "filter", "input": {"fields": f}, "predicate": binary(c("ts_us"), Op.Lt, binary(c("ts_usn"), Op.Plus, YM))})
    g.compile_check({"op": "sort", "input": {"fields": f}, "expr": [{"expr": c("dur_sn"), "asc": True, "nulls_first": False}]})
    g.compile_check({"op": "join_build", "input": {"fields": f}, "on": [c("dur_us")]})
    g.compile_check({"op": "partition", "input": {"fields": f}, "hash_expr": [c("dur_ns")], "partition_count": 4})


def test_a_projection_node_announces_a_duration_field():
    plan = {"ProjectionExec": {"input": {"MemoryExec": {"schema": FIELDS, "partitions": [0]}},
                               "expr": [binary(c("ts_ms"), Op.Minus, c("ts_msn")), c("dur_ns"), binary(c("d32n"), Op.Plus, MDN)], "expr_name": ["gap", "d", "due"]}}
    assert B.plan_schema(plan) == [{"name": "gap", "type": {"Duration": "Millisecond"}, "nullable": True}, {"name": "d", "type": {"Duration": "Nanosecond"}, "nullable": False},
                                   {"name": "due", "type": "Date32", "nullable": True}]


# ---------------------------------------------------------------- refusals
def test_refusals_by_name():
    for name, iv in INTERVALS:
        refused(binary(c("d64"), Op.Plus, iv), "Date64 + %s is not built" % name)
        refused(binary(c("d64n"), Op.Minus, iv), "Date64 - %s is not built" % name)
        refused(binary(iv, Op.Minus, c("d32")), "%s - Date32 is not built" % name)
        refused(binary(iv, Op.Minus, c("ts_us")), "%s - Timestamp(Microsecond) is not built" % name)
        refused(binary(iv, Op.Plus, iv), "%s + %s is not built" % (name, name))
        refused(binary(iv, Op.Minus, YM), "%s - Interval(YearMonth) is not built" % name)
        for op in (Op.Multiply, Op.Divide, Op.Modulo):
            refused(binary(iv, op, lit(2)), "'%s' with an Interval operand is not built" % op)
            refused(binary(c("d32"), op, iv), "'%s' with an Interval operand is not built" % op)
        for op in (Op.Eq, Op.NotEq, Op.Lt, Op.LtEq, Op.Gt, Op.GtEq):
            refused(binary(iv, op, iv), "a comparison with an Interval operand is not built")
            refused(binary(c("ts_us"), op, iv), "a comparison with an Interval operand is not built")
        for zoned in ("ts_ny", "ts_nyn"):
            refused(binary(c(zoned), Op.Plus, iv), "time zone other than UTC")
            refused(binary(iv, Op.Plus, c(zoned)), "time zone other than UTC")
        refused(binary(c("i64"), Op.Plus, iv), "unsupported operands for an Interval: Int64 + " + name)
        refused(binary(c("dur_s"), Op.Plus, iv), "Duration(Second) + %s is not built" % name)
        refused(iv, "Interval columns are not carried")
        refused(cast(c("i64"), {"Interval": name[9:-1]}), "Interval columns are not carried")
        refused(E.negative(iv), "the negative of an Interval is not built")
    for u in UNITS:
        dur = "dur_" + ABBR[u]
        refused(binary(c("d32"), Op.Plus, c(dur)), "Date32 + Duration(%s) is not built" % u)
        refused(binary(c("d32n"), Op.Minus, c(dur)), "Date32 - Duration(%s) is not built" % u)
        refused(binary(c(dur), Op.Minus, c("ts_" + ABBR[u])), "Duration(%s) - Timestamp(%s) is not built" % (u, u))
        for op in (Op.Multiply, Op.Divide, Op.Modulo):
            refused(binary(c(dur), op, lit(2)), "'%s' with a Duration operand is not built" % op)
            refused(binary(c("f64"), op, c(dur)), "'%s' with a Duration operand is not built" % op)
        refused(binary(c(dur), Op.Plus, lit(2)), "unsupported operands for '+'")
        refused(binary(c(dur), Op.Eq, c("i64")), "a Duration compares with a Duration")
        for to in ("Int32", "Float64", "Date32", "Utf8", ("Timestamp", u)):
            refused(cast(c(dur), to), "a Duration casts to and from Int64")
        refused(cast(c("ts_" + ABBR[u]), ("Duration", u)), "a Duration casts to and from Int64")
        refused(cast(c("f64"), ("Duration", u)), "a Duration casts to and from Int64")
        for fn in ("SUM", "AVG", "VARIANCE", "STDDEV_POP"):
            refused({"op": "aggregate", "mode": "Single", "input": {"fields": FIELDS}, "group_expr": [], "aggr_expr": [{"fn": fn, "expr": c(dur), "name": "a"}]},
                    "%s over Duration(%s)" % (fn, u))
    # two units: the plan carries the casts
    for a, op, b in (("ts_s", Op.Minus, "ts_ms"), ("ts_us", Op.Plus, "dur_ns"), ("ts_us", Op.Minus, "dur_s"), ("dur_ms", Op.Plus, "ts_s"), ("dur_s", Op.Plus, "dur_ms"),
                     ("dur_us", Op.Minus, "dur_ns"), ("dur_us", Op.Lt, "dur_ns")):
        refused(binary(c(a), op, c(b)), "the plan carries the casts")
    refused(cast(c("dur_s"), ("Duration", "Millisecond")), "a Duration casts to and from Int64")
    # an Interval as a field's type
    refused({"op": "project", "input": {"fields": [{"name": "iv", "type": {"Interval": "DayTime"}, "nullable": True}]}, "exprs": [{"expr": lit(1), "name": "x"}]},
            "Interval columns are not carried")


def test_malformed_interval_literals_name_the_member():
    def bad(type_, value, message):
        e = binary(c("d32"), Op.Plus, {"literal": {"type": {"Interval": type_}, "value": value}})
        status, _, text = failure(project(e))
        assert status == 1 and message in text, (status, text)
    bad("YearMonth", "1.5", "member 'months' is not an integer")
    bad("YearMonth", "x", "member 'months' is not an integer")
    bad("YearMonth", str(2 ** 31), "member 'months' is out of its 32 bits")
    bad("YearMonth", {"months": 1}, "member 'months' is not an integer")
    bad("DayTime", {"days": 1}, "member 'milliseconds' is missing")
    bad("DayTime", {"milliseconds": 1}, "member 'days' is missing")
    bad("DayTime", {"days": 1.5, "milliseconds": 0}, "member 'days' is not an integer")
    bad("DayTime", {"days": 1, "milliseconds": True}, "member 'milliseconds' is not an integer")
    bad("DayTime", {"days": -2 ** 31 - 1, "milliseconds": 0}, "member 'days' is out of its 32 bits")
    bad("DayTime", {"days": 0, "milliseconds": 2 ** 31}, "member 'milliseconds' is out of its 32 bits")
    bad("DayTime", "3", "member 'days' is missing")
    bad("MonthDayNano", {"months": 1, "days": 1}, "member 'nanoseconds' is missing")
    bad("MonthDayNano", {"months": None, "days": 1, "nanoseconds": 0}, "member 'months' is missing")
    bad("MonthDayNano", {"months": 1, "days": "a", "nanoseconds": 0}, "member 'days' is not an integer")
    bad("MonthDayNano", {"months": 1, "days": 1, "nanoseconds": str(2 ** 63)}, "member 'nanoseconds' is out of its 64 bits")
    bad("MonthDayNano", {"months": 2 ** 31, "days": 1, "nanoseconds": 0}, "member 'months' is out of its 32 bits")
    status, _, text = failure(project(binary(c("d32"), Op.Plus, {"literal": {"type": {"Interval": "Weeks"}, "value": "1"}})))
    assert status == 1 and "bad Interval unit 'Weeks'" in text
    status, _, text = failure(project(binary(c("ts_s"), Op.Plus, {"literal": {"type": {"Duration": "Hour"}, "value": "1"}})))
    assert status == 1 and "bad Duration unit 'Hour'" in text
    # the extremes of every member are taken
    assert outputs(binary(c("ts_ns"), Op.Plus, E.interval_month_day_nano(-2 ** 31, 2 ** 31 - 1, -2 ** 63)), binary(c("d32"), Op.Minus, E.interval_day_time(-2 ** 31, 2 ** 31 - 1)),
                   binary(c("d32"), Op.Minus, E.interval_year_month(-2 ** 31))) == [("Timestamp(Nanosecond)", False), ("Date32", False), ("Date32", False)]


# ---------------------------------------------------------------- the run-time source
def test_run_time_sources_compile_for_gfx950(tmp_path):
    """What hiprtc would be given for a projection and a filter that together use every rule (the command line of tools/jit_compile_check.py)."""
    # (the outputs of one projection are all live at once, next to its columns: three of them)
    proj1 = project(binary(c("d32n"), Op.Plus, YM), binary(c("d32"), Op.Minus, DT), binary(MDN, Op.Plus, c("d32n")), binary(c("ts_s"), Op.Plus, DT))
    proj2 = project(binary(c("ts_msn"), Op.Minus, MDN), binary(YM, Op.Plus, c("ts_us")), binary(c("ts_nsn"), Op.Minus, E.interval_month_day_nano(0, 0, 1)))
    proj3 = project(binary(c("ts_us"), Op.Minus, c("ts_usn")), binary(c("ts_us"), Op.Plus, c("dur_usn")), binary(c("dur_us"), Op.Plus, c("ts_us")),
                    binary(c("dur_us"), Op.Minus, c("dur_usn")), E.negative(c("dur_usn")), cast(c("dur_us"), "Int64"))
    filt = {"op": "filter", "input": {"fields": FIELDS},
            "predicate": E.and_(binary(c("ts_us"), Op.Lt, binary(c("ts_usn"), Op.Plus, YM)), binary(binary(c("ts_s"), Op.Minus, c("ts_sn")), Op.Gt, E.duration(3600, "Second")),
                                binary(c("d32"), Op.GtEq, binary(c("d32n"), Op.Minus, MDN)), binary(c("dur_ns"), Op.NotEq, c("dur_nsn")))}
    for name, desc, kid in (("proj1", proj1, 2), ("proj2", proj2, 2), ("proj3", proj3, 2), ("filt", filt, 1)):
        src = g.compile_jit_source(desc, kid)
        assert name == "proj3" or ("month_shift_fwd<i64>(" in src and "FLAG_TIME_RANGE" in src), name
        f = os.path.join(str(tmp_path), name + ".hip")
        with open(f, "w") as fh:
            fh.write(src)
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", "-x", "hip", f, "-Rpass-analysis=kernel-resource-usage",
                            "-I", CSRC, "-o", os.path.join(str(tmp_path), name + ".o")], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr[-3000:])
        assert "ScratchSize [bytes/lane]: 0" in r.stderr, name


def test_the_header_travels_to_the_run_time_compiler():
    spec = importlib.util.spec_from_file_location("gpuq_build", os.path.join(ROOT, "arrow-ballista_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "date_shift_op.h" in build.HEADERS and "date_shift_op.h" in build.EMBED
    with open(os.path.join(CSRC, "date_shift_op.h")) as fh:
        assert "#include" not in fh.read()      # hiprtc has no system headers, a plain C++ compiler no HIP ones


# ---------------------------------------------------------------- the header on the host
KS = [-25, -13, -12, -1, 0, 1, 11, 12, 13, 1200]


def test_the_month_shift_on_the_host_against_dateutil(tmp_path):
    """csrc/date_shift_op.h as plain C++ with a main of its own (tests/date_shift_host.cpp) under AddressSanitizer and UBSan: every
    seventh day and every month end of 1600 .. 2400, shifted by every k, line by line against the restatement."""
    import datetime
    spec = importlib.util.spec_from_file_location("gpuq_build", os.path.join(ROOT, "arrow-ballista_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    exe = os.path.join(str(tmp_path), "date_shift_host")
    r = subprocess.run([build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                        os.path.join(ROOT, "tests", "date_shift_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    days = list(range(X.days_of(1600, 1, 1), X.days_of(2400, 12, 31) + 1, 7))
    for y in range(1600, 2401):
        for m in range(1, 13):
            first_of_next = datetime.date(y + (m == 12), m % 12 + 1, 1)
            days.append((first_of_next - X.EPOCH).days - 1)
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(days) * len(KS)
    memo = {}
    i = 0
    for day in days:
        for k in KS:
            if (day, k) not in memo:
                memo[(day, k)] = "%d %d %d" % (day, k, X.shift_months(day, k))
            assert got[i] == memo[(day, k)], (i, got[i], memo[(day, k)])
            i += 1
