"""What the aggregate compile produces, as one line per case: the case id and a SHA-256 of everything the device would be given (no GPU
needed).  Hashed per case: the gpuq_compile_check description (scan program, every post program, accumulator kinds, output fields)
and the run-time source of each aggregate sink kernel (ids 3, 4, 11, 12, 13: tools/jit_compile_check.py).  A refusal is recorded by its
message.  Two builds that print the same lines compile every descriptor of the grid to the same programs, instruction for instruction:
    python tools/agg_compile_hashes.py > a.txt        (GPUQ_LIB=<another libgpuq.so> selects the build)
tests/test_cpu_agg_compile.py walks the same grid."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import arrow_ballista_amd as g
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit

D152 = {"Decimal128": [15, 2]}
AGG_SINKS = (3, 4, 11, 12, 13)
# argument columns of the grid, then the group column and the second argument of the two-argument functions
ARG_COLS = [("dec", D152, False), ("decn", D152, True), ("i64", "Int64", False), ("i64n", "Int64", True), ("i32", "Int32", False),
            ("u32", "UInt32", False), ("f64", "Float64", False), ("f64n", "Float64", True), ("daten", "Date32", True)]
FIELDS = [{"name": n, "type": t, "nullable": nl} for n, t, nl in ARG_COLS] + [{"name": "g", "type": "Utf8", "nullable": False},
                                                                              {"name": "y", "type": "Float64", "nullable": True}]
ONE_ARG = ["SUM", "AVG", "COUNT", "MIN", "MAX", "VARIANCE", "VAR_POP", "STDDEV", "STDDEV_POP"]
TWO_ARG = ["COVARIANCE", "COVAR_POP", "CORRELATION"]
OVER_DATE32 = {"COUNT", "MIN", "MAX"}      # every other function refuses a Date32 argument: "<FN> over Date32"
ALIASES = [("VAR", "VARIANCE"), ("VAR_SAMP", "VARIANCE"), ("variance", "VARIANCE"), ("VARIANCE_POP", "VAR_POP"), ("STDDEV_SAMP", "STDDEV"),
           ("stddev", "STDDEV"), ("COVAR", "COVARIANCE"), ("COVAR_SAMP", "COVARIANCE"), ("COVARIANCE_POP", "COVAR_POP"), ("CORR", "CORRELATION"),
           ("sum", "SUM"), ("Sum", "SUM"), ("count", "COUNT")]


def field_of(o):
    """An output field of a description as an input field of the next operator."""
    t = o["type"]
    if t.startswith("Decimal128("):
        p, s = t[len("Decimal128("):-1].split(",")
        t = {"Decimal128": [int(p), int(s)]}
    return {"name": o["name"], "type": t, "nullable": bool(o["nullable"])}


def aggregate(mode, fields, groups, aggs, **extra):
    return dict({"op": "aggregate", "mode": mode, "input": {"fields": fields}, "group_expr": [{"expr": col(n, fields), "name": n} for n in groups],
                 "aggr_expr": aggs}, **extra)


def agg_of(fn, column, fields=FIELDS, name="a"):
    a = {"fn": fn, "expr": col(column, fields), "name": name}
    if fn in TWO_ARG or any(fn == alias and of in TWO_ARG for alias, of in ALIASES):
        a["expr2"] = col("y", fields)
    return a


def final_of(partial_desc, partial_out, mode="Final"):
    """The Final over a Partial's own output fields: group columns rebound by name, state columns read by position."""
    fields = [field_of(o) for o in partial_out["outputs"]]
    return aggregate(mode, fields, [x["name"] for x in partial_desc["group_expr"]], [{"fn": a["fn"], "name": a["name"]} for a in partial_desc["aggr_expr"]])


def single_function_grid():
    """(fn, column name, column type, grouped) for every combination of the grid."""
    for fn in ONE_ARG + TWO_ARG:
        for cname, ctype, _ in ARG_COLS:
            for grouped in (False, True):
                yield fn, cname, ctype, grouped


NINE_FIELDS = [{"name": "s", "type": "Utf8", "nullable": False}, {"name": "dt", "type": "Date32", "nullable": False}, {"name": "q", "type": D152, "nullable": False},
               {"name": "d", "type": D152, "nullable": True}, {"name": "f", "type": "Float64", "nullable": False}]


def nine_aggregates(mode="Single"):
    """A result projection too large for one program: 10 accumulators, two post programs in Single mode."""
    aggs = [{"fn": fn, "expr": col(c, NINE_FIELDS), "name": "%s(%s)" % (fn, c)} for c in ("q", "d") for fn in ("SUM", "AVG", "MIN", "MAX")]
    aggs.append({"fn": "STDDEV", "expr": col("f", NINE_FIELDS), "name": "STDDEV(f)"})
    return aggregate(mode, NINE_FIELDS, ["s", "dt"], aggs)


SEVEN = [("k0", "Int64", False), ("k1", "Int64", True), ("k2", "Int32", False), ("k3", "UInt32", False), ("k4", "Date32", False), ("k5", "Utf8", False), ("k6", D152, False)]
SEVEN_FIELDS = [{"name": n, "type": t, "nullable": nl} for n, t, nl in SEVEN] + [{"name": "v", "type": D152, "nullable": True}]
# five keys that each need a slot of their own (Utf8 and Float64 do not pack): more than the table holds
SOLO_FIELDS = [{"name": "u%d" % i, "type": "Utf8" if i < 3 else "Float64", "nullable": False} for i in range(5)] + [{"name": "v", "type": "Int64", "nullable": False}]


def extra_cases():
    f = FIELDS
    yield "filter", aggregate("Single", f, ["g"], [dict(agg_of("SUM", "dec"), filter=binary(col("i64", f), Op.Gt, lit(3, "Int64"))),
                                                   {"fn": "COUNT", "name": "n", "filter": binary(col("f64n", f), Op.Lt, lit(0.5))}])
    yield "count_literal", aggregate("Partial", f, ["g"], [{"fn": "COUNT", "expr": lit(1), "name": "COUNT(*)"}])
    yield "group_by_only", aggregate("Single", f, ["g", "i32"], [])
    yield "predicate", aggregate("Single", f, ["g"], [agg_of("AVG", "decn"), agg_of("MAX", "i64n", name="m")], predicate=binary(col("daten", f), Op.LtEq, lit(9204, "Date32")))
    for mode in ("Single", "Partial"):
        yield "seven_keys_" + mode, aggregate(mode, SEVEN_FIELDS, [n for n, _, _ in SEVEN], [{"fn": "SUM", "expr": col("v", SEVEN_FIELDS), "name": "s"},
                                                                                            {"fn": "COUNT", "expr": col("v", SEVEN_FIELDS), "name": "c"}])
    yield "too_many_packed_keys", aggregate("Single", SOLO_FIELDS, ["u%d" % i for i in range(5)], [{"fn": "SUM", "expr": col("v", SOLO_FIELDS), "name": "s"}])
    for mode in ("Single", "Partial"):
        yield "nine_aggregates_" + mode, nine_aggregates(mode)


def describe(desc):
    """(text to hash, description or None).  A refusal is its message."""
    try:
        out = g.compile_check(desc)
    except g.GpuqError as e:
        return "refused: " + str(e), None
    text = json.dumps(out, sort_keys=True)
    for sink in AGG_SINKS:
        try:
            text += "\n//sink %d\n" % sink + g.compile_jit_source(dict(desc, jit_gmax=4), sink)
        except g.GpuqError as e:
            text += "\n//sink %d refused: %s" % (sink, e)
    return text, out


def cases():
    """(case id, descriptor) in a fixed order; a Final case is fed with the output fields of the Partial before it."""
    for fn, cname, _, grouped in single_function_grid():
        groups = ["g"] if grouped else []
        cid = "%s(%s)%s" % (fn, cname, " by g" if grouped else "")
        for mode in ("Single", "Partial"):
            yield cid + " " + mode, aggregate(mode, FIELDS, groups, [agg_of(fn, cname)])
        yield cid + " Final", ("final_of", aggregate("Partial", FIELDS, groups, [agg_of(fn, cname)]))
    for alias, _ in ALIASES:
        for mode in ("Single", "Partial"):
            yield "alias %s %s" % (alias, mode), aggregate(mode, FIELDS, ["g"], [agg_of(alias, "i64n")])
    for cid, desc in extra_cases():
        yield cid, desc
    yield "nine_aggregates Final", ("final_of", nine_aggregates("Partial"))
    yield "seven_keys Final", ("final_of", aggregate("Partial", SEVEN_FIELDS, [n for n, _, _ in SEVEN], [{"fn": "AVG", "expr": col("v", SEVEN_FIELDS), "name": "a"}]))


def main():
    for cid, desc in cases():
        if isinstance(desc, tuple):
            partial = desc[1]
            try:
                desc = final_of(partial, g.compile_check(partial))
            except g.GpuqError as e:
                print("%-44s %s" % (cid, hashlib.sha256(("partial refused: " + str(e)).encode()).hexdigest()))
                continue
        text, _ = describe(desc)
        print("%-44s %s" % (cid, hashlib.sha256(text.encode()).hexdigest()))


if __name__ == "__main__":
    main()
