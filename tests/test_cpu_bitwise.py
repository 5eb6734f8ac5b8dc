"""CPU: what the compile makes of BIT_AND / BIT_OR / BIT_XOR / BOOL_AND / BOOL_OR and of the scalar operators & | ^, without a device.
Output names, types and nullability in every mode; the Final over a Partial's own output gives the Single's outputs; the refusals by
their messages; shared accumulators; and the run-time sources of the aggregate sinks and of a projection / filter that use the new
accumulator kinds and opcodes cross-compile for gfx950 (the command line of tools/jit_compile_check.py)."""
import concurrent.futures
import importlib.util
import json
import os
import subprocess

import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("agg_compile_hashes", os.path.join(ROOT, "tools", "agg_compile_hashes.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)

INTS = ["Int8", "Int16", "Int32", "Int64", "UInt8", "UInt16", "UInt32", "UInt64"]
BIT_FNS = [("BIT_AND", "[bit_and]", 8), ("BIT_OR", "[bit_or]", 9), ("BIT_XOR", "[bit_xor]", 10)]
BOOL_FNS = [("BOOL_AND", "[bool_and]", 8), ("BOOL_OR", "[bool_or]", 9)]
D152 = {"Decimal128": [15, 2]}
# every legal argument type twice (required, nullable), then what the refusals are about and a group column
FIELDS = ([{"name": t.lower(), "type": t, "nullable": False} for t in INTS] + [{"name": t.lower() + "n", "type": t, "nullable": True} for t in INTS] +
          [{"name": "b", "type": "Boolean", "nullable": False}, {"name": "bn", "type": "Boolean", "nullable": True},
           {"name": "f64", "type": "Float64", "nullable": False}, {"name": "dec", "type": D152, "nullable": False}, {"name": "s", "type": "Utf8", "nullable": False},
           {"name": "d", "type": "Date32", "nullable": False}, {"name": "g", "type": "Int32", "nullable": False}])
TYPE_OF = {f["name"]: f for f in FIELDS}


def legal_cases():
    for fn, suffix, kind in BIT_FNS:
        for t in INTS:
            for c in (t.lower(), t.lower() + "n"):
                yield fn, suffix, kind, c, t
    for fn, suffix, kind in BOOL_FNS:
        for c in ("b", "bn"):
            yield fn, suffix, kind, c, "Boolean"


def test_every_function_type_grouping_and_mode():
    n = 0
    for fn, suffix, kind, c, t in legal_cases():
        for grouped in (False, True):
            groups = ["g"] if grouped else []
            aggs = [H.agg_of(fn, c, FIELDS)]
            nullable = TYPE_OF[c]["nullable"] or not grouped      # NULL where no non-NULL argument was seen; ungrouped over zero rows
            single = g.compile_check(H.aggregate("Single", FIELDS, groups, aggs))
            partial_desc = H.aggregate("Partial", FIELDS, groups, aggs)
            partial = g.compile_check(partial_desc)
            want = [{"name": "g", "type": "Int32", "nullable": 0}] if grouped else []
            assert [(o["name"], o["type"], int(o["nullable"])) for o in single["outputs"]] == [(w["name"], w["type"], w["nullable"]) for w in want] + [("a", t, int(nullable))], (fn, c, grouped)
            assert [(o["name"], o["type"], int(o["nullable"])) for o in partial["outputs"]] == [(w["name"], w["type"], w["nullable"]) for w in want] + [("a" + suffix, t, int(nullable))], (fn, c, grouped)
            # the cell, and the count of non-NULL arguments where the result can be NULL
            assert single["acc_kinds"] == partial["acc_kinds"] == ([kind] + ([1 if TYPE_OF[c]["nullable"] else 2] if nullable else [])), (fn, c, grouped, single["acc_kinds"])
            for mode in ("Final", "FinalPartitioned"):
                final = g.compile_check(H.final_of(partial_desc, partial, mode))
                assert final["outputs"] == single["outputs"], (fn, c, grouped, mode)
                assert final["acc_kinds"][0] == kind
            n += 1
    assert n == (3 * 8 * 2 + 2 * 2) * 2


def refusal(desc):
    with pytest.raises(g.GpuqError) as e:
        g.compile_check(desc)
    return str(e.value)


def test_refusals_say_which_function_over_which_type():
    for fn, _, _ in BIT_FNS:
        for c, shown in (("f64", "Float64"), ("dec", "Decimal128(15,2)"), ("s", "Utf8"), ("d", "Date32"), ("b", "Boolean")):
            for mode in ("Single", "Partial"):
                assert fn + " over " + shown in refusal(H.aggregate(mode, FIELDS, ["g"], [H.agg_of(fn, c, FIELDS)])), (fn, c)
    for fn, _, _ in BOOL_FNS:
        assert fn + " over Int32" in refusal(H.aggregate("Single", FIELDS, [], [H.agg_of(fn, "int32", FIELDS)]))
    # a Final whose state column is of no legal type is refused the same way
    assert "BIT_OR over Float64" in refusal(H.aggregate("Final", [TYPE_OF["g"], dict(TYPE_OF["f64"], name="a[bit_or]")], ["g"], [{"fn": "BIT_OR", "name": "a"}]))
    # DISTINCT stays a plan-level rewrite: the operator refuses it
    assert "DISTINCT" in refusal(H.aggregate("Single", FIELDS, ["g"], [dict(H.agg_of("BIT_XOR", "int32", FIELDS), distinct=True)]))
    # MEDIAN stays refused
    assert "aggregate function MEDIAN" in refusal(H.aggregate("Single", FIELDS, [], [H.agg_of("MEDIAN", "int32", FIELDS)]))

    def project(e):
        return {"op": "project", "input": {"fields": FIELDS}, "exprs": [{"expr": e, "name": "x"}]}
    assert "unsupported operands for '&': Int32, Int64" in refusal(project(binary(col("int32", FIELDS), Op.BitwiseAnd, col("int64", FIELDS))))
    assert "unsupported operands for '&': Float64, Float64" in refusal(project(binary(col("f64", FIELDS), Op.BitwiseAnd, col("f64", FIELDS))))
    assert "unsupported operands for '|': Decimal128(15,2), Decimal128(15,2)" in refusal(project(binary(col("dec", FIELDS), Op.BitwiseOr, col("dec", FIELDS))))
    assert "unsupported operands for '^': Boolean, Boolean" in refusal(project(binary(col("b", FIELDS), Op.BitwiseXor, col("b", FIELDS))))
    assert "unsupported operands for '&': Int32, Int64" in refusal(project(binary(col("int32", FIELDS), Op.BitwiseAnd, lit(4))))      # an untyped Python int is Int64
    for shift in ("<<", ">>", "BitwiseShiftLeft", "BitwiseShiftRight"):
        assert "unsupported binary operator '%s'" % shift in refusal(project(binary(col("int32", FIELDS), shift, col("int32", FIELDS))))


def test_operator_names_types_and_programs():
    for t in INTS:
        a, b = col(t.lower(), FIELDS), col(t.lower() + "n", FIELDS)
        d = g.compile_check({"op": "project", "input": {"fields": FIELDS}, "exprs": [{"expr": binary(a, op, b), "name": op} for op in (Op.BitwiseAnd, Op.BitwiseOr, Op.BitwiseXor)] +
                             [{"expr": binary(a, Op.BitwiseXor, lit(None)), "name": "null"}, {"expr": binary(a, Op.BitwiseAnd, a), "name": "req"}]})
        assert [(o["type"], int(o["nullable"])) for o in d["outputs"]] == [(t, 1)] * 4 + [(t, 0)], t
        # one instruction each (+ two for the NULL literal) and no wrap after them: & | ^ of two extended values is an extended value
        # (the two UInt64 columns are zero-extended where they enter, as for every other use)
        assert len(d["program"]["insns"]) == 3 + 2 + 1 + 1 + (2 if t == "UInt64" else 0), (t, d["program"]["insns"])
        spelled = {}
        for names in (("&", "|", "^"), ("BitwiseAnd", "BitwiseOr", "BitwiseXor"), ("&", "|", "BIT_XOR")):
            p = g.compile_check({"op": "project", "input": {"fields": FIELDS}, "exprs": [{"expr": binary(a, op, b), "name": "x%d" % i} for i, op in enumerate(names)]})
            spelled[names] = json.dumps(p, sort_keys=True)
        assert len(set(spelled.values())) == 1, t
    d = g.compile_check({"op": "filter", "input": {"fields": FIELDS}, "predicate": binary(binary(col("int32n", FIELDS), Op.BitwiseAnd, lit(4, "Int32")), Op.Eq, lit(4, "Int32"))})
    assert d["program"]["pred_reg"] >= 0


def test_letter_case_does_not_matter():
    for fn, _, _, c, _ in legal_cases():
        for mode in ("Single", "Partial"):
            up = g.compile_check(H.aggregate(mode, FIELDS, ["g"], [H.agg_of(fn, c, FIELDS)]))
            for spelling in (fn.lower(), fn.title()):
                assert json.dumps(g.compile_check(H.aggregate(mode, FIELDS, ["g"], [H.agg_of(spelling, c, FIELDS)])), sort_keys=True) == json.dumps(up, sort_keys=True), (spelling, c, mode)


def test_accumulators_are_shared():
    f = FIELDS
    d = g.compile_check(H.aggregate("Single", f, ["g"], [H.agg_of("SUM", "int64n", f, "s"), H.agg_of("BIT_OR", "int64n", f, "o")]))
    assert sorted(d["acc_kinds"]) == [0, 1, 9]      # the sum, ONE count of the non-NULL arguments, the or
    d = g.compile_check(H.aggregate("Single", f, ["g"], [H.agg_of("BIT_OR", "int16", f, "o1"), H.agg_of("BIT_OR", "int16", f, "o2"), H.agg_of("BIT_XOR", "int16", f, "x")]))
    assert d["acc_kinds"] == [9, 10]
    assert [o["name"] for o in d["outputs"]] == ["g", "o1", "o2", "x"]
    # BOOL_AND(b) and BIT_AND(i) are the same kind over different arguments: two cells
    d = g.compile_check(H.aggregate("Single", f, ["g"], [H.agg_of("BOOL_AND", "b", f, "ba"), H.agg_of("BIT_AND", "int32", f, "ia")]))
    assert d["acc_kinds"] == [8, 8]
    # a per-aggregate FILTER is CASE WHEN p THEN x END: nothing further, the result becomes nullable
    d = g.compile_check(H.aggregate("Single", f, ["g"], [dict(H.agg_of("BIT_XOR", "uint8", f, "x"), filter=binary(col("int32", f), Op.Gt, lit(0, "Int32")))]))
    assert [(o["type"], int(o["nullable"])) for o in d["outputs"]] == [("Int32", 0), ("UInt8", 1)] and d["acc_kinds"][0] == 10


def hipcc_device_compile(tmp_path, name, text):
    f = os.path.join(str(tmp_path), name + ".hip")
    with open(f, "w") as fh:
        fh.write(text)
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", "-x", "hip", f, "-Rpass-analysis=kernel-resource-usage",
                        "-I", os.path.join(ROOT, "arrow-ballista_amd", "csrc"), "-o", os.path.join(str(tmp_path), name + ".o")], capture_output=True, text=True)
    return name, r.returncode, r.stderr[-3000:]


def test_run_time_sources_compile_for_gfx950(tmp_path):
    """The sources hiprtc would be given: the four aggregate sinks over a BIT_XOR + BIT_AND (+ BOOL_OR) descriptor, and the projection
    and the filter sinks over & | ^."""
    f = FIELDS
    aggr = H.aggregate("Single", f, ["g"], [H.agg_of("BIT_XOR", "int64n", f, "x"), H.agg_of("BIT_AND", "uint64", f, "a"), H.agg_of("BOOL_OR", "bn", f, "o")], jit_gmax=4)
    a, b, c = col("uint64n", f), col("uint64", f), col("int8n", f)
    proj = {"op": "project", "input": {"fields": f}, "exprs": [{"expr": binary(a, Op.BitwiseAnd, b), "name": "and"}, {"expr": binary(a, Op.BitwiseOr, b), "name": "or"},
                                                               {"expr": binary(c, Op.BitwiseXor, lit(-1, "Int8")), "name": "xor"}]}
    filt = {"op": "filter", "input": {"fields": f}, "predicate": binary(binary(binary(a, Op.BitwiseXor, b), Op.BitwiseAnd, lit(2**63 + 4, "UInt64")), Op.Eq, lit(2**63 + 4, "UInt64"))}
    jobs = [("agg%d" % k, g.compile_jit_source(aggr, k)) for k in (3, 4, 12, 13)] + [("filter", g.compile_jit_source(filt, 1)), ("project", g.compile_jit_source(proj, 2))]
    assert "JIT_ACC_KIND[12] = {10,1,8,9,1" in jobs[0][1]      # the specialised LDS aggregate folds its switch over these
    assert " ^ " in jobs[5][1] and " & " in jobs[5][1] and " | " in jobs[5][1]
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        for name, rc, err in ex.map(lambda j: hipcc_device_compile(tmp_path, *j), jobs):
            assert rc == 0, (name, err)
