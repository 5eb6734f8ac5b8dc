"""CPU: what the compile makes of the scalar functions coalesce, nullif, nanvl, isnan, iszero, abs, signum, ceil, floor, trunc, round,
sqrt, without a device.  Output type and nullability for every function x legal argument type x nullability;
every refusal by its message; the run-time sources of projections and a filter that together use every function
cross-compile for gfx950 (the command line of tools/jit_compile_check.py); and the resource guard: no kernel of the three files that hold
the interpreter has a lower occupancy than tests/golden/interpreter_kernel_resources.json records for the commit before these opcodes."""
import concurrent.futures
import json
import os
import re
import subprocess

import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd import expr as E
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, cast, col, lit, scalar_function

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arrow-ballista_amd", "csrc")

INTS = ["Int8", "Int16", "Int32", "Int64", "UInt8", "UInt16", "UInt32", "UInt64"]
FLOATS = ["Float32", "Float64"]
DEC = {"Decimal128": [38, 4]}
TS = {"Timestamp": ["Nanosecond", None]}
OTHERS = [("dec", DEC, "Decimal128(38,4)"), ("d32", "Date32", "Date32"), ("d64", "Date64", "Date64"), ("ts", TS, None), ("b", "Boolean", "Boolean"), ("s", "Utf8", "Utf8")]
# every type twice: NAME required, NAMEn nullable (and NAMEm, a second nullable column of the type)
FIELDS = []
for _t in INTS + FLOATS:
    FIELDS += [{"name": _t.lower(), "type": _t, "nullable": False}, {"name": _t.lower() + "n", "type": _t, "nullable": True}, {"name": _t.lower() + "m", "type": _t, "nullable": True}]
for _n, _t, _ in OTHERS:
    FIELDS += [{"name": _n, "type": _t, "nullable": False}, {"name": _n + "n", "type": _t, "nullable": True}, {"name": _n + "m", "type": _t, "nullable": True}]
FIELDS.append({"name": "dec152", "type": {"Decimal128": [15, 2]}, "nullable": False})


def c(name):
    return col(name, FIELDS)


def project(*es):
    return {"op": "project", "input": {"fields": FIELDS}, "exprs": [{"expr": e, "name": "x%d" % i} for i, e in enumerate(es)]}


def outputs(*es):
    """[(type, nullable)] of a projection of es."""
    return [(o["type"], bool(o["nullable"])) for o in g.compile_check(project(*es))["outputs"]]


def shown(name):
    """The type of column `name` as the compile prints it."""
    return outputs(c(name))[0][0]


def refusal(e):
    with pytest.raises(g.GpuqError) as err:
        g.compile_check(project(e))
    return str(err.value)


ALL_TYPES = [t.lower() for t in INTS + FLOATS] + [n for n, _, _ in OTHERS]


def test_coalesce_types_and_nullability():
    for t in ALL_TYPES:
        req, n1, n2 = c(t), c(t + "n"), c(t + "m")
        ty = shown(t)
        assert outputs(E.coalesce(req), E.coalesce(n1), E.coalesce(n1, n2), E.coalesce(n1, req), E.coalesce(n1, n2, n1, n2), E.coalesce(n1, n2, req, n1),
                       E.coalesce(n1, lit(None))) == [(ty, False), (ty, True), (ty, True), (ty, False), (ty, True), (ty, False), (ty, True)], t
    # a literal ends the list like any argument that cannot be NULL
    assert outputs(E.coalesce(c("int32n"), lit(-1, "Int32"))) == [("Int32", False)]
    assert outputs(scalar_function("COALESCE", [c("sn"), lit("none")])) == [("Utf8", False)]


def test_nullif_types_and_nullability():
    for t in ALL_TYPES:
        ty = shown(t)
        assert outputs(E.nullif(c(t), c(t)), E.nullif(c(t), c(t + "n")), E.nullif(c(t + "n"), c(t)), E.nullif(c(t + "n"), c(t + "m")),
                       E.nullif(c(t), lit(None))) == [(ty, True)] * 5, t
    assert outputs(E.nullif(c("dec"), lit(0, ("Decimal128", 38, 4)))) == [("Decimal128(38,4)", True)]


def test_float_tests_and_nanvl():
    for t in ("float32", "float64"):
        ty = shown(t)
        assert outputs(E.isnan(c(t)), E.isnan(c(t + "n")), E.iszero(c(t)), E.iszero(c(t + "n"))) == [("Boolean", False), ("Boolean", True)] * 2, t
        assert outputs(E.nanvl(c(t), c(t)), E.nanvl(c(t + "n"), c(t)), E.nanvl(c(t), c(t + "n")), E.nanvl(c(t + "n"), c(t + "m"))) == [(ty, False), (ty, True), (ty, True), (ty, True)], t


def test_abs_keeps_the_type():
    for t in [x.lower() for x in INTS + FLOATS] + ["dec", "dec152"]:
        ty = shown(t)
        assert outputs(E.abs_(c(t))) == [(ty, False)], t
        if t != "dec152":
            assert outputs(E.abs_(c(t + "n"))) == [(ty, True)], t
    # an unsigned integer's abs is the column itself: no instruction beyond the load (UInt64: its zero-extension)
    assert len(g.compile_check(project(E.abs_(c("uint16"))))["program"]["insns"]) == 0
    # a float's abs is one AND of the re-typed pattern with an immediate
    assert len(g.compile_check(project(E.abs_(c("float64n"))))["program"]["insns"]) == 2


ROUNDING = [E.ceil, E.floor, E.trunc, E.round_, E.sqrt, E.signum, lambda x: E.round_(x, 0), lambda x: E.round_(x, 2), lambda x: E.round_(x, 22)]


def test_rounding_sign_and_sqrt_give_the_float_type():
    for fn in ROUNDING:
        for t in FLOATS:
            assert outputs(fn(c(t.lower())), fn(c(t.lower() + "n"))) == [(t, False), (t, True)], t
        for t in INTS:      # an integer argument is cast to Float64 first
            assert outputs(fn(c(t.lower())), fn(c(t.lower() + "n"))) == [("Float64", False), ("Float64", True)], t
    # the integral results need no rounding to Float32 behind them: load, one instruction
    for fn in (E.ceil, E.floor, E.trunc):
        assert len(g.compile_check(project(fn(c("float32n"))))["program"]["insns"]) == 1
    # round(x) and round(x, 0) are one program, and neither rounds to Float32 behind the integral result
    r1, r0 = (g.compile_check(project(fn(c("float32n"))))["program"] for fn in (E.round_, lambda x: E.round_(x, 0)))
    assert r1 == r0 and len(r1["insns"]) < len(g.compile_check(project(E.round_(c("float32n"), 1)))["program"]["insns"])
    # round(x, n): an integer literal of any integer type
    assert outputs(E.scalar_function("round", [c("float64"), lit(3, "Int32")]), E.scalar_function("round", [c("float64"), lit(3, "UInt8")])) == [("Float64", False)] * 2


def test_the_shifts_stay_refused():
    """<< and >> are not built (tests/test_cpu_bitwise.py pins the same refusal)."""
    for shift in ("<<", ">>", "BitwiseShiftLeft", "BitwiseShiftRight"):
        assert "unsupported binary operator '%s'" % shift in refusal(binary(c("int32"), shift, c("int32")))


def test_names_are_matched_without_case():
    for spelled, e in (("Coalesce", E.coalesce(c("int8n"), c("int8"))), ("NULLIF", E.nullif(c("sn"), c("s"))), ("NaNvl", E.nanvl(c("float32n"), c("float32"))),
                       ("IsNaN", E.isnan(c("float64"))), ("ISZERO", E.iszero(c("float64"))), ("Abs", E.abs_(c("dec"))), ("SIGNUM", E.signum(c("int32"))), ("Ceil", E.ceil(c("float64"))),
                       ("FLOOR", E.floor(c("float64"))), ("Trunc", E.trunc(c("float64"))), ("ROUND", E.round_(c("float64n"), 2)), ("Sqrt", E.sqrt(c("float32")))):
        other = {"scalar_function": dict(e["scalar_function"], name=spelled)}
        assert json.dumps(g.compile_check(project(other)), sort_keys=True) == json.dumps(g.compile_check(project(e)), sort_keys=True), spelled


def test_refusals_by_message():
    assert "coalesce over mixed types Int32, Int64" in refusal(E.coalesce(c("int32n"), c("int64")))
    assert "coalesce over mixed types Decimal128(38,4), Decimal128(15,2)" in refusal(E.coalesce(c("decn"), c("dec152")))
    assert "coalesce over mixed types Float32, Float64" in refusal(E.coalesce(c("float32n"), lit(0.0)))
    assert "round(x, n): n outside 0..22" in refusal(E.round_(c("float64"), 23))
    assert "round(x, n): n outside 0..22" in refusal(E.round_(c("float64"), -1))
    assert "round(x, n): n must be a non-NULL integer literal" in refusal(scalar_function("round", [c("float64"), c("int64")]))
    assert "round(x, n): n must be a non-NULL integer literal" in refusal(scalar_function("round", [c("float64"), lit(2.0)]))
    assert "n must be a non-NULL literal" in refusal(scalar_function("round", [c("float64"), lit(None, "Int64")]))
    for fn in ("ceil", "floor", "trunc", "round", "sqrt", "signum"):      # a decimal arrives under the plan's cast to Float64
        assert fn + " over Decimal128(38,4)" in refusal(scalar_function(fn, [c("dec")])), fn
        assert outputs(scalar_function(fn, [cast(c("decn"), "Float64")])) == [("Float64", True)], fn
        assert fn + " over Utf8" in refusal(scalar_function(fn, [c("s")])), fn
    for fn in ("isnan", "iszero"):
        assert fn + " over Int32" in refusal(scalar_function(fn, [c("int32")])), fn
        assert fn + " over Decimal128(38,4)" in refusal(scalar_function(fn, [c("dec")])), fn
    assert "nanvl over Decimal128(38,4)" in refusal(E.nanvl(c("dec"), c("dec")))
    assert "nanvl over Float64, Float32" in refusal(E.nanvl(c("float64"), c("float32")))
    assert "abs over Utf8" in refusal(E.abs_(c("s")))
    assert "abs over Date32" in refusal(E.abs_(c("d32")))
    assert "abs over Boolean" in refusal(E.abs_(c("b")))
    assert "nullif over Int32, Int64" in refusal(E.nullif(c("int32"), c("int64")))
    # what is still not built says what is
    for fn in ("ln", "exp", "power", "sin", "log10", "upper", "date_trunc"):
        msg = refusal(scalar_function(fn, [c("float64")]))
        assert "scalar function '%s' is not built on the device" % fn in msg
        for built in ("date_part", "substr", "coalesce", "nullif", "nanvl", "isnan", "iszero", "abs", "signum", "ceil", "floor", "trunc", "round", "sqrt"):
            assert built in msg, (fn, built)
    # argument counts
    assert "nullif takes (a, b)" in refusal(scalar_function("nullif", [c("int32")]))
    assert "trunc takes (x)" in refusal(scalar_function("trunc", [c("float64"), lit(2)]))
    assert "coalesce takes" in refusal(scalar_function("coalesce", []))


def test_every_operator_takes_the_functions():
    """Aggregate arguments and group keys, join filters and keys, sort keys: the compile of each operator accepts them (no layer of its own)."""
    f = FIELDS
    d = g.compile_check({"op": "aggregate", "mode": "Single", "input": {"fields": f}, "group_expr": [{"expr": E.coalesce(c("int32n"), lit(-1, "Int32")), "name": "k"}],
                         "aggr_expr": [{"fn": "SUM", "expr": E.round_(c("float64n"), 2), "name": "s"}, {"fn": "MAX", "expr": E.abs_(c("int64")), "name": "m"}]})
    assert [(o["name"], o["type"], bool(o["nullable"])) for o in d["outputs"]] == [("k", "Int32", False), ("s", "Float64", True), ("m", "Int64", False)]
    g.compile_check({"op": "filter", "input": {"fields": f}, "predicate": binary(E.abs_(c("float64n")), Op.Lt, lit(0.5))})
    g.compile_check({"op": "sort", "input": {"fields": f}, "expr": [{"expr": E.abs_(c("int32n")), "asc": True, "nulls_first": False}, {"expr": E.floor(c("float64")), "asc": False, "nulls_first": True}]})
    g.compile_check({"op": "join_build", "input": {"fields": f}, "on": [E.coalesce(c("int64n"), lit(0))], "predicate": E.iszero(c("float64"))})
    g.compile_check({"op": "join_probe", "input": {"fields": f}, "on": [E.abs_(c("int64n"))], "predicate": binary(E.signum(c("float64n")), Op.Gt, lit(0.0)), "join_type": "Inner"})
    g.compile_check({"op": "partition", "input": {"fields": f}, "hash_expr": [E.coalesce(c("uint32n"), c("uint32"))], "partition_count": 8})


# ------------------------------------------------------------------------------------ cross-compiles (no device)
def hipcc_device(tmp_path, name, path_or_text, is_file=False):
    f = path_or_text
    if not is_file:
        f = os.path.join(str(tmp_path), name + ".hip")
        with open(f, "w") as fh:
            fh.write(path_or_text)
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", "-x", "hip", f, "-Rpass-analysis=kernel-resource-usage",
                        "-I", CSRC, "-o", os.path.join(str(tmp_path), name + ".o")], capture_output=True, text=True)
    return name, r.returncode, r.stderr


def test_run_time_sources_compile_for_gfx950(tmp_path):
    """The sources hiprtc would be given: four projections and a filter that together use every function."""
    ps = [project(E.round_(E.sqrt(E.abs_(c("float64n"))), 2), E.round_(E.abs_(c("float32n")), 22)),
          project(E.coalesce(E.nullif(c("int32n"), c("int32")), E.abs_(c("int32n")), c("int32")), E.signum(c("float32n")), E.abs_(c("decn"))),
          project(E.nanvl(E.floor(c("float64n")), E.ceil(c("float64m"))), E.trunc(c("float32")), E.round_(c("int16n")), E.coalesce(c("sn"), c("sm"), lit("none"))),
          project(E.nullif(c("float64n"), c("float64")), E.abs_(c("int8n")), E.sqrt(c("float32n")), E.abs_(c("uint64n")))]
    flt = {"op": "filter", "input": {"fields": FIELDS}, "predicate": E.or_(
        E.and_(E.not_(E.isnan(c("float64n"))), binary(E.abs_(c("float64n")), Op.Lt, lit(0.5))), E.iszero(E.trunc(c("float32n"))),
        binary(E.coalesce(c("int64n"), c("int64")), Op.Eq, lit(3)), binary(E.signum(c("int8")), Op.Gt, lit(0.0)))}
    jobs = [("project%d" % i, g.compile_jit_source(p, 2)) for i, p in enumerate(ps)] + [("filter", g.compile_jit_source(flt, 1))]
    text = "\n".join(t for _, t in jobs)
    for word in ("floor(", "ceil(", "trunc(", "sqrt(", "__double_as_longlong(", "__longlong_as_double("):
        assert word in text, word
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        for name, rc, err in ex.map(lambda j: hipcc_device(tmp_path, *j), jobs):
            assert rc == 0, (name, err[-3000:])


def kernel_resources(remarks):
    """{kernel: {"vgprs", "occupancy", "scratch"}} from -Rpass-analysis=kernel-resource-usage remarks."""
    out, name = {}, None
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def test_resource_guard(tmp_path):
    """run_program is one inlined switch: every interpreter kernel pays the registers of its most expensive case.  The three kernel
    files are compiled as the build compiles them; no kernel may have a lower occupancy than the commit before the new opcodes had (the
    golden file, recorded from that commit with this function), and the build's own scratch check passes on the remarks."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gpuq_build", os.path.join(ROOT, "arrow-ballista_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    with open(os.path.join(ROOT, "tests", "golden", "interpreter_kernel_resources.json")) as fh:
        before = json.load(fh)
    files = ["kernels_scan.hip", "kernels_hash.hip", "kernels_sort.hip"]
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(files)) as ex:
        results = list(ex.map(lambda f: hipcc_device(tmp_path, f[:-4], os.path.join(CSRC, f), True), files))
    seen = 0
    for name, rc, err in results:
        assert rc == 0, (name, err[-3000:])
        build._check_scratch(name, err)
        now = kernel_resources(err)
        for kernel, was in before[name].items():
            assert kernel in now, (name, kernel)
            print("%s %s: VGPRs %d -> %d, occupancy %d -> %d" % (name, kernel, was["vgprs"], now[kernel]["vgprs"], was["occupancy"], now[kernel]["occupancy"]))
            assert now[kernel]["occupancy"] >= was["occupancy"], (name, kernel, was, now[kernel])
            seen += 1
    assert seen >= 20
