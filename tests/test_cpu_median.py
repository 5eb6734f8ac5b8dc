"""MEDIAN without a device: how a node that holds one is typed (AggregateExec.schema() asks the native executor, which lowers MEDIAN in
the plan and never hands it to the aggregate operator), what is refused and in which words, and the build of the segment kernels."""
import importlib.util
import os
import re
import subprocess

import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd import binding as B
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arrow-ballista_amd", "csrc")
ARG_TYPES = ["Int8", "Int16", "Int32", "Int64", "UInt8", "UInt16", "UInt32", "UInt64", "Float32", "Float64", {"Decimal128": [38, 4]}]


def leaf(*fields):
    """A host-only input: a schema, no data."""
    return g.MemoryExec([None], schema=[{"name": n, "type": t, "nullable": nullable} for n, t, nullable in fields])


def median(c, s, name="m", **kw):
    return dict({"fn": "MEDIAN", "expr": col(c, s), "name": name}, **kw)


@pytest.mark.parametrize("arg", ARG_TYPES, ids=str)
def test_schema_is_keys_then_the_arguments_type_nullable(arg):
    src = leaf(("k", "Int32", False), ("s", "Utf8", True), ("v", arg, False))
    s = src.schema()
    node = g.AggregateExec("Single", [(col("s", s), "name"), (col("k", s), "k")], [median("v", s), median("v", s, "mf", filter=binary(col("k", s), Op.Gt, lit(3, "Int32")))], src)
    assert node.schema() == [{"name": "name", "type": "Utf8", "nullable": True}, {"name": "k", "type": "Int32", "nullable": False},
                             {"name": "m", "type": arg, "nullable": True}, {"name": "mf", "type": arg, "nullable": True}]
    # ungrouped: the MEDIANs alone
    assert g.AggregateExec("Single", [], [median("v", s)], src).schema() == [{"name": "m", "type": arg, "nullable": True}]


def test_schema_of_a_node_mixing_median_with_other_aggregates():
    src = leaf(("k", "Int64", True), ("v", "Int16", True), ("d", {"Decimal128": [15, 2]}, True))
    s = src.schema()
    plain = [{"fn": "SUM", "expr": col("v", s), "name": "s"}, {"fn": "COUNT", "expr": col("v", s), "name": "c"}, {"fn": "AVG", "expr": col("d", s), "name": "a"}]
    mixed = [plain[0], median("v", s, "mv"), plain[1], median("d", s, "md"), plain[2]]
    got = g.AggregateExec("Single", [(col("k", s), "k")], mixed, src).schema()
    # the plain columns: as the node without its MEDIANs announces them
    alone = {f["name"]: f for f in g.AggregateExec("Single", [(col("k", s), "k")], plain, src).schema()}
    assert [f["name"] for f in got] == ["k", "s", "mv", "c", "md", "a"]
    assert got[2] == {"name": "mv", "type": "Int16", "nullable": True} and got[4] == {"name": "md", "type": {"Decimal128": [15, 2]}, "nullable": True}
    for f in got:
        if f["name"] in alone and f["name"] != "k":
            assert f["type"] == alone[f["name"]]["type"] and f["nullable"] is True
    assert got[0] == alone["k"]


@pytest.mark.parametrize("arg", ["Date32", "Utf8", "Boolean"])
def test_other_argument_types_are_refused_by_name(arg):
    src = leaf(("k", "Int32", False), ("v", arg, True))
    s = src.schema()
    with pytest.raises(g.GpuqError, match="MEDIAN over " + arg):
        g.AggregateExec("Single", [(col("k", s), "k")], [median("v", s)], src).schema()


def test_refusals():
    src = leaf(("k", "Int32", False), ("f", "Float64", False), ("f32", "Float32", True), ("v", "Int64", True))
    s = src.schema()
    for mode in ("Partial", "Final", "FinalPartitioned"):
        with pytest.raises(g.GpuqError, match="MEDIAN.*mode " + mode):
            g.AggregateExec(mode, [(col("k", s), "k")], [median("v", s)], src).schema()
    for key, tname in (("f", "Float64"), ("f32", "Float32")):
        with pytest.raises(g.GpuqError, match="MEDIAN.*" + tname + " group key"):
            g.AggregateExec("Single", [(col("k", s), "k"), (col(key, s), key)], [median("v", s)], src).schema()
    with pytest.raises(g.GpuqError, match="MEDIAN"):
        g.AggregateExec("Single", [(col("k", s), "k")], [median("v", s, distinct=True)], src).schema()
    with pytest.raises(g.GpuqError, match="MEDIAN"):
        g.AggregateExec("Single", [(col("k", s), "k")], [median("v", s), {"fn": "COUNT", "expr": col("v", s), "name": "c", "distinct": True}], src).schema()
    # the approximate ones are t-digest answers, not this one: still unknown functions
    for fn in ("APPROX_MEDIAN", "APPROX_PERCENTILE_CONT"):
        with pytest.raises(g.GpuqError):
            g.AggregateExec("Single", [(col("k", s), "k")], [{"fn": fn, "expr": col("v", s), "name": "m"}], src).schema()
    # the operator itself keeps refusing MEDIAN: it is lowered in the plan, not compiled
    with pytest.raises(g.GpuqError):
        B.compile_check({"op": "aggregate", "mode": "Single", "input": {"fields": s}, "group_expr": [], "aggr_expr": [median("v", s)]})


def test_segment_kernels_build_for_gfx950(tmp_path):
    """kernels_segment.hip is part of the library (not of the sources kept for run-time specialisation), cross-compiles for gfx950 with
    the build's flags, and the build's scratch check passes on its remarks."""
    spec = importlib.util.spec_from_file_location("gpuq_build", os.path.join(ROOT, "arrow-ballista_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "kernels_segment.hip" in build.HIP_SOURCES and "kernels_segment.hip" not in build.EMBED
    r = subprocess.run([build._hipcc(), "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, "kernels_segment.hip"), "-o", os.path.join(str(tmp_path), "kernels_segment.o"),
                        "--offload-arch=" + build.ARCH, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    build._check_scratch("kernels_segment.hip", r.stderr)
    names = set(re.findall(r"Function Name: (\S+)", r.stderr))
    for kernel in ("k_segment_heads", "k_segment_starts", "k_segment_median"):
        assert any(kernel in n for n in names), (kernel, sorted(names))
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert scratch and max(scratch) == 0, scratch
