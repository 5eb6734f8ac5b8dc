"""APPROX_DISTINCT without a device: the accuracy of the sketch (on the numpy restatement, tests/hll_sketch.py, which the GPU tests then
hold the kernels to bit for bit), how a node that holds one is typed, what is refused and in which words, the build of the kernels, and
the estimator's host build under the sanitizers against the restatement."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import arrow_ballista_amd as g
import hll_sketch as H
from arrow_ballista_amd import binding as B
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arrow-ballista_amd", "csrc")
# four standard errors of a HyperLogLog with m registers: 4 x 1.04 / sqrt(16384) = 3.25 %
REL_BOUND = 4 * 1.04 / np.sqrt(H.M)
FAMILIES = {"arange": lambda d: np.arange(d), "random": lambda d: np.random.default_rng(7).integers(-2**62, 2**62, d), "stride": lambda d: -1000003 * np.arange(d)}


def build_module():
    spec = importlib.util.spec_from_file_location("gpuq_build", os.path.join(ROOT, "arrow-ballista_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    return build


# ------------------------------------------------------------------------------------ the restatement against the truth
@pytest.mark.parametrize("family", ["arange", "random"])
def test_small_cardinalities_are_exact(family):
    for d in range(17):
        v = FAMILIES[family](d)
        assert len(set(v.tolist())) == d
        assert H.approx_distinct(np.repeat(v, 3), "Int64") == d, d


def test_the_reference_known_answer():
    """ballista/client/src/context.rs:817-829: approx_distinct(id) over alltypes_plain is 8."""
    assert H.approx_distinct(np.array([4, 5, 6, 7, 2, 3, 0, 1], dtype=np.int32), "Int32") == 8


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("d", [1_000, 5_000, 20_000, 50_000, 100_000, 300_000, 1_000_000])
def test_relative_error_within_four_standard_errors(family, d):
    v = FAMILIES[family](d)
    exact = len(np.unique(v))
    assert exact == d
    e = H.approx_distinct(v, "Int64")
    print("%s %d: estimate %d, relative error %.4f (bound %.4f)" % (family, d, e, abs(e - d) / d, REL_BOUND))
    assert abs(e - d) / d <= REL_BOUND


def test_values_count_by_value_not_by_bytes():
    nan2 = np.array([0x7FF8000000000000, 0xFFF0000000000001], dtype=np.uint64).view(np.float64)
    assert H.approx_distinct(np.array([-0.0, 0.0, nan2[0], nan2[1]]), "Float64") == 2
    assert H.approx_distinct(np.array([-0.0, 0.0, np.nan, -np.nan, 1.0], dtype=np.float32), "Float32") == 3
    small = np.array([0, 1, 2, 100, 127, 1, 2])
    assert (H.words(small.astype(np.int8), "Int8")[0] == H.words(small.astype(np.uint8), "UInt8")[0]).all()
    assert H.words(np.array([-1], dtype=np.int8), "Int8")[0][0] == H.MASK64 and H.words(np.array([255], dtype=np.uint8), "UInt8")[0][0] == 255
    assert H.approx_distinct([10**30, 10**30 + 2**64, -10**30], "Decimal") == 3      # the high word counts
    assert H.approx_distinct(["", "a", "a\0", "fifteen bytes.."], "Utf8") == 4        # the length counts
    assert H.approx_distinct(np.arange(5), "Int64", valid=np.zeros(5, dtype=bool)) == 0


# ------------------------------------------------------------------------------------ schema and refusals
def leaf(*fields):
    """A host-only input: a schema, no data."""
    return g.MemoryExec([None], schema=[{"name": n, "type": t, "nullable": nullable} for n, t, nullable in fields])


def approx(c, s, name="d", fn="APPROX_DISTINCT", **kw):
    return dict({"fn": fn, "expr": col(c, s), "name": name}, **kw)


ARG_TYPES = ["Int8", "Int16", "Int32", "Int64", "UInt8", "UInt16", "UInt32", "UInt64", "Date32", "Date64", {"Timestamp": ["Nanosecond", None]}, {"Decimal128": [38, 4]},
             "Float32", "Float64", "Utf8"]


@pytest.mark.parametrize("arg", ARG_TYPES, ids=str)
def test_schema_is_keys_then_uint64_not_nullable(arg):
    src = leaf(("k", "Int32", False), ("s", "Utf8", True), ("v", arg, True))
    s = src.schema()
    node = g.AggregateExec("Single", [(col("s", s), "name"), (col("k", s), "k")],
                           [approx("v", s), approx("v", s, "df", fn="approx_distinct", filter=binary(col("k", s), Op.Gt, lit(3, "Int32")))], src)
    assert node.schema() == [{"name": "name", "type": "Utf8", "nullable": True}, {"name": "k", "type": "Int32", "nullable": False},
                             {"name": "d", "type": "UInt64", "nullable": False}, {"name": "df", "type": "UInt64", "nullable": False}]
    assert g.AggregateExec("Single", [], [approx("v", s)], src).schema() == [{"name": "d", "type": "UInt64", "nullable": False}]


def test_schema_of_a_node_mixing_it_with_other_aggregates():
    src = leaf(("k", "Int64", True), ("v", "Int16", True), ("d", {"Decimal128": [15, 2]}, True))
    s = src.schema()
    plain = [{"fn": "SUM", "expr": col("v", s), "name": "s"}, {"fn": "COUNT", "expr": col("v", s), "name": "c"}]
    median = {"fn": "MEDIAN", "expr": col("d", s), "name": "md"}
    mixed = [plain[0], approx("v", s, "dv"), plain[1], median, approx("d", s, "dd")]
    got = g.AggregateExec("Single", [(col("k", s), "k")], mixed, src).schema()
    alone = {f["name"]: f for f in g.AggregateExec("Single", [(col("k", s), "k")], plain, src).schema()}
    assert [f["name"] for f in got] == ["k", "s", "dv", "c", "md", "dd"]
    assert got[2] == {"name": "dv", "type": "UInt64", "nullable": False} and got[5] == {"name": "dd", "type": "UInt64", "nullable": False}
    assert got[4] == {"name": "md", "type": {"Decimal128": [15, 2]}, "nullable": True}
    assert got[0] == alone["k"] and got[1] == alone["s"] and got[3]["type"] == alone["c"]["type"]


@pytest.mark.parametrize("arg", ["Boolean"])
def test_other_argument_types_are_refused_by_name(arg):
    src = leaf(("k", "Int32", False), ("v", arg, True))
    s = src.schema()
    with pytest.raises(g.GpuqError, match="APPROX_DISTINCT over " + arg):
        g.AggregateExec("Single", [(col("k", s), "k")], [approx("v", s)], src).schema()


def test_refusals():
    src = leaf(("k", "Int32", False), ("f", "Float64", False), ("f32", "Float32", True), ("v", "Int64", True))
    s = src.schema()
    for mode in ("Partial", "Final", "FinalPartitioned"):
        with pytest.raises(g.GpuqError, match="APPROX_DISTINCT.*mode " + mode + ".*binary column.*no Binary type"):
            g.AggregateExec(mode, [(col("k", s), "k")], [approx("v", s)], src).schema()
    for key, tname in (("f", "Float64"), ("f32", "Float32")):
        with pytest.raises(g.GpuqError, match="APPROX_DISTINCT.*" + tname + " group key"):
            g.AggregateExec("Single", [(col("k", s), "k"), (col(key, s), key)], [approx("v", s)], src).schema()
    with pytest.raises(g.GpuqError, match=r"APPROX_DISTINCT\(DISTINCT"):
        g.AggregateExec("Single", [(col("k", s), "k")], [approx("v", s, distinct=True)], src).schema()
    with pytest.raises(g.GpuqError, match="DISTINCT aggregate on a node with an APPROX_DISTINCT"):
        g.AggregateExec("Single", [(col("k", s), "k")], [approx("v", s), {"fn": "COUNT", "expr": col("v", s), "name": "c", "distinct": True}], src).schema()
    # a node that also holds a MEDIAN keeps MEDIAN's words
    with pytest.raises(g.GpuqError, match="MEDIAN.*Float64 group key"):
        g.AggregateExec("Single", [(col("f", s), "f")], [approx("v", s), {"fn": "MEDIAN", "expr": col("v", s), "name": "m"}], src).schema()
    # the operator itself keeps refusing the function: it is lowered in the plan, not compiled
    with pytest.raises(g.GpuqError, match="APPROX_DISTINCT"):
        B.compile_check({"op": "aggregate", "mode": "Single", "input": {"fields": s}, "group_expr": [], "aggr_expr": [approx("v", s)]})


# ------------------------------------------------------------------------------------ the build
def test_hll_kernels_build_for_gfx950(tmp_path):
    """kernels_hll.hip is part of the library (not of the sources kept for run-time specialisation), cross-compiles for gfx950 with the
    build's flags, and uses no scratch."""
    build = build_module()
    assert "kernels_hll.hip" in build.HIP_SOURCES and "kernels_hll.hip" not in build.EMBED
    r = subprocess.run([build._hipcc(), "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, "kernels_hll.hip"), "-o", os.path.join(str(tmp_path), "kernels_hll.o"),
                        "--offload-arch=" + build.ARCH, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    build._check_scratch("kernels_hll.hip", r.stderr)
    names = set(re.findall(r"Function Name: (\S+)", r.stderr))
    for kernel in ("k_hll_sketch", "k_hll_merge_runs", "k_hll_merge"):
        assert any(kernel in n for n in names), (kernel, sorted(names))
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert scratch and max(scratch) == 0, scratch


MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "hll_estimate.h"
// one histogram per argument, "k:count,k:count,..."; prints its estimate, then hash, index and rank of a few words
int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    uint32_t* C = (uint32_t*)calloc(gpuq::HLL_BINS, sizeof(uint32_t));      // exactly 52 counters on the heap: a read past them is seen
    char* s = argv[a];
    while (*s) { const long k = strtol(s, &s, 10); ++s; const long c = strtol(s, &s, 10); if (*s == ',') ++s; C[k] = (uint32_t)c; }
    printf("%llu\n", (unsigned long long)gpuq::hll_estimate(C));
    free(C);
  }
  const uint64_t w[4][2] = {{0, 0}, {1, 0}, {0xFFFFFFFFFFFFFFFFull, 0}, {0x0123456789ABCDEFull, 0xFEDCBA9876543210ull}};
  for (int i = 0; i < 4; ++i) { const uint64_t h = gpuq::hll_hash(w[i][0], w[i][1]); printf("%llu %u %u\n", (unsigned long long)h, gpuq::hll_index(h), gpuq::hll_rho(h)); }
  return 0;
}
"""


def test_estimator_host_build_under_the_sanitizers(tmp_path):
    """csrc/hll_estimate.h as plain C++ with a main of its own, under AddressSanitizer and UndefinedBehaviorSanitizer: hand-made
    histograms (the empty sketch, a few registers, a dense sketch, the saturated ends) give the restatement's numbers."""
    build = build_module()
    src, exe = os.path.join(str(tmp_path), "hll_main.cpp"), os.path.join(str(tmp_path), "hll_main")
    with open(src, "w") as f:
        f.write(MAIN)
    r = subprocess.run([build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rng = np.random.default_rng(3)
    dense = np.bincount(H.registers(*H.words(rng.integers(-2**62, 2**62, 200_000), "Int64")), minlength=H.Q + 2)
    sparse = np.bincount(H.registers(*H.words(np.arange(9), "Int64")), minlength=H.Q + 2)
    hists = [{0: H.M}, {0: H.M - 8, 1: 4, 2: 3, 3: 1}, dict(enumerate(sparse)), dict(enumerate(dense)), {0: 1, 10: H.M - 1}, {51: H.M}, {50: H.M - 1, 51: 1}, {0: 1, 51: H.M - 1}]
    args = [",".join("%d:%d" % (k, c) for k, c in h.items() if c) for h in hists]
    out = subprocess.run([exe] + args, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.split("\n")
    want = [H.estimate_histogram([h.get(k, 0) for k in range(H.Q + 2)]) for h in hists]
    assert [int(x) for x in lines[:len(hists)]] == want
    assert want[0] == 0 and want[1] == 8 and want[2] == 9 and abs(want[3] - 200_000) <= REL_BOUND * 200_000 and want[5] == H.MASK64
    lo, hi = np.array([0, 1, H.MASK64, 0x0123456789ABCDEF], dtype=np.uint64), np.array([0, 0, 0, 0xFEDCBA9876543210], dtype=np.uint64)
    h = H.hash64(lo, hi)
    for i in range(4):
        reg = H.registers(lo[i:i + 1], hi[i:i + 1])
        assert lines[len(hists) + i].split() == [str(int(h[i])), str(int(np.flatnonzero(reg)[0])), str(int(reg.max()))]
