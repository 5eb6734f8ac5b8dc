"""DISTINCT aggregates beside plain ones and over several arguments, without a device: the restatement the GPU tests compare against
(tests/distinct_exact.py) pinned on a hand-written table, how such a node is typed (AggregateExec.schema() asks the native executor, which
lowers it in the plan), what is refused and in which words, the build of the kernels, and the row rule of the reduction folded on the
host under AddressSanitizer and UBSan."""
import importlib.util
import math
import os
import random
import re
import struct
import subprocess
from fractions import Fraction

import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd import binding as B
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit

import distinct_exact as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arrow-ballista_amd", "csrc")
REFUSED_BEFORE = "DISTINCT aggregates are not supported on device"


def leaf(*fields):
    """A host-only input: a schema, no data."""
    return g.MemoryExec([None], schema=[{"name": n, "type": t, "nullable": nullable} for n, t, nullable in fields])


def agg(fn, c, s, name, **kw):
    return dict({"fn": fn, "expr": col(c, s), "name": name}, **kw)


# ---------------------------------------------------------------- the restatement
def test_the_restatement_on_a_known_table():
    #        k    v (Int8)  f (Float64)
    rows = [("a", 5,        1.5),
            ("a", 5,        1.5),
            ("a", -3,       -0.0),
            ("a", None,     0.0),
            ("b", 127,      None),
            ("b", 127,      None),
            ("b", 1,        None),
            ("c", None,     2.0),
            ("c", None,     2.0),
            ("a", 6,        0.0),
            ("b", -128,     None),
            ("c", None,     float("nan"))]
    keys = [(r[0],) for r in rows]
    v = D.sets(keys, [r[1] for r in rows], "Int8")
    assert {k: sorted(s.values()) for k, s in v.items()} == {("a",): [-3, 5, 6], ("b",): [-128, 1, 127], ("c",): []}
    assert {k: D.count(s) for k, s in v.items()} == {("a",): 3, ("b",): 3, ("c",): 0}
    assert {k: D.total(s, "Int8") for k, s in v.items()} == {("a",): 8, ("b",): 0, ("c",): None}
    #   5 ^ -3 ^ 6 = 0b00000101 ^ 0b11111101 ^ 0b00000110 = 0b11111110 = -2;  127 ^ 1 ^ -128 = 0b01111111 ^ 1 ^ 0b10000000 = 0b11111110 = -2
    assert {k: D.bit_xor(s, "Int8") for k, s in v.items()} == {("a",): -2, ("b",): -2, ("c",): None}
    f = D.sets(keys, [r[2] for r in rows], "Float64")
    assert {k: D.count(s) for k, s in f.items()} == {("a",): 3, ("b",): 0, ("c",): 2}      # 1.5, -0.0 and 0.0; 2.0 and a NaN
    assert D.total(f[("a",)], "Float64") == (Fraction(3, 2), Fraction(3, 2), 3) and D.total(f[("b",)], "Float64") is None and math.isnan(D.total(f[("c",)], "Float64"))
    # ungrouped; wrapping at the result's width; NaNs by payload
    assert D.total(D.sets([()] * 3, [2**63 - 1, 1, 1], "Int64")[()], "Int64") == -2**63
    assert D.total(D.sets([()] * 2, [2**64 - 1, 1], "UInt64")[()], "UInt64") == 0
    assert D.total(D.sets([()] * 2, [10**38, 10**38 * 3], "Decimal")[()], "Decimal") == 4 * 10**38 - 2**128
    nan2 = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000001))[0]
    assert D.count(D.sets([()] * 3, [float("nan"), nan2, float("nan")], "Float64")[()]) == 2
    assert D.float_sum_ok(1.5, (Fraction(3, 2), Fraction(3, 2), 3)) and not D.float_sum_ok(1.5000000000000009, (Fraction(3, 2), Fraction(3, 2), 3))


# ---------------------------------------------------------------- typing
def test_schema_of_mixed_nodes():
    src = leaf(("k", "Int32", False), ("v", "Int16", True), ("u", "UInt32", True), ("d", {"Decimal128": [15, 2]}, True), ("f", "Float32", True), ("s", "Utf8", True), ("t", "Date32", True))
    s = src.schema()
    plain = [agg("SUM", "v", s, "sv"), agg("COUNT", "v", s, "n"), agg("AVG", "d", s, "ad")]
    mixed = [agg("COUNT", "v", s, "cv", distinct=True), plain[0], agg("SUM", "v", s, "dv", distinct=True), agg("SUM", "u", s, "du", distinct=True), plain[1],
             agg("SUM", "d", s, "dd", distinct=True), agg("SUM", "f", s, "df", distinct=True), agg("BIT_XOR", "v", s, "xv", distinct=True), plain[2],
             agg("MIN", "f", s, "mf", distinct=True), agg("COUNT", "s", s, "cs", distinct=True), agg("COUNT", "t", s, "ct", distinct=True),
             agg("COUNT", "v", s, "cvf", distinct=True, filter=binary(col("k", s), Op.Gt, lit(3, "Int32")))]
    got = g.AggregateExec("Single", [(col("k", s), "k")], mixed, src).schema()
    assert [f["name"] for f in got] == ["k", "cv", "sv", "dv", "du", "n", "dd", "df", "xv", "ad", "mf", "cs", "ct", "cvf"]
    by = {f["name"]: f for f in got}
    for name in ("cv", "cs", "ct", "cvf"):
        assert by[name] == {"name": name, "type": "Int64", "nullable": False}
    # SUM / BIT_XOR: the operator's type for the plain function, nullable
    alone = {f["name"]: f for f in g.AggregateExec("Single", [(col("k", s), "k")], [agg("SUM", "v", s, "dv"), agg("SUM", "u", s, "du"), agg("SUM", "d", s, "dd"), agg("SUM", "f", s, "df"),
                                                                                   agg("BIT_XOR", "v", s, "xv"), agg("MIN", "f", s, "mf")] + plain, src).schema()}
    assert [by[n]["type"] for n in ("dv", "du", "dd", "df", "xv")] == ["Int64", "UInt64", {"Decimal128": [25, 2]}, "Float64", "Int16"]
    for name in ("dv", "du", "dd", "df", "xv", "mf", "sv", "n", "ad"):
        assert by[name]["type"] == alone[name]["type"] and by[name]["nullable"] is True, name
    assert by["k"] == alone["k"]
    # ungrouped, two arguments; an all-DISTINCT node with four keys
    assert g.AggregateExec("Single", [], [agg("COUNT", "v", s, "a", distinct=True), agg("COUNT", "u", s, "b", distinct=True)], src).schema() == \
        [{"name": "a", "type": "Int64", "nullable": False}, {"name": "b", "type": "Int64", "nullable": False}]
    four = g.AggregateExec("Single", [(col(c, s), c) for c in ("k", "v", "u", "t")], [agg("COUNT", "d", s, "a", distinct=True)], src).schema()
    assert [f["name"] for f in four] == ["k", "v", "u", "t", "a"] and four[4] == {"name": "a", "type": "Int64", "nullable": False}


def test_the_two_level_rewrite_is_typed_as_before():
    """Every aggregate DISTINCT over the same argument, no filter, at most three keys: GROUP BY (keys, x), then GROUP BY keys -- the
    outer node is the plain aggregate over the deduplicated column, announced in the declared (nullable) form."""
    fields = [{"name": "k", "type": "Int32", "nullable": False}, {"name": "v", "type": "Int16", "nullable": True}]
    node = {"AggregateExec": {"input": {"MemoryExec": {"schema": fields, "partitions": [0]}}, "mode": "Single", "group_expr": [{"expr": col("k", fields), "name": "k"}],
                              "aggr_expr": [agg("COUNT", "v", fields, "c", distinct=True), agg("SUM", "v", fields, "s", distinct=True), agg("AVG", "v", fields, "a", distinct=True)]}}
    assert B.plan_schema(node) == [{"name": "k", "type": "Int32", "nullable": False}, {"name": "c", "type": "Int64", "nullable": True}, {"name": "s", "type": "Int64", "nullable": True},
                                   {"name": "a", "type": "Float64", "nullable": True}]


# ---------------------------------------------------------------- refusals
def test_refusals_name_the_function():
    src = leaf(("k", "Int32", False), ("f", "Float64", False), ("f32", "Float32", True), ("v", "Int64", True), ("w", "Int64", True), ("b", "Boolean", True),
               ("d", {"Decimal128": [10, 2]}, True), ("t", "Date32", True), ("s", "Utf8", True))
    s = src.schema()
    k = [(col("k", s), "k")]
    other = agg("SUM", "w", s, "sw")

    def refused(match, aggs, keys=k, mode="Single"):
        with pytest.raises(g.GpuqError, match=match) as e:
            g.AggregateExec(mode, keys, aggs, src).schema()
        # GPUQ_ERR_UNSUPPORTED, GPUQ_REFUSAL_NONE
        assert e.value.status == 3 and e.value.refusal == B.REFUSAL_NONE and REFUSED_BEFORE not in str(e.value), str(e.value)
    for mode in ("Partial", "Final", "FinalPartitioned"):
        refused(r"COUNT\(DISTINCT.*mode " + mode, [agg("COUNT", "v", s, "c", distinct=True), other], mode=mode)
    for key, tname in (("f", "Float64"), ("f32", "Float32")):
        refused(r"COUNT\(DISTINCT\).*" + tname + " group key", [agg("COUNT", "v", s, "c", distinct=True), other], keys=k + [(col(key, s), key)])
    for fn in ("AVG", "VARIANCE", "VARIANCE_POP", "STDDEV", "STDDEV_POP"):
        refused(fn + r"\(DISTINCT", [agg(fn, "v", s, "a", distinct=True), other])
    for fn in ("COVARIANCE", "CORRELATION"):
        refused(fn + r"\(DISTINCT", [dict(agg(fn, "v", s, "a", distinct=True), expr2=col("w", s)), other])
    refused(r"COUNT\(DISTINCT\) over Boolean", [agg("COUNT", "b", s, "c", distinct=True), other])
    refused(r"SUM\(DISTINCT\) over Boolean", [agg("SUM", "b", s, "c", distinct=True), other])
    refused(r"SUM\(DISTINCT\) over Date32", [agg("SUM", "t", s, "c", distinct=True), other])
    refused(r"SUM\(DISTINCT\) over Utf8", [agg("SUM", "s", s, "c", distinct=True), other])
    refused(r"BIT_XOR\(DISTINCT\) over Float64", [agg("BIT_XOR", "f", s, "c", distinct=True), other])
    refused(r"BIT_XOR\(DISTINCT\) over Decimal128", [agg("BIT_XOR", "d", s, "c", distinct=True), other])
    # next to a MEDIAN or an APPROX_DISTINCT: the words those functions' tests pin
    with pytest.raises(g.GpuqError, match="a DISTINCT aggregate on a node with a MEDIAN"):
        g.AggregateExec("Single", k, [agg("MEDIAN", "v", s, "m"), agg("COUNT", "v", s, "c", distinct=True)], src).schema()
    with pytest.raises(g.GpuqError, match="a DISTINCT aggregate on a node with an APPROX_DISTINCT"):
        g.AggregateExec("Single", k, [agg("APPROX_DISTINCT", "v", s, "m"), agg("COUNT", "v", s, "c", distinct=True)], src).schema()
    # the operator itself keeps refusing the flag: a node is lowered in the plan, not compiled
    with pytest.raises(g.GpuqError, match=REFUSED_BEFORE):
        B.compile_check({"op": "aggregate", "mode": "Single", "input": {"fields": s}, "group_expr": [], "aggr_expr": [agg("COUNT", "v", s, "c", distinct=True)]})


# ---------------------------------------------------------------- the build
def _build_module():
    spec = importlib.util.spec_from_file_location("gpuq_build", os.path.join(ROOT, "arrow-ballista_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    return build


def test_distinct_kernels_build_for_gfx950(tmp_path):
    """kernels_distinct.hip is part of the library (not of the sources kept for run-time specialisation), cross-compiles for gfx950 with
    the build's flags, and the build's scratch check passes on its remarks."""
    build = _build_module()
    assert "kernels_distinct.hip" in build.HIP_SOURCES and "kernels_distinct.hip" not in build.EMBED
    assert {"window_scan_dev.h", "distinct_scan_op.h"} <= set(build.HEADERS)
    r = subprocess.run([build._hipcc(), "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, "kernels_distinct.hip"), "-o", os.path.join(str(tmp_path), "kernels_distinct.o"),
                        "--offload-arch=" + build.ARCH, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    build._check_scratch("kernels_distinct.hip", r.stderr)
    names = set(re.findall(r"Function Name: (\S+)", r.stderr))
    for kernel in ("k_distinct_tile_totals", "k_window_tiles_scan", "k_distinct_downsweep", "k_distinct_valid"):
        assert any(kernel in n for n in names), (kernel, sorted(names))
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert scratch and max(scratch) == 0, scratch


def test_the_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "gpuq.h")).read()
    assert re.search(r"\bint gpuq_segment_distinct\(gpuq_ctx\* ctx, void\* stream, const gpuq_column\* value_col, const int32_t\* starts, int64_t n_groups, int64_t n_rows,", header)
    L = B.lib()
    assert L.gpuq_segment_distinct.argtypes is not None and len(L.gpuq_segment_distinct.argtypes) == 12
    r = subprocess.run(["nm", "-D", "--defined-only", B.lib_path()], capture_output=True, text=True)
    assert r.returncode == 0 and re.search(r" T gpuq_segment_distinct$", r.stdout, re.M)


# ---------------------------------------------------------------- the row rule and the scan's operator, on the host
ACC_SUM, ACC_COUNT, ACC_FSUM, ACC_BXOR = 0, 1, 5, 10      # AccKind, csrc/gpuq_kernels.h
M64, M128 = (1 << 64) - 1, (1 << 128) - 1


@pytest.fixture(scope="module")
def scan_exe(tmp_path_factory):
    """tests/distinct_scan_host.cpp, host code only, under AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded)"""
    build = _build_module()
    exe = str(tmp_path_factory.mktemp("distinct_scan") / "distinct_scan_host")
    r = subprocess.run([build._hipcc(), "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I", build.CSRC,
                        os.path.join(ROOT, "tests", "distinct_scan_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def fold(exe, kind, rows):
    """rows: [(seg_head, valid, lo, hi)] -> the three groupings' [(count, lo, hi)]"""
    text = "%d %d\n" % (kind, len(rows)) + "".join("%d %d %d %d\n" % r for r in rows)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    blocks, cur = [], []
    for line in r.stdout.split("\n"):
        if line == "-":
            blocks.append(cur)
            cur = []
        elif line:
            cur.append(tuple(int(x) for x in line.split()))
    assert len(blocks) == 3 and all(len(b) == len(rows) for b in blocks)
    return blocks


def sorted_segments(rng, draw):
    """[[value or None]] per segment: ascending, NULLs last; lengths around the 7-row tiles of the host program, runs that cross them,
    an all-NULL segment, one value repeated across three tiles, a last value equal to the next segment's first."""
    segs = []
    for length in (1, 6, 7, 8, 1, 20, 3, 13, 14, 2, 9):
        vals = sorted(draw() for _ in range(rng.randint(1, max(1, length // 2))))
        seg = sorted(rng.choice(vals) for _ in range(length))
        nulls = rng.randint(0, 2) if length > 2 else 0
        segs.append(seg[:length - nulls] + [None] * nulls)
    segs[6] = [None, None, None]
    segs[5] = [segs[5][0]] * 20
    segs[8][0] = segs[7][-1] if segs[7][-1] is not None else segs[8][0]
    segs[8] = sorted([v for v in segs[8] if v is not None]) + [None] * segs[8].count(None)
    return segs


@pytest.mark.parametrize("kind", [ACC_COUNT, ACC_SUM, ACC_BXOR, ACC_FSUM], ids=["COUNT", "SUM", "BIT_XOR", "FSUM"])
def test_three_groupings_agree_with_the_set_of_every_segment(scan_exe, kind):
    rng = random.Random(kind)
    if kind == ACC_FSUM:      # sums of small multiples of 1/4 are exact in Float64: every grouping must give the same bits
        draw = lambda: rng.randint(-40, 40) / 4.0
        words = lambda v: (struct.unpack("<Q", struct.pack("<d", v))[0], 0)
    else:                     # 128-bit two's complement, near the ends of the range: sums wrap
        draw = lambda: rng.choice([rng.randint(-5, 5), rng.randint(-2**127, -2**127 + 5), rng.randint(2**127 - 6, 2**127 - 1), rng.randint(-2**64, 2**64)])
        words = lambda v: ((v & M128) & M64, (v & M128) >> 64)
    segs = sorted_segments(rng, draw)
    rows, last = [], []
    for seg in segs:
        for i, v in enumerate(seg):
            rows.append((1 if i == 0 else 0, 0 if v is None else 1) + (words(v) if v is not None else (0, 0)))
        last.append(len(rows) - 1)
    blocks = fold(scan_exe, kind, rows)
    for seg, at in zip(segs, last):
        if kind == ACC_FSUM:
            s = D.sets([()] * len(seg), seg, "Float64")[()]
            n, exact = D.count(s), D.total(s, "Float64")
            want = (n, struct.unpack("<Q", struct.pack("<d", float(exact[0])))[0], 0) if n else None
        else:
            s = D.sets([()] * len(seg), seg, "Decimal")[()]
            n = D.count(s)
            if kind == ACC_COUNT:
                want = (n, n, 0)
            elif kind == ACC_SUM:
                want = (n,) + words(D.total(s, "Decimal")) if n else None
            else:
                x = 0
                for v in s.values():
                    x ^= v & M64
                want = (n, x, None)
        for b in blocks:
            got = b[at]
            assert got[0] == n, (seg, got)
            if n and kind != ACC_COUNT:
                assert got[1] == want[1] and (want[2] is None or got[2] == want[2]), (seg, got, want)
    assert blocks[0] == blocks[1] == blocks[2] or kind == ACC_BXOR      # (the unused high word of a bitwise cell is not part of the result)
