"""BoundedWindowAggExec without a device: the restatement the GPU tests compare against pinned on a table with known answers, how the
node is typed (gpuq_plan_schema through plan.BoundedWindowAggExec.schema()), what it refuses and in which words, the build of the
window kernels, and the scan's operator (csrc/window_scan_op.h) folded on the host under AddressSanitizer / UBSan in three groupings.

Two refusals of the node need a device and are GPU tests (tests/test_gpu_window.py): partition_by / order_by strings beyond 15 bytes,
and 2^31 rows in a partition of the plan, which the four entry points refuse before they look at a pointer."""
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
from arrow_ballista_amd import expr as E
from arrow_ballista_amd.expr import col, lit

import window_exact as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arrow-ballista_amd", "csrc")
TS = {"Timestamp": ["Microsecond", None]}
INTS = ["Int8", "Int16", "Int32", "Int64", "UInt8", "UInt16", "UInt32", "UInt64"]
ARG_TYPES = INTS + ["Float32", "Float64", {"Decimal128": [38, 4]}, {"Decimal128": [12, 2]}, "Date32", TS]


def leaf(*fields):
    """A host-only input: a schema, no data."""
    return g.MemoryExec([None], schema=[{"name": n, "type": t, "nullable": nullable} for n, t, nullable in fields])


SRC = leaf(("k", "Int32", True), ("o", "Int64", False), ("v", "Int32", True), ("f", "Float64", True), ("f32", "Float32", True), ("s", "Utf8", True), ("b", "Boolean", True),
           ("d", {"Decimal128": [12, 2]}, True))
OVER = dict(partition_by=[col("k")], order_by=[E.sort_expr(col("o"))])


# ---------------------------------------------------------------- the restatement, on a table whose answers were written down by hand
KNOWN = {"k": [1, 1, 1, 1, 1, 2, 2, 2, None, None, 3, 3],
         "o": [1, 1, 2, 3, 3, 1, 2, 2, 1, 1, 5, 6],
         "v": [5, None, 3, -2, 7, None, None, 4, 10, 20, 1, 2]}
N_ = None


def test_the_restatement_on_a_known_table():
    w = W.Walk(KNOWN, ["k"], ["o"])
    assert w.row_number() == [1, 2, 3, 4, 5, 1, 2, 3, 1, 2, 1, 2]
    assert w.rank() == [1, 1, 3, 4, 4, 1, 2, 2, 1, 1, 1, 2]
    assert w.dense_rank() == [1, 1, 2, 3, 3, 1, 2, 2, 1, 1, 1, 2]
    assert w.shift("v", -1) == [N_, 5, N_, 3, -2, N_, N_, N_, N_, 10, N_, 1]                      # LAG(v, 1): a NULL value is a value
    assert w.shift("v", 2, -1) == [3, -2, 7, -1, -1, 4, -1, -1, -1, -1, -1, -1]                    # LEAD(v, 2, -1)
    assert w.shift("v", 0) == KNOWN["v"]
    assert w.count("v", "range") == [1, 1, 2, 4, 4, 0, 1, 1, 2, 2, 1, 2]
    assert w.count("v", "rows") == [1, 1, 2, 3, 4, 0, 0, 1, 1, 2, 1, 2]
    assert w.sum("v", "range") == [5, 5, 8, 13, 13, N_, 4, 4, 30, 30, 1, 3]
    assert w.sum("v", "rows") == [5, 5, 8, 6, 13, N_, N_, 4, 10, 30, 1, 3]
    assert w.minmax("v", True, "rows") == [5, 5, 3, -2, -2, N_, N_, 4, 10, 10, 1, 1]
    assert w.minmax("v", False, "range") == [5, 5, 5, 7, 7, N_, 4, 4, 20, 20, 1, 2]
    assert w.sum("v", (1, 1)) == [5, 8, 1, 8, 5, N_, 4, 4, 30, 30, 3, 3]
    assert w.count("v", (None, 1)) == [1, 2, 3, 4, 4, 0, 1, 1, 2, 2, 2, 2]
    assert w.sum("v", (0, 0)) == [5, N_, 3, -2, 7, N_, N_, 4, 10, 20, 1, 2]
    assert w.sum("v", (10 ** 6, 10 ** 6)) == [13] * 5 + [4] * 3 + [30] * 2 + [3] * 2
    avg = w.sum_exact("v", "rows")
    assert avg[3] == (Fraction(6), Fraction(10), 3) and avg[5] is None and avg[4][0] / avg[4][2] == Fraction(13, 4)
    assert w.avg_decimal("v", "rows", 1) == [50, 50, 40, 20, 32, N_, N_, 40, 100, 150, 10, 15]
    assert W.Walk({"v": [-7, 2]}).avg_decimal("v", "rows", 0) == [-7, -2]                          # -5 / 2 truncates toward zero
    # no partition_by: one partition; no order_by: every row of a partition is a peer
    assert W.Walk(KNOWN, [], ["o"]).row_number() == list(range(1, 13))
    assert W.Walk(KNOWN, ["k"], []).sum("v", "range") == [13] * 5 + [4] * 3 + [30] * 2 + [3] * 2
    assert W.Walk(KNOWN, ["k"], []).rank() == [1] * 12
    # fixed widths wrap
    assert W.wrap(200, 8) == -56 and W.wrap(200, 8, signed=False) == 200 and W.wrap(-1, 64, signed=False) == 2 ** 64 - 1
    assert W.Walk({"v": [2 ** 63 - 1, 1, -5]}).sum("v", "rows") == [2 ** 63 - 1, -2 ** 63, -2 ** 63 - 5 + 2 ** 64]


# ---------------------------------------------------------------- typing
def agg_type(fn, arg):
    """the type the aggregate operator gives `fn` over `arg` in mode Single (one AGG_FNS row)"""
    src = leaf(("x", arg, True))
    return g.AggregateExec("Single", [], [{"fn": fn, "expr": col("x", src.schema()), "name": "r"}], src).schema()[0]["type"]


@pytest.mark.parametrize("arg", ARG_TYPES, ids=str)
def test_schema_of_every_function_over_every_argument_type(arg):
    src = leaf(("k", "Utf8", True), ("o", "Int64", False), ("x", arg, True))
    over = dict(partition_by=[col("k")], order_by=[E.sort_expr(col("o"), asc=False)])
    summable = arg not in ("Date32", TS)
    w = [E.window("ROW_NUMBER", [], "rn", **over), E.window("rank", [], "rk", **over), E.window("Dense_Rank", [], "dr", **over),
         E.lag(col("x"), "lag", **over), E.lead(col("x"), "lead", 3, **over), E.window("COUNT", [col("x")], "c", **over),
         E.window("MIN", [col("x")], "mn", **over), E.window("MAX", [col("x")], "mx", frame=E.rows_between(None, 0), **over)]
    if summable:
        w += [E.window("SUM", [col("x")], "s", **over), E.window("AVG", [col("x")], "a", frame=E.rows_between(None, 0), **over)]
    got = g.BoundedWindowAggExec(src, w).schema()
    assert got[:3] == src.schema()
    want = [("rn", "UInt64", False), ("rk", "UInt64", False), ("dr", "UInt64", False), ("lag", arg, True), ("lead", arg, True), ("c", "Int64", False), ("mn", arg, True), ("mx", arg, True)]
    if summable:
        want += [("s", agg_type("SUM", arg), True), ("a", agg_type("AVG", arg), True)]
    assert got[3:] == [{"name": n, "type": t, "nullable": nl} for n, t, nl in want]
    if not summable:
        for fn in ("SUM", "AVG"):
            with pytest.raises(g.GpuqError, match=fn + " over "):
                g.BoundedWindowAggExec(src, [E.window(fn, [col("x")], "s", **over)]).schema()


def test_schema_known_types():
    src = leaf(("k", "Int32", False), ("i", "Int32", True), ("d", {"Decimal128": [12, 2]}, False), ("u", "UInt16", True), ("f", "Float32", True), ("s", "Utf8", True))
    w = [E.window("SUM", [col("i")], "si", **OVER_K), E.window("SUM", [col("d")], "sd", **OVER_K), E.window("SUM", [col("u")], "su", **OVER_K), E.window("SUM", [col("f")], "sf", **OVER_K),
         E.window("AVG", [col("i")], "ai", **OVER_K), E.window("AVG", [col("d")], "ad", **OVER_K), E.window("COUNT", [col("s")], "cs", **OVER_K),
         E.window("SUM", [col("i")], "sl", frame=E.rows_between(3, 2), **OVER_K), E.lag(col("d"), "ld", 2, lit(5, ("Decimal128", 12, 2)), **OVER_K)]
    got = {f["name"]: (f["type"], f["nullable"]) for f in g.BoundedWindowAggExec(src, w).schema()[6:]}
    assert got == {"si": ("Int64", True), "sd": ({"Decimal128": [22, 2]}, True), "su": ("UInt64", True), "sf": ("Float64", True), "ai": ("Float64", True),
                   "ad": ({"Decimal128": [16, 6]}, True), "cs": ("Int64", False), "sl": ("Int64", True), "ld": ({"Decimal128": [12, 2]}, True)}
    assert got["sd"][0] == agg_type("SUM", {"Decimal128": [12, 2]})


OVER_K = dict(partition_by=[col("k")], order_by=[])


# ---------------------------------------------------------------- refusals
def frame(units, s, e):
    return E.window_frame(units, E.frame_bound(*s), E.frame_bound(*e))


REFUSED = {
    "end UNBOUNDED FOLLOWING": ([E.window("SUM", [col("v")], "x", frame=frame("ROWS", ("PRECEDING",), ("FOLLOWING",)), **OVER)], {}, r"SUM.*ROWS UNBOUNDED PRECEDING \.\. UNBOUNDED FOLLOWING"),
    "start FOLLOWING": ([E.window("COUNT", [col("v")], "x", frame=frame("ROWS", ("FOLLOWING", 1), ("FOLLOWING", 2)), **OVER)], {}, r"COUNT.*ROWS 1 FOLLOWING \.\. 2 FOLLOWING.*start bound of FOLLOWING"),
    "RANGE with an offset": ([E.window("AVG", [col("v")], "x", frame=frame("RANGE", ("PRECEDING", 1), ("CURRENT_ROW",)), **OVER)], {}, r"AVG.*RANGE 1 PRECEDING \.\. CURRENT ROW.*numeric offset"),
    "GROUPS": ([E.window("SUM", [col("v")], "x", frame=frame("GROUPS", ("PRECEDING",), ("CURRENT_ROW",)), **OVER)], {}, r"SUM.*GROUPS"),
    "mode Linear": ([E.window("SUM", [col("v")], "x", **OVER)], {"partition_search_mode": "Linear"}, r"partition_search_mode Linear"),
    "mode PartiallySorted": ([E.window("SUM", [col("v")], "x", **OVER)], {"partition_search_mode": "PartiallySorted"}, r"partition_search_mode PartiallySorted"),
    "two partition_bys": ([E.window("SUM", [col("v")], "x", **OVER), E.window("MAX", [col("v")], "y", partition_by=[col("o")], order_by=OVER["order_by"])], {}, r"'y' \(MAX\) differs.*partition_by or order_by"),
    "two order_bys": ([E.window("SUM", [col("v")], "x", **OVER), E.window("RANK", [], "y", partition_by=[col("k")], order_by=[E.sort_expr(col("o"), asc=False)])], {}, r"'y' \(RANK\) differs"),
    "Float64 partition_by": ([E.window("ROW_NUMBER", [], "x", partition_by=[col("f")])], {}, r"Float64 partition_by.*\"f\""),
    "Float32 partition_by": ([E.window("SUM", [col("v")], "x", partition_by=[col("k"), col("f32")])], {}, r"Float32 partition_by.*\"f32\""),
    "FIRST_VALUE": ([E.window("FIRST_VALUE", [col("v")], "x", **OVER)], {}, r"window function FIRST_VALUE"),
    "LAST_VALUE": ([E.window("last_value", [col("v")], "x", **OVER)], {}, r"window function LAST_VALUE"),
    "NTH_VALUE": ([E.window("NTH_VALUE", [col("v"), lit(2)], "x", **OVER)], {}, r"window function NTH_VALUE"),
    "another aggregate": ([E.window("STDDEV", [col("v")], "x", **OVER)], {}, r"window function STDDEV"),
    "NTILE": ([E.window("NTILE", [lit(4)], "x", **OVER)], {}, r"window function NTILE"),
    "sliding MIN": ([E.window("MIN", [col("v")], "x", frame=E.rows_between(1, 0), **OVER)], {}, r"MIN.*ROWS 1 PRECEDING \.\. CURRENT ROW.*sliding"),
    "sliding MAX": ([E.window("MAX", [col("v")], "x", frame=E.rows_between(None, 1), **OVER)], {}, r"MAX.*ROWS UNBOUNDED PRECEDING \.\. 1 FOLLOWING.*sliding"),
    "sliding Float64 SUM": ([E.window("SUM", [col("f")], "x", frame=E.rows_between(2, 2), **OVER)], {}, r"SUM.*ROWS 2 PRECEDING \.\. 2 FOLLOWING.*Float64.*sliding frames over floats"),
    "sliding Float32 AVG": ([E.window("AVG", [col("f32")], "x", frame=E.rows_between(0, 1), **OVER)], {}, r"AVG.*ROWS 0 PRECEDING \.\. 1 FOLLOWING.*Float32"),
    "LAG over Utf8": ([E.lag(col("s"), "x", **OVER)], {}, r"LAG over Utf8"),
    "LEAD over Boolean": ([E.lead(col("b"), "x", **OVER)], {}, r"LEAD over Boolean"),
    "SUM over Utf8": ([E.window("SUM", [col("s")], "x", **OVER)], {}, r"SUM over Utf8"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals_are_unsupported_and_named(case):
    w, kw, pattern = REFUSED[case]
    with pytest.raises(g.GpuqError, match=pattern) as e:
        g.BoundedWindowAggExec(SRC, w, **kw).schema()
    assert e.value.status == 3 and e.value.refusal == B.REFUSAL_NONE, (e.value.status, e.value.refusal)


def test_the_unbounded_node_stays_not_native():
    plan = {"WindowAggExec": {"input": {"MemoryExec": {"schema": SRC.schema(), "partitions": [0]}}, "window_expr": [E.window("SUM", [col("v")], "x", partition_by=[col("k")])]}}
    with pytest.raises(g.GpuqError, match="WindowAggExec") as e:
        B.plan_schema(plan)
    assert e.value.status == 3 and e.value.refusal == B.REFUSAL_NODE_NOT_NATIVE


MALFORMED = {
    "frame value not a number": (E.window("SUM", [col("v")], "x", frame={"units": "ROWS", "start_bound": {"type": "PRECEDING", "value": "x"}, "end_bound": {"type": "CURRENT_ROW", "value": None}}, **OVER),
                                 r"SUM.*start_bound value \"x\""),
    "negative frame value": (E.window("AVG", [col("v")], "x", frame={"units": "ROWS", "start_bound": {"type": "PRECEDING", "value": 1}, "end_bound": {"type": "FOLLOWING", "value": -2}}, **OVER),
                             r"AVG.*end_bound value -2 is negative"),
    "negative offset": (E.lag(col("v"), "x", offset=-1, **OVER), r"LAG.*offset -1 is negative"),
    "unknown bound type": (E.window("SUM", [col("v")], "x", frame={"units": "ROWS", "start_bound": {"type": "BEFORE", "value": 1}, "end_bound": {"type": "CURRENT_ROW"}}, **OVER), r"SUM.*start_bound.*BEFORE"),
    "unknown units": (E.window("SUM", [col("v")], "x", frame={"units": "LINES", "start_bound": {"type": "PRECEDING"}, "end_bound": {"type": "CURRENT_ROW"}}, **OVER), r"SUM.*LINES"),
    "rank with an argument": (E.window("RANK", [col("v")], "x", **OVER), r"RANK takes no arguments"),
    "offset not a literal": (E.window("LAG", [col("v"), col("o")], "x", **OVER), r"LAG.*offset must be a literal"),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_expressions_are_invalid_and_named(case):
    w, pattern = MALFORMED[case]
    with pytest.raises(g.GpuqError, match=pattern) as e:
        g.BoundedWindowAggExec(SRC, [w]).schema()
    assert e.value.status == 1


def test_the_frame_of_a_rank_or_a_shift_is_not_read():
    """ROW_NUMBER, the ranks and LAG / LEAD do not look at their frame: whatever it holds, it is neither parsed nor refused"""
    odd = {"units": "GROUPS", "start_bound": {"type": "FOLLOWING", "value": "1 day"}, "end_bound": {"type": "FOLLOWING", "value": None}}
    w = [E.window("ROW_NUMBER", [], "rn", frame=odd, **OVER), E.window("RANK", [], "rk", frame=odd, **OVER), E.window("LAG", [col("v")], "l", frame=odd, **OVER)]
    got = g.BoundedWindowAggExec(SRC, w).schema()[-3:]
    assert [(f["name"], f["type"], f["nullable"]) for f in got] == [("rn", "UInt64", False), ("rk", "UInt64", False), ("l", "Int32", True)]


def test_unknown_mode_and_empty_window_expr_are_invalid():
    for w, kw in (([E.window("SUM", [col("v")], "x", **OVER)], {"partition_search_mode": "Hashed"}), ([], {})):
        with pytest.raises(g.GpuqError) as e:
            g.BoundedWindowAggExec(SRC, w, **kw).schema()
        assert e.value.status == 1


# ---------------------------------------------------------------- the build
def _build_module():
    spec = importlib.util.spec_from_file_location("gpuq_build", os.path.join(ROOT, "arrow-ballista_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    return build


def test_window_kernels_build_for_gfx950(tmp_path):
    """kernels_window.hip is part of the library (not of the sources kept for run-time specialisation), cross-compiles for gfx950 with
    the build's flags, and the build's scratch check passes on its remarks."""
    build = _build_module()
    assert "kernels_window.hip" in build.HIP_SOURCES and "kernels_window.hip" not in build.EMBED and "window_scan_op.h" in build.HEADERS
    r = subprocess.run([build._hipcc(), "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, "kernels_window.hip"), "-o", os.path.join(str(tmp_path), "kernels_window.o"),
                        "--offload-arch=" + build.ARCH, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    build._check_scratch("kernels_window.hip", r.stderr)
    names = set(re.findall(r"Function Name: (\S+)", r.stderr))
    for kernel in ("k_window_tile_totals", "k_window_tiles_scan", "k_window_downsweep", "k_window_rank", "k_window_shift", "k_window_frame"):
        assert any(kernel in n for n in names), (kernel, sorted(names))
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert scratch and max(scratch) == 0, scratch


# ---------------------------------------------------------------- the scan's operator, on the host
ACC_SUM, ACC_COUNT, ACC_MIN, ACC_MAX, ACC_FSUM, ACC_FMIN, ACC_FMAX = 0, 1, 3, 4, 5, 6, 7      # AccKind, csrc/gpuq_kernels.h
M64, M128 = (1 << 64) - 1, (1 << 128) - 1


@pytest.fixture(scope="module")
def scan_exe(tmp_path_factory):
    """tests/window_scan_host.cpp, host code only, under AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded)"""
    build = _build_module()
    exe = str(tmp_path_factory.mktemp("window_scan") / "window_scan_host")
    r = subprocess.run([build._hipcc(), "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I", build.CSRC,
                        os.path.join(ROOT, "tests", "window_scan_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def fold(exe, kind, rows):
    """rows: [(head, valid, lo, hi)] -> the three groupings' [(count, lo, hi)]"""
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


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def bits_f64(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def total_key(b):
    s = b - (1 << 64) if b >> 63 else b
    return s ^ ((s >> 63) & ((1 << 63) - 1))


def signed64(b):
    return b - (1 << 64) if b >> 63 else b


def shapes(rng):
    """[(head, valid)] per row: heads at the edges of the 7-row tiles, an all-NULL partition, a partition across several tiles,
    partitions of one row, a NULL at a head, and a tail that fills no tile"""
    sizes = [7, 1, 6, 7, 8, 5, 1, 1, 23, 3, 14, 2]      # heads at 0, 7, 8, 14, 21, 29, 34, 35, 36, 59, 62, 76; 78 rows
    all_null = {5}
    rows = []
    for p, size in enumerate(sizes):
        for i in range(size):
            valid = 0 if p in all_null or (i == 0 and p % 3 == 1) else int(rng.random() < 0.8)
            rows.append((1 if i == 0 else 0, valid))
    assert [i for i, r in enumerate(rows) if r[0]][:5] == [0, 7, 8, 14, 21] and len(rows) % 7 != 0
    return rows


def walk_cells(kind, rows):
    """the Python walk: [(count, value or None)], value an exact int (SUM mod 2^128, MIN / MAX signed 64-bit) or a bit pattern (floats'
    MIN / MAX) or, for ACC_FSUM, (exact Fraction, sum of magnitudes)"""
    out, cnt, acc, mag = [], 0, None, Fraction(0)
    for head, valid, lo, hi in rows:
        if head:
            cnt, acc, mag = 0, None, Fraction(0)
        if valid:
            cnt += 1
            if kind == ACC_SUM:
                acc = ((acc or 0) + (lo | hi << 64)) & M128
            elif kind == ACC_COUNT:
                acc = cnt
            elif kind in (ACC_MIN, ACC_MAX):
                v = signed64(lo)
                acc = v if acc is None else (min(acc, v) if kind == ACC_MIN else max(acc, v))
            elif kind == ACC_FSUM:
                acc = (acc or Fraction(0)) + Fraction(bits_f64(lo))
                mag += abs(Fraction(bits_f64(lo)))
            else:
                acc = lo if acc is None else (min(acc, lo, key=total_key) if kind == ACC_FMIN else max(acc, lo, key=total_key))
        out.append((cnt, (acc, mag) if kind == ACC_FSUM else acc))
    return out


@pytest.mark.parametrize("kind", [ACC_SUM, ACC_COUNT, ACC_MIN, ACC_MAX, ACC_FMIN, ACC_FMAX], ids=["SUM", "COUNT", "MIN", "MAX", "FMIN", "FMAX"])
def test_scan_operator_is_the_same_in_every_grouping_and_equals_the_walk(scan_exe, kind):
    rng = random.Random(kind)
    rows = []
    for head, valid in shapes(rng):
        if kind in (ACC_FMIN, ACC_FMAX):
            lo, hi = f64_bits(rng.choice([0.0, -0.0, 1.5, -2.25, 1e300, -1e300, float("inf"), float("-inf"), float("nan"), rng.uniform(-9, 9)])), 0
        elif kind == ACC_SUM:
            v = rng.choice([0, 1, -1, 2 ** 63 - 1, -2 ** 63, 2 ** 126, -2 ** 126, rng.randrange(-10 ** 37, 10 ** 37)]) & M128      # sums wrap at 128 bits
            lo, hi = v & M64, v >> 64
        else:
            v = rng.choice([0, -1, 2 ** 63 - 1, -2 ** 63, rng.randrange(-10 ** 6, 10 ** 6)]) & M64
            lo, hi = v, (M64 if v >> 63 else 0)
        rows.append((head, valid, lo, hi))
    a, b, c = fold(scan_exe, kind, rows)
    assert a == b == c
    for i, ((cnt, lo, hi), (wcnt, want)) in enumerate(zip(a, walk_cells(kind, rows))):
        assert cnt == wcnt, i
        if cnt == 0:
            continue
        if kind == ACC_SUM:
            assert lo | hi << 64 == want, i
        elif kind == ACC_COUNT:
            assert lo == want and hi == 0, i
        elif kind in (ACC_MIN, ACC_MAX):
            assert signed64(lo) == want, i
        else:
            assert lo == want, i


def test_scan_operator_float_sums_stay_within_the_any_order_bound(scan_exe):
    """The three groupings add in different orders: each row's running sum lies within (k - 1) u sum|x| of the exact sum of its k
    values (tests/float_agg_exact.py's bound for SUM), and the count is the same everywhere."""
    rng = random.Random(5)
    rows = [(head, valid, f64_bits(rng.choice([1e16, -1e16, 1.0, 3.5e-7, rng.uniform(-1e3, 1e3)])), 0) for head, valid in shapes(rng)]
    want = walk_cells(ACC_FSUM, rows)
    for block in fold(scan_exe, ACC_FSUM, rows):
        for i, ((cnt, lo, hi), (wcnt, (exact, mag))) in enumerate(zip(block, want)):
            assert cnt == wcnt, i
            if cnt:
                got = bits_f64(lo)
                assert math.isfinite(got) and abs(Fraction(got) - exact) <= (cnt - 1) * W.U * mag, (i, got, float(exact))


def test_scan_operator_with_no_head_in_the_first_tiles(scan_exe):
    """a carry that crosses two whole tiles with no head on the way, and rows before any head: they continue the identity"""
    rows = [(0, 1, i + 1, 0) for i in range(20)] + [(1, 1, 100, 0)] + [(0, 1, 1, 0)] * 9
    a, b, c = fold(scan_exe, ACC_SUM, rows)
    assert a == b == c
    assert [r[1] for r in a[:20]] == [i * (i + 1) // 2 for i in range(1, 21)] and [r[1] for r in a[20:]] == list(range(100, 110))
    assert [r[0] for r in a] == list(range(1, 21)) + list(range(1, 11))
