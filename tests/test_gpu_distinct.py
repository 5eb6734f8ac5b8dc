"""DISTINCT aggregates on the device: the entry point gpuq_segment_distinct alone (a column sorted inside its segments, reduced over its
run heads by a segmented scan), then AggregateExec in mode Single through the native executor -- DISTINCT beside plain aggregates, over
several arguments, with a FILTER, with four keys -- against the restatement of tests/distinct_exact.py (a dict of sets per group, Python
ints wrapped at the result's width, Fractions for floats).  Counts, integer and decimal sums and XORs are compared exactly; a Float64 SUM
against the exact rational within (k - 1) u sum|x| (distinct_exact.float_sum_ok), and two runs of it bit for bit."""
import ctypes as C
import decimal
import struct

import numpy as np
import pyarrow as pa
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd import binding as B
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit

import distinct_exact as D

pytestmark = pytest.mark.gpu

CTX = decimal.Context(prec=60)
M64, M128 = (1 << 64) - 1, (1 << 128) - 1
#          type id, numpy dtype (None: 16 bytes, encoded here), bytes
TYPES = {"Int8": (B.T_INT8, np.int8, 1), "UInt8": (B.T_UINT8, np.uint8, 1), "Int16": (B.T_INT16, np.int16, 2), "UInt16": (B.T_UINT16, np.uint16, 2),
         "Int32": (B.T_INT32, np.int32, 4), "UInt32": (B.T_UINT32, np.uint32, 4), "Float32": (B.T_FLOAT32, np.float32, 4), "Date32": (B.T_DATE32, np.int32, 4),
         "Int64": (B.T_INT64, np.int64, 8), "UInt64": (B.T_UINT64, np.uint64, 8), "Float64": (B.T_FLOAT64, np.float64, 8), "Decimal": (B.T_DECIMAL128, None, 16),
         "Utf8": (B.T_UTF8, None, 16)}
SUMMABLE = [t for t in TYPES if t not in ("Date32", "Utf8")]
BITWISE = [t for t in TYPES if t not in ("Date32", "Utf8", "Float32", "Float64")]
# segment lengths: heads on both sides of a 256-row block edge and a 2,048-row tile edge; the 5,000-row segment crosses two tile edges
SIZES = [1, 254, 1, 1, 2, 3, 63, 64, 65, 255, 256, 257, 825, 1, 1, 5000, 10, 9, 10, 11, 12, 1]
LONG = 15


def f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


# ------------------------------------------------------------------------------------ the entry point on its own
def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def bitmap(valid):
    return np.packbits(np.concatenate([valid, np.zeros((-len(valid)) % 64 + 64, dtype=bool)]), bitorder="little")


def packed15(s):
    b = s.encode()
    assert len(b) <= 15
    return (int.from_bytes(b.ljust(15, b"\0"), "big") << 8) | len(b)


def encode(vals, tname):
    """The column's data buffer: Arrow layout, a NULL's bytes arbitrary (0x5A: never looked at)."""
    _, dt, width = TYPES[tname]
    if dt is not None:
        a = np.array([0 if v is None else v for v in vals] + [0], dtype=dt)      # (one spare element: never an empty buffer)
        raw = a.view(np.uint8).copy()
    else:
        ints = [0 if v is None else (packed15(v) if tname == "Utf8" else int(v) & M128) for v in vals] + [0]
        raw = np.frombuffer(b"".join(x.to_bytes(16, "little") for x in ints), dtype=np.uint8).copy()
    for i, v in enumerate(vals):
        if v is None:
            raw[i * width:(i + 1) * width] = 0x5A
    return raw


def sort_key(tname):
    """Ascending inside a segment, NULLs last; floats in totalOrder (equal bit patterns are then adjacent)."""
    def key(v):
        if v is None:
            return (1, 0)
        if tname in D.FLOATS:
            b, top = D.identity(v, tname), (63 if tname == "Float64" else 31)
            return (0, (1 << (top + 1)) - 1 - b if b >> top else b | (1 << top))      # negative: all bits flipped; else the sign bit set
        return (0, v)
    return key


def run_distinct(tc, tname, vals, starts, want=("count", "sum", "xor", "valid"), sum_width=8, n_groups=None):
    """One call of gpuq_segment_distinct; {name: per-segment list}, every output checked untouched beyond n_groups."""
    import torch
    tid, _, width = TYPES[tname]
    n, G = len(vals), (len(starts) - 1 if n_groups is None else n_groups)
    data, valid, st = to_device(encode(vals, tname)), to_device(bitmap(np.array([v is not None for v in vals], dtype=bool))), to_device(np.array(starts, dtype=np.int32))
    c = B.gpuq_column()
    c.type, c.repr, c.data, c.validity, c.length = tid, (B.REPR_PACKED15 if tname == "Utf8" else B.REPR_ARROW), data.data_ptr(), valid.data_ptr(), n
    if tname == "Decimal":
        c.precision, c.scale = 38, 4
    words = (G + 63) // 64
    count = torch.full((G + 2,), 0x77, dtype=torch.int64, device="cuda")
    total = torch.full(((G + 2) * sum_width,), 0x77, dtype=torch.uint8, device="cuda")
    bxor = torch.full((G + 2,), 0x77, dtype=torch.int64, device="cuda")
    vbits = torch.full((words + 2,), 0x77, dtype=torch.int64, device="cuda")
    ptr = lambda name, t: t.data_ptr() if name in want else None
    tc.ctx.check(tc.ctx.L.gpuq_segment_distinct(tc.ctx.h, tc.stream_ptr(), C.byref(c), st.data_ptr(), G, n, ptr("count", count), ptr("sum", total), sum_width, ptr("xor", bxor), 8,
                                                ptr("valid", vbits)))
    tc.sync()
    out = {}
    count, total, bxor, vbits = count.cpu().numpy(), total.cpu().numpy(), bxor.cpu().numpy().view(np.uint64), vbits.cpu().numpy().view(np.uint64)
    assert count[G:].tolist() == [0x77] * 2 and set(total[G * sum_width:].tolist()) == {0x77} and bxor[G:].tolist() == [0x77] * 2 and vbits[words:].tolist() == [0x77] * 2
    for name, a in (("count", count), ("sum", total), ("xor", bxor), ("valid", vbits)):
        if name not in want:
            assert set(a.tolist()) == {0x77}, name      # a NULL pointer: not written
    out["count"] = count[:G].tolist()
    out["sum"] = [int.from_bytes(total[i * sum_width:(i + 1) * sum_width].tobytes(), "little") for i in range(G)]
    out["xor"] = bxor[:G].tolist()
    out["valid"] = [bool((int(vbits[i >> 6]) >> (i & 63)) & 1) for i in range(G)]
    if "valid" in want and G % 64:
        assert int(vbits[words - 1]) >> (G % 64) == 0      # whole words: the bits beyond the last segment are written, as zeroes
    return out


def check_segments(tc, tname, vals, starts, want=("count", "sum", "xor", "valid"), sum_width=8):
    got = run_distinct(tc, tname, vals, starts, want, sum_width)
    again = run_distinct(tc, tname, vals, starts, want, sum_width)
    assert got == again      # the same bits run after run, a Float64 SUM included
    sets = []
    for g_, (a, b) in enumerate(zip(starts[:-1], starts[1:])):
        s = D.sets([()] * (b - a), vals[a:b], tname).get((), {})
        sets.append(s)
        if "count" in want:
            assert got["count"][g_] == D.count(s), (tname, g_)
        if "valid" in want:
            assert got["valid"][g_] == (D.count(s) > 0), (tname, g_)
        if "sum" in want:
            exact = D.total(s, tname)
            if exact is None:
                assert got["sum"][g_] == 0, (tname, g_)
            elif tname in D.FLOATS:
                assert D.float_sum_ok(f64(got["sum"][g_]), exact), (tname, g_, f64(got["sum"][g_]), exact)
            else:      # the 128-bit cell's low sum_width bytes
                assert got["sum"][g_] == sum(int(v) for v in s.values()) & ((1 << (8 * sum_width)) - 1), (tname, g_)
        if "xor" in want:
            x = 0
            for v in s.values():
                x ^= int(v) & M64      # the low 64 bits of the two's-complement pattern
            assert got["xor"][g_] == x, (tname, g_)
    return sets


def drawer(r, tname):
    if tname == "Decimal":      # near +-10^38, where 128-bit sums wrap, and small ones
        return lambda: int(r.choice([1, -1])) * (10**38 - 1 - int(r.integers(0, 200000))) if r.random() < 0.5 else int(r.integers(-50, 50))
    if tname == "Utf8":
        words = ["", "a", "ab", "ab ", "b", "fifteen bytes..", "zz", "Zz"] + ["w%05d" % i for i in range(6000)]
        return lambda: words[int(r.integers(0, len(words)))]
    if tname == "Float64":      # -0.0 / 0.0, two NaN payloads and infinities among ordinary values
        special = [0.0, -0.0, f64(0x7FF8000000000000), f64(0x7FF8000000000001), float("inf"), 1.5, -1.5]
        return lambda: special[int(r.integers(0, len(special)))] if r.random() < 0.3 else float(r.standard_normal() * 1e3)
    if tname == "Float32":
        special = [np.float32(0.0), np.float32(-0.0), np.float32("nan"), np.float32(1.5)]
        return lambda: float(special[int(r.integers(0, len(special)))]) if r.random() < 0.3 else float(np.float32(r.standard_normal() * 1e3))
    ii = np.iinfo(TYPES[tname][1])
    if tname in ("Int64", "UInt64"):      # near the ends of the range: 64-bit sums wrap
        return lambda: int(ii.max) - int(r.integers(0, 3000)) if r.random() < 0.5 else int(ii.min) + int(r.integers(0, 3000))
    return lambda: int(r.integers(ii.min, ii.max, endpoint=True))


def shaped_table(r, tname, long_segment):
    """(vals, starts) over SIZES with, on top: an all-NULL segment, NULLs after the values, the last value of one segment equal to the
    first of the next, empty segments (first, doubled in the middle, last), and the 5,000-row segment `long_segment`: "equal" (one run
    across two tile edges), "different" (every value another one), "tile_last" (a run that starts on row 4095, a tile's last row)."""
    draw, key = drawer(r, tname), sort_key(tname)
    segs = []
    for size in SIZES:
        pool = [draw() for _ in range(max(1, size // 3))]
        segs.append(sorted((pool[int(i)] for i in r.integers(0, len(pool), size)), key=key))
    segs[16] = [None] * 10
    for gi, keep in ((17, 4), (18, 5), (19, 1), (20, 2)):
        segs[gi][keep:] = [None] * (len(segs[gi]) - keep)
    c = segs[9][len(segs[9]) // 2]      # segment 8 ends with c, segment 9 begins with it: it counts in both
    segs[8] = [v if key(v) <= key(c) else c for v in segs[8]][:-1] + [c]
    segs[9] = [c] + [v if key(v) >= key(c) else c for v in segs[9]][1:]
    if long_segment == "equal":
        segs[LONG] = [draw()] * 5000
    elif long_segment == "different":
        pool = {}
        while len(pool) < 5000:
            v = draw()
            pool.setdefault(D.identity(v, tname), v)
        segs[LONG] = sorted(pool.values(), key=key)
    else:
        a, b = sorted({D.identity(v, tname): v for v in (draw() for _ in range(40))}.values(), key=key)[:2]
        head = sum(SIZES[:LONG])
        assert head == 2049
        segs[LONG] = [a] * (4095 - head) + [b] * (5000 - (4095 - head))
    starts, vals = [0, 0], []      # an empty first segment, two empty ones after segment 11, an empty last one
    for gi, seg in enumerate(segs):
        vals += seg
        starts.append(len(vals))
        if gi == 11:
            starts += [len(vals)] * 2
    starts.append(len(vals))
    return vals, starts


@pytest.mark.parametrize("long_segment", ["equal", "different", "tile_last"])
@pytest.mark.parametrize("tname", list(TYPES))
def test_entry_point_segment_shapes(tc, tname, long_segment):
    if long_segment == "different" and TYPES[tname][2] == 1:
        long_segment = "two_hundred"      # (a byte has 256 values: the 5,000 rows hold as many different ones as there are, each in a run)
    r = np.random.default_rng(len(tname) * 7 + len(long_segment))
    vals, starts = shaped_table(r, tname, "tile_last" if long_segment == "two_hundred" else long_segment)
    if long_segment == "two_hundred":
        lo = np.iinfo(TYPES[tname][1]).min
        a = sum(SIZES[:LONG])
        vals[a:a + 5000] = sorted(lo + (i % 200) for i in range(5000))
    want = ("count", "valid") + (("sum",) if tname in SUMMABLE else ()) + (("xor",) if tname in BITWISE else ())
    sets = check_segments(tc, tname, vals, starts, want)
    long_set = sets[1 + LONG + (2 if LONG > 11 else 0)]
    assert len(long_set) == {"equal": 1, "different": 5000, "tile_last": 2, "two_hundred": 200}[long_segment]
    assert [len(s) for s in sets[:1] + sets[13:15] + sets[-1:]] == [0, 0, 0, 0] and len(sets) == len(SIZES) + 4
    assert vals[starts[10] - 1] == vals[starts[10]] and vals[starts[10]] is not None      # segment 8's last row and segment 9's first (one empty segment ahead)


@pytest.mark.parametrize("tname", ["Int64", "Decimal"])
def test_entry_point_sum_in_sixteen_bytes(tc, tname):
    """The integer / decimal SUM is a 128-bit cell: stored whole, a SUM of Int64 near the ends of its range does not wrap, one of
    Decimal128 near +-10^38 wraps at 128 bits."""
    r = np.random.default_rng(16)
    vals, starts = shaped_table(r, tname, "different")
    sets = check_segments(tc, tname, vals, starts, ("sum", "valid"), sum_width=16)
    wide = [sum(int(v) for v in s.values()) for s in sets]
    assert any(not -2**63 <= w < 2**63 for w in wide) and (tname == "Int64" or any(not -2**127 <= w < 2**127 for w in wide))


@pytest.mark.parametrize("want", [("count",), ("valid",), ("sum",), ("xor",), ("sum", "xor"), ("count", "xor", "valid")], ids="+".join)
def test_entry_point_every_output_is_optional(tc, want):
    r = np.random.default_rng(5)
    vals, starts = shaped_table(r, "Int32", "tile_last")
    check_segments(tc, "Int32", vals, starts, want)


@pytest.mark.parametrize("n", [1, 7, 2048, 2049, 6145])
def test_entry_point_one_segment_over_all_rows(tc, n):
    for tname in ("Int16", "Float64"):
        r = np.random.default_rng(n)
        draw = drawer(r, tname)
        vals = sorted((draw() for _ in range(n - n // 5)), key=sort_key(tname)) + [None] * (n // 5)
        sets = check_segments(tc, tname, vals, [0, n], ("count", "sum", "valid"))
        assert len(sets) == 1 and (n < 100 or len(sets[0]) > 50)


def test_entry_point_no_segments_and_no_rows(tc):
    # n_groups = 0 writes nothing (run_distinct checks every output untouched), with rows and without
    assert run_distinct(tc, "Int32", [1, 2, 3], [0], n_groups=0)["count"] == []
    assert run_distinct(tc, "Int32", [], [0], n_groups=0)["count"] == []
    # segments over no rows: 0 / NULL
    got = run_distinct(tc, "Int32", [], [0, 0, 0, 0])
    assert got == {"count": [0, 0, 0], "sum": [0, 0, 0], "xor": [0, 0, 0], "valid": [False, False, False]}


def test_entry_point_floats_count_by_their_bytes(tc):
    nan_a, nan_b, nan_neg = f64(0x7FF8000000000000), f64(0x7FF8000000000001), f64(0xFFF8000000000000)
    vals = [nan_neg, -1.0, -0.0, -0.0, 0.0, 0.0, 1.0, nan_a, nan_a, nan_b, None]
    assert vals == sorted(vals, key=sort_key("Float64"))      # (bit for bit: NaN != NaN, but the list compares by identity first)
    got = run_distinct(tc, "Float64", vals, [0, len(vals)], ("count", "valid"))
    assert got["count"] == [7] and got["valid"] == [True]      # -NaN, -1, -0.0, 0.0, 1, NaN, the other NaN
    got = run_distinct(tc, "Float64", [-0.0, 0.0, 2.5, None, -0.0, -0.0], [0, 4, 6], ("count", "sum"))
    assert got["count"] == [3, 1] and [f64(x) for x in got["sum"]] == [2.5, -0.0] and got["sum"][1] == 0x8000000000000000      # a set of one -0.0 sums to -0.0
    got32 = run_distinct(tc, "Float32", [-0.0, 0.0, 0.1, 0.1], [0, 4], ("count", "sum"))
    assert got32["count"] == [3] and f64(got32["sum"][0]) == float(np.float32(0.1))      # widened first: the sum is the Float32's value as a double


def test_entry_point_refusals(tc):
    with pytest.raises(g.GpuqError, match=r"SUM\(DISTINCT\) over Date32"):
        run_distinct(tc, "Date32", [1, 2], [0, 2], ("sum",))
    with pytest.raises(g.GpuqError, match=r"BIT_XOR\(DISTINCT\) over Float64"):
        run_distinct(tc, "Float64", [1.0, 2.0], [0, 2], ("xor",))
    with pytest.raises(g.GpuqError, match=r"SUM\(DISTINCT\) over Utf8"):
        run_distinct(tc, "Utf8", ["a"], [0, 1], ("sum",))


def test_2_to_the_31_rows_are_refused_by_the_entry_point(tc):
    """2^31 rows or more in a partition: the lowering makes the same test on its projection's row count, and the entry point refuses the
    count before it looks at a pointer -- status 3 (GPUQ_ERR_UNSUPPORTED), refusal kind NONE, the limit named; the context goes on"""
    L, ctx, stream = B.lib(), tc.ctx.h, tc.stream_ptr()
    n = 2 ** 31
    column = B.gpuq_column()
    column.type, column.length = B.T_INT64, n
    with pytest.raises(g.GpuqError, match=r"gpuq_segment_distinct \(DISTINCT aggregates\): >= 2\^31 rows in one call") as e:
        tc.ctx.check(L.gpuq_segment_distinct(ctx, stream, C.byref(column), None, 0, n, None, None, 8, None, 8, None))
    assert e.value.status == 3 and e.value.refusal == B.REFUSAL_NONE
    assert run_distinct(tc, "Int32", [1, 1, 2], [0, 3], ("count",))["count"] == [2]


# ------------------------------------------------------------------------------------ through the native executor
def mixed_table(seed, n=4000, ngroups=37):
    r = np.random.default_rng(seed)
    words = np.array(["", "a", "ab", "ab ", "b", "fifteen bytes..", "zz", "Zz"], dtype=object)
    return {"k": r.integers(0, ngroups, n).astype(np.int32), "v": r.integers(-40, 40, n), "v_ok": r.random(n) >= 0.15,
            "w": np.round(r.standard_normal(n) * 3, 1).astype(np.float64), "w_ok": r.random(n) >= 0.15, "f": r.integers(0, 10, n).astype(np.int32),
            "u": r.integers(2**63 - 30, 2**63 + 30, n, dtype=np.uint64), "s": words[r.integers(0, len(words), n)], "s_ok": r.random(n) >= 0.1,
            "d": r.integers(0, 25, n).astype(np.int32), "k2": r.integers(0, 3, n).astype(np.int16), "k3": r.integers(0, 2, n).astype(np.int8), "k4": r.integers(5, 7, n), "n": n}


def mixed_arrow(d):
    return pa.table({"k": pa.array(d["k"]), "v": pa.array(d["v"], mask=~d["v_ok"]), "w": pa.array(d["w"], mask=~d["w_ok"]), "f": pa.array(d["f"]), "u": pa.array(d["u"]),
                     "s": pa.array(d["s"], pa.utf8(), mask=~d["s_ok"]), "d": pa.array(d["d"], pa.date32()), "k2": pa.array(d["k2"]), "k3": pa.array(d["k3"]), "k4": pa.array(d["k4"])})


def column(d, name, sel=None):
    """A column of mixed_table as a list of Python values, None = NULL."""
    ok = d.get(name + "_ok", np.ones(d["n"], dtype=bool))
    sel = np.ones(d["n"], dtype=bool) if sel is None else sel
    return [(v.item() if hasattr(v, "item") else v) if o and s else None for v, o, s in zip(d[name], ok, sel)]


def run_node(tc, table, keys, aggs_of, below=None):
    src = g.MemoryExec([table])
    inp = below(src) if below else src
    s = inp.schema()
    node = g.AggregateExec("Single", [(col(k, s), k) for k in keys], aggs_of(s), inp)
    return g.plan.materialize(tc, node.execute(0, tc)).to_arrow(tc.ctx), node


def rows_of(t, nkeys):
    keys = list(zip(*[t.column(i).to_pylist() for i in range(nkeys)])) if nkeys else [()] * t.num_rows
    assert len(set(keys)) == len(keys) == t.num_rows
    return dict(zip(keys, zip(*[t.column(i).to_pylist() for i in range(nkeys, t.num_columns)]))) if t.num_columns > nkeys else {}


def dagg(fn, c, name, **kw):
    return lambda s: dict({"fn": fn, "expr": col(c, s), "name": name, "distinct": True}, **{k: (v(s) if callable(v) else v) for k, v in kw.items()})


def pagg(fn, c, name):
    return lambda s: {"fn": fn, "expr": col(c, s), "name": name}


def expected(keys, specs):
    """{key: tuple}: specs = [(fn, values, tname)] over the sets of every group."""
    per = [D.sets(keys, vals, tname) for _, vals, tname in specs]
    out = {}
    for k in per[0] if per else []:
        out[k] = tuple(D.count(p[k]) if fn == "COUNT" else D.total(p[k], tname) if fn == "SUM" else D.bit_xor(p[k], tname) for (fn, _, tname), p in zip(specs, per))
    return out


def assert_rows(got, exp, names):
    assert set(got) == set(exp)
    for k in exp:
        for name, x, y in zip(names, got[k], exp[k]):
            if isinstance(y, (tuple, float)):
                assert x is not None and D.float_sum_ok(x, y), (k, name, x, y)
            else:
                assert x == y, (k, name, x, y)


def test_distinct_beside_plain_aggregates(tc):
    d = mixed_table(3)
    t = mixed_arrow(d)
    star = lambda s: {"fn": "COUNT", "expr": lit(1), "name": "n"}
    aggs = [dagg("COUNT", "v", "cv"), pagg("SUM", "v", "sv"), star, dagg("SUM", "v", "dv"), dagg("MIN", "w", "mw")]
    got, node = run_node(tc, t, ["k"], lambda s: [a(s) for a in aggs])
    assert got.schema.names == ["k", "cv", "sv", "n", "dv", "mw"] and [f["name"] for f in node.schema()] == got.schema.names
    assert [got.column(c).type for c in ("cv", "sv", "n", "dv", "mw")] == [pa.int64(), pa.int64(), pa.int64(), pa.int64(), pa.float64()]
    assert [pa.int64() if f["type"] == "Int64" else pa.float64() for f in node.schema()[1:]] == [got.column(i).type for i in range(1, 6)]
    keys = [(int(k),) for k in d["k"]]
    exp = expected(keys, [("COUNT", column(d, "v"), "Int64"), ("SUM", column(d, "v"), "Int64")])
    rows = rows_of(got, 1)
    assert len(rows) == 37
    assert_rows({k: (r[0], r[3]) for k, r in rows.items()}, exp, ["cv", "dv"])
    assert all(r[0] < r[2] for r in rows.values())      # duplicates there were: fewer values than rows
    # the plain columns, and the one where DISTINCT changes nothing: what the same node without the DISTINCT entries returns, exactly
    ref, _ = run_node(tc, t, ["k"], lambda s: [pagg("SUM", "v", "sv")(s), star(s), pagg("MIN", "w", "mw")(s)])
    assert {k: (r[1], r[2], r[4]) for k, r in rows.items()} == rows_of(ref, 1)


def test_two_and_three_arguments(tc):
    d = mixed_table(4)
    t = mixed_arrow(d)
    keys = [(int(k),) for k in d["k"]]
    specs = [("COUNT", column(d, "v"), "Int64"), ("COUNT", column(d, "f"), "Int32"), ("SUM", column(d, "w"), "Float64"), ("BIT_XOR", column(d, "f"), "Int32"),
             ("SUM", column(d, "u"), "UInt64"), ("COUNT", column(d, "w"), "Float64")]
    got, _ = run_node(tc, t, ["k"], lambda s: [dagg("COUNT", "v", "cv")(s), dagg("COUNT", "f", "cf")(s)])
    assert_rows(rows_of(got, 1), expected(keys, specs[:2]), ["cv", "cf"])
    aggs = [dagg("COUNT", "v", "cv"), dagg("COUNT", "f", "cf"), dagg("SUM", "w", "sw"), dagg("BIT_XOR", "f", "xf"), dagg("SUM", "u", "su"), dagg("COUNT", "w", "cw")]
    got, _ = run_node(tc, t, ["k"], lambda s: [a(s) for a in aggs])
    assert [got.column(c).type for c in ("sw", "xf", "su")] == [pa.float64(), pa.int32(), pa.uint64()]
    exp = expected(keys, specs)
    assert_rows(rows_of(got, 1), exp, ["cv", "cf", "sw", "xf", "su", "cw"])
    assert any(e[4] < 2**63 for e in exp.values())      # the UInt64 sums wrapped


def test_filter_beside_the_same_argument_without_it(tc):
    d = mixed_table(5)
    pred = lambda s: binary(col("f", s), Op.Lt, lit(3, "Int32"))
    got, _ = run_node(tc, mixed_arrow(d), ["k"], lambda s: [dagg("COUNT", "v", "c")(s), dagg("COUNT", "v", "cf", filter=pred)(s), dagg("SUM", "v", "sf", filter=pred)(s), pagg("COUNT", "v", "n")(s)])
    keys = [(int(k),) for k in d["k"]]
    exp = expected(keys, [("COUNT", column(d, "v"), "Int64"), ("COUNT", column(d, "v", d["f"] < 3), "Int64"), ("SUM", column(d, "v", d["f"] < 3), "Int64")])
    rows = rows_of(got, 1)
    assert_rows({k: r[:3] for k, r in rows.items()}, exp, ["c", "cf", "sf"])
    assert any(r[1] < r[0] for r in rows.values())      # a row the filter does not pass counts as a NULL argument
    assert {k: r[3] for k, r in rows.items()} == {(k,): int((d["v_ok"] & (d["k"] == k)).sum()) for k in range(37)}


def test_all_distinct_with_four_keys(tc):
    d = mixed_table(6)
    got, _ = run_node(tc, mixed_arrow(d), ["k2", "k3", "k4", "f"], lambda s: [dagg("COUNT", "v", "c")(s), dagg("SUM", "v", "s")(s)])
    keys = [tuple(int(d[c][i]) for c in ("k2", "k3", "k4", "f")) for i in range(d["n"])]
    exp = expected(keys, [("COUNT", column(d, "v"), "Int64"), ("SUM", column(d, "v"), "Int64")])
    assert len(exp) == 3 * 2 * 2 * 10
    assert_rows(rows_of(got, 4), exp, ["c", "s"])


def test_utf8_and_date32_arguments(tc):
    d = mixed_table(7)
    got, _ = run_node(tc, mixed_arrow(d), ["k"], lambda s: [dagg("COUNT", "s", "cs")(s), dagg("COUNT", "d", "cd")(s), pagg("MAX", "d", "md")(s)])
    keys = [(int(k),) for k in d["k"]]
    exp = expected(keys, [("COUNT", column(d, "s"), "Utf8"), ("COUNT", column(d, "d"), "Date32")])
    rows = rows_of(got, 1)
    assert_rows({k: r[:2] for k, r in rows.items()}, exp, ["cs", "cd"])
    assert max(e[0] for e in exp.values()) == 8 and got.column("md").type == pa.date32()      # "ab" and "ab " are two strings, "" is one


def test_fused_filter_and_computed_projection_below(tc):
    d = mixed_table(8)

    def below(src):
        s = src.schema()
        proj = g.ProjectionExec([(col("k", s), "k"), (binary(binary(col("v", s), Op.Multiply, lit(2)), Op.Plus, col("f", s)), "x"), (col("f", s), "f")], src)
        ps = proj.schema()
        return g.FilterExec(binary(col("f", ps), Op.Gt, lit(1, "Int32")), proj)
    got, _ = run_node(tc, mixed_arrow(d), ["k"], lambda s: [dagg("COUNT", "x", "c")(s), dagg("SUM", "x", "s")(s), pagg("COUNT", "x", "n")(s)], below)
    sel = d["f"] > 1
    x = [None if v is None else v * 2 + int(f) for v, f in zip(column(d, "v"), d["f"])]
    keys = [(int(k),) for k, s_ in zip(d["k"], sel) if s_]
    xs = [v for v, s_ in zip(x, sel) if s_]
    exp = expected(keys, [("COUNT", xs, "Int64"), ("SUM", xs, "Int64")])
    rows = rows_of(got, 1)
    assert_rows({k: r[:2] for k, r in rows.items()}, exp, ["c", "s"])
    assert {k: r[2] for k, r in rows.items()} == {(k,): int((d["v_ok"] & sel & (d["k"] == k)).sum()) for k in range(37)}


def test_ungrouped(tc):
    d = mixed_table(9)
    got, _ = run_node(tc, mixed_arrow(d), [], lambda s: [dagg("COUNT", "v", "cv")(s), pagg("SUM", "v", "sv")(s), dagg("SUM", "w", "sw")(s), dagg("COUNT", "s", "cs")(s)])
    exp = expected([()] * d["n"], [("COUNT", column(d, "v"), "Int64"), ("SUM", column(d, "w"), "Float64"), ("COUNT", column(d, "s"), "Utf8")])
    assert got.num_rows == 1
    row = tuple(c.to_pylist()[0] for c in got.columns)
    assert_rows({(): (row[0], row[2], row[3])}, exp, ["cv", "sw", "cs"])
    assert row[1] == int(d["v"][d["v_ok"]].sum()) and exp[()][0] == 80 and exp[()][2] == 8


def test_no_rows(tc):
    t = mixed_arrow(mixed_table(2, n=0))
    aggs = lambda s: [dagg("COUNT", "v", "c")(s), pagg("COUNT", "v", "n")(s), dagg("SUM", "v", "s")(s), dagg("BIT_XOR", "f", "x")(s), dagg("SUM", "w", "sw")(s)]
    got, _ = run_node(tc, t, ["k"], aggs)
    assert got.num_rows == 0 and got.schema.names == ["k", "c", "n", "s", "x", "sw"]
    got, _ = run_node(tc, t, [], aggs)      # ungrouped: one row, COUNT 0, SUM / BIT_XOR NULL
    assert [c.to_pylist() for c in got.columns] == [[0], [0], [None], [None], [None]]
    assert [c.type for c in got.columns] == [pa.int64(), pa.int64(), pa.int64(), pa.int32(), pa.float64()]


def test_one_plan_handle_two_executions_and_the_export_types(tc):
    """The first execution runs synchronously; later ones may defer the nodes around the node, never the node itself."""
    d = mixed_table(10)
    t = mixed_arrow(d).append_column("m", pa.array([decimal.Decimal(int(v)).scaleb(-2, CTX) for v in d["v"]], pa.decimal128(12, 2)))
    src = g.MemoryExec([t])
    s = src.schema()
    flt = g.FilterExec(binary(col("f", s), Op.Lt, lit(8, "Int32")), src)
    aggs = [dagg("COUNT", "v", "c"), pagg("SUM", "v", "sv"), dagg("SUM", "m", "sm"), dagg("SUM", "w", "sw"), dagg("BIT_XOR", "k2", "x2"), dagg("COUNT", "s", "cs")]
    agg = g.AggregateExec("Single", [(col("k", s), "k")], [a(s) for a in aggs], flt)
    os_ = agg.schema()
    plan = g.NativePlan(g.SortExec([{"expr": col("k", os_), "asc": True, "nulls_first": False}], agg), tc)
    runs = [plan.execute(0).to_arrow() for _ in range(2)]
    assert runs[1].equals(runs[0])
    got = runs[0]
    assert got.schema.names == ["k", "c", "sv", "sm", "sw", "x2", "cs"]
    assert [got.column(i).type for i in range(7)] == [pa.int32(), pa.int64(), pa.int64(), pa.decimal128(22, 2), pa.float64(), pa.int16(), pa.int64()]
    sel = d["f"] < 8
    keys = [(int(k),) for k, s_ in zip(d["k"], sel) if s_]
    pick = lambda name: [v for v, s_ in zip(column(d, name), sel) if s_]
    exp = expected(keys, [("COUNT", pick("v"), "Int64"), ("SUM", [int(v) for v in d["v"][sel]], "Decimal"), ("SUM", pick("w"), "Float64"), ("BIT_XOR", pick("k2"), "Int16"),
                          ("COUNT", pick("s"), "Utf8")])
    rows = rows_of(got, 1)
    assert list(rows) == sorted(exp)
    assert_rows({k: (r[0], None if r[2] is None else int(r[2].scaleb(2, CTX)), r[3], r[4], r[5]) for k, r in rows.items()}, exp, ["c", "sm", "sw", "x2", "cs"])


def test_refusals_at_run_time(tc):
    d = mixed_table(11, n=200)
    t = mixed_arrow(d).append_column("name", pa.array(["twenty bytes of name %02d" % (i % 7) for i in range(200)]))
    src = g.MemoryExec([t])
    s = src.schema()
    other = pagg("SUM", "v", "sv")(s)
    with pytest.raises(g.GpuqError, match=r"COUNT\(DISTINCT\).*longer than 15 bytes"):
        g.AggregateExec("Single", [(col("name", s), "name")], [dagg("COUNT", "v", "c")(s), other], src).execute(0, tc)
    with pytest.raises(g.GpuqError, match=r"COUNT\(DISTINCT\).*longer than 15 bytes"):
        g.AggregateExec("Single", [(col("k", s), "k")], [dagg("COUNT", "name", "c")(s), other], src).execute(0, tc)
    with pytest.raises(g.GpuqError, match=r"COUNT\(DISTINCT\).*Float64 group key"):
        g.AggregateExec("Single", [(col("w", s), "w")], [dagg("COUNT", "v", "c")(s), other], src).execute(0, tc)
    with pytest.raises(g.GpuqError, match=r"AVG\(DISTINCT"):
        g.AggregateExec("Single", [(col("k", s), "k")], [dagg("AVG", "v", "c")(s), other], src).execute(0, tc)
