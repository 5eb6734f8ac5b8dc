"""Hand-assembled Parquet pages for the device page decoder (csrc/kernels_scanfmt.hip: k_pq_decode, pq_hybrid, pq_unpack,
k_pq_dict_fixed, k_pq_dict_strings; csrc/scanfmt.cpp: the host page walk).

A writer emits only the part of the format it likes.  parquet-cpp never writes a dictionary index width of 0, a bit-packed run of
more than 63 groups, an uncompressed v2 page inside a compressed chunk or BIT_PACKED levels; parquet-rs (the reference's writer,
behind `tpch convert`) writes width 0 for a one-entry dictionary and leaves a v2 page uncompressed (is_compressed = false) when the
codec does not shrink it; Impala writes PLAIN_DICTIONARY on v1 pages and INT96 timestamps.  The emitters here write any legal page
and, for the refused cases, one targeted illegal edit, and record the expected column alongside: the expected values come from the
run program that was emitted, never from decoding the bytes.  test_cpu_parquet_pages.py proves every case against Arrow C++'s
reader before a kernel sees it.  Plain Python, numpy and pyarrow's CPU codecs: nothing here touches the GPU.

Formats: parquet-format/src/main/thrift/parquet.thrift (PageHeader, DataPageHeader, DataPageHeaderV2, DictionaryPageHeader,
SchemaElement, LogicalType), parquet-format/Encodings.md (PLAIN, RLE / bit-packed hybrid, the deprecated BIT_PACKED, dictionary
encoding), thrift/doc/specs/thrift-compact-protocol.md.
"""
import decimal
import functools
import struct
import zlib
from collections import namedtuple

import numpy as np
import pyarrow as pa

from compressed_streams import PQ_CODECS, _Struct, _zz, varint

BOOL, INT32, INT64, INT96, FLOAT, DOUBLE, BYTE_ARRAY, FLBA = range(8)
PLAIN, PLAIN_DICTIONARY, RLE, BIT_PACKED, DELTA_BINARY_PACKED, RLE_DICTIONARY = 0, 2, 3, 4, 5, 8
MAX_PAGE_VALUES = 1100


# ---------------------------------------------------------------- Thrift compact: the field kinds _Struct lacks
class TStruct(_Struct):
    def bool(self, fid, v):                  # the value lives in the field header's type nibble
        self._hdr(fid, 1 if v else 2)
        return self

    def i8(self, fid, v):
        self._hdr(fid, 3)
        self.b.append(v & 0xFF)
        return self

    def i16(self, fid, v):
        self._hdr(fid, 4)
        self.b += _zz(v)
        return self

    def double(self, fid, v):
        self._hdr(fid, 7)
        self.b += struct.pack("<d", v)
        return self

    def structs(self, fid, items):
        return self.list(fid, 12, [s.bytes() for s in items])

    def set(self, fid, etype, items):
        self._hdr(fid, 10)
        self.b += bytes([(len(items) << 4) | etype]) + b"".join(items)
        return self

    def map(self, fid, ktype, vtype, pairs):
        self._hdr(fid, 11)
        self.b += varint(len(pairs))
        if pairs:
            self.b.append((ktype << 4) | vtype)
            for k, v in pairs:
                self.b += k + v
        return self

    def unknown_fields(self, first=20):
        """one field of every Thrift type at ids no reader knows; the jumps to 50 and 51 need the long-form field id (delta > 15)"""
        f = first
        self.bool(f, True).bool(f + 1, False).i8(f + 2, -3).i16(f + 3, -300).i32(f + 4, 70000).i64(f + 5, -(1 << 40)).double(f + 6, 2.5)
        self.string(f + 7, b"unknown").list(f + 8, 5, [_zz(1), _zz(-1)]).set(f + 9, 8, [varint(2) + b"ab"])
        self.map(f + 10, 5, 8, [(_zz(7), varint(1) + b"x")]).struct(f + 11, TStruct().i32(1, 1).struct(2, TStruct().bool(1, True)))
        self.list(f + 30, 2, [b"\x01", b"\x02", b"\x01"]).map(f + 50, 5, 5, [])
        self.list(f + 51, 6, [_zz(k) for k in range(20)])          # 15 or more elements: the size follows as a varint
        return self


# ---------------------------------------------------------------- the RLE / bit-packed hybrid (Encodings.md) and BIT_PACKED levels
class Hybrid:
    """An explicit run program: .rle() and .packed() append one run each and record the values a decoder must produce."""

    def __init__(self, bw):
        self.bw, self.b, self.values = bw, bytearray(), []

    def rle(self, count, value, header_width=None, value_bytes=None):
        """`count` times `value`; header_width forces a non-minimal varint, value_bytes truncates (or pads) the value's bytes"""
        nb = (self.bw + 7) // 8
        self.b += varint(count << 1, header_width) + value.to_bytes(max(nb, 4), "little")[:nb if value_bytes is None else value_bytes]
        self.values += [value] * count
        return self

    def packed(self, vals, groups=None, header_width=None, drop=0):
        """one bit-packed run of `groups` groups of 8 (default: as many as vals needs, the last padded with zeros), LSB first;
        drop removes that many bytes from the run's end"""
        groups = (len(vals) + 7) // 8 if groups is None else groups
        padded = list(vals) + [0] * (groups * 8 - len(vals))
        acc = 0
        for i, v in enumerate(padded):
            assert 0 <= v < (1 << self.bw) or self.bw == 0 and v == 0
            acc |= v << (i * self.bw)
        body = acc.to_bytes(groups * self.bw, "little")
        self.b += varint((groups << 1) | 1, header_width) + body[:len(body) - drop]
        self.values += padded
        return self

    def auto(self, vals):
        """any value list as runs: eight or more equal values become an RLE run, the rest bit-packed groups"""
        i = 0
        while i < len(vals):
            j = i
            while j < len(vals) and vals[j] == vals[i]:
                j += 1
            if j - i >= 8 or j == len(vals) and j - i >= 1 and i % 3 == 0:
                self.rle(j - i, vals[i])
                i = j
            else:
                k = min(len(vals), i + 8 * max(1, (j - i) // 8))
                self.packed(vals[i:k])
                i = k
        return self

    def stream(self):
        return bytes(self.b)


def bit_packed_levels(levels, bw=1):
    """the deprecated BIT_PACKED level encoding: values packed back to back from the MOST significant bit of each byte, no length
    prefix, ceil(n * bw / 8) bytes"""
    out = bytearray((len(levels) * bw + 7) // 8)
    for i, v in enumerate(levels):
        for k in range(bw):
            if (v >> (bw - 1 - k)) & 1:
                bit = i * bw + k
                out[bit >> 3] |= 0x80 >> (bit & 7)
    return bytes(out)


# ---------------------------------------------------------------- schema leaves, PLAIN values
Leaf = namedtuple("Leaf", "phys optional arrow length converted logical scale precision", defaults=(0, None, None, 0, 0))
FLBA_PRECISION = [2, 4, 6, 9, 11, 14, 16, 18, 21, 23, 26, 28, 31, 33, 35, 38]      # decimal digits that fit 1..16 bytes


def pa_type(leaf):
    a = leaf.arrow
    if a == "decimal":
        return pa.decimal128(leaf.precision, leaf.scale)
    if a.startswith("timestamp"):
        return pa.timestamp(a[10:-1])
    return {"bool": pa.bool_, "string": pa.string}.get(a, getattr(pa, a, None))()


def _logical(lg):
    u = TStruct()
    if lg[0] == "string":
        return u.struct(1, TStruct())
    if lg[0] == "decimal":
        return u.struct(5, TStruct().i32(1, lg[2]).i32(2, lg[1]))
    if lg[0] == "date":
        return u.struct(6, TStruct())
    if lg[0] == "ts":            # isAdjustedToUTC = false: a timestamp without a zone
        return u.struct(8, TStruct().bool(1, False).struct(2, TStruct().struct({"ms": 1, "us": 2, "ns": 3}[lg[1]], TStruct())))
    assert lg[0] == "int"
    return u.struct(10, TStruct().i8(1, lg[1]).bool(2, lg[2]))


def _schema_elem(name, L):
    s = TStruct().i32(1, L.phys)
    if L.length:
        s.i32(2, L.length)
    s.i32(3, 1 if L.optional else 0).string(4, name.encode())
    if L.converted is not None:
        s.i32(6, L.converted)
    if L.precision:
        s.i32(7, L.scale).i32(8, L.precision)
    if L.logical:
        s.struct(10, _logical(L.logical))
    return s


def int96(ns):
    days, nanos = divmod(ns, 86400 * 10**9)
    return struct.pack("<qi", nanos, days + 2440588)      # nanoseconds of the day, Julian day


def plain(leaf, vals):
    """PLAIN encoding of physical values: ints (INT96: nanoseconds since 1970; FLOAT / DOUBLE: the bit pattern), bytes"""
    p = leaf.phys
    if p == BOOL:
        return sum(int(bool(v)) << i for i, v in enumerate(vals)).to_bytes((len(vals) + 7) // 8, "little")
    if p == BYTE_ARRAY:
        return b"".join(struct.pack("<I", len(v)) + v for v in vals)
    if p == FLBA:
        return b"".join(v.to_bytes(leaf.length, "big", signed=True) for v in vals)
    if p == INT96:
        return b"".join(int96(v) for v in vals)
    return b"".join(struct.pack({INT32: "<i", INT64: "<q", FLOAT: "<I", DOUBLE: "<Q"}[p], v) for v in vals)


def logical(leaf, v):
    """the Arrow value of a physical value (floats stay bit patterns, timestamps and dates stay integers)"""
    if v is None:
        return None
    a = leaf.arrow
    if a == "decimal":
        return decimal.Decimal(v).scaleb(-leaf.scale, decimal.Context(prec=40))
    if a.startswith("uint"):
        return v & ((1 << int(a[4:])) - 1)
    if a == "string":
        return v.decode()
    if a == "bool":
        return bool(v)
    return v


def expected_array(leaf, values):
    t = pa_type(leaf)
    if pa.types.is_floating(t):
        bits, fl = (np.uint32, np.float32) if t == pa.float32() else (np.uint64, np.float64)
        return pa.array(np.array([v or 0 for v in values], dtype=bits).view(fl), mask=np.array([v is None for v in values], dtype=bool))
    return pa.array(values, type=t)


def mismatch(col, leaf, values):
    """None when the decoded column equals the recorded one exactly (type, NULL positions, values; floats by bit pattern)"""
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    want = expected_array(leaf, values)
    if col.type != want.type:
        return "type %s, expected %s" % (col.type, want.type)
    if len(col) != len(want):
        return "%d rows, expected %d" % (len(col), len(want))
    if col.null_count != want.null_count or not col.is_null().equals(want.is_null()):
        return "NULLs at %s..., expected %s..." % (np.flatnonzero(np.asarray(col.is_null()))[:5], np.flatnonzero(np.asarray(want.is_null()))[:5])
    if pa.types.is_floating(col.type):
        bits = np.uint32 if col.type == pa.float32() else np.uint64
        a, b = np.asarray(col.fill_null(0.0)).view(bits), np.asarray(want.fill_null(0.0)).view(bits)
        bad = np.flatnonzero(a != b)
    else:
        if col.equals(want):
            return None
        a, b = col.to_pylist(), want.to_pylist()
        bad = [i for i in range(len(a)) if a[i] != b[i]]
    return None if len(bad) == 0 else "row %d is %r, expected %r (%d rows differ)" % (bad[0], a[bad[0]], b[bad[0]], len(bad))


# ---------------------------------------------------------------- pages, chunks, files
class Page:
    """kind: "dict", "v1", "v2" or "index".  levels: the definition-level stream without its length (None: the column is REQUIRED);
    values: everything after the levels (a dictionary-encoded page's width byte included).  The remaining arguments overrule what a
    well-formed header would say."""

    def __init__(self, kind, n=0, values=b"", levels=None, enc=PLAIN, compressed=True, def_enc=RLE, rep_enc=RLE, prefix=True, level_len=None, rep_len=0,
                 nulls=0, stats=False, crc=False, unknown=False):
        self.__dict__.update(locals())
        del self.self


Chunk = namedtuple("Chunk", "pages codec num_values", defaults=("none", None))
Case = namedtuple("Case", "name leaf chunk expect values reason streams")


def _compress(codec, data):
    return data if codec == "none" else pa.compress(data, codec=codec, asbytes=True)


def _stats():
    return TStruct().string(1, b"\xff\xff").string(2, b"\x00").i64(3, 1).i64(4, 2).string(5, b"\xff\xff").string(6, b"\x00")


def _page_bytes(pg, codec):
    if pg.kind == "v2":
        lv = pg.levels or b""
        payload = lv + (_compress(codec, pg.values) if pg.compressed else pg.values)
        ulen = len(lv) + len(pg.values)
        h = TStruct().i32(1, pg.n).i32(2, pg.nulls).i32(3, pg.n).i32(4, pg.enc).i32(5, len(lv) if pg.level_len is None else pg.level_len).i32(6, pg.rep_len)
        if not pg.compressed or pg.unknown:
            h.bool(7, pg.compressed)
        if pg.stats:
            h.struct(8, _stats())
        typ, fid = 3, 8
    elif pg.kind == "v1":
        raw = pg.values
        if pg.levels is not None:
            raw = (struct.pack("<I", len(pg.levels) if pg.level_len is None else pg.level_len) if pg.prefix else b"") + pg.levels + raw
        payload, ulen = _compress(codec, raw), len(raw)
        h = TStruct().i32(1, pg.n).i32(2, pg.enc).i32(3, pg.def_enc).i32(4, pg.rep_enc)
        if pg.stats:
            h.struct(5, _stats())
        typ, fid = 0, 5
    elif pg.kind == "dict":
        payload, ulen = _compress(codec, pg.values), len(pg.values)
        h = TStruct().i32(1, pg.n).i32(2, pg.enc)
        if pg.unknown:
            h.bool(3, False)
        typ, fid = 2, 7
    else:                                    # INDEX_PAGE: readers step over it
        payload, ulen, h, typ, fid = pg.values, len(pg.values), TStruct(), 1, 6
    if pg.unknown:
        h.unknown_fields(20)
    hdr = TStruct().i32(1, typ).i32(2, ulen).i32(3, len(payload))
    if pg.crc:
        hdr.i32(4, struct.unpack("<i", struct.pack("<I", zlib.crc32(payload)))[0])
    hdr.struct(fid, h)
    if pg.unknown:
        hdr.unknown_fields(20)
    return hdr.bytes() + payload, len(hdr.bytes()) + ulen


def parquet_file(leaves, groups):
    """leaves: [(name, Leaf)]; groups: one [Chunk per leaf] per row group.  A row group has as many rows as its first chunk declares."""
    body = bytearray(b"PAR1")
    gmeta, rows_total = [], 0
    for chunks in groups:
        cmetas, rows = [], None
        for (name, L), ch in zip(leaves, chunks):
            first, data_at, u_total = len(body), None, 0
            for pg in ch.pages:
                if pg.kind != "dict" and data_at is None:
                    data_at = len(body)
                b, u = _page_bytes(pg, ch.codec)
                body += b
                u_total += u
            nv = sum(p.n for p in ch.pages if p.kind in ("v1", "v2")) if ch.num_values is None else ch.num_values
            cm = (TStruct().i32(1, L.phys).list(2, 5, [_zz(PLAIN), _zz(RLE), _zz(RLE_DICTIONARY)]).list(3, 8, [varint(len(name)) + name.encode()])
                  .i32(4, PQ_CODECS[ch.codec]).i64(5, nv).i64(6, u_total).i64(7, len(body) - first).i64(9, first if data_at is None else data_at))
            if ch.pages and ch.pages[0].kind == "dict":
                cm.i64(11, first)
            cmetas.append(TStruct().i64(2, first).struct(3, cm))
            rows = nv if rows is None else rows
        gmeta.append(TStruct().structs(1, cmetas).i64(2, len(body)).i64(3, rows))
        rows_total += rows
    root = TStruct().string(4, b"schema").i32(5, len(leaves))
    meta = (TStruct().i32(1, 1).structs(2, [root] + [_schema_elem(n, L) for n, L in leaves]).i64(3, rows_total).structs(4, gmeta)
            .string(6, b"parquet_pages.py").bytes())
    return bytes(body) + meta + struct.pack("<I", len(meta)) + b"PAR1"


def file_of(cs):
    """cases of one leaf as the row groups of a one-column file"""
    assert all(c.leaf == cs[0].leaf for c in cs)
    return parquet_file([("v", cs[0].leaf)], [[c.chunk] for c in cs])


def columns_file_of(cs):
    """cases of equal row counts as the columns of a one-row-group file; the columns are named c0, c1, ..."""
    assert len({len(c.values) for c in cs}) == 1
    return parquet_file([("c%d" % i, c.leaf) for i, c in enumerate(cs)], [[c.chunk for c in cs]])


# ---------------------------------------------------------------- case construction
I32R, I32O = Leaf(INT32, False, "int32"), Leaf(INT32, True, "int32")
STRO = Leaf(BYTE_ARRAY, True, "string", converted=0)
DICT8 = [-7, 0, 1 << 30, -(1 << 31), 5, 6, 77, (1 << 31) - 1]


class _Build:
    """pages of one chunk and the rows they must decode to"""

    def __init__(self, leaf, dict_vals=None, dict_enc=PLAIN, codec="none", dict_kw=None):
        self.leaf, self.dict_vals, self.codec, self.rows, self.streams, self.next = leaf, dict_vals, codec, [], [], 1000
        self.pages = [] if dict_vals is None else [Page("dict", len(dict_vals), plain(leaf, dict_vals), enc=dict_enc, **(dict_kw or {}))]

    def page(self, n, levels=None, idx=None, kind="v1", enc=None, vals=None, width_byte=True, **kw):
        """n rows: levels (a Hybrid of width 1; None: nothing is NULL) and either idx (a Hybrid of dictionary indices) or PLAIN values
        (vals, or a running counter)"""
        if levels is None and self.leaf.optional:
            levels = Hybrid(1).rle(n, 1)
        lv = levels.values[:n] if levels else [1] * n
        assert len(lv) == n <= MAX_PAGE_VALUES
        present = sum(lv)
        if levels:
            self.streams.append((1, n, levels.stream(), lv))
        if idx is not None:
            ix = idx.values[:present]
            assert len(ix) == present
            pv = [self.dict_vals[i] for i in ix]
            body = (bytes([idx.bw]) if width_byte else b"") + idx.stream()
            enc = RLE_DICTIONARY if enc is None else enc
            if idx.bw:
                self.streams.append((idx.bw, present, idx.stream(), ix))
        else:
            if vals is None:
                vals = list(range(self.next, self.next + present))
                self.next += present
            pv, enc = list(vals[:present]), PLAIN if enc is None else enc
            body = plain(self.leaf, pv) if enc == PLAIN else kw.pop("body")
        it = iter(pv)
        self.rows += [next(it) if l else None for l in lv]
        self.pages.append(Page(kind, n, body, levels.stream() if levels else None, enc, nulls=n - present, **kw))
        return self

    def case(self, name, expect="valid", reason="", num_values=None):
        return Case(name, self.leaf, Chunk(self.pages, self.codec, num_values), expect, [logical(self.leaf, v) for v in self.rows], reason, self.streams)


def _run_program(ops, bw, vmax, rng):
    """ops: ("rle", count[, header_width]) or ("bp", n_values[, groups[, header_width]]) -> Hybrid with values drawn below vmax"""
    h = Hybrid(bw)
    for op in ops:
        if op[0] == "rle":
            h.rle(op[1], int(rng.integers(0, vmax)), *op[2:])
        else:
            h.packed([int(v) for v in rng.integers(0, vmax, op[1])], *op[2:])
    return h


ALTERNATING = [x for L in (1, 7, 8, 9, 63, 64, 65) for x in (("rle", L), ("bp", L))]
# name -> (run program, n values read from it): n below the program's total leaves a padded last group or an overshooting run
PROGRAMS = {
    "rle_only": ([("rle", 100)], 100),
    "packed_only": ([("bp", 96)], 96),
    "alternating_1_7_8_9_63_64_65": (ALTERNATING, sum(op[1] if op[0] == "rle" else (op[1] + 7) // 8 * 8 for op in ALTERNATING)),
    "packed_63_groups": ([("bp", 504)], 504),
    "packed_64_groups_two_byte_header": ([("bp", 512)], 512),          # parquet-cpp caps a run at 63 groups: (64 << 1 | 1) needs 2 bytes
    "packed_130_groups": ([("bp", 1040)], 1040),
    "packed_last_group_padded": ([("rle", 5), ("bp", 3)], 8),
    "packed_run_overshoots": ([("rle", 3), ("bp", 64)], 23),
    "rle_run_overshoots": ([("rle", 10), ("rle", 1000)], 50),
    "rle_three_byte_header": ([("bp", 8), ("rle", 20000)], 1000),      # 20000 << 1 >= 2^14
    "rle_five_byte_nonminimal_header": ([("rle", 300, 5), ("bp", 8, 1, 3), ("rle", 9, 2)], 317),
}


def _hybrid_cases():
    C = []
    for name, (ops, n) in PROGRAMS.items():
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        C.append(_Build(I32O).page(n, _run_program(ops, 1, 2, rng)).case("levels/" + name))
        C.append(_Build(I32R, DICT8).page(n, idx=_run_program(ops, 3, 8, rng)).case("indices/" + name))
    # the last group announces 3 bytes; the 3 values read need 2, and only those are there (old parquet-mr writers cut the padding).
    # Arrow C++ reads it, so does the device; one byte fewer and both refuse (refused/indices_packed_last_group_values_cut).
    C.append(_Build(I32R, DICT8).page(8, idx=Hybrid(3).rle(5, 1).packed([1, 2, 3], drop=1)).case("indices/packed_last_group_padding_cut"))
    return C


def _width_cases():
    """every index width 0..32; above 3 bits the indices stay below 8 (the high bits are zero, the width byte is what it is).  Each
    stream has bit-packed runs behind RLE runs of 1, 2, 3 and 4 value bytes, so the runs start at odd and even byte offsets; within a
    run of an odd width `bit & 7` takes every value."""
    C = []
    for bw in range(33):
        rng = np.random.default_rng(bw)
        vmax = min(1 << bw, 8)
        h = _run_program([("bp", 16), ("rle", 3), ("bp", 24), ("rle", 2), ("bp", 9), ("rle", 1), ("rle", 12)], bw, vmax, rng)
        C.append(_Build(I32R, DICT8[:vmax]).page(67, idx=h).case("width/%02d" % bw))
    # parquet-rs writes width 0 for a one-entry dictionary, with its runs: their values take no bytes.  (Width 0 with nothing behind
    # the width byte is refused by Arrow C++ -- "Unexpected end of stream" -- and is among the refused cases.)
    C.append(_Build(I32R, [42]).page(70, idx=Hybrid(0).rle(70, 0)).case("width/00_with_run"))
    C.append(_Build(I32O, [42]).page(70, _levels_of([int(i % 3 != 1) for i in range(70)]), idx=Hybrid(0).packed([0] * 24).rle(30, 0), kind="v2").case("width/00_packed_and_rle_runs"))
    odd = Hybrid(7).rle(1, 5).packed([int(v) for v in np.random.default_rng(7).integers(0, 8, 40)])
    C.append(_Build(I32O, DICT8).page(41, Hybrid(1).rle(41, 1), idx=odd, kind="v2").case("width/07_at_odd_offset"))
    return C


def _levels_of(pattern):
    return Hybrid(1).auto(pattern)


def _optional_cases():
    C = []
    n = 130
    for name, lv in [("all_null", [0] * n), ("no_null", [1] * n), ("null_at_row_0", [0] + [1] * (n - 1)), ("null_at_last_row", [1] * (n - 1) + [0]),
                     ("every_third", [int(i % 3 != 0) for i in range(n)])]:
        for kind in ("v1", "v2"):
            C.append(_Build(I32O).page(n, _levels_of(lv), kind=kind).case("optional/%s_%s" % (name, kind)))
            C.append(_Build(STRO, [b"", b"a", "café ☃".encode()]).page(n, _levels_of(lv), idx=Hybrid(2).auto([i % 3 for i in range(sum(lv))]), kind=kind)
                     .case("optional/%s_%s_string_dict" % (name, kind)))
    # row0 of the second and third page is no multiple of 64: the validity words are shared between pages
    rng = np.random.default_rng(37)
    b = _Build(I32O)
    for k in (37, 64, 91):
        b.page(k, _levels_of([int(v) for v in rng.integers(0, 2, k)]), kind="v1" if k != 64 else "v2")
    C.append(b.case("optional/pages_37_64_91"))
    b = _Build(Leaf(BOOL, True, "bool"))
    for k in (37, 64, 91):
        lv = [int(v) for v in rng.integers(0, 2, k)]
        b.page(k, _levels_of(lv), vals=[int(v) for v in rng.integers(0, 2, k)])
    C.append(b.case("optional/pages_37_64_91_bool"))
    # an all-NULL dictionary-encoded v2 page: with the width byte, and (no value, so no index stream at all) without it.  Arrow C++
    # reads the latter (DictDecoder::SetData accepts a zero-length buffer), so it is valid here too.
    C.append(_Build(I32O, DICT8).page(70, _levels_of([0] * 70), idx=Hybrid(3), kind="v2").page(5, idx=Hybrid(3).rle(5, 2)).case("optional/all_null_dict_v2_width_byte"))
    C.append(_Build(I32O, DICT8).page(70, _levels_of([0] * 70), idx=Hybrid(3), kind="v2", width_byte=False).page(5, idx=Hybrid(3).rle(5, 2))
             .case("optional/all_null_dict_v2_no_width_byte"))
    return C


def _incompressible(n, seed):
    return [int(v) for v in np.random.default_rng(seed).integers(-2**31, 2**31, n)]


def _page_kind_cases():
    C = []
    rng = np.random.default_rng(5)
    for kind in ("v1", "v2"):
        for denc, penc, nm in ((PLAIN_DICTIONARY, PLAIN_DICTIONARY, "plain_dictionary"), (PLAIN, RLE_DICTIONARY, "rle_dictionary")):
            ix = Hybrid(3).auto([int(v) for v in rng.integers(0, 8, 150)])
            C.append(_Build(I32O, DICT8, dict_enc=denc).page(200, _levels_of([int(i % 4 != 1) for i in range(200)]), idx=ix, kind=kind, enc=penc).case("kinds/%s_%s" % (nm, kind)))
    # the writer's dictionary overflowed: dictionary-encoded pages, then PLAIN pages, in one chunk
    C.append(_Build(I32R, DICT8).page(100, idx=Hybrid(3).auto([i % 8 for i in range(100)])).page(77).page(30, idx=Hybrid(4).auto([7 - i % 8 for i in range(30)]), kind="v2").page(9, kind="v2")
             .case("kinds/dictionary_then_plain_fallback"))
    # parquet-rs leaves a v2 page uncompressed (is_compressed = false) when the codec does not shrink it: stored next to compressed pages
    for codec in ("snappy", "zstd", "lz4_raw"):
        b = _Build(I32O, DICT8, codec=codec)
        b.page(300, _levels_of([int(i % 5 != 0) for i in range(300)]), kind="v2", vals=[7] * 300)
        b.page(257, _levels_of([int(i % 7 != 3) for i in range(257)]), kind="v2", compressed=False, vals=_incompressible(257, 1))
        b.page(64, kind="v1", vals=_incompressible(64, 2))
        b.page(90, _levels_of([1] * 45 + [0] * 45), idx=Hybrid(3).auto([i % 8 for i in range(45)]), kind="v2", compressed=False)
        b.page(120, idx=Hybrid(3).auto([i % 5 for i in range(120)]), kind="v2")
        C.append(b.case("kinds/v2_uncompressed_pages_in_%s_chunk" % codec))
        C.append(_Build(I32R, codec=codec).page(100, kind="v2", compressed=False).page(1000, kind="v2", vals=[3] * 1000).case("kinds/v2_uncompressed_required_%s" % codec))
    # a v2 BOOLEAN page, values RLE encoded: 4-byte length, then a hybrid stream of 1-bit values
    lv = [int(v) for v in rng.integers(0, 2, 300)]
    bits = Hybrid(1).rle(20, 1).packed([int(v) for v in rng.integers(0, 2, 64)]).rle(200, 0).packed([1, 0, 1])
    body = struct.pack("<I", len(bits.stream())) + bits.stream()
    b = _Build(Leaf(BOOL, True, "bool")).page(300, _levels_of(lv), kind="v2", enc=RLE, vals=bits.values, body=body)
    b.streams.append((1, sum(lv), bits.stream(), bits.values[:sum(lv)]))
    C.append(b.case("kinds/v2_boolean_rle_with_nulls"))
    return C


N_TYPE_ROWS = 75      # not a multiple of 8 (BOOLEAN), NULLs at row 0 and row 74


def _type_cases():
    """one column per type, PLAIN and dictionary encoded, all of N_TYPE_ROWS rows: the columns of one file"""
    C = []
    lv = [0] + [int(i % 6 != 2) for i in range(1, N_TYPE_ROWS - 1)] + [0]
    present = sum(lv)

    def both(name, leaf, pool):
        for opt in (True, False):
            L = leaf._replace(optional=opt)
            n_vals = present if opt else N_TYPE_ROWS
            vs = [pool[i % len(pool)] for i in range(n_vals)]
            C.append(_Build(L).page(N_TYPE_ROWS, _levels_of(lv) if opt else None, vals=vs).case("types/%s_plain_%s" % (name, "optional" if opt else "required")))
            if L.phys != BOOL:
                ix = Hybrid(max(1, (len(pool) - 1).bit_length())).auto([i % len(pool) for i in range(n_vals)])
                C.append(_Build(L, list(pool)).page(N_TYPE_ROWS, _levels_of(lv) if opt else None, idx=ix, kind="v2" if opt else "v1")
                         .case("types/%s_dictionary_%s" % (name, "optional" if opt else "required")))

    both("boolean", Leaf(BOOL, True, "bool"), [1, 1, 0, 1, 0, 0, 0, 1, 1, 1, 0])
    both("int8", Leaf(INT32, True, "int8", converted=15), [-128, 127, -1, 0, 5])
    both("int16", Leaf(INT32, True, "int16", logical=("int", 16, True)), [-32768, 32767, -1, 0])
    both("uint8", Leaf(INT32, True, "uint8", logical=("int", 8, False)), [0, 255, 128, 1])
    both("uint16", Leaf(INT32, True, "uint16", converted=12), [0, 65535, 32768])
    both("uint32", Leaf(INT32, True, "uint32", logical=("int", 32, False)), [0, -1, -(1 << 31), (1 << 31) - 1])      # physical int32: 2^32-1, 2^31
    both("date32", Leaf(INT32, True, "date32", logical=("date",)), [-25567, 0, 19000, -1])
    both("decimal_9_2", Leaf(INT32, True, "decimal", converted=5, scale=2, precision=9), [-999999999, 999999999, -1, 0, 12345])
    both("int64", Leaf(INT64, True, "int64"), [-(1 << 63), (1 << 63) - 1, -1, 0])
    both("uint64", Leaf(INT64, True, "uint64", logical=("int", 64, False)), [-1, -(1 << 63), 0, 1])
    for unit in ("ms", "us", "ns"):
        both("timestamp_" + unit, Leaf(INT64, True, "timestamp[%s]" % unit, logical=("ts", unit)), [-86400001, 0, 1700000000123, -1])
    both("decimal_18_2", Leaf(INT64, True, "decimal", logical=("decimal", 18, 2), scale=2, precision=18), [-(10**18 - 1), 10**18 - 1, -1, 0])
    both("float", Leaf(FLOAT, True, "float32"), [0x80000000, 0x7FC00001, 0xFFC12345, 0x7F800000, 0x3F800000, 0x00000001, 0x7FA00000])      # -0.0, NaN payloads
    both("double", Leaf(DOUBLE, True, "float64"), [1 << 63, 0x7FF8000000000001, 0xFFF8DEADBEEF0001, 0x7FF0000000000000, 0x3FF0000000000000, 1])
    day = 86400 * 10**9
    both("int96", Leaf(INT96, True, "timestamp[ns]"), [-day * 25567 + 1, -1, 0, 1235865600 * 10**9, day * 20000 + 86399999999999, -day - 123456789])
    for length in range(1, 17):
        top = 10 ** FLBA_PRECISION[length - 1] - 1
        leaf = Leaf(FLBA, True, "decimal", length=length, converted=5, logical=("decimal", FLBA_PRECISION[length - 1], 2), scale=2, precision=FLBA_PRECISION[length - 1])
        both("flba_decimal_%02d" % length, leaf, [top, -top, -1, 0, 1, -(top // 3)])
    both("string", STRO, [b"", b"a", "café ☃".encode(), b"x" * 40, "\U0001F600".encode(), b"a-string-longer-than-fifteen-bytes"])
    return C


def _header_cases():
    b = _Build(I32O, DICT8, dict_kw=dict(unknown=True, crc=True))
    b.page(70, _levels_of([int(i % 3 != 0) for i in range(70)]), idx=Hybrid(3).auto([i % 8 for i in range(47)]), stats=True, crc=True)
    b.pages.append(Page("index", 0, b"\x00" * 13))
    b.page(33, _levels_of([1] * 33), kind="v2", stats=True, crc=True, unknown=True)
    b.pages.append(Page("index", 0, b"\x15\x00" * 9, unknown=True))
    b.page(65, _levels_of([0] * 65), unknown=True)
    return [b.case("headers/statistics_crc_unknown_fields_index_pages")]


def _random_cases(seed=2025, count=100):
    """seeded random run programs: widths, run kinds and lengths, NULL patterns, page splits, page versions, codecs"""
    C = []
    rng = np.random.default_rng(seed)
    leaves = [I32O, I32R, STRO, Leaf(INT64, True, "int64")]
    pools = {BYTE_ARRAY: [b"", b"a", b"BUILDING", "café".encode(), b"x" * 40, b"row", b"q", b"zz"], INT32: DICT8, INT64: [v * (1 << 31) for v in DICT8]}

    def program(total, vmax, bw):
        h, left = Hybrid(bw), total
        while left > 0:
            k = int(rng.choice([1, 2, 7, 8, 9, 31, 63, 64, 65, 100, 250]))
            if rng.random() < 0.5:
                h.rle(k, int(rng.integers(0, vmax)), header_width=int(rng.integers(1, 4)) if k < 64 else None)
                left -= k
            else:
                h.packed([int(v) for v in rng.integers(0, vmax, min(k, 250))], header_width=2 if rng.random() < 0.2 else None)
                left -= (min(k, 250) + 7) // 8 * 8
        return h

    for i in range(count):
        leaf = leaves[i % len(leaves)]
        codec = ["none", "snappy", "zstd", "lz4_raw"][int(rng.integers(0, 4))]
        pool = pools[leaf.phys]
        use_dict = rng.random() < 0.7
        b = _Build(leaf, pool if use_dict else None, codec=codec, dict_enc=int(rng.choice([PLAIN, PLAIN_DICTIONARY])))
        for _ in range(int(rng.integers(1, 4))):
            n = int(rng.choice([1, 37, 63, 64, 65, 91, 200, 513, 700]))
            lv = program(n, 2, 1) if leaf.optional else None
            present = sum(lv.values[:n]) if lv else n
            kind = "v2" if rng.random() < 0.5 else "v1"
            kw = dict(compressed=bool(rng.random() < 0.6)) if kind == "v2" else {}
            if use_dict and rng.random() < 0.8:
                bw = int(rng.choice([3, 3, 4, 5, 8, 11, 16, 17, 23, 32]))
                b.page(n, lv, idx=program(present, 8, bw), kind=kind, enc=int(rng.choice([PLAIN_DICTIONARY, RLE_DICTIONARY])), **kw)
            else:
                b.page(n, lv, kind=kind, vals=[pool[int(v)] for v in rng.integers(0, 8, present)], **kw)
        C.append(b.case("random/%03d" % i))
    return C


def _refused_cases():
    C = []
    M, U = "malformed", "unsupported"

    def lvl(name, levels, n, reason, expect=M, kind="v1", **kw):
        """an OPTIONAL INT32 PLAIN page with the given level stream (a well-formed page in front of it)"""
        b = _Build(I32O).page(20, kind=kind)
        present = kw.pop("present", n)
        b.pages.append(Page(kind, n, plain(I32O, list(range(present))), levels, **kw))
        C.append(Case("refused/" + name, I32O, Chunk(b.pages), expect, None, reason, []))

    def idx(name, stream, n, reason, dict_vals=DICT8, expect=M, width=None, **kw):
        b = _Build(I32R, dict_vals).page(20, idx=Hybrid(3).rle(20, 0))
        b.pages.append(Page("v1", n, bytes([3 if width is None else width]) + stream, None, RLE_DICTIONARY, **kw))
        C.append(Case("refused/" + name, I32R, Chunk(b.pages), expect, None, reason, []))

    # 1. BIT_PACKED definition levels (v1 only; no length prefix).  Arrow C++ decodes them; the device does not: status 3, by name.
    # The spec packs them from the most significant bit; Arrow C++ reads them from the least significant one.  The two bytes here
    # (0xBD, 0xE7) read the same in both directions, so the recorded column is what either reading gives.
    lv16 = [1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 0, 0, 1, 1, 1]
    assert bit_packed_levels(lv16) == bit_packed_levels(lv16[7::-1] + lv16[:7:-1]) == b"\xbd\xe7"
    b = _Build(I32O).page(20)
    it = iter(range(12))
    b.rows += [next(it) if l else None for l in lv16]
    b.pages.append(Page("v1", 16, plain(I32O, list(range(12))), bit_packed_levels(lv16), def_enc=BIT_PACKED, prefix=False))
    C.append(b.case("refused/bit_packed_definition_levels", U, "scanfmt.cpp: definition_level_encoding 4 of an optional column"))
    # 2. an RLE run header without its value bytes
    lvl("levels_rle_header_without_value_last", Hybrid(1).rle(10, 1).rle(10, 0, value_bytes=0).stream(), 20, "pq_hybrid: the run's value byte lies past the stream", present=20)
    lvl("levels_rle_header_without_value_middle", Hybrid(1).rle(8, 1).rle(8, 1, value_bytes=0).packed([1] * 8).stream(), 24,
        "the next run's header (3) is taken as the value: out of range, and the stream then ends early", present=24)
    lvl("levels_rle_header_without_value_v2", Hybrid(1).rle(10, 1).rle(10, 0, value_bytes=0).stream(), 20, "pq_hybrid, v2 level bytes", kind="v2", present=20)
    idx("indices_rle_header_without_value_last", Hybrid(3).rle(10, 2).rle(10, 0, value_bytes=0).stream(), 20, "pq_hybrid: the run's value byte lies past the page")
    idx("indices_rle_header_without_value_middle", Hybrid(3).rle(4, 1).rle(4, 2, value_bytes=0).rle(1, 2).stream(), 9,
        "08 01 | 08 | 02 02: the third header is taken as the second run's value, the value 02 as a header without value")
    idx("indices_rle_two_value_bytes_one_present", Hybrid(9).rle(10, 2).rle(10, 1, value_bytes=1).stream(), 20, "width 9: two value bytes, one present", width=9)
    # bit-packed run cut short.  Arrow C++ refuses a bit-packed run whose bytes end before the values asked for do; so does the device.
    # (Bytes missing only from the padding of the last group, beyond the values read, are tolerated by both: indices/packed_last_group_padding_cut.)
    idx("indices_packed_run_cut_short", Hybrid(3).packed([1] * 64, drop=9).stream(), 64, "pq_hybrid: the run's bytes for the values read lie past the page")
    idx("indices_packed_last_group_values_cut", Hybrid(3).rle(5, 1).packed([1, 2, 3], drop=2).stream(), 8, "pq_hybrid: 9 bits of indices are read, 8 are there")
    lvl("levels_packed_run_cut_short",Hybrid(1).packed([1] * 64, drop=3).stream(), 64, "pq_hybrid: 5 of 8 level bytes", present=64)
    # 3. definition levels above the column's maximum
    for v in (2, 3):
        lvl("level_value_%d_at_width_1" % v, Hybrid(1).rle(6, 1).rle(6, v).stream(), 12, "an RLE run's value %d > max level 1" % v, present=12)
    # 4. counts and lengths
    lvl("levels_run_count_0", Hybrid(1).rle(6, 1).rle(0, 1).rle(6, 1).stream(), 12, "pq_hybrid: run count 0", present=12)
    lvl("levels_packed_count_0", Hybrid(1).rle(6, 1).packed([], groups=0).rle(6, 1).stream(), 12, "pq_hybrid: 0 groups", present=12)
    idx("indices_run_count_0", Hybrid(3).rle(6, 1).rle(0, 1).rle(6, 1).stream(), 12, "pq_hybrid: run count 0")
    lvl("levels_shorter_than_num_values", Hybrid(1).rle(6, 1).packed([1] * 8).stream(), 30, "14 levels for 30 values", present=30)
    lvl("levels_v1_prefix_past_page", Hybrid(1).rle(12, 1).stream(), 12, "k_pq_decode: dend > end", level_len=5000, present=12)
    lvl("levels_v1_prefix_huge", Hybrid(1).rle(12, 1).stream(), 12, "k_pq_decode: dend > end, length 0xFFFFFFF0", level_len=0xFFFFFFF0, present=12)
    lvl("levels_v2_length_exceeds_page", Hybrid(1).rle(12, 1).stream(), 12, "scanfmt.cpp: v2 page levels exceed the page", kind="v2", level_len=5000, present=12)
    lvl("v2_repetition_levels", Hybrid(1).rle(12, 1).stream(), 12, "scanfmt.cpp: repetition levels in a flat column", kind="v2", rep_len=2, present=12)
    # 5. dictionary indices
    idx("index_width_0_empty_stream", b"", 12, "width 0, no run behind the width byte: the headers must still announce the values (Arrow C++: Unexpected end of stream)", dict_vals=[42], width=0)
    for w in (33, 255):
        idx("index_width_%d" % w, Hybrid(3).rle(12, 1).stream(), 12, "k_pq_decode: bw > 32", width=w)
    idx("index_equal_to_dictionary_size", Hybrid(3).rle(11, 1).rle(1, 5).stream(), 12, "k_pq_decode: k >= D.n", dict_vals=DICT8[:5])
    idx("index_above_dictionary_size", Hybrid(3).packed([0, 1, 2, 3, 4, 0, 7, 1]).rle(4, 1).stream(), 12, "k_pq_decode: k >= D.n, in a bit-packed run", dict_vals=DICT8[:5])
    # pq_unpack's 5-byte window and its mask at width >= 32: an index whose only set bits are the top ones, at a bit offset of 7 and
    # of 0.  A window or mask that drops them would turn these into valid small indices.
    idx("index_top_bit_at_width_31_bit_offset_7", Hybrid(31).packed([0, 0x40000001, 0, 0, 0, 0, 0, 0]).rle(4, 1).stream(), 12, "k_pq_decode: k >= D.n, bits 61..62 of the run", width=31)
    idx("index_top_bit_at_width_32", Hybrid(32).packed([0, 1, 2, 0x80000002, 0, 0, 0, 0]).rle(4, 1).stream(), 12, "k_pq_decode: k >= D.n compared unsigned", width=32)
    idx("index_far_above_dictionary_size",Hybrid(32).rle(12, 0xFFFFFFFF).stream(), 12, "k_pq_decode: k >= D.n as unsigned", width=32)
    # 6. dictionary pages
    b = _Build(I32R, DICT8).page(20, idx=Hybrid(3).rle(20, 1))
    b.pages[0].n = 9
    C.append(b.case("refused/fixed_dictionary_num_values_exceeds_bytes", M, "scanfmt.cpp: dictionary page shorter than its value count")._replace(values=None))
    sdict = [b"a", b"bc", b"def"]
    b = _Build(STRO, sdict).page(20, idx=Hybrid(2).rle(20, 1))
    b.pages[0].n = 4
    C.append(b.case("refused/string_dictionary_num_values_exceeds_bytes", M, "k_pq_dict_strings: end - q < 4")._replace(values=None))
    b = _Build(STRO, sdict).page(20, idx=Hybrid(2).rle(20, 1))
    b.pages[0].values = b.pages[0].values[:-7] + struct.pack("<I", 300) + b"def"
    C.append(b.case("refused/string_dictionary_length_past_page", M, "k_pq_dict_strings: len > end - q")._replace(values=None))
    b = _Build(I32R).page(20)
    b.pages.append(Page("v1", 12, b"\x03" + Hybrid(3).rle(12, 1).stream(), None, RLE_DICTIONARY))
    C.append(b.case("refused/dictionary_page_missing", M, "scanfmt.cpp: dictionary-encoded page before any dictionary page")._replace(values=None))
    # 7. PLAIN pages shorter than their present values, every physical type
    shorts = [(Leaf(BOOL, False, "bool"), [1] * 20, 1), (I32R, [1] * 20, 1), (Leaf(INT64, False, "int64"), [1] * 20, 1), (Leaf(INT96, False, "timestamp[ns]"), [1] * 20, 1),
              (Leaf(FLOAT, False, "float32"), [1] * 20, 3), (Leaf(DOUBLE, False, "float64"), [1] * 20, 8), (Leaf(FLBA, False, "decimal", length=5, converted=5, scale=2, precision=11), [1] * 20, 1),
              (Leaf(BYTE_ARRAY, False, "string", converted=0), [b"ab"] * 20, 1)]
    for leaf, vals, cut in shorts:
        b = _Build(leaf).page(20, vals=vals).page(20, vals=vals)
        b.pages[1].values = b.pages[1].values[:-cut]
        C.append(b.case("refused/plain_page_short_phys_%d" % leaf.phys, M, "k_pq_decode: need > have (BYTE_ARRAY: the serial walk)")._replace(values=None))
    b = _Build(I32O).page(20, _levels_of([1] * 10 + [0] * 10)).page(20, _levels_of([1] * 20))
    b.pages[1].values = b.pages[1].values[:40]
    C.append(b.case("refused/plain_page_short_optional", M, "20 levels say present, 10 values follow")._replace(values=None))
    b = _Build(STRO).page(20, vals=[b"abc"] * 20)
    b.pages[0].values = b.pages[0].values[:7 * 9] + struct.pack("<I", 1 << 20) + b.pages[0].values[7 * 9 + 4:]
    C.append(b.case("refused/byte_array_length_past_page", M, "k_pq_decode: q > end in the serial walk")._replace(values=None))
    b = _Build(STRO).page(20, vals=[b"abc"] * 20)
    b.pages[0].values = b.pages[0].values[:7 * 9] + struct.pack("<I", 0xFFFFFFFF) + b.pages[0].values[7 * 9 + 4:]
    C.append(b.case("refused/byte_array_length_minus_one", M, "a length of 2^32-1 must not wrap the walk backwards")._replace(values=None))
    # 8. the chunk's value count against its pages
    for nm, nv in (("more", 50), ("fewer", 70)):
        C.append(_Build(I32R).page(30).page(30).case("refused/pages_hold_%s_than_num_values" % nm, M, "scanfmt.cpp: pages hold 60 values, the chunk declares %d" % nv, num_values=nv)._replace(values=None))
    # 9. an encoding the device does not decode.  A well-formed DELTA_BINARY_PACKED page: block size 128, 4 miniblocks, 5 values,
    # first value 7 (zigzag 14), one block: min delta 1 (zigzag 2), four miniblock widths of 0.
    delta = varint(128) + varint(4) + varint(5) + varint(14) + varint(2) + b"\x00\x00\x00\x00"
    b = _Build(I32R).page(20)
    b.page(5, enc=DELTA_BINARY_PACKED, vals=[7, 8, 9, 10, 11], body=delta)
    C.append(b.case("refused/delta_binary_packed_page", U, "scanfmt.cpp: data page encoding 5"))
    return C


# malformed cases Arrow C++'s reader accepts all the same: name -> why (at most 3; test_cpu_parquet_pages.py holds it to that)
PYARROW_READS_ANYWAY = {
    "refused/pages_hold_fewer_than_num_values": "Arrow C++ stops at the end of the chunk's bytes and returns the 60 values it found; the footer's count goes unchecked",
    "refused/pages_hold_more_than_num_values": "Arrow C++ reads whole pages until it has the row group's 50 rows and drops the rest; the count is not compared",
}


@functools.lru_cache(maxsize=None)
def corpus():
    return tuple(_hybrid_cases() + _width_cases() + _optional_cases() + _page_kind_cases() + _type_cases() + _header_cases() + _random_cases() + _refused_cases())


def cases(prefix="", expect=None):
    return [c for c in corpus() if c.name.startswith(prefix) and (expect is None or c.expect == expect)]


def batches():
    """the valid cases as few files: the type cases as the columns of one file, every other family as row groups per leaf"""
    out = [("types/*", "columns", cases("types/", "valid"))]
    for fam in ("levels/", "indices/", "width/", "optional/", "kinds/", "headers/", "random/"):
        by_leaf = {}
        for c in cases(fam, "valid"):
            by_leaf.setdefault(c.leaf, []).append(c)
        for k, (leaf, cs) in enumerate(by_leaf.items()):
            out.append(("%s*%d" % (fam, k), "groups", cs))
    return out
