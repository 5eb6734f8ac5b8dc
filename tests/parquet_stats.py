"""Parquet files with chosen chunk Statistics, for row-group pruning (csrc/parquet_prune.h, gpuq_parquet_prune).

Two sources.  pyarrow writes min_value / max_value / null_count per row group, for every type the pruning compares: those files make
the soundness corpus, each with predicates stated twice -- as the expression JSON the executor carries and as a pyarrow compute
expression the test evaluates over the rows of every dropped group.  What pyarrow cannot write is assembled by hand with TStruct from
parquet_pages.py: statistics in the deprecated fields only, values of the wrong length, min > max, no null_count, unknown Thrift
fields inside the Statistics struct.  Plain Python and pyarrow's CPU code: nothing here touches the GPU.

parquet.thrift: Statistics {1 max, 2 min (deprecated: written in signed order whatever the type), 3 null_count, 4 distinct_count,
5 max_value, 6 min_value, 7 is_max_value_exact, 8 is_min_value_exact}; ColumnMetaData field 12.
"""
import decimal
import io
import struct
from collections import namedtuple

import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.parquet as pq

import parquet_pages as PP
from arrow_ballista_amd import expr as E
from compressed_streams import PQ_CODECS, _zz, varint
from parquet_pages import BYTE_ARRAY, FLBA, INT32, INT64, Leaf, Page, TStruct


# ---------------------------------------------------------------- hand-built files
def statistics(max_deprecated=None, min_deprecated=None, null_count=None, distinct=None, max_value=None, min_value=None, max_exact=None, min_exact=None,
               unknown=False):
    s = TStruct()
    if max_deprecated is not None:
        s.string(1, max_deprecated)
    if min_deprecated is not None:
        s.string(2, min_deprecated)
    if null_count is not None:
        s.i64(3, null_count)
    if distinct is not None:
        s.i64(4, distinct)
    if max_value is not None:
        s.string(5, max_value)
    if min_value is not None:
        s.string(6, min_value)
    if max_exact is not None:
        s.bool(7, max_exact)
    if min_exact is not None:
        s.bool(8, min_exact)
    if unknown:
        s.unknown_fields(20)
    return s


def stats_file(leaf, groups, name="v"):
    """One REQUIRED column `name` of `leaf`; groups: [(physical values, Statistics TStruct or None)], one PLAIN v1 page each.
    Returns (file bytes, [(start, end) of every Statistics struct inside the footer, as file offsets])."""
    body = bytearray(b"PAR1")
    metas = []
    for vals, st in groups:
        first = len(body)
        b, u = PP._page_bytes(Page("v1", len(vals), PP.plain(leaf, vals)), "none")
        body += b
        cm = (TStruct().i32(1, leaf.phys).list(2, 5, [_zz(PP.PLAIN), _zz(PP.RLE)]).list(3, 8, [varint(len(name)) + name.encode()])
              .i32(4, PQ_CODECS["none"]).i64(5, len(vals)).i64(6, u).i64(7, len(body) - first).i64(9, first))
        if st is not None:
            cm.struct(12, st)
        metas.append((TStruct().structs(1, [TStruct().i64(2, first).struct(3, cm)]).i64(2, len(body)).i64(3, len(vals)), st))
    root = TStruct().string(4, b"schema").i32(5, 1)
    meta = (TStruct().i32(1, 1).structs(2, [root, PP._schema_elem(name, leaf)]).i64(3, sum(len(v) for v, _ in groups)).structs(4, [m for m, _ in metas])
            .string(6, b"parquet_stats.py").bytes())
    data = bytes(body) + meta + struct.pack("<I", len(meta)) + b"PAR1"
    spans, at = [], len(body)
    for _, st in metas:
        if st is not None:
            k = data.index(st.bytes(), at)
            spans.append((k, k + len(st.bytes())))
            at = k + len(st.bytes())
    return data, spans


def le32(v):
    return struct.pack("<i", v)


def le64(v):
    return struct.pack("<q", v)


I32 = Leaf(INT32, False, "int32")
U32 = Leaf(INT32, False, "uint32", logical=("int", 32, False))
STR = Leaf(BYTE_ARRAY, False, "string", converted=0)


# ---------------------------------------------------------------- pyarrow-written files and two-way predicates
def write(table, rows_per_group, **kw):
    buf = io.BytesIO()
    pq.write_table(table, buf, row_group_size=rows_per_group, **kw)
    return buf.getvalue()


def row_group_tables(data):
    f = pq.ParquetFile(io.BytesIO(data))
    return [f.read_row_group(g) for g in range(f.metadata.num_row_groups)]


def first_page_offsets(data):
    """file offset of the first page of the first column chunk of every row group, from pyarrow's reading of the footer"""
    md = pq.ParquetFile(io.BytesIO(data)).metadata
    out = []
    for g in range(md.num_row_groups):
        c = md.row_group(g).column(0)
        out.append(c.dictionary_page_offset if c.has_dictionary_page and c.dictionary_page_offset else c.data_page_offset)
    return out


# A column type of the corpus: the engine's type descriptor, the Arrow type, and values in LITERAL form (what expr.lit takes: ints for
# integers, days, timestamp counts and unscaled decimals; str; bool; float).
Kind = namedtuple("Kind", "name gpuq arrow scale", defaults=(0,))


def array(kind, vals):
    t = kind.arrow
    if pa.types.is_decimal(t):
        return pa.array([None if v is None else decimal.Decimal(v).scaleb(-kind.scale, decimal.Context(prec=40)) for v in vals], type=t)
    if pa.types.is_date32(t):
        return pa.array(vals, type=pa.int32()).cast(t)
    if pa.types.is_timestamp(t):
        return pa.array(vals, type=pa.int64()).cast(t)
    return pa.array(vals, type=t)


def scalar(kind, v):
    return array(kind, [v])[0]


Pred = namedtuple("Pred", "text json arrow")      # what it says, the executor's JSON, pyarrow's expression
OPS = [("=", lambda a, b: a == b), ("!=", lambda a, b: a != b), ("<", lambda a, b: a < b), ("<=", lambda a, b: a <= b), (">", lambda a, b: a > b), (">=", lambda a, b: a >= b)]
FLIP = {"=": "=", "!=": "!=", "<": ">", "<=": ">=", ">": "<", ">=": "<="}


def column(name):
    return E.col(name)


def literal(kind, v):
    return E.lit(v, kind.gpuq)


def compare(kind, name, op, v):
    fn = dict(OPS)[op]
    return Pred("%s %s %r" % (name, op, v), E.binary(column(name), op, literal(kind, v)), fn(pc.field(name), scalar(kind, v)))


def predicates(kind, name, literals):
    """every comparison against every literal, both ways round and negated; IN; IS [NOT] NULL; AND / OR of neighbours"""
    out = []
    for v in literals:
        for op, fn in OPS:
            p = compare(kind, name, op, v)
            out.append(p)
            out.append(Pred("%r %s %s" % (v, FLIP[op], name), E.binary(literal(kind, v), FLIP[op], column(name)), p.arrow))
            out.append(Pred("NOT " + p.text, E.not_(p.json), ~p.arrow))
    for a, b in zip(literals, literals[1:]):
        out.append(Pred("%s IN (%r, %r)" % (name, a, b), E.in_list(column(name), [literal(kind, a), literal(kind, b)]), pc.field(name).isin(array(kind, [a, b]))))
        lo, hi = compare(kind, name, ">=", a), compare(kind, name, "<", b)
        out.append(Pred("%s AND %s" % (lo.text, hi.text), E.and_(lo.json, hi.json), lo.arrow & hi.arrow))
        lt, gt = compare(kind, name, "<", a), compare(kind, name, ">", b)
        out.append(Pred("%s OR %s" % (lt.text, gt.text), E.or_(lt.json, gt.json), lt.arrow | gt.arrow))
    out.append(Pred(name + " IS NULL", E.is_null(column(name)), pc.field(name).is_null()))
    out.append(Pred(name + " IS NOT NULL", E.is_not_null(column(name)), pc.field(name).is_valid()))
    out.append(Pred(name + " = NULL", E.binary(column(name), "=", E.lit(None, "Null")), pc.field(name) == pa.scalar(None, kind.arrow)))
    return out


def ts(unit):
    return Kind("timestamp_" + unit, {"Timestamp": [{"ms": "Millisecond", "us": "Microsecond"}[unit], None]}, pa.timestamp(unit))


def dec(p, s):
    return Kind("decimal_%d_%d" % (p, s), {"Decimal128": [p, s]}, pa.decimal128(p, s), s)


File = namedtuple("File", "name data fields kind groups")      # fields: the FILE schema as field dicts; groups: literal-form values per row group


def typed_file(kind, groups, nullable=True, **kw):
    """one column "v" of `kind`; groups of equal length become the row groups"""
    assert len({len(g) for g in groups}) == 1
    t = pa.table({"v": array(kind, [v for g in groups for v in g])})
    return File(kind.name, write(t, len(groups[0]), **kw), [{"name": "v", "type": kind.gpuq, "nullable": nullable}], kind, groups)


def corpus():
    """[(File, literals to compare against)]: 4-6 row groups of 3-8 rows each, one file per type"""
    out = []

    def add(kind, groups, literals, **kw):
        out.append((typed_file(kind, groups, **kw), literals))
    for bits, t in [(8, pa.int8()), (16, pa.int16()), (32, pa.int32()), (64, pa.int64())]:
        top = (1 << (bits - 1)) - 1
        add(Kind("int%d" % bits, "Int%d" % bits, t), [[-top - 1, -5, -1, None], [0, 1, 2, 3], [5, 5, 5, 5], [9, 40, top, None]], [-top - 1, -1, 0, 3, 5, 9, top])
    add(Kind("uint32", "UInt32", pa.uint32()), [[0, 1, 2], [2**31 - 1, 2**31, 2**31 + 1], [2**32 - 2, 2**32 - 1, 7], [3000000000, 3000000001, None]],
        [0, 2, 7, 2**31 - 1, 2**31, 3000000000, 2**32 - 1])
    add(Kind("uint64", "UInt64", pa.uint64()), [[0, 1, 2], [2**63 - 1, 2**63, 2**63 + 1], [2**64 - 2, 2**64 - 1, 7], [2**63 + 5, 2**63 + 6, None]],
        [0, 2, 7, 2**63 - 1, 2**63, 2**63 + 5, 2**64 - 1])
    add(Kind("date32", "Date32", pa.date32()), [[-30000, -365, -1], [0, 1, 2], [10957, 10958, None], [19000, 19001, 19002]], [-30000, -1, 0, 2, 10957, 19002])
    for unit in ("ms", "us"):
        add(ts(unit), [[-10**12, -1, 0], [1, 2, 3], [10**12, 10**12 + 1, None], [10**15, 10**15 + 7, 10**15 + 9]], [-10**12, 0, 2, 10**12, 10**15 + 9])
    add(dec(9, 2), [[-99999, -100, -1], [0, 1, 2], [100, 101, None], [99999, 5000, 5001]], [-99999, -1, 0, 2, 100, 99999], store_decimal_as_integer=True)
    add(dec(15, 2), [[-10**14, -100, -1], [0, 1, 2], [100, 101, None], [10**14, 5000, 5001]], [-10**14, -1, 0, 2, 100, 10**14], store_decimal_as_integer=True)
    for p in (5, 20, 38):      # FIXED_LEN_BYTE_ARRAY of 3, 9 and 16 bytes
        m = 10**p - 1
        add(dec(p, 2), [[-m, -256, -1], [0, 1, 255], [256, 257, None], [m, 65536, 65537]], [-m, -256, -1, 0, 255, 256, m])
    add(Kind("utf8", "Utf8", pa.string()), [["", "a", "ab"], ["ab", "abc", "abd"], ["b", "é", None], ["ÿ", "€", "z"], ["zz", "zzz", "zzzz"]],
        ["", "a", "ab", "abc", "b", "z", "zz", "é", "€"])
    add(Kind("boolean", "Boolean", pa.bool_()), [[True, True, True], [False, False, False], [True, False, None], [None, None, None]], [True, False])
    nan = float("nan")
    add(Kind("float64", "Float64", pa.float64()), [[nan, 1.0, 2.0], [-0.0, 0.0, -1.0], [nan, nan, nan], [5.0, None, 6.0]], [0.0, -0.0, 1.0, 5.0, 7.0])
    # special row groups: one that is all NULL, and a file without statistics
    add(Kind("int64_all_null_group", "Int64", pa.int64()), [[0, 1, 2, 3], [None, None, None, None], [10, 11, None, 13], [20, 21, 22, 23]], [0, 3, 10, 12, 23])
    add(Kind("int64_no_statistics", "Int64", pa.int64()), [[0, 1, 2], [10, 11, 12], [20, 21, None], [None, None, None]], [0, 11, 20], write_statistics=False)
    return out


def hand_built():
    """{name: (file bytes, Statistics spans, field dicts)}: what pyarrow cannot write.  Four row groups holding 0..2, 10..12, 20..22,
    30..32 (as int32 / uint32) or "a".."c", ... (as strings)."""
    ints = [[0, 1, 2], [10, 11, 12], [20, 21, 22], [30, 31, 32]]
    strs = [[b"a", b"b", b"c"], [b"k", b"l", b"m"], [b"p", b"q", b"r"], [b"x", b"y", b"z"]]
    f32 = [{"name": "v", "type": "Int32", "nullable": False}]
    out = {}
    out["deprecated_int32"] = stats_file(I32, [(g, statistics(max_deprecated=le32(g[-1]), min_deprecated=le32(g[0]), null_count=0)) for g in ints]) + (f32,)
    out["deprecated_uint32"] = stats_file(U32, [(g, statistics(max_deprecated=le32(g[-1]), min_deprecated=le32(g[0]), null_count=0)) for g in ints]) + (
        [{"name": "v", "type": "UInt32", "nullable": False}],)
    out["deprecated_string"] = stats_file(STR, [(g, statistics(max_deprecated=g[-1], min_deprecated=g[0], null_count=0)) for g in strs]) + (
        [{"name": "v", "type": "Utf8", "nullable": False}],)
    out["wrong_length"] = stats_file(I32, [(g, statistics(null_count=0, max_value=le32(g[-1])[:3] if k % 2 else le64(g[-1]), min_value=le32(g[0]))) for k, g in enumerate(ints)]) + (f32,)
    out["min_above_max"] = stats_file(I32, [(g, statistics(null_count=0, max_value=le32(g[0]), min_value=le32(g[-1]))) for g in ints]) + (f32,)
    out["no_null_count"] = stats_file(I32, [(g, statistics(max_value=le32(g[-1]), min_value=le32(g[0]))) for g in ints]) + (f32,)
    out["unknown_fields"] = stats_file(I32, [(g, statistics(null_count=0, distinct=3, max_value=le32(g[-1]), min_value=le32(g[0]), max_exact=True, min_exact=False, unknown=True))
                                             for g in ints]) + (f32,)
    return out
