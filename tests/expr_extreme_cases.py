"""Value tables and expression lists of the expression-extremes tests (test_cpu_expr_exact.py checks them against the reference on the
CPU, test_gpu_expr_extremes.py runs them on the device).  Every table is built from boundary vectors, not random draws: the cross
product of two vectors (one per operand column) plus a Float64 column that cycles through its own vector, a NULL in every column,
tiled to several waves with a ragged tail (n % 64 != 0).  Column values are Python ints (decimals: the unscaled value)."""
import decimal

from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, case, cast, col, date_part, in_list, is_not_null, is_null, lit, negative, not_, substr

import expr_exact as X

F53 = float(2**53)
FLOATS = [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 5e-324, F53 - 1.0, F53, F53 + 2.0, -1.5, None]
PATTERN = 2**63 + 2**11 + 1          # + 2^64 * h: (double)hi * 2^64 + (double)lo rounds twice, float(int) once
PATTERN_H = {20: (1, 2, 4), 25: (1, 3, 2**18 - 1), 38: (1, 2**31 + 1, 2**62 - 1)}


def D(p, s):
    return ("Decimal128", p, s)


def dec_vector(p):
    m = 10**p - 1
    vs = {0, 1, -1, m, -m, m // 2, -(m // 2), 10**(p - 1), -10**(p - 1)}
    if p >= 19:
        for c in (2**63, 2**64):
            for d in (-1, 0, 1):
                vs |= {v for v in (c + d, -(c + d)) if abs(v) <= m}
        for h in PATTERN_H.get(p, ()):
            v = 2**64 * h + PATTERN
            assert v <= m
            vs |= {v, -v}
    return sorted(vs) + [None]


def int_vector(t):
    bits, signed = X._INT[t]
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
    vs = {lo, lo + 1, -1, 0, 1, hi - 1, hi}
    for c in (2**31, 2**32, 2**53):
        vs |= {sg * (c + d) for sg in (1, -1) for d in (-1, 0, 1)}
    return sorted(v for v in vs if lo <= v <= hi) + [None]


def _days(y, m, d):
    import datetime
    return datetime.date(y, m, d).toordinal() - datetime.date(1970, 1, 1).toordinal()


def date_vector():
    vs = {-719162, -1, 0, 2932896}
    for y in (1900, 2000, 2100, 2400):
        vs |= {_days(y, 2, 28), _days(y, 3, 1), _days(y, 3, 1) - 1, _days(y, 12, 31), _days(y + 1, 1, 1)}      # Mar 1 - 1 is Feb 29 in a leap year
    return sorted(vs) + [None]


class Table:
    """name, schema (field dicts), cols (name -> list of Python values), n rows."""

    def __init__(self, name, fields, cols):
        self.name, self.cols = name, cols
        self.n = len(cols["id"])
        self.schema = [{"name": k, "type": X._type(t), "nullable": k not in ("id", "g")} for k, t in fields]
        assert self.n % 64 != 0 and self.n > 128

    def arrow(self):
        import pyarrow as pa
        arrs = []
        for f in self.schema:
            t, v = f["type"], self.cols[f["name"]]
            if X.is_dec(t):
                p, s = t["Decimal128"]
                v = [None if x is None else decimal.Decimal((0 if x >= 0 else 1, tuple(int(c) for c in str(abs(x))), -s)) for x in v]
                pt = pa.decimal128(p, s)
            else:
                pt = {"Int8": pa.int8(), "Int16": pa.int16(), "Int32": pa.int32(), "Int64": pa.int64(), "UInt8": pa.uint8(), "UInt16": pa.uint16(),
                      "UInt32": pa.uint32(), "UInt64": pa.uint64(), "Float64": pa.float64(), "Utf8": pa.string(), "Date32": pa.date32(), "Boolean": pa.bool_()}[t]
            a = pa.array(v, pa.int32()).cast(pa.date32()) if t == "Date32" else pa.array(v, pt)
            arrs.append(a)
        return pa.Table.from_arrays(arrs, schema=pa.schema([pa.field(f["name"], a.type, nullable=f["nullable"]) for f, a in zip(self.schema, arrs)]))


def cross_table(name, ta, va, tb, vb, tiles=None):
    """a x b, tiled to a few thousand rows; f cycles through FLOATS; id is the row number, g = id % 7 the group key."""
    if tiles is None:
        tiles = -(-2000 // (len(va) * len(vb)))
    a = [x for x in va for _ in vb] * tiles
    b = [y for _ in va for y in vb] * tiles
    while len(a) % 64 == 0 or len(a) <= 128:
        a.append(va[0]); b.append(vb[0])
    n = len(a)
    cols = {"id": list(range(n)), "g": [i % 7 for i in range(n)], "a": a, "b": b, "f": [FLOATS[i % len(FLOATS)] for i in range(n)]}
    return Table(name, [("id", "Int32"), ("g", "Int32"), ("a", ta), ("b", tb), ("f", "Float64")], cols)


# ------------------------------------------------------------------------------------------------ expression lists
def _common(s, A, B):
    return [("a_lt_b", binary(A, Op.Lt, B)), ("a_eq_b", binary(A, Op.Eq, B)), ("a_f64", cast(A, "Float64")), ("a_lt_f", binary(A, Op.Lt, col("f", s))),
            ("f_eq_b", binary(col("f", s), Op.Eq, B)), ("a_gt_half", binary(A, Op.Gt, lit(0.5))), ("b_notnull", is_not_null(B)), ("neg_a", negative(A)),
            ("kleene", binary(binary(A, Op.Lt, B), Op.Or, binary(not_(binary(A, Op.Eq, B)), Op.And, is_null(B)))),
            ("case_ab", case([(binary(A, Op.Gt, B), A)], B))]


def decimal_exprs(t):
    """Every operator over two decimal columns whose types leave room for every result (p1 + p2 + 1 <= 38, p1 + 4 + s2 <= 38)."""
    s = t.schema
    A, B = col("a", s), col("b", s)
    (p1, s1), (p2, s2) = (X._ps(f["type"]) for f in s[2:4])
    assert p1 + p2 + 1 <= 38 and p1 + 4 + s2 <= 38
    k7 = lit(7, D(3, 2))
    out = [("add", binary(A, Op.Plus, B)), ("sub", binary(A, Op.Minus, B)), ("mul", binary(A, Op.Multiply, B)), ("div", binary(A, Op.Divide, B)), ("mod", binary(A, Op.Modulo, B)),
           ("add_lit", binary(A, Op.Plus, lit(10**p1 - 1, D(p1, s1)))), ("div_lit", binary(A, Op.Divide, k7)),
           ("lit_div", binary(lit(-(10**9 - 1), D(9, 0)), Op.Divide, B)), ("mod_lit", binary(A, Op.Modulo, k7)), ("a_ne_lit", binary(A, Op.NotEq, lit(10**(p1 - 1), D(p1 + 1, s1 + 1)))),
           ("mul_gt_b", binary(binary(A, Op.Multiply, B), Op.Gt, B)), ("add_sub_a", binary(binary(A, Op.Plus, B), Op.Minus, A)),
           ("mul_f64", cast(binary(A, Op.Multiply, B), "Float64")), ("nega_div_b", binary(negative(A), Op.Divide, B)),
           ("sub_lt_mul", binary(binary(A, Op.Minus, B), Op.Lt, binary(A, Op.Multiply, B))),
           ("up", cast(A, D(p1 + 3, s1 + 2))), ("in_list", in_list(A, [lit(1, D(p1, s1)), lit(-(10**p1 - 1), D(p1, s1)), lit(0, D(1, 0))]))]
    out += [("a_i64", cast(A, "Int64")), ("b_i16_gt", binary(cast(B, "Int16"), Op.Gt, lit(5, "Int16")))]          # Decimal -> integer: to scale 0, then wraps
    if s1 >= 2:
        out.append(("down", cast(A, D(p1, s1 - 2))))
        out.append(("down0", cast(A, D(p1, 0))))
    return out + _common(s, A, B)


def decimal38_exprs(t):
    """Decimal(38, s): what stays inside 38 digits for every value -- same-scale comparisons, %, NEGATIVE, the casts to Float64."""
    s = t.schema
    A, B = col("a", s), col("b", s)
    p1, s1 = X._ps(s[2]["type"])
    return [("mod", binary(A, Op.Modulo, B)), ("mod_lit", binary(A, Op.Modulo, lit(10**19 + 1, D(38, s1)))), ("a_lt_lit", binary(A, Op.Lt, lit(-(2**64), D(38, s1)))),
            ("in_list", in_list(A, [lit(10**38 - 1, D(38, s1)), lit(-(2**64) - 1, D(38, s1))])), ("down0", cast(A, D(38, 0)))] + _common(s, A, B)


def int_exprs(t):
    """Every operator over two columns of one integer type, and the casts to every other numeric type."""
    s = t.schema
    A, B = col("a", s), col("b", s)
    ty = s[2]["type"]
    bits, signed = X._INT[ty]
    hi = (1 << (bits - 1)) - 1 if signed else (1 << bits) - 1
    out = [("add", binary(A, Op.Plus, B)), ("sub", binary(A, Op.Minus, B)), ("mul", binary(A, Op.Multiply, B)), ("div", binary(A, Op.Divide, B)), ("mod", binary(A, Op.Modulo, B)),
           ("add_lit", binary(A, Op.Plus, lit(hi, ty))), ("div_lit", binary(A, Op.Divide, lit(hi, ty))),
           ("mul_gt_b", binary(binary(A, Op.Multiply, B), Op.Gt, B)), ("add_sub_a", binary(binary(A, Op.Plus, B), Op.Minus, A)), ("add_lt_a", binary(binary(A, Op.Plus, B), Op.Lt, A)),
           ("mul_f64", cast(binary(A, Op.Multiply, B), "Float64")), ("sub_div_b", binary(binary(A, Op.Minus, B), Op.Divide, B)),
           ("in_list", in_list(A, [lit(1, ty), lit(hi, ty), lit(hi - 1, ty)])),
           ("dec_mul", binary(cast(A, D(20, 0)), Op.Multiply, lit(10**15 - 1, D(15, 2)))), ("a_lt_dec", binary(A, Op.Lt, lit(-5, D(3, 1))))]
    if signed:
        out += [("div_m1", binary(A, Op.Divide, lit(-1, ty))), ("mod_m1", binary(A, Op.Modulo, lit(-1, ty))), ("nega_div_b", binary(negative(A), Op.Divide, B)),
                ("neg_lt_a", binary(negative(A), Op.Lt, A))]
    flip = ("U" + ty) if signed else ty[1:]                                             # the same width, the other signedness
    for to in sorted({flip, "Int8" if ty != "Int8" else "Int16", "UInt16" if ty != "UInt16" else "UInt8", "Int64" if ty != "Int64" else "UInt32"}):
        out.append(("to_" + to, cast(A, to)))
    narrow = "Int8" if ty != "Int8" else "UInt8"
    out.append(("narrow_gt", binary(cast(A, narrow), Op.Gt, lit(5, narrow))))          # the narrowed value as an intermediate
    out.append(("mul_narrow_i64", cast(cast(binary(A, Op.Multiply, B), narrow), "Int64")))
    common = [(n, e) for n, e in _common(s, A, B) if signed or n != "neg_a"]
    return out + common


def decimal38_sum_exprs(t):
    """+ and - at the capped precision (the checked instructions) over values whose every sum and difference still fits 38 digits."""
    s = t.schema
    A, B = col("a", s), col("b", s)
    sc = X._ps(s[2]["type"])[1]
    half = (10**38 - 1) // 2
    return [("add", binary(A, Op.Plus, B)), ("sub", binary(A, Op.Minus, B)), ("add_lit", binary(A, Op.Plus, lit(half, D(38, sc)))), ("lit_sub", binary(lit(-half, D(38, sc)), Op.Minus, B)),
            ("sub_lt_a", binary(binary(A, Op.Minus, B), Op.Lt, A)), ("add_f64", cast(binary(A, Op.Plus, B), "Float64")), ("nega_sub_b", binary(negative(A), Op.Minus, B)),
            ("add_isnull", is_null(binary(A, Op.Plus, B)))]


def mixed_int_exprs(t):
    """Every operator over two integer columns of different types: the result type is Int64 when either side is 64 bits wide, else Int32."""
    s = t.schema
    A, B = col("a", s), col("b", s)
    return [("add", binary(A, Op.Plus, B)), ("sub", binary(A, Op.Minus, B)), ("mul", binary(A, Op.Multiply, B)), ("div", binary(A, Op.Divide, B)), ("mod", binary(A, Op.Modulo, B)),
            ("b_div_a", binary(B, Op.Divide, A)), ("b_sub_a", binary(B, Op.Minus, A)), ("a_lt_b", binary(A, Op.Lt, B)), ("a_eq_b", binary(A, Op.Eq, B)),
            ("add_lt_b", binary(binary(A, Op.Plus, B), Op.Lt, B)), ("mul_gt_b", binary(binary(A, Op.Multiply, B), Op.Gt, B)), ("mul_f64", cast(binary(A, Op.Multiply, B), "Float64")),
            ("sub_i16", cast(binary(A, Op.Minus, B), "Int16")), ("case_ab", case([(binary(A, Op.Gt, B), A)], B)), ("b_to_a", cast(B, s[2]["type"]))]


def int_decimal_exprs(t):
    """Every operator between an integer column (coerced to Decimal(10 | 20, 0)) and a decimal column, and the Decimal -> integer casts."""
    s = t.schema
    A, B = col("a", s), col("b", s)
    return [("add", binary(A, Op.Plus, B)), ("sub", binary(B, Op.Minus, A)), ("mul", binary(A, Op.Multiply, B)), ("div", binary(A, Op.Divide, B)), ("b_div_a", binary(B, Op.Divide, A)),
            ("mod", binary(A, Op.Modulo, B)), ("b_mod_a", binary(B, Op.Modulo, A)), ("a_lt_b", binary(A, Op.Lt, B)), ("a_eq_b", binary(A, Op.Eq, B)),
            ("mul_gt_a", binary(binary(A, Op.Multiply, B), Op.Gt, A)), ("add_f64", cast(binary(A, Op.Plus, B), "Float64")),
            ("b_i64", cast(B, "Int64")), ("b_i32", cast(B, "Int32")), ("b_u8", cast(B, "UInt8")), ("mul_i64", cast(binary(A, Op.Multiply, B), "Int64")),
            ("b_i8_lt_a", binary(cast(cast(B, "Int8"), "Int64"), Op.Lt, cast(A, "Int64")))]


def date_exprs(t):
    s = t.schema
    A, B = col("a", s), col("b", s)
    return [("year", date_part("YEAR", A)), ("month", date_part("MONTH", A)), ("day", date_part("DAY", A)), ("diff", binary(A, Op.Minus, B)),
            ("plus", binary(B, Op.Plus, lit(1, "Int32"))), ("y2000", binary(date_part("YEAR", A), Op.Eq, lit(2000.0))), ("a_lt_b", binary(A, Op.Lt, B)),
            ("feb29", binary(binary(date_part("MONTH", B), Op.Eq, lit(2.0)), Op.And, binary(date_part("DAY", B), Op.Eq, lit(29.0)))),
            ("a_i64", cast(A, "Int64")), ("diff_f64", cast(binary(A, Op.Minus, B), "Float64")), ("a_isnull", is_null(A))]


# ------------------------------------------------------------------------------------------------ the tables
DEC_PAIRS = [((18, 4), (15, 2)), ((18, 0), (19, 0)), ((20, 0), (9, 2)), ((25, 6), (9, 3))]
INT_TYPES = ["Int8", "Int16", "Int32", "Int64", "UInt8", "UInt16", "UInt32", "UInt64"]
_CACHE = {}


def _make(name):
    kind, _, rest = name.partition(":")
    if kind == "dec":
        (p1, s1), (p2, s2) = DEC_PAIRS[int(rest)]
        t = cross_table(name, D(p1, s1), dec_vector(p1), D(p2, s2), dec_vector(p2))
        return t, decimal_exprs(t)
    if kind == "dec38":
        sc = int(rest)
        t = cross_table(name, D(38, sc), dec_vector(38), D(38, sc), dec_vector(38))
        return t, decimal38_exprs(t)
    if kind == "int":
        v = int_vector(rest)
        t = cross_table(name, rest, v, rest, v)
        return t, int_exprs(t)
    if kind == "date":
        v = date_vector()
        t = cross_table(name, "Date32", v, "Date32", v)
        return t, date_exprs(t)
    if kind == "dec38h":          # Decimal(38, s) values of at most half the range: every sum and difference fits 38 digits
        sc = int(rest)
        v = [x for x in dec_vector(38) if x is None or abs(x) <= (10**38 - 1) // 2]
        t = cross_table(name, D(38, sc), v, D(38, sc), v)
        return t, decimal38_sum_exprs(t)
    if kind == "mix":             # two integer columns of different types
        ta, tb = rest.split(":")
        t = cross_table(name, ta, int_vector(ta), tb, int_vector(tb))
        return t, mixed_int_exprs(t)
    if kind == "mixd":            # an integer column and a decimal column
        ta, p, sc = rest.split(":")
        t = cross_table(name, ta, int_vector(ta), D(int(p), int(sc)), dec_vector(int(p)))
        return t, int_decimal_exprs(t)
    raise KeyError(name)


MIXED = ["mix:Int16:Int32", "mix:Int32:Int64", "mix:UInt32:Int64", "mixd:Int32:9:2", "mixd:Int64:15:2"]
TABLES = ["dec:%d" % i for i in range(len(DEC_PAIRS))] + ["dec38:6", "dec38h:6"] + ["int:" + t for t in INT_TYPES] + MIXED + ["date:"]


def table_and_exprs(name):
    if name not in _CACHE:
        _CACHE[name] = _make(name)
    return _CACHE[name]


_REF = {}


def reference(name):
    """{expr name: (type, values)} over the table, computed once."""
    if name not in _REF:
        t, exprs = table_and_exprs(name)
        _REF[name] = {n: X.evaluate(e, t.schema, t.cols) for n, e in exprs}
    return _REF[name]


# ------------------------------------------------------------------------------------------------ the overflow plans
def _pairs_table(name, ta, tb, pairs, n=193):
    va = [pairs[i % len(pairs)][0] for i in range(n)]
    vb = [pairs[i % len(pairs)][1] for i in range(n)]
    va[5] = None
    vb[11] = None
    cols = {"id": list(range(n)), "g": [i % 7 for i in range(n)], "a": va, "b": vb, "f": [FLOATS[i % len(FLOATS)] for i in range(n)]}
    return Table(name, [("id", "Int32"), ("g", "Int32"), ("a", ta), ("b", tb), ("f", "Float64")], cols)


def overflow_cases():
    """[(name, table, expr)]: every row whose operands are not NULL is OVERFLOW -- arrow-arith raises on each of them.  Each case
    overflows in ONE place: a rescale beyond 127 bits, a product beyond 127 bits, a product between 10^38 and 2^127, a sum and a
    difference of two Decimal(38, 0) values that fit their type while the result does not."""
    big = [10**38 - 1, -(10**38 - 1), 10**37, -(10**37), 2**126 + 1, -(2**126) - 1]
    small = [10**8, -(10**8), 10**9 - 1, -(10**9 - 1), 3 * 10**8, -7 * 10**8]
    t = _pairs_table("overflow", D(38, 6), D(38, 4), [(x, y) for y in small for x in big])
    A, B = col("a", t.schema), col("b", t.schema)
    out = [("div_38_6_by_38_4", t, binary(A, Op.Divide, B)),                         # a * 10^8 leaves 128 bits
           ("mul_38_38", t, binary(A, Op.Multiply, B)),                              # >= 10^45
           ("cmp_rescale", t, binary(A, Op.Lt, cast(B, D(38, 10)))),                 # a * 10^4 for the comparison at scale 10
           ("mod_rescale", t, binary(A, Op.Modulo, cast(B, D(38, 12)))),             # a * 10^6
           ("add_rescaled", t, binary(binary(A, Op.Multiply, lit(10**9, D(10, 0))), Op.Plus, B))]
    m = 10**38 - 1
    same = [(m, 1), (-m, -1), (m, 10**37), (-m, -(10**37)), (m - 5, 6), (-m, -m), (5 * 10**37, 5 * 10**37)]       # a + b = 10^38 at the least: fits 127 bits, not 38 digits
    ta = _pairs_table("overflow_add", D(38, 0), D(38, 0), same)
    ts = _pairs_table("overflow_sub", D(38, 0), D(38, 0), [(x, -y) for x, y in same])
    out.append(("add_38_digits", ta, binary(col("a", ta.schema), Op.Plus, col("b", ta.schema))))
    out.append(("sub_38_digits", ts, binary(col("a", ts.schema), Op.Minus, col("b", ts.schema))))
    p19 = 10**19
    tm = _pairs_table("overflow_mul", D(20, 0), D(20, 0), [(sa * x, sb * y) for x in (p19, 12 * 10**18) for y in (p19, 13 * 10**18) for sa in (1, -1) for sb in (1, -1)])
    out.append(("mul_between_38_digits_and_127_bits", tm, binary(col("a", tm.schema), Op.Multiply, col("b", tm.schema))))      # 10^38 .. 1.56 * 10^38 < 2^127
    return out


def utf8_tables():
    """(name, values): Utf8 for substr -- ASCII at every length up to 16 bytes, and a non-ASCII character behind the kept part, in the
    skipped prefix (a two-byte character in front: skipped whole by start = 3) and inside the kept part, at 14, 15 and 16 bytes."""
    ascii_ = ["", "a", "ab", "abc", "abcdefghijklmn", "abcdefghijklmno", "0123456789", None]
    long16 = ["abcdefghijklmnop", "abc", None]                                               # 16 bytes: exact only while the kept part ends inside 15
    after = ["abcdefghijklé", "abcdefghijklmé", "abcdefghijklmné", "abcdé", None]            # 14, 15, 16 bytes
    prefix = ["éabc", "éabcdefghijkl", "éabcdefghijklm", "éabcdefghijklmn", "éa", None]      # 5, 14, 15, 16, 3 bytes
    inside = ["aéb", "aébc", "abédefghijklm", "abcéefghijklmn", "abécefghijklmno", None]
    out = []
    for name, vals in (("ascii", ascii_), ("long16", long16), ("after", after), ("prefix", prefix), ("inside", inside)):
        n = 131
        out.append((name, [vals[i % len(vals)] for i in range(n)]))
    return out


def substr_is_exact(values, start, length):
    """Whether the device can answer substr(v, start, length) for every value.  Its packed form holds 15 bytes and it counts BYTES, which
    is the documented limit: where it keeps anything, every byte up to the end of the kept part has to be ASCII (then bytes are
    characters) and that end has to lie inside the first 15 bytes.  Where it keeps nothing the answer is '' whatever was skipped."""
    for v in values:
        if v is None:
            continue
        b = v.encode()
        skip = start - 1
        keep = max(0, len(b) - skip)
        if length is not None:
            keep = min(keep, length)
        if keep and (skip + keep > 15 or any(x >= 0x80 for x in b[:skip + keep])):
            return False
    return True


# ------------------------------------------------------------------------------------------------ float accumulators, every strategy
FLOAT_ACC_RUNS = (1, 2, 63, 64, 65, 130)      # key runs that start, end and span a 64-lane wave
_FMAX = 1.7976931348623157e308
_FX_ALL = [0.0, -0.0, float("inf"), float("-inf"), 5e-324, _FMAX, -_FMAX, float("nan"), None]
# fx by group: 0-2 everything; 3 the zeros and the subnormal; 4 the two zeros alone (MIN is -0.0, MAX +0.0 only under the total
# order); 5 everything but NaN; 6 NULL in every row
_FX_BY_GROUP = [_FX_ALL, _FX_ALL, _FX_ALL, [5e-324, 0.0, -0.0, None], [0.0, -0.0, None, -0.0, 0.0], [v for v in _FX_ALL if v == v], [None]]
_ACC_INTS = [-2**63, 2**63 - 1, 0, -1, 1, 2**62, -2**62, 2**53 + 1, None, 7]
_ACC_TABLES = {}


def float_acc_table(order):
    """2275 rows, 7 groups.  "clustered": key runs of every FLOAT_ACC_RUNS length for every key, neighbouring runs under different
    keys; "shuffled": the same rows in a fixed random order.  fx: Float64 specials (_FX_BY_GROUP), fs: Float64 multiples of 2^-10
    below 2^20 in magnitude (any sum of them in any order is exact), i: Int64 with both bounds.  id is the clustered row number."""
    if order not in _ACC_TABLES:
        import random
        g = [r % 7 for r in range(42) for _ in range(FLOAT_ACC_RUNS[r % 6])]
        n = len(g)
        fx = [_FX_BY_GROUP[k][i % len(_FX_BY_GROUP[k])] for i, k in enumerate(g)]
        fs = [None if i % 13 == 5 else ((i * 2654435761) % (2**30) - 2**29) / 1024.0 for i in range(n)]
        iv = [None if k == 6 else _ACC_INTS[i % len(_ACC_INTS)] for i, k in enumerate(g)]
        rows = list(range(n))
        if order == "shuffled":
            random.Random(20240607).shuffle(rows)
        else:
            assert order == "clustered"
        cols = {"id": rows, "g": [g[r] for r in rows], "fx": [fx[r] for r in rows], "fs": [fs[r] for r in rows], "i": [iv[r] for r in rows]}
        _ACC_TABLES[order] = Table("float_acc_" + order, [("id", "Int32"), ("g", "Int32"), ("fx", "Float64"), ("fs", "Float64"), ("i", "Int64")], cols)
    return _ACC_TABLES[order]


def f64_total_key(x):
    """IEEE-754 totalOrder of a double as a signed integer, from its bit pattern: what the project defines MIN / MAX of Float64 by."""
    b = X.f64_bits(x)
    s = b - 2**64 if b >= 2**63 else b
    return s ^ 0x7FFFFFFFFFFFFFFF if s < 0 else s


def fkey_or(x):
    """A value as something == compares bit for bit: a double's bit pattern (NaN included), anything else itself."""
    return X.f64_bits(x) if isinstance(x, float) else x


def float_acc_reference(t):
    """{group: {accumulator name: value}}: MIN / MAX of fx by the total order, SUM of fs in exact rationals, MIN / MAX of i, the counts."""
    import fractions
    out = {}
    for k in sorted(set(t.cols["g"])):
        at = [j for j, gk in enumerate(t.cols["g"]) if gk == k]
        fx, fs, iv = ([t.cols[c][j] for j in at if t.cols[c][j] is not None] for c in ("fx", "fs", "i"))
        total = sum(fractions.Fraction(v) for v in fs)
        assert fractions.Fraction(float(total)) == total
        out[k] = {"min_fx": min(fx, key=f64_total_key) if fx else None, "max_fx": max(fx, key=f64_total_key) if fx else None,
                  "sum_fs": float(total) if fs else None, "cnt_fs": len(fs), "cnt_all": len(at),
                  "min_i": min(iv) if iv else None, "max_i": max(iv) if iv else None, "cnt_i": len(iv)}
    return out
