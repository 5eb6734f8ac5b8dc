"""An exact reference for the expression layer: Python `int` for integers and unscaled decimals, Python `float` for Float64.

A second opinion on expr_compile.cpp / gpuq_dev.h: it shares nothing with them or with oracle/ but the shape of the expression
dicts (arrow_ballista_amd/expr.py) and of the type descriptors ("Int32", {"Decimal128": [p, s]}).

    evaluate(expr, schema, cols) -> (declared result type, [value | None | OVERFLOW per row])

`schema` is a list of {"name", "type"} dicts, `cols` maps a column name to a list of Python values: int for every integer type,
Date32 (days) and Decimal128 (the UNSCALED value), float for Float64, bool, str; None is NULL.

The rules (arrow-rs / DataFusion, as the device code cites them):

Decimal   + -   scale max(s1,s2), precision min(38, max(p1-s1, p2-s2) + scale + 1)
          *     (min(38, p1+p2+1), min(38, s1+s2))
          /     scale rs = min(38, s1+4), precision min(38, p1 + rs-s1+s2); value l * 10^(rs-s1+s2) / r truncated toward zero; x/0 -> NULL
          %     scale max(s1,s2), precision min(38, min(p1-s1, p2-s2) + scale), sign of the dividend; x%0 -> NULL
          integer operands coerce to Decimal(3 | 5 | 10 | 20, 0) by width; a comparison rescales both sides to max(s1,s2)
          a cast that reduces the scale rounds half away from zero
Integer   + - * and NEGATIVE wrap at the node's type width, at every node (arrow's *_wrapping kernels)
          / truncates toward zero, x/0 and x%0 -> NULL; INT_MIN / -1 = INT_MIN and INT_MIN % -1 = 0 (the wrapping answer)
          two operands of one type keep it; otherwise Int64 when either is 64 bits wide, else Int32; Date32 +- int -> Date32,
          Date32 - Date32 -> Int32;  a cast between integer types wraps; Decimal -> integer goes to scale 0 (half away from zero), then wraps
Float64   from an integer: float(int), correctly rounded.  From a decimal: float(int) / 10.0**s (the two operations arrow-rs does)
          a comparison with a float operand casts both sides and uses the IEEE total order: NaN = NaN, -0.0 < 0.0
Boolean   AND, OR, NOT are Kleene; IS NULL / IS NOT NULL never return NULL
CASE      the first WHEN that is true (not NULL); no ELSE -> NULL.  IN list = OR of equalities (Kleene)
date_part YEAR / MONTH / DAY of a Date32 through datetime.date.fromordinal (0001-01-01 .. 9999-12-31), as Float64
substr    counts characters: str slicing of the decoded value
OVERFLOW  where arrow-arith raises: the exact result does not fit the declared result precision, or an operand rescaled by a power
          of ten does not fit 127 bits.  It is sticky: a node with an OVERFLOW operand is OVERFLOW (NULL wins only where the
          OVERFLOW operand is not evaluated at all: the branches of a CASE that are not taken)
"""
import datetime
import math
import struct


class _Overflow:
    def __repr__(self):
        return "OVERFLOW"


OVERFLOW = _Overflow()

_INT = {"Int8": (8, True), "Int16": (16, True), "Int32": (32, True), "Int64": (64, True),
        "UInt8": (8, False), "UInt16": (16, False), "UInt32": (32, False), "UInt64": (64, False)}
_DEC_OF_WIDTH = {8: 3, 16: 5, 32: 10, 64: 20}
_EPOCH_ORDINAL = datetime.date(1970, 1, 1).toordinal()
LIMIT127 = 1 << 127


def is_int(t):
    return isinstance(t, str) and t in _INT


def is_dec(t):
    return isinstance(t, dict) and "Decimal128" in t


def dec(p, s):
    return {"Decimal128": [min(38, p), min(38, s)]}


def _ps(t):
    return t["Decimal128"][0], t["Decimal128"][1]


def _type(t):
    if isinstance(t, (list, tuple)) and t[0] == "Decimal128":
        return {"Decimal128": [int(t[1]), int(t[2])]}
    return t


def wrap(v, t):
    bits, signed = (32, True) if t == "Date32" else _INT[t]
    v &= (1 << bits) - 1
    return v - (1 << bits) if signed and v >> (bits - 1) else v


def as_decimal(t):
    if is_dec(t):
        return t
    if is_int(t):
        return dec(_DEC_OF_WIDTH[_INT[t][0]], 0)
    raise TypeError("no decimal form of %r" % (t,))


def tdiv(a, b):
    q = abs(a) // abs(b)
    return -q if (a < 0) != (b < 0) else q


def tmod(a, b):
    return a - b * tdiv(a, b)


def round_half_away(v, k):
    """v / 10^k rounded half away from zero."""
    d = 10 ** k
    q, r = divmod(abs(v), d)
    if 2 * r >= d:
        q += 1
    return -q if v < 0 else q


def total_order_key(x):
    b = struct.unpack("<q", struct.pack("<d", x))[0]
    return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFF)


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _fits(v, p):
    return abs(v) < 10 ** p


def _rescale_up(v, k):
    """v * 10^k, or OVERFLOW when that leaves 127 bits."""
    r = v * 10 ** k
    return r if -LIMIT127 <= r < LIMIT127 else OVERFLOW


def _map(f, *cols):
    """Row-wise f over non-NULL, non-OVERFLOW operands (OVERFLOW is sticky, then NULL)."""
    out = []
    for vs in zip(*cols):
        if any(v is OVERFLOW for v in vs):
            out.append(OVERFLOW)
        elif any(v is None for v in vs):
            out.append(None)
        else:
            out.append(f(*vs))
    return out


def _to_f64(t, vals):
    if t == "Float64":
        return vals
    if is_int(t) or t == "Date32":
        return _map(float, vals)
    if t == "Boolean":
        return _map(lambda v: 1.0 if v else 0.0, vals)
    if is_dec(t):
        s = _ps(t)[1]
        return _map((lambda v: float(v)) if s == 0 else (lambda v: float(v) / 10.0 ** s), vals)
    raise TypeError("no Float64 form of %r" % (t,))


def _to_scale(t, vals, s):
    """Decimal (or integer) operand at scale s >= its own."""
    d = as_decimal(t)
    k = s - _ps(d)[1]
    return vals if k == 0 else _map(lambda v: _rescale_up(v, k), vals)


def cast(t, vals, to):
    to = _type(to)
    if t == to:
        return to, vals
    if t == "Null":
        return to, [None] * len(vals)
    if to == "Float64":
        return to, _to_f64(t, vals)
    if is_dec(to):
        p, s = _ps(to)
        fs = _ps(as_decimal(t))[1]
        if s >= fs:
            r = _to_scale(t, vals, s)
        else:
            r = _map(lambda v: round_half_away(v, fs - s), vals)
        return to, [OVERFLOW if (v is not None and v is not OVERFLOW and not _fits(v, p)) else v for v in r]
    if is_int(to) or to == "Date32":
        if is_int(t) or t == "Date32":
            return to, _map(lambda v: wrap(v, to), vals)
        if t == "Boolean":
            return to, _map(int, vals)
        if is_dec(t):               # to scale 0 as a decimal cast does (half away from zero), then as an integer cast: wraps
            k = _ps(t)[1]
            return to, _map(lambda v: wrap(round_half_away(v, k), to), vals)
        if t == "Float64":          # NaN, infinities and out-of-range values are out of scope: int() raises for the first two
            return to, _map(lambda v: wrap(int(v), to), vals)
    if to == "Boolean" and is_int(t):
        return to, _map(lambda v: v != 0, vals)
    raise TypeError("cast %r -> %r is not part of the reference" % (t, to))


_CMP = {"=": lambda a, b: a == b, "!=": lambda a, b: a != b, "<": lambda a, b: a < b, "<=": lambda a, b: a <= b,
        ">": lambda a, b: a > b, ">=": lambda a, b: a >= b}
_NORM = {"Plus": "+", "Minus": "-", "Multiply": "*", "Divide": "/", "Modulo": "%", "Eq": "=", "NotEq": "!=", "Lt": "<", "LtEq": "<=",
         "Gt": ">", "GtEq": ">=", "And": "AND", "Or": "OR", "and": "AND", "or": "OR", "<>": "!=", "==": "="}


def _kleene_and(a, b):
    if a is OVERFLOW or b is OVERFLOW:
        return OVERFLOW
    if a is False or b is False:
        return False
    return None if a is None or b is None else True


def _kleene_or(a, b):
    if a is OVERFLOW or b is OVERFLOW:
        return OVERFLOW
    if a is True or b is True:
        return True
    return None if a is None or b is None else False


def _int_result_type(lt, rt, op):
    if lt == rt and is_int(lt):
        return lt
    if lt == "Date32" and rt == "Date32" and op == "-":
        return "Int32"
    if lt == "Date32" or rt == "Date32":
        return "Date32"
    return "Int64" if any(is_int(t) and _INT[t][0] == 64 for t in (lt, rt)) else "Int32"


def binary(op, lt, lv, rt, rv):
    op = _NORM.get(op, op)
    n = len(lv)
    if op in ("AND", "OR"):
        assert lt == "Boolean" and rt == "Boolean"
        return "Boolean", [(_kleene_and if op == "AND" else _kleene_or)(a, b) for a, b in zip(lv, rv)]
    if lt == "Null" and rt != "Null":
        lt, lv = rt, [None] * n
    if rt == "Null" and lt != "Null":
        rt, rv = lt, [None] * n
    if op in _CMP:
        f = _CMP[op]
        if lt == "Float64" or rt == "Float64":
            a, b = _to_f64(lt, lv), _to_f64(rt, rv)
            return "Boolean", _map(lambda x, y: f(total_order_key(x), total_order_key(y)), a, b)
        if is_dec(lt) or is_dec(rt):
            s = max(_ps(as_decimal(lt))[1], _ps(as_decimal(rt))[1])
            return "Boolean", _map(f, _to_scale(lt, lv, s), _to_scale(rt, rv, s))
        if (lt == "Utf8") != (rt == "Utf8"):
            raise TypeError("cannot compare %r with %r" % (lt, rt))
        if lt == "Utf8":
            return "Boolean", _map(lambda x, y: f(x.encode(), y.encode()), lv, rv)
        return "Boolean", _map(f, lv, rv)
    assert op in "+-*/%", op
    if lt == "Float64" or rt == "Float64":
        a, b = _to_f64(lt, lv), _to_f64(rt, rv)

        def fdiv(x, y):
            if y == 0.0:
                return math.nan if (x == 0.0 or x != x) else math.copysign(math.inf, x) * math.copysign(1.0, y)
            return x / y
        fo = {"+": lambda x, y: x + y, "-": lambda x, y: x - y, "*": lambda x, y: x * y, "/": fdiv}[op]
        return "Float64", _map(fo, a, b)
    if is_dec(lt) or is_dec(rt):
        (p1, s1), (p2, s2) = _ps(as_decimal(lt)), _ps(as_decimal(rt))
        if op in "+-":
            s = max(s1, s2)
            t = dec(max(p1 - s1, p2 - s2) + s + 1, s)
            r = _map((lambda a, b: a + b) if op == "+" else (lambda a, b: a - b), _to_scale(lt, lv, s), _to_scale(rt, rv, s))
        elif op == "*":
            t = dec(p1 + p2 + 1, s1 + s2)
            r = _map(lambda a, b: a * b, lv, rv)
        elif op == "/":
            rs = min(38, s1 + 4)
            k = rs - s1 + s2
            t = dec(p1 + k, rs)
            r = _map(lambda a, b: None if b == 0 else tdiv(a, b), _map(lambda v: _rescale_up(v, k), lv), rv)
        else:
            s = max(s1, s2)
            t = dec(min(p1 - s1, p2 - s2) + s, s)
            r = _map(lambda a, b: None if b == 0 else tmod(a, b), _to_scale(lt, lv, s), _to_scale(rt, rv, s))
        p = _ps(t)[0]
        return t, [OVERFLOW if (v is not None and v is not OVERFLOW and not _fits(v, p)) else v for v in r]
    ok = lambda t: is_int(t) or t == "Date32"      # noqa: E731
    if ok(lt) and ok(rt):
        t = _int_result_type(lt, rt, op)
        fo = {"+": lambda a, b: a + b, "-": lambda a, b: a - b, "*": lambda a, b: a * b,
              "/": lambda a, b: None if b == 0 else tdiv(a, b), "%": lambda a, b: None if b == 0 else tmod(a, b)}[op]
        return t, _map(lambda a, b: (lambda z: None if z is None else wrap(z, t))(fo(a, b)), lv, rv)
    raise TypeError("operands of %r: %r, %r" % (op, lt, rt))


def _select_types(tt, ft):
    if tt == "Null":
        return ft
    if ft == "Null" or tt == ft:
        return tt
    if tt == "Float64" or ft == "Float64":
        return "Float64"
    if is_dec(tt) or is_dec(ft):
        (p1, s1), (p2, s2) = _ps(as_decimal(tt)), _ps(as_decimal(ft))
        s = max(s1, s2)
        return dec(max(p1 - s1, p2 - s2) + s, s)
    if is_int(tt) and is_int(ft):
        return "Int64"
    raise TypeError("CASE branches %r, %r" % (tt, ft))


def evaluate(e, schema, cols):
    """(declared type, values) of expression dict `e` over the columns `cols` (name -> list)."""
    n = len(next(iter(cols.values()))) if cols else 0
    (kind, v), = e.items()
    ev = lambda x: evaluate(x, schema, cols)      # noqa: E731
    if kind == "column":
        f = next(f for f in schema if f["name"] == v["name"])
        return _type(f["type"]), list(cols[v["name"]])
    if kind == "literal":
        t = _type(v["type"])
        x = v.get("value")
        if x is not None and t not in ("Utf8", "Boolean", "Float64"):
            x = int(x)
        return t, [x] * n
    if kind == "binary_expr":
        (lt, lv), (rt, rv) = ev(v["l"]), ev(v["r"])
        return binary(v["op"], lt, lv, rt, rv)
    if kind in ("cast", "try_cast"):
        t, vals = ev(v["expr"])
        return cast(t, vals, v["arrow_type"])
    if kind == "not_expr":
        t, vals = ev(v["expr"])
        return "Boolean", _map(lambda x: not x, vals)
    if kind in ("is_null_expr", "is_not_null_expr"):
        t, vals = ev(v["expr"])
        want = kind == "is_null_expr"
        return "Boolean", [OVERFLOW if x is OVERFLOW else ((x is None) == want) for x in vals]
    if kind == "negative":
        t, vals = ev(v["expr"])
        if t == "Float64":
            return t, _map(lambda x: -x, vals)
        if is_dec(t):
            return t, _map(lambda x: -x, vals)
        return t, _map(lambda x: wrap(-x, t), vals)
    if kind == "in_list":
        xt, xv = ev(v["expr"])
        acc = [False] * n
        for it in v["list"]:
            it_t, it_v = ev(it)
            acc = [_kleene_or(a, b) for a, b in zip(acc, binary("=", xt, xv, it_t, it_v)[1])]
        if v.get("negated"):
            acc = _map(lambda x: not x, acc)
        return "Boolean", acc
    if kind == "case_":
        base = ev(v["expr"]) if v.get("expr") is not None else None
        branches = []
        for wt in v["when_then_expr"]:
            w = ev(wt["when_expr"])
            if base is not None:
                w = binary("=", base[0], base[1], w[0], w[1])
            branches.append((w[1], ev(wt["then_expr"])))
        els = ev(v["else_expr"]) if v.get("else_expr") is not None else ("Null", [None] * n)
        t = els[0]
        for _, (tt, _) in reversed(branches):      # the device folds from the last WHEN outward
            t = _select_types(tt, t)
        conv = [(w, cast(tt, tv, t)[1]) for w, (tt, tv) in branches]
        ev_else = cast(els[0], els[1], t)[1]
        out = []
        for i in range(n):
            for w, tv in conv:
                if w[i] is OVERFLOW:
                    out.append(OVERFLOW)
                    break
                if w[i] is True:
                    out.append(tv[i])
                    break
            else:
                out.append(ev_else[i])
        return t, out
    if kind == "scalar_function":
        name = (v.get("name") or v.get("fun")).lower()
        args = v["args"]
        if name in ("date_part", "datepart"):
            part = args[0]["literal"]["value"].upper()
            t, vals = ev(args[1])
            assert t == "Date32"
            pick = {"YEAR": lambda d: d.year, "MONTH": lambda d: d.month, "DAY": lambda d: d.day}[part]
            return "Float64", _map(lambda x: float(pick(datetime.date.fromordinal(x + _EPOCH_ORDINAL))), vals)
        if name in ("substr", "substring"):
            t, vals = ev(args[0])
            start = int(args[1]["literal"]["value"])
            ln = int(args[2]["literal"]["value"]) if len(args) == 3 else None
            assert t == "Utf8" and start >= 1
            return "Utf8", _map(lambda x: x[start - 1:] if ln is None else x[start - 1:start - 1 + ln], vals)
    raise TypeError("expression node %r is not part of the reference" % kind)
