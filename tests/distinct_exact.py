"""What agg(DISTINCT x) computes, restated in exact arithmetic: the reference of tests/test_cpu_distinct.py and tests/test_gpu_distinct.py.
A group's DISTINCT aggregate runs over the *set* of its non-NULL values; two values are the same when their bytes are the same (a float
by its bit pattern: -0.0 and 0.0 are two values, NaNs differ by payload).  Integers are Python ints wrapped to the result's width at the
end (wrapping commutes with + and ^), decimals Python ints wrapped at 128 bits, floats fractions.Fraction with the sum of magnitudes next
to them, for the error bound.  test_the_restatement_on_a_known_table pins all of it on a dozen rows whose answers were written by hand."""
import math
import struct
from fractions import Fraction

from window_exact import wrap

U = Fraction(1, 2 ** 53)      # unit roundoff of Float64
FLOATS = ("Float32", "Float64")
#            result bits, signed      (SUM of the narrow integers is Int64 / UInt64; BIT_XOR keeps the argument's type)
SUM_WIDTH = {"Int8": (64, True), "Int16": (64, True), "Int32": (64, True), "Int64": (64, True), "UInt8": (64, False), "UInt16": (64, False), "UInt32": (64, False),
             "UInt64": (64, False), "Decimal": (128, True)}
XOR_WIDTH = {"Int8": (8, True), "Int16": (16, True), "Int32": (32, True), "Int64": (64, True), "UInt8": (8, False), "UInt16": (16, False), "UInt32": (32, False),
             "UInt64": (64, False)}


def identity(v, tname):
    """What two values are compared by: their bytes."""
    if tname == "Float64":
        return struct.unpack("<Q", struct.pack("<d", v))[0]
    if tname == "Float32":
        return struct.unpack("<I", struct.pack("<f", v))[0]
    return v


def sets(keys, vals, tname):
    """keys: one tuple per row (() when ungrouped); vals: one value per row, None = NULL (a row its FILTER does not pass is a NULL too).
    {key: {identity: value}} in order of first appearance; a group whose values are all NULL has an empty set."""
    out = {}
    for k, v in zip(keys, vals):
        s = out.setdefault(k, {})
        if v is not None:
            s.setdefault(identity(v, tname), v)
    return out


def count(s):
    return len(s)


def total(s, tname):
    """SUM(DISTINCT): None over the empty set; an int wrapped at the result's width; for floats (exact sum, sum of magnitudes, k) as
    Fractions -- or a float (nan / inf / -inf) when the set holds a value that is not finite, by IEEE's rules for sums."""
    if not s:
        return None
    if tname in FLOATS:
        vals = [float(v) for v in s.values()]
        if any(math.isnan(v) for v in vals) or (math.inf in vals and -math.inf in vals):
            return math.nan
        if math.inf in vals or -math.inf in vals:
            return math.inf if math.inf in vals else -math.inf
        return sum((Fraction(v) for v in vals), Fraction(0)), sum((abs(Fraction(v)) for v in vals), Fraction(0)), len(vals)
    bits, signed = SUM_WIDTH[tname]
    return wrap(sum(int(v) for v in s.values()), bits, signed)


def bit_xor(s, tname):
    if not s:
        return None
    bits, signed = XOR_WIDTH[tname]
    x = 0
    for v in s.values():
        x ^= int(v) & ((1 << bits) - 1)
    return wrap(x, bits, signed)


def float_sum_ok(got, exact):
    """A Float64 sum of k values in any order of combination is within (k - 1) u sum|x| of the exact one (tests/float_agg_exact.py has
    the derivation: each of the k - 1 additions rounds once, to first order)."""
    if isinstance(exact, float):
        return (math.isnan(got) and math.isnan(exact)) or got == exact
    s, mag, k = exact
    return math.isfinite(got) and abs(Fraction(got) - s) <= (k - 1) * U * mag
