"""The order of ORDER BY, stated exactly and without any packed form: a comparison of two rows under a sort spec, in plain Python.

  integers, decimals (unscaled), dates, booleans   compare as Python ints
  floats                                           IEEE-754 totalOrder of the bit pattern, sign and magnitude:
                                                   -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN, NaNs among themselves by payload.
                                                   The pattern comes from `struct`; a Float32 is widened to a double first (the cast arrow makes)
  strings                                          compare as `bytes` (a str is its UTF-8): "" < "a" < "a\\0" < "a\\0\\0" < "ab"
  NULL                                             before or after every value by `nulls_first`, whatever the direction; NULLs tie
  DESC                                             inverts the comparison of two values (functools.cmp_to_key); no value is negated

`stable_perm` is the stable permutation: ties keep their input order.  tests/test_cpu_sort_order_exact.py pins this file."""
import functools
import struct
from collections import namedtuple

Key = namedtuple("Key", "kind desc nulls_first")      # kind: "int" | "float" | "utf8"

_MAG = (1 << 63) - 1


def f64_pattern(x):
    """The 64 bits of x as a double (x: anything float() takes -- a numpy float32 widens here, payload of a NaN and all)."""
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def total_order_rank(x):
    """An int that orders as totalOrder does: the magnitude for a clear sign bit, below every one of those and reversed for a set one."""
    p = f64_pattern(x)
    mag = p & _MAG
    return mag if not p >> 63 else -mag - 1


def _cmp(a, b):
    return (a > b) - (a < b)


def cmp_values(kind, a, b):
    if kind == "int":
        return _cmp(int(a), int(b))
    if kind == "float":
        return _cmp(total_order_rank(a), total_order_rank(b))
    if kind == "utf8":
        return _cmp(a.encode("utf-8") if isinstance(a, str) else bytes(a), b.encode("utf-8") if isinstance(b, str) else bytes(b))
    raise ValueError(kind)


def cmp_rows(spec, a, b):
    """-1 / 0 / +1: row a before / tied with / after row b.  Rows are sequences with one entry per key of spec, None for NULL."""
    for key, x, y in zip(spec, a, b):
        if x is None or y is None:
            c = 0 if (x is None and y is None) else (-1 if (x is None) == bool(key.nulls_first) else 1)
        else:
            c = cmp_values(key.kind, x, y)
            if key.desc:
                c = -c
        if c:
            return c
    return 0


def _identity(spec, row):
    """A row as a hashable value that is the same for two rows only if they are the same data (floats by pattern, strings by bytes)."""
    return tuple(None if v is None else f64_pattern(v) if k.kind == "float" else v.encode("utf-8") if isinstance(v, str) else bytes(v) if k.kind == "utf8" else int(v)
                 for k, v in zip(spec, row))


def dense_ranks(spec, rows):
    """rank[i] < rank[j] exactly when row i orders before row j, equal exactly when they tie.  Rows that are the same data are compared
    once: a table that repeats a few rows many times costs a sort of the few."""
    first = {}
    for i, r in enumerate(rows):
        first.setdefault(_identity(spec, r), i)
    reps = sorted(first.values(), key=functools.cmp_to_key(lambda i, j: cmp_rows(spec, rows[i], rows[j])))
    rank_of, rank = {}, -1
    for n, i in enumerate(reps):
        if n == 0 or cmp_rows(spec, rows[reps[n - 1]], rows[i]) != 0:
            rank += 1
        rank_of[_identity(spec, rows[i])] = rank
    return [rank_of[_identity(spec, r)] for r in rows]


def stable_perm(spec, rows):
    """The row indices in sorted order, ties in input order (sorted() is stable)."""
    ranks = dense_ranks(spec, rows)
    return sorted(range(len(rows)), key=ranks.__getitem__)


def tied_rows(spec, rows):
    """How many rows tie with some other row."""
    ranks = dense_ranks(spec, rows)
    count = {}
    for r in ranks:
        count[r] = count.get(r, 0) + 1
    return sum(c for c in count.values() if c > 1)
