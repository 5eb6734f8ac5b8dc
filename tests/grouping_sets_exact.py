"""Grouping sets (GROUP BY ROLLUP / CUBE / GROUPING SETS) restated row by row.  A helper for the tests, not a test.

What the node means (DataFusion 34; include/gpuq.h, gpuq_grouping_expand, has the rules): `sets` is S grouping sets, one bool per group
expression, True = the key is NULL in that set.  Every input row is counted once per set, its key tuple NULL wherever the set masks a
key, and all tuples of all sets go into ONE dict.  There is no grouping id: a row whose key is really NULL (None) lands in the group of the
set that masks that key, and two equal sets count every row twice.

`groups(keys, sets)` is that dict -- key tuple -> the list of input rows, one entry per (row, set) -- and the functions below fold one
group's rows exactly: Python ints wrapped at the operator's widths (window_exact.wrap), truncating decimal AVG, float_agg_exact.Stats /
Tolerances for the float functions."""
from fractions import Fraction

import float_agg_exact as X
from window_exact import wrap


def rollup(nk):
    return [[k >= keep for k in range(nk)] for keep in range(nk, -1, -1)]


def cube(nk):
    return [[bool((m >> (nk - 1 - k)) & 1) for k in range(nk)] for m in range(1 << nk)]


def groups(keys, sets, keep=None):
    """keys: one tuple per input row (None = NULL); keep: the rows the fused predicate passes (None: all).  {key tuple: [row, ...]}"""
    out = {}
    for i, k in enumerate(keys):
        if keep is not None and not keep[i]:
            continue
        for s in sets:
            assert len(s) == len(k)
            out.setdefault(tuple(None if masked else v for v, masked in zip(k, s)), []).append(i)
    return out


def picked(vals, rows, where=None):
    """the non-NULL values of the group's rows (where: a per-row FILTER; a row it does not pass counts as NULL)"""
    return [vals[i] for i in rows if vals[i] is not None and (where is None or where[i])]


def count_star(rows, where=None):
    return len(rows) if where is None else sum(1 for i in rows if where[i])


def count(vals, rows, where=None):
    return len(picked(vals, rows, where))


def total(vals, rows, bits=64, signed=True, where=None):
    """SUM of integers (bits = 64) or of a decimal's unscaled values (bits = 128), wrapping; NULL over no values"""
    v = picked(vals, rows, where)
    return wrap(sum(int(x) for x in v), bits, signed) if v else None


def minimum(vals, rows, where=None):
    v = picked(vals, rows, where)
    return min(v) if v else None


def maximum(vals, rows, where=None):
    v = picked(vals, rows, where)
    return max(v) if v else None


def bit_fold(op, vals, rows, bits, signed=True, where=None):
    v = picked(vals, rows, where)
    if not v:
        return None
    acc = int(v[0]) & ((1 << bits) - 1)
    for x in v[1:]:
        x = int(x) & ((1 << bits) - 1)
        acc = acc & x if op == "AND" else acc | x if op == "OR" else acc ^ x
    return wrap(acc, bits, signed)


def bool_and(vals, rows, where=None):
    v = picked(vals, rows, where)
    return all(v) if v else None


def bool_or(vals, rows, where=None):
    v = picked(vals, rows, where)
    return any(v) if v else None


def avg_decimal(unscaled, rows, where=None):
    """AVG of Decimal128(p, s) as the unscaled value of Decimal128(p + 4, s + 4): sum * 10^4 / count, truncating toward zero"""
    v = picked(unscaled, rows, where)
    if not v:
        return None
    num = sum(int(x) for x in v) * 10 ** 4
    q = abs(num) // len(v)
    return q if num >= 0 else -q


def stats(xs, rows, ys=None):
    """float_agg_exact.Stats of the group over x (rows where x is valid) or over the pair (rows where both are)"""
    idx = [i for i in rows if xs[i] is not None and (ys is None or ys[i] is not None)]
    return X.Stats([xs[i] for i in idx], [ys[i] for i in idx] if ys is not None else None)


def value_range(vals, rows=None):
    """R of float_agg_exact.Tolerances: max - min over all rows that take part in the operator"""
    v = [x for i, x in enumerate(vals) if x is not None and (rows is None or i in rows)]
    return Fraction(max(v)) - Fraction(min(v)) if v else Fraction(0)
