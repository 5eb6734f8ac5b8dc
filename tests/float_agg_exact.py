"""Exact references and stated error bounds for the float aggregates: VARIANCE / VAR_POP / STDDEV / STDDEV_POP / COVAR / COVAR_POP /
CORR and the Float64 SUM / AVG.  A helper for the tests, not a test.  Everything is `fractions.Fraction` over the f64 values the
device sees (an Int32 / Int64 below 2^53 / Float32 argument widens to f64 exactly); square roots are taken in `decimal` at 80 digits.

Per group, over the rows that take part (valid, and passing the predicate): n, mu, M2 = sum (x - mu)^2, Cxy = sum (x - mux)(y - muy),
sum x, sum |x|, and from those every function's value as a rational (`values`).

Tolerance of a central sum (u = 2^-53):
    m2:    max(F, 16 W)       F = (3n + 8) u (M2 + n R^2)
    algo:  max(F, 16 W)       F = (3n + 8) u sqrt((M2x + n Rx^2)(M2y + n Ry^2))
R = max - min of the argument over ALL rows that take part in the operator, whatever their group.  F is the worst case of power sums
about any origin K inside the data's range, added in any order: with d = fl(x - K), |d| <= R(1 + u), Sxx' = sum d^2 <= M2 + n R^2 (to
first order), the three terms are (n + 1) u Sxx' for the sum of squares, 2 (n - 1) u Sxx' for (sum d)^2 / n (Cauchy-Schwarz) and
2 u Sxx' for the rounding of x - K; the rest of 3n + 8 covers the last subtraction and division.  F holds for sigma = 0 and n = 1 too.
W is the largest error, against the exact value, of the oracle's own f64 Welford recurrence (oracle/oracle_np.py `_var_state`) over 8
seeded row orders of the group; 16 allows for the order-to-order spread of a sequential recurrence: "no worse than the engine this
project stands in for".
    mean state:  2 u |mu| + (n + 2) u R
    VAR:         tol(m2) / d + 4 u |VAR|          (d = n or n - 1)
    STDDEV:      tol(VAR) / (2 sigma) + 4 u sigma;  sigma = 0: sqrt(tol(VAR))
    CORR:        through Cxy / sqrt(M2x M2y), first order, + 4 u |CORR|
    SUM:         (n - 1) u sum |x|            AVG: that / n + u |AVG|

What the bound does NOT promise: R spans every group of one operator execution, so when groups sit at different offsets (family
"group_offsets": group g at g * 1e6 + N(0, 1)) R ~ 1e7 and F is ~ n u n R^2 however tight each group is -- the device picks ONE origin
per argument and run, and a group far from it cancels like (distance / sigma)^2.  The bound is loose there by design and a test over
that family only pins that the result is no worse than that.

Left out: Int64 values of 2^53 and more (the cast to f64 rounds the input) and Decimal arguments with a scale (the cast divides by
10^s in f64: the device does not see the decimal's value).  Both would put a rounding of the INPUT into the comparison."""
import decimal
import functools
import math
from fractions import Fraction

import numpy as np
import pyarrow as pa

from oracle import oracle_np as O

U = Fraction(1, 2 ** 53)
SIZES = (1, 2, 3, 63, 64, 65, 1000, 5000)
N_ROWS = sum(SIZES)
ONE_ARG = ("VARIANCE", "VAR_POP", "STDDEV", "STDDEV_POP")
TWO_ARG = ("COVAR", "COVAR_POP", "CORR")
_CTX = decimal.Context(prec=80)


def fsqrt(q):
    """sqrt of a non-negative Fraction as a Fraction, good to ~80 digits"""
    if q == 0:
        return Fraction(0)
    d = _CTX.divide(decimal.Decimal(q.numerator), decimal.Decimal(q.denominator))
    return Fraction(_CTX.sqrt(d))


# ------------------------------------------------------------------------------------ data families
def _groups(r):
    g = np.repeat(np.arange(len(SIZES), dtype=np.int64), SIZES)
    return g[r.permutation(N_ROWS)]


def _f64_1e9(r, g):
    return 1e9 + r.normal(0, 1, N_ROWS)


def _f64_1e6(r, g):
    return 1e6 + r.uniform(0, 0.01, N_ROWS)


def _ts_us(r, g):
    return (1_700_000_000_000_000 + r.integers(0, 1_000_000, N_ROWS)).astype(np.int64)


def _ts_s(r, g):
    return (1_700_000_000 + r.integers(0, 86_400, N_ROWS)).astype(np.int64)


def _f64_n1e3(r, g):
    return r.normal(0, 1e3, N_ROWS)


def _f32_1e4(r, g):
    return (1e4 + r.uniform(0, 1, N_ROWS)).astype(np.float32)


def _i32_2p30(r, g):
    return (2 ** 30 + r.integers(0, 100, N_ROWS)).astype(np.int32)


def _equal(r, g):
    return np.full(N_ROWS, 1e9 + 0.1)


def _group_offsets(r, g):
    return g.astype(np.float64) * 1e6 + r.normal(0, 1, N_ROWS)


# name -> (x of (rng, groups), y of (rng, groups, x) or None: an independent second draw of x's own distribution)
FAMILIES = {
    "f64_1e9": (_f64_1e9, None),
    "f64_1e6": (_f64_1e6, None),
    "ts_us": (_ts_us, None),
    "ts_s": (_ts_s, None),
    "f64_n1e3": (_f64_n1e3, None),
    "f32_1e4": (_f32_1e4, None),
    "i32_2p30": (_i32_2p30, None),
    "equal": (_equal, None),
    "pair_linear": (_f64_1e9, lambda r, g, x: 3.0 * x + r.normal(0, 1, N_ROWS)),
    "pair_independent": (_f64_1e9, lambda r, g, x: 1e9 + r.normal(0, 50, N_ROWS)),
    "group_offsets": (_group_offsets, None),
}
# where raw power sums (today's parent) must miss the tolerance by three orders of magnitude and more
ILL_CONDITIONED = ("f64_1e9", "f64_1e6", "ts_us", "f32_1e4", "i32_2p30")
_ARROW = {np.dtype(np.float64): pa.float64(), np.dtype(np.float32): pa.float32(), np.dtype(np.int64): pa.int64(), np.dtype(np.int32): pa.int32()}


@functools.lru_cache(maxsize=None)
def family(name, seed=0, nulls=0.0):
    """pa.Table: g Int64 (group, never NULL), x, y (NULL with probability `nulls` each, independently), p Int32 in [0, 10) (what a predicate
    filters on).  A function of (name, seed, nulls) alone."""
    fx, fy = FAMILIES[name]
    r = np.random.default_rng([seed, sorted(FAMILIES).index(name)])
    g = _groups(r)
    x = fx(r, g)
    y = fy(r, g, x) if fy else fx(r, g)
    p = r.integers(0, 10, N_ROWS).astype(np.int32)
    mx = (r.random(N_ROWS) < nulls) if nulls > 0 else None
    my = (r.random(N_ROWS) < nulls) if nulls > 0 else None
    cols = {"g": pa.array(g), "x": pa.array(x, type=_ARROW[x.dtype], mask=mx), "y": pa.array(y, type=_ARROW[y.dtype], mask=my), "p": pa.array(p)}
    return pa.Table.from_arrays(list(cols.values()), schema=pa.schema([pa.field(k, v.type, nullable=k in "xy" and nulls > 0) for k, v in cols.items()]))


def keep_of(t, pred_lt=None):
    """rows the predicate p < pred_lt keeps (all of them without one)"""
    p = t["p"].to_numpy()
    return np.ones(len(p), bool) if pred_lt is None else p < pred_lt


def partition_of(t, parts=3):
    """A partition per row for the two-phase runs: the terciles of x (a NULL x goes by its row number), so that the partitions' rows sit
    at different offsets inside the family's range and their means differ."""
    x = f64_column(t, "x")
    valid = sorted((v, i) for i, v in enumerate(x) if v is not None)
    pid = [i % parts for i in range(len(x))]
    for rank, (_, i) in enumerate(valid):
        pid[i] = rank * parts // len(valid)
    return pid


def f64_column(t, name):
    """the column as the f64 values the device computes with (None where NULL)"""
    return [None if v is None else float(v) for v in t[name].to_pylist()]


# ------------------------------------------------------------------------------------ exact statistics
class Stats:
    """One group of one argument pair: exact sums over the rows that take part."""

    def __init__(self, xs, ys=None):
        self.xs, self.ys = xs, ys
        self.n = n = len(xs)
        X = [Fraction(v) for v in xs]
        self.sum_x = sum(X, Fraction(0))
        self.sum_abs_x = sum((abs(v) for v in X), Fraction(0))
        self.mean_x = self.sum_x / n if n else Fraction(0)
        self.m2_x = sum((v * v for v in X), Fraction(0)) - (self.sum_x * self.sum_x / n if n else 0)
        if ys is not None:
            Y = [Fraction(v) for v in ys]
            sy = sum(Y, Fraction(0))
            self.mean_y = sy / n if n else Fraction(0)
            self.m2_y = sum((v * v for v in Y), Fraction(0)) - (sy * sy / n if n else 0)
            self.c_xy = sum((a * b for a, b in zip(X, Y)), Fraction(0)) - (self.sum_x * sy / n if n else 0)

    def values(self):
        """{function: exact value as a Fraction, or None where the function is NULL}"""
        n = self.n
        v = {"SUM": self.sum_x if n else None, "AVG": self.mean_x if n else None,
             "VAR_POP": self.m2_x / n if n else None, "VARIANCE": self.m2_x / (n - 1) if n > 1 else None}
        v["STDDEV_POP"] = None if v["VAR_POP"] is None else fsqrt(v["VAR_POP"])
        v["STDDEV"] = None if v["VARIANCE"] is None else fsqrt(v["VARIANCE"])
        if self.ys is not None:
            v["COVAR_POP"] = self.c_xy / n if n else None
            v["COVAR"] = self.c_xy / (n - 1) if n > 1 else None
            flat = self.m2_x == 0 or self.m2_y == 0
            v["CORR"] = None if n == 0 else (Fraction(0) if flat else self.c_xy / fsqrt(self.m2_x * self.m2_y))
        return v


def welford(xs, ys):
    """the oracle's recurrence over the rows in the given order: (m2_x, m2_y, algo, mean_x, mean_y)"""
    st = O._var_state(list(zip(xs, ys if ys is not None else [0.0] * len(xs))))
    return st["v1"], st["v2"], st["al"], st["m1"], st["m2"]


def power_sums(xs, ys, kx, ky):
    """sequential f64 power sums about (kx, ky) in the given order, as the device derives its states from them: (m2_x, m2_y, algo, mean_x, mean_y).
    kx = ky = 0.0 is the arithmetic of raw power sums."""
    n = len(xs)
    sx = sy = sxx = syy = sxy = 0.0
    for i in range(n):
        d = xs[i] - kx
        e = (ys[i] - ky) if ys is not None else 0.0
        sx += d; sy += e; sxx += d * d; syy += e * e; sxy += d * e
    if n == 0:
        return 0.0, 0.0, 0.0, 0.0, 0.0
    return sxx - sx * sx / n, syy - sy * sy / n, sxy - sx * sy / n, kx + sx / n, ky + sy / n


class Tolerances:
    """The bounds of one group.  rx, ry: the operator-wide ranges R of the two arguments (Fractions)."""

    def __init__(self, st, rx, ry=None, orders=8, seed=0):
        self.st, n = st, st.n
        self.rx, self.ry = rx, ry
        w_x = w_y = w_c = Fraction(0)
        r = np.random.default_rng([seed, n])
        for _ in range(orders if n > 1 else 1):
            o = r.permutation(n)
            xs = [st.xs[i] for i in o]
            ys = [st.ys[i] for i in o] if st.ys is not None else None
            v1, v2, al, _, _ = welford(xs, ys)
            w_x = max(w_x, abs(Fraction(v1) - st.m2_x))
            if ys is not None:
                w_y = max(w_y, abs(Fraction(v2) - st.m2_y)); w_c = max(w_c, abs(Fraction(al) - st.c_xy))
        k = (3 * n + 8) * U
        self.f_x = k * (st.m2_x + n * rx * rx)
        self.m2_x = max(self.f_x, 16 * w_x)
        self.mean_x = 2 * U * abs(st.mean_x) + (n + 2) * U * rx
        if st.ys is not None:
            self.f_y = k * (st.m2_y + n * ry * ry)
            self.m2_y = max(self.f_y, 16 * w_y)
            self.f_c = k * fsqrt((st.m2_x + n * rx * rx) * (st.m2_y + n * ry * ry))
            self.c_xy = max(self.f_c, 16 * w_c)
            self.mean_y = 2 * U * abs(st.mean_y) + (n + 2) * U * ry
        self.sum_x = max(n - 1, 0) * U * st.sum_abs_x

    def of(self, fn):
        """the bound on |device - exact| for a function's value (None where the value is NULL)"""
        st, n = self.st, self.st.n
        v = st.values()[fn]
        if v is None:
            return None
        if fn == "SUM":
            return self.sum_x
        if fn == "AVG":
            return self.sum_x / n + U * abs(v)
        if fn in ("VAR_POP", "VARIANCE", "STDDEV_POP", "STDDEV"):
            d = n if fn.endswith("_POP") else n - 1
            var = st.m2_x / d
            tvar = self.m2_x / d + 4 * U * var
            if not fn.startswith("STDDEV"):
                return tvar
            return fsqrt(tvar) if var == 0 else tvar / (2 * fsqrt(var)) + 4 * U * fsqrt(var)
        if fn in ("COVAR_POP", "COVAR"):
            d = n if fn.endswith("_POP") else n - 1
            return self.c_xy / d + 4 * U * abs(v)
        if fn == "CORR":
            if st.m2_x == 0 or st.m2_y == 0:
                return Fraction(0)      # a zero variance is exact about an origin that is a data value: the device must say 0.0 as the oracle does
            return self.c_xy / fsqrt(st.m2_x * st.m2_y) + abs(v) * (self.m2_x / (2 * st.m2_x) + self.m2_y / (2 * st.m2_y)) + 4 * U * abs(v)
        raise KeyError(fn)


@functools.lru_cache(maxsize=None)
def reference(name, seed=0, nulls=0.0, pred_lt=None, grouped=True, partition=None):
    """{group (or () ungrouped): (Stats, Tolerances)} of the family's table over x and the pair (x, y): key "x" -> one-argument statistics
    (rows where x is valid), key "xy" -> the pair (rows where both are).  partition: only the rows `partition_of` gives that number."""
    t = family(name, seed, nulls)
    keep = keep_of(t, pred_lt)
    pid = partition_of(t) if partition is not None else None
    rows = [i for i in range(t.num_rows) if pid is None or pid[i] == partition]
    g, x, y = t["g"].to_pylist(), f64_column(t, "x"), f64_column(t, "y")
    out = {}
    for which in ("x", "xy"):
        part = [i for i in rows if keep[i] and x[i] is not None and (which == "x" or y[i] is not None)]
        rx = Fraction(max(x[i] for i in part)) - Fraction(min(x[i] for i in part)) if part else Fraction(0)
        ry = Fraction(max(y[i] for i in part)) - Fraction(min(y[i] for i in part)) if part and which == "xy" else None
        by = {}
        for i in rows:
            if keep[i]:
                by.setdefault((g[i],) if grouped else (), [])      # a group whose rows are all NULL still has a row
        if not grouped:
            by.setdefault((), [])
        for i in part:
            by[(g[i],) if grouped else ()].append(i)
        res = {}
        for k, idx in by.items():
            st = Stats([x[i] for i in idx], [y[i] for i in idx] if which == "xy" else None)
            res[k] = (st, Tolerances(st, rx, ry))
        out[which] = res
    return out
