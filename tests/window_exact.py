"""What a BoundedWindowAggExec computes, restated row by row in exact arithmetic: the reference of tests/test_cpu_window.py and
tests/test_gpu_window.py.  Integers are Python ints wrapped to the result's fixed width at the end (wrapping commutes with + and -),
decimals Python ints wrapped at 128 bits, floats fractions.Fraction (with the sum of magnitudes next to them, for the error bound).

A table is a dict of equally long lists (None = NULL).  Partitions are maximal runs of adjacent rows equal on every partition column,
peer groups maximal runs equal on partition + order columns; None equals None.  test_the_restatement_on_a_known_table pins all of it
on a dozen rows whose answers were written down by hand."""
from fractions import Fraction

U = Fraction(1, 2 ** 53)      # unit roundoff of Float64


def wrap(v, bits, signed=True):
    v &= (1 << bits) - 1
    return v - (1 << bits) if signed and v >> (bits - 1) else v


def runs(table, cols, n):
    """start index of the run every row lies in, and the index one past its end"""
    start, end = [0] * n, [n] * n
    s = 0
    for i in range(1, n + 1):
        if i == n or any(table[c][i] != table[c][i - 1] for c in cols):
            for j in range(s, i):
                start[j], end[j] = s, i
            s = i
    return start, end


class Walk:
    def __init__(self, table, partition_by=(), order_by=()):
        self.t = table
        self.n = len(next(iter(table.values()))) if table else 0
        self.ps, self.pe = runs(table, list(partition_by), self.n)
        self.qs, self.qe = runs(table, list(partition_by) + list(order_by), self.n)

    def row_number(self):
        return [i - self.ps[i] + 1 for i in range(self.n)]

    def rank(self):
        return [self.qs[i] - self.ps[i] + 1 for i in range(self.n)]

    def dense_rank(self):
        out, d = [], 0
        for i in range(self.n):
            d = 1 if i == self.ps[i] else d + (1 if i == self.qs[i] else 0)
            out.append(d)
        return out

    def shift(self, col, delta, default=None):
        """LAG: delta = -offset, LEAD: delta = +offset.  A NULL value is a value."""
        v = self.t[col]
        return [v[i + delta] if self.ps[i] <= i + delta < self.pe[i] else default for i in range(self.n)]

    def frame(self, i, frame):
        """[lo, hi] of row i: "range" (up to the last peer), "rows" (up to the row), or (k, m) rows around it, k None = UNBOUNDED"""
        if frame == "range":
            return self.ps[i], self.qe[i] - 1
        if frame == "rows":
            return self.ps[i], i
        k, m = frame
        return (self.ps[i] if k is None else max(self.ps[i], i - k)), min(self.pe[i] - 1, i + m)

    def _prefix(self, col, value=lambda x: x):
        ps, pc, pa = [0], [0], [0]      # sums, counts of non-NULL values, sums of magnitudes
        for x in self.t[col]:
            ps.append(ps[-1] + (value(x) if x is not None else 0))
            pc.append(pc[-1] + (x is not None))
            pa.append(pa[-1] + (abs(value(x)) if x is not None else 0))
        return ps, pc, pa

    def count(self, col, frame="range"):
        _, pc, _ = self._prefix(col, lambda x: 0)      # (values of any type: only their presence counts)
        return [pc[hi + 1] - pc[lo] for lo, hi in (self.frame(i, frame) for i in range(self.n))]

    def sum(self, col, frame="range", bits=64, signed=True):
        """exact, wrapped to `bits`; None while the frame holds no value"""
        ps, pc, _ = self._prefix(col)
        return [wrap(ps[hi + 1] - ps[lo], bits, signed) if pc[hi + 1] - pc[lo] else None for lo, hi in (self.frame(i, frame) for i in range(self.n))]

    def sum_exact(self, col, frame="range", value=Fraction):
        """[(exact sum as a Fraction, sum of magnitudes, number of values) or None]: floats, and the quotients of AVG"""
        ps, pc, pa = self._prefix(col, value)
        out = []
        for i in range(self.n):
            lo, hi = self.frame(i, frame)
            k = pc[hi + 1] - pc[lo]
            out.append((Fraction(ps[hi + 1] - ps[lo]), Fraction(pa[hi + 1] - pa[lo]), k) if k else None)
        return out

    def avg_decimal(self, col, frame="range", digits=4):
        """sum * 10^digits / count, truncating toward zero, as the aggregate operator's Decimal128 AVG"""
        out = []
        for e in self.sum_exact(col, frame, value=int):
            if e is None:
                out.append(None)
                continue
            num, k = int(e[0]) * 10 ** digits, e[2]
            q = abs(num) // k
            out.append(-q if num < 0 else q)
        return out

    def minmax(self, col, minimum, frame="range", key=lambda x: x):
        """running MIN / MAX (frames that start at the partition's head); key orders the values (floats: total order)"""
        v, best, run = self.t[col], [], None
        for i in range(self.n):
            if i == self.ps[i]:
                run = None
            if v[i] is not None and (run is None or (key(v[i]) < key(run) if minimum else key(v[i]) > key(run))):
                run = v[i]
            best.append(run)
        out = []
        for i in range(self.n):
            lo, hi = self.frame(i, frame)
            assert lo == self.ps[i], "MIN / MAX over a sliding frame is refused"
            out.append(best[hi])
        return out
