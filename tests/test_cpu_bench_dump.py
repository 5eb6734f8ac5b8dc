"""CPU: what `bench.py --dump-outputs DIR` writes (bench.dump_q3_outputs), on stand-in q3 results: one float64 file per result
column, rows in the result's order with ties ordered by key, a fixed sample above the size cap; and --steps below 1 is refused."""
import datetime
import decimal
import os
import subprocess
import sys

import numpy as np
import pyarrow as pa

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = ("l_orderkey", "revenue", "o_orderdate", "o_shippriority")


class _Result:
    """The one method of NativeResult that dump_q3_outputs uses."""

    def __init__(self, table):
        self.table = table

    def to_arrow(self):
        return self.table


def _q3_result(keys, revenue, days, prio):
    return _Result(pa.table({"l_orderkey": pa.array(keys, pa.int64()),
                             "revenue": pa.array([decimal.Decimal(r) for r in revenue], pa.decimal128(38, 4)),
                             "o_orderdate": pa.array([datetime.date(1970, 1, 1) + datetime.timedelta(days=d) for d in days], pa.date32()),
                             "o_shippriority": pa.array(prio, pa.int32())}))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_values_and_order_of_ties(tmp_path):
    res = _q3_result([7, 5, 3, 9, 1], ["10.5000", "3.0000", "3.0000", "3.0000", "-2.1234"], [9131, 9132, 9132, 9133, 9131], [0, 1, 0, 0, 0])
    bench.dump_q3_outputs(res, str(tmp_path))
    got = _load(tmp_path)
    assert sorted(got) == sorted(COLS)
    assert all(v.dtype == np.float64 for v in got.values())
    # rows 1 and 2 tie on (revenue, date): key order; row 3 has another date and stays where the result put it
    assert got["l_orderkey"].tolist() == [7, 3, 5, 9, 1]
    assert got["o_shippriority"].tolist() == [0, 0, 1, 0, 0]
    assert np.allclose(got["revenue"], [10.5, 3.0, 3.0, 3.0, -2.1234], rtol=1e-15, atol=0)
    assert got["o_orderdate"].tolist() == [9131, 9132, 9132, 9133, 9131]


def test_sample_above_the_cap_is_fixed(tmp_path, monkeypatch):
    n = 1000
    rng = np.random.default_rng(5)
    rev = np.sort(rng.integers(0, 50, n))[::-1]           # many ties, as in a real result
    keys = rng.permutation(n) + 1
    days = np.zeros(n, np.int64)
    res = _q3_result(keys.tolist(), ["%d.0000" % r for r in rev], days.tolist(), [0] * n)
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 8 * (len(COLS) + 1) * 100)
    bench.dump_q3_outputs(res, str(tmp_path / "a"))
    bench.dump_q3_outputs(res, str(tmp_path / "b"))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(COLS + ("row_index",))
    assert all(len(v) == 100 for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["row_index"].astype(np.int64)
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < n
    canon = sorted(zip(-rev, keys))                         # revenue DESC, ties by key: what the whole dump would hold
    assert [(-r, k) for r, k in (canon[i] for i in idx)] == list(zip(a["revenue"].astype(np.int64), a["l_orderkey"].astype(np.int64)))


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
