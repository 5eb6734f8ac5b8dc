"""bench.py end to end at SF1 in a process of its own: a plain run prints the headline alone, and --dump-outputs writes the q3
result of the last timed step, which must be the C oracle's answer over the same generated tables, row for row."""
import decimal
import json
import os
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pytest

import tpch_util as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_oracle_answer(tc, tmp_path):
    # tc: only for the suite's device check; the benchmark runs in a process of its own
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--sf", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "rows/s" and line["higher_is_better"] is True and line["dtype"] == "i128"
    assert not {"host", "roofline", "operators", "check", "cpu_baseline", "extra"} & set(line)

    n_li, n_cust = T.LINEITEM_ROWS[1], 150_000
    exp, st = T.q3_oracle_c(T.gen_q3_tables_host(n_li, n_cust))       # (revenue DESC, o_orderdate, l_orderkey): the dump's order
    assert line["config"]["result_groups"] == st["groups"] == len(exp) > 10_000
    got = {k: np.load(out / (k + ".npy")) for k in ("l_orderkey", "revenue", "o_orderdate", "o_shippriority")}
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in got)
    assert all(v.dtype == np.float64 and v.shape == (len(exp),) for v in got.values())
    assert np.array_equal(got["l_orderkey"], np.array([e[0] for e in exp], np.float64))
    rev = pa.array([decimal.Decimal(e[1]).scaleb(-4) for e in exp], pa.decimal128(38, 4))      # the result's type: Decimal128, scale 4
    assert np.array_equal(got["revenue"], rev.cast(pa.float64()).to_numpy())
    assert np.array_equal(got["o_orderdate"], np.array([e[2] for e in exp], np.float64))
    assert np.array_equal(got["o_shippriority"], np.array([e[3] for e in exp], np.float64))
