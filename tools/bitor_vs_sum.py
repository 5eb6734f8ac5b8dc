"""BIT_OR / BIT_XOR / BIT_AND(x) against SUM(x) over the same column and grouping, one process, alternating rounds of ten deferred executions of
a native plan each.  python tools/bitor_vs_sum.py [rows [out.json]]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, pyarrow as pa
import arrow_ballista_amd as g
from arrow_ballista_amd.expr import col

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 26
r = np.random.default_rng(1)
t = pa.table({"k3": pa.array(r.integers(0, 3, n, dtype=np.int32)), "k1000": pa.array(r.integers(0, 1000, n, dtype=np.int32)),
              "k1m": pa.array(r.integers(0, 1 << 20, n, dtype=np.int64)),
              "x": pa.array(r.integers(0, 1 << 62, n, dtype=np.int64))})      # non-negative: SUM's high word moves only on a carry
tc = g.TaskContext(device=0)
src = g.MemoryExec([g.plan.materialize(tc, g.MemoryExec([t]).execute(0, tc))])
s = src.schema()
out = {"rows": n, "cases": []}
for strategy, key, eg in (("tiny", None, 0), ("tiny", "k3", 0), ("lds", "k1000", 0), ("hash", "k1000", 0), ("hash", "k1m", 1 << 20), ("radix", "k1m", 1 << 20)):
    plans = {}
    for fn in ("BIT_OR", "SUM", "BIT_XOR", "BIT_AND"):
        groups = [(col(key, s), key)] if key else []
        plans[fn] = g.NativePlan(g.AggregateExec("Single", groups, [{"fn": fn, "expr": col("x", s), "name": "v"}], src, strategy=strategy, expected_groups=eg), tc)
    for p in plans.values():
        for _ in range(4):
            p.execute(0)
    tc.ctx.jit_wait()
    for p in plans.values():
        for _ in range(3):
            p.execute(0)
    ms = {fn: [] for fn in plans}
    reps = 10
    for rnd in range(5):
        for fn, p in plans.items():
            tc.sync(); t0 = time.perf_counter()
            for _ in range(reps):
                p.execute(0)
            tc.sync(); ms[fn].append((time.perf_counter() - t0) * 1e3 / reps)
    case = {"strategy": strategy, "key": key, "ms_per_run": {fn: {"median": float(np.median(v)), "min": float(min(v))} for fn, v in ms.items()}}
    out["cases"].append(case)
    print(json.dumps(case), flush=True)
if len(sys.argv) > 2:
    json.dump(out, open(sys.argv[2], "w"), indent=1)
