"""h2o q6 (median v3, sd v3 by id4 id5; benchmarks/db-benchmark/groupby-datafusion.py) next to a bare SortExec over the same three keys: the
same table (the h2o recipe of bench_extras.py, id4 / id5 / v3 only), one process, the plans alternated, both results with a MEDIAN checked
against numpy.  The sort is what the MEDIAN lowering sits on: its time is the floor.

    python tools/median_q6.py [rows = 10000000] [out.json]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, pyarrow as pa
import arrow_ballista_amd as g
import bench_extras as X
from arrow_ballista_amd.expr import col

n, k, reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000, 100, 9
tc = g.TaskContext(device=0)
r = np.random.default_rng(11)
x = pa.table({"id4": pa.array(r.integers(1, k + 1, n).astype(np.int32)), "id5": pa.array(r.integers(1, k + 1, n).astype(np.int32)),
              "v3": pa.array(np.round(r.random(n) * 100, 6), pa.float64())})
x = x.cast(pa.schema([pa.field(f.name, f.type, nullable=False) for f in x.schema]))
dx = g.MemoryExec([g.DeviceTable.from_arrow(x, tc.device)])
s = dx.schema()
keys = [(col(c, s), c) for c in ("id4", "id5")]
A = lambda fn, name: {"fn": fn, "expr": col("v3", s), "name": name}
asc = lambda c: {"expr": col(c, s), "asc": True, "nulls_first": False}
plans = {
    "sort id4,id5,v3 (SortExec, 3 columns out)": g.NativePlan(g.SortExec([asc("id4"), asc("id5"), asc("v3")], dx), tc),
    "q6 median(v3) by id4,id5": g.NativePlan(g.AggregateExec("Single", keys, [A("MEDIAN", "median_v3")], dx), tc),
    "q6 median(v3) stddev(v3) by id4,id5": g.NativePlan(g.AggregateExec("Single", keys, [A("MEDIAN", "median_v3"), A("STDDEV", "sd")], dx), tc),
    "q6 stddev(v3) by id4,id5": g.NativePlan(g.AggregateExec("Single", keys, [A("STDDEV", "sd")], dx), tc),
}
times = {name: [] for name in plans}
res = {}
for name, p in plans.items():
    for _ in range(2):
        res[name] = p.execute(0)
tc.ctx.jit_wait()
for name, p in plans.items():
    res[name] = p.execute(0)
tc.sync()
for _ in range(reps):
    for name, p in plans.items():
        tc.sync(); t0 = time.perf_counter(); res[name] = p.execute(0); tc.sync(); times[name].append((time.perf_counter() - t0) * 1e3)
out = {"what": "h2o q6 next to a bare SortExec over (id4, id5, v3): same table, same process, plans alternated; host clock around plan.execute + stream sync, ms",
       "rows": n, "groups": res["q6 median(v3) by id4,id5"].num_rows, "reps": reps, "plans": {}}
for name, t in times.items():
    out["plans"][name] = {"min_ms": min(t), "median_ms": float(np.median(t)), "max_ms": max(t), "all_ms": [round(v, 3) for v in t]}
floor = out["plans"]["sort id4,id5,v3 (SortExec, 3 columns out)"]["median_ms"]
for name in ("q6 median(v3) by id4,id5", "q6 median(v3) stddev(v3) by id4,id5"):
    out["plans"][name]["ratio_to_sort"] = out["plans"][name]["median_ms"] / floor
    out["plans"][name]["matches_numpy"] = bool(X._q6_matches_numpy(np, x, res[name].to_arrow(), "stddev" in name))
info = tc.ctx.info()
out["device"] = info.get("name"), info.get("arch")
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))
