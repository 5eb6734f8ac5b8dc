"""What the moment aggregates cost: VARIANCE + STDDEV over 2^24 Float64 rows, grouped by ~1000 Int32 keys and ungrouped, as deferred
executions of a native plan.  One process measures one build and prints one JSON line; two builds are compared by
running it in alternating pairs, a fresh process per run, in one session on one box:
    GPUQ_LIB=<the other libgpuq.so> python tools/moment_agg_ab.py [rows]        (GPUQ_LIB unset: this tree's build)
A third case, "grouped_tail", is the grouped one under a predicate that keeps the last 2^16 rows only (t >= n - 2^16 over a row
number column): the origin is then searched through all the rows in front of them.
Per case: the median and the minimum over 7 rounds of 10 executions, and the results of two groups (what the two builds must agree on,
to the accuracy each has)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, pyarrow as pa
import arrow_ballista_amd as g
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 24
r = np.random.default_rng(1)
t = pa.table({"k": pa.array(r.integers(0, 1000, n, dtype=np.int32)), "x": pa.array(r.normal(0.0, 1e3, n)), "t": pa.array(np.arange(n, dtype=np.int64))})      # (near zero: both builds are accurate there)
tc = g.TaskContext(device=0)
src = g.MemoryExec([g.plan.materialize(tc, g.MemoryExec([t]).execute(0, tc))])
s = src.schema()
aggs = [{"fn": "VARIANCE", "expr": col("x", s), "name": "v"}, {"fn": "STDDEV", "expr": col("x", s), "name": "sd"}]
out = {"lib": os.environ.get("GPUQ_LIB", "tree"), "rows": n, "cases": {}}
tail = g.FilterExec(binary(col("t", s), Op.GtEq, lit(n - (1 << 16), "Int64")), src)
for name, groups, inp in (("grouped", [(col("k", s), "k")], src), ("ungrouped", [], src), ("grouped_tail", [(col("k", s), "k")], tail)):
    p = g.NativePlan(g.AggregateExec("Single", groups, aggs, inp), tc)
    for _ in range(4):
        p.execute(0)
    tc.ctx.jit_wait()
    for _ in range(5):
        res = p.execute(0)
    rows = sorted(zip(*[c.to_pylist() for c in res.to_arrow().columns]))
    ms, reps = [], 10
    for rnd in range(7):
        tc.sync(); t0 = time.perf_counter()
        for _ in range(reps):
            p.execute(0)
        tc.sync(); ms.append((time.perf_counter() - t0) * 1e3 / reps)
    st = p.exec_stats()
    out["cases"][name] = {"ms_per_run": {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}, "agg_path": [o["agg_path"] for o in p.profile_all() if o["op"] == "aggregate"],
                          "deferred": bool(st["deferred"]), "host_syncs": int(st["host_syncs"]), "rows_out": len(rows), "first_row": list(rows[0]), "last_row": list(rows[-1])}
print(json.dumps(out), flush=True)
