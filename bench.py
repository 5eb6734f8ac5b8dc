#!/usr/bin/env python3
"""bench.py -- hot-path throughput of the gpuq operator engine on MI355X.

Contract (driver): python bench.py --gpus N --steps K --warmup W ; for N>1 launched by
torch.distributed.run, one rank per GPU over RCCL.  Prints ONE JSON line on rank 0.

Workload at N=1 (BASELINE.json configs[2], the largest single-GPU configuration of the metric "rows/sec hash-join probe +
TPC-H SF100 q1/q3/q5 wall-time"): TPC-H SF100 q3 -- FilterExec x3 -> HashJoinExec(customer |x| orders) ->
HashJoinExec(.. |x| lineitem) -> AggregateExec -> ProjectionExec -> SortExec (reference benchmarks/queries/q3.sql,
benchmarks/src/bin/tpch.rs:286-351) over synthetic TPC-H-shaped tables resident in HBM (lineitem 600,037,902 rows, orders
150,009,476, customer 15,000,000; SURVEY.md section 8d generator).  A "step" = one full q3 through the native plan executor.
value = lineitem rows through the query per second.
A plain run sets up, warms up, times --steps steps and prints the headline (metric, value, ms_per_step, config); --dump-outputs DIR
writes the result of the last timed step (dump_q3_outputs).  Everything below the headline is measured only with --full:
roofline: the hash-join probe of lineitem (the operator with the most kernel time); algorithmic bytes = SURVEY.md section 8d's
24 B per probe row + 12 B per emitted pair x the counts measured on this input; duration = HIP events around the probe
operator's kernels on the stream they run on.  "host": how the steps ran (deferred: one host round trip per step).
"check": the SF100 result against an independent torch computation over the same columns (sum of revenue, number of groups).
cpu_baseline: the C oracle's q3 ("port", OpenMP over all host cores) on an SF10 sample of the same generator, min and mean of 3, with
q1 and q5 and a pyarrow Acero proxy beside it.
"extra": the join-probe micro-grid (2^28 probes x {2^20, 2^24, 2^27} build keys x hit rates x uniform / Zipf) and SF100 q1 / q5 wall times.

Workload at N>1 (strong scaling: the job stays SF100, every rank holds 1/N of each table): ONE native plan per rank with the
exchanges inside (csrc/plan_exec.cpp RepartitionExec / BroadcastExec over csrc/exchange.cpp).  The headline plan is the one a
cost-based planner picks for q3 -- the build side of orders |x| lineitem is 20 x smaller than the probe side, so it is
BROADCAST and lineitem stays where it is: customer keys broadcast, orders joined locally, the joined orders (14.6 M rows at
SF100) all-gathered (one grouped ncclSend / ncclRecv round per column buffer), CollectLeft join + partial aggregate per rank,
partial states hash-repartitioned on the group key, final aggregate, sorted runs gathered and merged.  value = lineitem rows of
the whole job per second, time = MAX over ranks between barriers.  "extra": the BASELINE configs[3] shape ("hash-partitioned RCCL
all-to-all": BOTH sides of orders |x| lineitem repartitioned on the order key -- it moves 13 GB of lineitem columns where the
broadcast moves 0.2 GB, and is reported for that reason) on q3 and on q5, and q1 (partial states gathered).
GPUQ_BENCH_BACKEND=gloo rehearses the N>1 path with ranks sharing a GPU (host-staged transport).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0            # MI355X HBM3E spec (MI355X_MICROARCH.md); ~6300 GB/s measured copy ceiling


Q3_SLOT_BYTES = 16              # one 16-byte slot touch per probe (key + row id), SURVEY.md section 8d
Q3_PROBE_KEY_BYTES = 8
Q3_PAIR_BYTES = 12              # u64 build idx + u32 probe idx per emitted pair in section 8d's formula


def main_q3():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sf", type=float, default=100.0, help="scale factor of the WHOLE job (default 100 = BASELINE configs[2]); N ranks hold 1/N of every table each")
    ap.add_argument("--full", action="store_true", help="also measure and check what the headline does not need: per-operator times and the probe roofline "
                    "(HIP events around every operator in the timed steps), the result against plain torch ops, the CPU baseline and the secondary legs")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--cpu-sample-sf", type=float, default=10.0)
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the secondary legs (N=1: probe micro-grid, SF100 q1 / q5; N>1: q3 with the build side broadcast, distributed q5, q1)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the result of the last timed step to DIR/<column>.npy (float64; see dump_q3_outputs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    import torch
    import torch.distributed as dist
    from benchmarks import tpch as T
    import arrow_ballista_amd as g
    from arrow_ballista_amd import parallel

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # GPUQ_BENCH_BACKEND=gloo: rehearsal of the N>1 path on a box with fewer GPUs than ranks (ranks share devices, the exchange
    # runs over the host-staged transport); the measured configuration is always nccl = RCCL, one rank per GPU.
    backend = os.environ.get("GPUQ_BENCH_BACKEND", "nccl")
    assert torch.cuda.is_available(), "bench.py needs a GPU: the product path has no CPU fallback"
    if backend != "nccl":
        local_rank = local_rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local_rank)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    tc = g.TaskContext(device=local_rank)
    comm = parallel.Comm(tc) if world > 1 else None

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed_steps(fn, steps):
        """K steps between fences, MAX over ranks."""
        import gc
        gc.collect(); gc.freeze(); gc.disable()
        fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = fn()
        fence()
        dt = time.perf_counter() - t0
        gc.enable()
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device=tc.device if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt, out

    sf = args.sf
    n_total = T.LINEITEM_ROWS.get(int(sf), int(6_000_000 * sf)) if sf == int(sf) else int(6_000_000 * sf)
    # strong scaling: the job is SF`sf`; rank r holds rows [r * n_li, (r + 1) * n_li) of lineitem and the matching ranges of orders / customer
    n_li = n_total if world == 1 else n_total // world // 4 * 4
    n_orders = (n_li + 3) // 4
    n_cust_total, n_supp = int(150_000 * sf), int(10_000 * sf)
    n_cust = n_cust_total if world == 1 else n_cust_total // world // 5 * 5
    li = T.gen_lineitem_device(tc, n_li, n_supp=n_supp, columns=("l_orderkey", "l_suppkey", "l_extendedprice", "l_discount", "l_shipdate"), row0=rank * n_li)
    od = T.gen_orders_device(tc, n_orders, n_cust_total, row0=rank * n_orders)
    cu = T.gen_customer_device(tc, n_cust, row0=rank * n_cust)
    if world == 1:
        plan = g.NativePlan(T.q3_plan(g.MemoryExec([cu]), g.MemoryExec([od]), g.MemoryExec([li])), tc)
    else:
        plan = g.NativePlan(T.q3_dist_plan(g.MemoryExec([cu]), g.MemoryExec([od]), g.MemoryExec([li]), world, "partitioned"), tc)
        plan.set_comm(comm)

    fence()
    t0 = time.perf_counter()
    res = plan.execute(0)
    tc.sync()
    first_ms = (time.perf_counter() - t0) * 1e3          # cold: the interpreter kernels run while a worker thread specialises every pipeline (jit "auto")
    tc.ctx.jit_wait()                                    # the code objects the first execution asked for
    for _ in range(max(args.warmup, 2)):
        res = plan.execute(0)
    tc.ctx.jit_wait()                                    # ... and the variants the warm-up asked for (layouts learned on the way)
    # the two runs around the probe's pair count (--full) run in a plain run too: the timed steps start from the same state either way
    res = plan.execute(0)
    m0 = plan.metrics() if args.full else None
    res = plan.execute(0)
    tc.sync()
    if args.full:
        m1 = plan.metrics()
        # pairs emitted by the lineitem probe in one run = the larger of the two joins' output rows
        matches = max([int(b["output_rows"]) - int(a["output_rows"]) for a, b in zip(m0, m1) if b["node"] == "HashJoinExec"] or [0])
        plan.profile(True)
    dt, res = timed_steps(lambda: plan.execute(0), args.steps)
    if args.full:
        ops = plan.profile_all()
        plan.profile(False)
        host = plan.exec_stats()
    groups = res.num_rows
    if args.dump_outputs and rank == 0:
        dump_q3_outputs(res, args.dump_outputs)

    rows_job = n_li * world
    line = {
        "metric": "tpch_sf100_q3_lineitem_rows_per_sec", "value": rows_job * args.steps / dt, "unit": "rows/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": "i128", "data": "synthetic",
        "config": {"workload": ("TPC-H SF%g q3 (BASELINE configs[2]): filter x3 + hash join customer|x|orders + hash join |x| lineitem + aggregate + sort, " % sf)
                               + ("one task on 1 x MI355X" if world == 1 else
                                  "%d ranks x 1/%d of every table: customer keys and the joined orders broadcast over RCCL (grouped send/recv per column buffer), lineitem stays in place, "
                                  "join + partial aggregate per rank, partial states repartitioned on the group key, final aggregate, sorted runs gathered and merged" % (world, world)),
                   "lineitem_rows": rows_job, "lineitem_rows_per_gpu": n_li, "orders_rows_per_gpu": n_orders, "customer_rows_per_gpu": n_cust, "result_groups": groups,
                   "input": "Arrow-physical columns resident in HBM", "first_run_ms": first_ms, "first_run_note": "jit auto: interpreter kernels while the pipelines are specialised in the background (round 2: 1.3-1.7 s waiting for hiprtc)", "aggregate_strategy": "auto",
                   "parallelism": "single partition" if world == 1 else "partition-per-gpu x%d, exchange inside the native plan (%s)" % (world, comm.transport)},
    }
    if args.full:
        # measured counts of the lineitem probe on this input (outside the timed region): rows that pass the fused filter = probes
        shipdate = li.columns[[c.name for c in li.columns].index("l_shipdate")].data[: 4 * n_li].view(torch.int32)
        probes = int((shipdate > T.Q3_DATE).sum().item())
        # host side of a step: deferred = no operator read anything back (counts travel as device words, operators keep what their first run
        # learned); settles = host round trips per step (one: the plan's end), host_syncs = read-backs of operators that ran synchronously
        line["host"] = {"deferred": host["deferred"], "round_trips_per_step": host["settles"] + host["host_syncs"], "settles": host["settles"],
                        "operator_read_backs": host["host_syncs"], "deferred_runs_redone": host["retries"]}
        probe_ops = sorted((o for o in ops if o["op"] == "join_probe"), key=lambda o: -o["kernel_ms"])
        if probe_ops and probe_ops[0]["launches"] > 0:
            po = probe_ops[0]
            avg_ms = po["kernel_ms"] / po["launches"]
            alg = (Q3_PROBE_KEY_BYTES + Q3_SLOT_BYTES) * probes + Q3_PAIR_BYTES * matches
            achieved = alg / (avg_ms * 1e-3) / 1e9
            # traffic: HBM bytes per launch from the PMC passes (FETCH_SIZE x 2 + WRITE_SIZE, MI355X_MICROARCH.md) of an EARLIER run of this
            # command, read from profiles/ -- counters cannot be collected inside this process; traffic_source says which file
            traffic, traffic_source = None, None
            for name in ("r03_traffic.json", "r02_traffic.json"):
                tp = os.path.join(ROOT, "profiles", name)
                if sf == 100 and world == 1 and os.path.exists(tp):
                    traffic, traffic_source = json.load(open(tp)).get("traffic_bytes_per_launch"), "profiles/" + name + " (PMC passes of an earlier run of this command, not this run)"
                    break
            import re
            lab = re.search(r'"label":"(\w+)"', po.get("desc", ""))
            line["roofline"] = {"bound": "hbm", "kernel": "HashJoinExec probe of lineitem (fused filter l_shipdate > date + key lookup + pair emit; rank 0's launch)",
                                "kernel_name": "gpuq_jit_join_probe_unique" + ("_" + lab.group(1) if lab else ""),
                                "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
                                "avg_launch_ms": avg_ms, "launches": po["launches"], "algorithmic_bytes_per_launch": alg,
                                "probe_rows": probes, "matches": matches, "rows_scanned": n_li,
                                "probe_rows_per_s": probes / (avg_ms * 1e-3), "rows_scanned_per_s": n_li / (avg_ms * 1e-3)}
        # the dominant kernel of every operator the plan compiled (HIP events around it); the smaller launches around them (scans of segment
        # counts, table initialisation, the aggregate's extract / emit) are inside ms_per_step, not in this list
        import re as _re
        def _lab(o):
            m = _re.search(r'"label":"(\w+)"', o.get("desc", ""))
            return m.group(1) if m else None
        line["operators"] = [{"op": o["op"], "label": _lab(o), "kernel_ms_per_step": o["kernel_ms"] / max(1, args.steps),
                              "op_ms_per_step": o.get("op_ms", 0.0) / max(1, args.steps), "launches": o["launches"]}
                             for o in sorted(ops, key=lambda o: -o.get("op_ms", o["kernel_ms"])) if o["launches"] > 0 or o.get("op_ms", 0) > 0]
        # op_ms: HIP events around everything the operator's calls queue (dominant kernel + table initialisation, scans, compaction, the
        # aggregate's extract / result projection); their sum against ms_per_step is what the step spends outside operators
        line["operators_ms_per_step"] = sum(o["op_ms_per_step"] for o in line["operators"])
        line["operators_share_of_step"] = line["operators_ms_per_step"] / line["ms_per_step"]
        if world == 1:
            line["check"] = check_q3_result(torch, T, tc, res, li, od, cu)
    del plan, res
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline(args.cpu_sample_sf)
    if args.full and not args.no_extras:
        import bench_extras
        tc.ctx.set_jit("wait")      # the secondary legs time steady state from their second run on: a large input waits for its specialised kernels
        if world == 1:
            del li, od, cu
            torch.cuda.empty_cache()
            # SURVEY.md section 8d grid: |B| in {2^20, 2^24, 2^27} x hit rate {1.0, 0.5, 0.1} uniform, and Zipf(1.05) probe keys
            extra = {"join_probe": [bench_extras.join_probe_micro(tc, g, b, 28, h) for b in (20, 24, 27) for h in (1.0, 0.5, 0.1)]
                                   + [bench_extras.join_probe_micro(tc, g, b, 28, 1.0, zipf=1.05) for b in (20, 24, 27)]}
            torch.cuda.empty_cache()
            extra["sf100_q1"] = bench_extras.q1_pipeline(tc, T, g, 100)
            extra["sf100_q6"] = bench_extras.q6_pipeline(tc, T, g, 100)
            tp = bench_extras.tpch_pipelines(tc, T, g, 100)
            extra["sf100_q3"], extra["sf100_q5"] = tp["q3"], tp["q5"]
            torch.cuda.empty_cache()
            # BASELINE configs[4]: the per-GPU shard of the SF300 lineitem sort (the N>1 run below does the range exchange around it)
            extra["sort_sf300_shard"] = bench_extras.sort_shard(tc, T, g)
            torch.cuda.empty_cache()
            # the scan leaves at SF1 (host bytes -> Arrow-layout columns in HBM): '|' text, Parquet plain and Snappy (decoded without a serial walk), pyarrow on the host beside them
            extra["scan_decode_sf1"] = bench_extras.scan_decode(tc, T, g, sf=1)
        else:
            # second legs, every rank takes part: q3 with the build side of orders |x| lineitem BROADCAST instead (what a cost-based
            # planner picks when the build side is 20 x smaller: 1/60 of the bytes cross the links), distributed q5, and q1
            extra = {}
            k = max(3, args.steps // 4)
            p2 = g.NativePlan(T.q3_dist_plan(g.MemoryExec([cu]), g.MemoryExec([od]), g.MemoryExec([li]), world, "broadcast"), tc)
            p2.set_comm(comm)
            for _ in range(3):
                p2.execute(0)
            d2, r2 = timed_steps(lambda: p2.execute(0), k)
            extra["q3_build_side_broadcast"] = {"ms_per_step": d2 / k * 1e3, "lineitem_rows_per_s": rows_job * k / d2, "result_groups": r2.num_rows}
            # BASELINE configs[3]: q5, the 6-way join with orders |x| lineitem hash-partitioned across the ranks (T.q5_dist_plan)
            sper = n_supp // world
            su = T.gen_supplier_device(tc, sper if rank < world - 1 else n_supp - sper * (world - 1), row0=rank * sper)
            nation, region = T.nation_region_arrow()
            p5 = g.NativePlan(T.q5_dist_plan(g.MemoryExec([cu]), g.MemoryExec([od]), g.MemoryExec([li]), g.MemoryExec([su]), g.MemoryExec([nation]), g.MemoryExec([region]), world), tc)
            p5.set_comm(comm)
            for _ in range(3):
                p5.execute(0)
            tc.ctx.jit_wait()
            d5, r5 = timed_steps(lambda: p5.execute(0), k)
            extra["q5_partitioned_join"] = {"ms_per_step": d5 / k * 1e3, "lineitem_rows_per_s": rows_job * k / d5, "result_groups": r5.num_rows}
            # BASELINE configs[4]: ORDER BY l_extendedprice across the ranks -- RangeRepartitionExec (sample -> splitters -> one range
            # exchange -> ordered fan-in); every rank ends with one ascending range
            from arrow_ballista_amd.expr import col as _col
            lsrc = g.MemoryExec([g.DeviceTable([c for c in li.columns if c.name in ("l_orderkey", "l_extendedprice")], li.num_rows)])
            lss = lsrc.schema()
            ps_ = g.NativePlan(g.RangeRepartitionExec(lsrc, [{"expr": _col("l_extendedprice", lss), "asc": True, "nulls_first": False}], world), tc)
            ps_.set_comm(comm)
            for _ in range(2):
                ps_.execute(0)
            ds, rs_ = timed_steps(lambda: ps_.execute(0), k)
            extra["sort_by_extendedprice_range_partitioned"] = {"ms_per_step": ds / k * 1e3, "lineitem_rows_per_s": rows_job * k / ds, "rows_on_rank0": rs_.num_rows}
            del p2, r2, p5, r5, su, li, od, cu, ps_, rs_, lsrc
            torch.cuda.empty_cache()
            l1 = T.gen_lineitem_device(tc, n_li, row0=rank * n_li)
            p3 = g.NativePlan(T.q1_dist_plan(l1), tc)
            p3.set_comm(comm)
            for _ in range(3):
                p3.execute(0)
            tc.ctx.jit_wait()
            d3, r3 = timed_steps(lambda: p3.execute(0), k)
            extra["q1_partial_states_gathered"] = {"ms_per_step": d3 / k * 1e3, "lineitem_rows_per_s": rows_job * k / d3, "result_groups": r3.num_rows}
        line["extra"] = extra
    if rank == 0:
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        comm.close()
        dist.destroy_process_group()


DUMP_BYTES_MAX = 64 << 20


def dump_q3_outputs(res, out_dir):
    """The q3 result of the last timed step as out_dir/<column>.npy, float64, one file per result column: l_orderkey, revenue (the
    Decimal128 value, as pyarrow casts it), o_orderdate (days since 1970-01-01), o_shippriority.  Rows stay in the order the plan
    returned them (ORDER BY revenue DESC, o_orderdate); only inside a run of rows with equal revenue and date, whose order the query
    leaves open, are they put in l_orderkey order, so that two builds write the same files when they compute the same answer.  At
    SF100 that is 1.2 M rows x 4 columns x 8 B = 38 MB; a result above DUMP_BYTES_MAX is cut to a fixed sample of rows (seed 0, in
    result order) and row_index.npy holds their positions."""
    import numpy as np
    import pyarrow as pa
    t = res.to_arrow()
    cols = {}
    for name in t.column_names:
        a = t.column(name).combine_chunks()
        if pa.types.is_date32(a.type):
            a = a.cast(pa.int32())
        cols[name] = a.cast(pa.float64()).to_numpy(zero_copy_only=False)
    n = t.num_rows
    tie = np.ones(n, dtype=bool)
    tie[1:] = (cols["revenue"][1:] != cols["revenue"][:-1]) | (cols["o_orderdate"][1:] != cols["o_orderdate"][:-1])
    order = np.lexsort((cols["l_orderkey"], np.cumsum(tie)))
    keep = DUMP_BYTES_MAX // (8 * (len(cols) + 1))
    rows = np.arange(n) if n <= keep else np.sort(np.random.default_rng(0).choice(n, size=keep, replace=False))
    out = {k: v[order[rows]] for k, v in cols.items()}
    if n > keep:
        out["row_index"] = rows.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for name, v in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), v)


def check_q3_result(torch, T, tc, res, li, od, cu):
    """The SF100 result against an independent computation with plain torch ops over the same HBM-resident columns (no gpuq kernel
    involved): the customers of the segment -> a Boolean table by key, the orders before the date whose customer is in it -> a
    Boolean table by order key, the lineitems shipped after the date whose order is in it; sum over them of l_extendedprice *
    (100 - l_discount) must equal the sum of the result's revenue column, the number of distinct orders among them its row count."""
    def colv(t, name, dtype, width):
        c = t.columns[[c.name for c in t.columns].index(name)]
        return c.data[: width * t.num_rows].view(dtype)
    ck = colv(cu, "c_custkey", torch.int64, 8)
    seg = cu.columns[[c.name for c in cu.columns].index("c_mktsegment")]
    offs = seg.offsets[: cu.num_rows + 1].to(torch.int64)              # (int32 tensor)
    first = seg.data[offs[:-1].clamp(max=seg.data.numel() - 1)]
    building = (first == ord("B")) & ((offs[1:] - offs[:-1]) == 8)      # the generator's five segments: only BUILDING starts with B
    in_seg = torch.zeros(int(ck.max().item()) + 2, dtype=torch.bool, device=ck.device)
    in_seg[ck[building]] = True
    ok, oc, odate = colv(od, "o_orderkey", torch.int64, 8), colv(od, "o_custkey", torch.int64, 8), colv(od, "o_orderdate", torch.int32, 4)
    o_live = (odate < T.Q3_DATE) & in_seg[oc.clamp(max=in_seg.numel() - 1)]
    in_ord = torch.zeros(int(ok.max().item()) + 2, dtype=torch.bool, device=ok.device)
    in_ord[ok[o_live]] = True
    del o_live, in_seg
    lk, ship = colv(li, "l_orderkey", torch.int64, 8), colv(li, "l_shipdate", torch.int32, 4)
    live = (ship > T.Q3_DATE) & in_ord[lk.clamp(max=in_ord.numel() - 1)]
    ext = colv(li, "l_extendedprice", torch.int64, 16)[0::2]          # low halves of the Decimal128 cells (15 digits: the high halves are sign extension)
    disc = colv(li, "l_discount", torch.int64, 16)[0::2]
    exp_rev = int((ext[live] * (100 - disc[live])).sum().item())
    hit = torch.zeros_like(in_ord)
    hit[lk[live]] = True
    exp_groups = int(hit.sum().item())
    del live, hit, in_ord
    t = res.to_device_table(tc.device)
    rc = t.columns[[c.name for c in t.columns].index("revenue")]
    got_rev = int(rc.data[: 16 * t.num_rows].view(torch.int64)[0::2].sum().item())
    return {"what": "SF result vs plain torch ops over the same columns: sum(revenue) and number of groups", "sum_revenue_matches": got_rev == exp_rev,
            "groups_match": t.num_rows == exp_groups, "sum_revenue_unscaled": got_rev, "groups": t.num_rows}


def cpu_baseline(sample_sf):
    """The oracle (C restatement, OpenMP over all host cores: "port") on an SF`sample_sf` sample of the same generator, data in host memory:
    q3 is the headline (`value`), q1 and q5 beside it; 3 runs each, min and mean (the reference's harness prints per-iteration and
    average times, benchmarks/src/bin/tpch.rs:333-344).  pyarrow Acero (hash join / group-by / sort on all host threads, money as int64
    cents) runs the same q3 / q5 as a second, independent CPU engine -- a proxy, not the reference's DataFusion path."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tpch_util as TO           # the oracle side lives with the tests
    n_li = TO.LINEITEM_ROWS.get(int(sample_sf), int(6_000_000 * sample_sf))
    n_cust, n_supp = int(150_000 * sample_sf), int(10_000 * sample_sf)
    h = TO.gen_q5_tables_host(n_li, n_cust, n_supp)

    def timed3(fn):
        ts, out = [], None
        for _ in range(3):
            t0 = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t0)
        return ts, out
    t3, (_r3, st3) = timed3(lambda: TO.q3_oracle_c(h, cap=0))
    t5, (_r5, st5) = timed3(lambda: TO.q5_oracle_c(h))
    hq1 = TO.gen_lineitem_host(n_li)
    t1, r1 = timed3(lambda: TO.q1_oracle_raw(n_li, host=hq1))
    del hq1

    def entry(ts, extra):
        return dict({"wall_ms_min": min(ts) * 1e3, "wall_ms_mean": sum(ts) / len(ts) * 1e3, "lineitem_rows_per_s": n_li / min(ts)}, **extra)
    cpu = ""
    try:
        cpu = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
        mem = [l for l in open("/proc/meminfo") if l.startswith("MemTotal")][0].split()[1]
        cpu += ", %d GiB RAM" % (int(mem) >> 20)
    except Exception:
        pass
    out = {"value": n_li / min(t3), "unit": "rows/s", "cores": TO.oracle_lib().oracle_num_threads(), "kind": "port", "wall_ms": min(t3) * 1e3, "wall_ms_mean": sum(t3) / 3 * 1e3,
           "host": cpu,
           "sample": "C oracle q3 (3 filters, 2 chained-hash-table joins, per-thread hash aggregate, sort) over synthetic SF%g tables (%d lineitem rows, %d groups), "
                     "min of 3 (mean beside it), data in host memory; the GPU line above is SF100: the sample is bounded so that the default run stays within minutes" % (sample_sf, n_li, st3["groups"]),
           "q1": entry(t1, {"groups": len(r1)}), "q3": entry(t3, {"groups": st3["groups"]}), "q5": entry(t5, {"groups": len(_r5), "pairs": st5["pairs"]})}
    del h
    try:
        import bench_extras
        out["proxy_acero"] = bench_extras.cpu_proxy_acero(TO, int(sample_sf))
    except Exception as e:      # the proxy is an extra: never lose the line over it
        out["proxy_acero"] = {"error": str(e)[:200]}
    return out


if __name__ == "__main__":
    main_q3()
