"""Secondary measurements attached to bench.py's JSON line under "extra" (--extras): the hash-join probe
micro-benchmark of SURVEY.md §8(d) (the other half of BASELINE.json's metric) and the q3 / q5 operator
pipelines.  Kernel times come from HIP events around the launch (gpuq_op_profile)."""
import ctypes as C
import os
import time

HBM_PEAK_GBS = 8000.0


def _sync(tc):
    tc.sync()


def join_probe_micro(tc, g, log2_build, log2_probe, hit_rate, reps=3, zipf=None):
    """build: 2^b unique int64 keys (shuffled); probe: 2^p uniform keys, `hit_rate` of them present.
    Algorithmic bytes: 24 B per probe row (8 key + 16 slot touch) + 12 B per emitted pair."""
    import torch
    from arrow_ballista_amd.expr import col
    dev = tc.device
    nb, npb = 1 << log2_build, 1 << log2_probe
    gen = torch.Generator(device=dev); gen.manual_seed(1234 + log2_build)
    bkeys = torch.randperm(nb, device=dev, generator=gen, dtype=torch.int64) * 2 + 1           # odd keys
    span = int(nb / max(hit_rate, 1e-9))
    if zipf:
        # Zipf(a) ranks over the build keys (skewed probe side), inverse-CDF of the continuous approximation
        # P(rank > x) = x^(1-a); rank r probes the r-th build key, so the hit rate is 100 %
        u = torch.rand(npb, device=dev, generator=gen, dtype=torch.float64)
        ranks = torch.clamp((1.0 - u * (1.0 - float(nb) ** (1.0 - zipf))) ** (1.0 / (1.0 - zipf)), max=float(nb)).to(torch.int64) - 1
        pkeys = bkeys[torch.clamp(ranks, 0, nb - 1)]
        del u, ranks
    else:
        pkeys = torch.randint(0, span, (npb,), device=dev, generator=gen, dtype=torch.int64) * 2 + 1   # odd key < 2*nb exists
    btab = g.DeviceTable([g.DeviceColumn("k", "Int64", bkeys.view(torch.uint8), nb, nullable=False)], nb)
    ptab = g.DeviceTable([g.DeviceColumn("k", "Int64", pkeys.view(torch.uint8), npb, nullable=False)], npb)
    bs, ps = btab.schema(), ptab.schema()
    bop = tc.op({"op": "join_build", "input": {"fields": bs}, "on": [col("k", bs)]})
    pop = tc.op({"op": "join_probe", "input": {"fields": ps}, "on": [col("k", ps)], "join_type": "Inner"})
    binp, _k1 = btab.input_struct()
    pinp, _k2 = ptab.input_struct()
    h = C.c_void_p()
    bop.profile(True)
    tc.ctx.check(tc.ctx.L.gpuq_join_build_run(bop.h, tc.stream_ptr(), C.byref(binp), 0, nb, C.byref(h)))
    build_ms, _ = bop.profile(False)
    ob = torch.empty(npb, dtype=torch.int32, device=dev)
    opb = torch.empty(npb, dtype=torch.int32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    best = None
    # device time of the whole call (probe kernel + segment scan + compaction into probe order) between two events on the stream the
    # call is queued on; the operator's own profile brackets the probe kernel alone
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(reps + 1):
        e0.record()
        tc.ctx.check(tc.ctx.L.gpuq_join_probe_run(pop.h, tc.stream_ptr(), h, C.byref(pinp), 0, ob.data_ptr(), opb.data_ptr(), npb, cnt.data_ptr()))
        e1.record()
        _sync(tc)
        ms = e0.elapsed_time(e1)
        if r > 0:
            best = ms if best is None or ms < best else best
    matches = int(cnt[0].item())
    pop.check(tc.stream_ptr())
    tc.ctx.L.gpuq_join_table_free(h)
    # spot-check: every emitted pair joins equal keys
    k = min(matches, 1 << 16)
    ok = bool((bkeys[ob[:k].long()] == pkeys[opb[:k].long()]).all().item()) if k else True
    exp = int(((pkeys < 2 * nb)).sum().item())
    alg_bytes = 24 * npb + 12 * matches
    return {"build_rows": nb, "probe_rows": npb, "hit_rate": hit_rate, "probe_keys": ("zipf(%.2f)" % zipf) if zipf else "uniform", "matches": matches, "matches_expected": exp, "pairs_valid": ok,
            "probe_ms": best, "probe_rows_per_s": npb / (best * 1e-3), "algorithmic_GBs": alg_bytes / (best * 1e-3) / 1e9,
            "frac_hbm_peak": alg_bytes / (best * 1e-3) / 1e9 / HBM_PEAK_GBS, "build_ms": build_ms, "build_rows_per_s": nb / (build_ms * 1e-3)}


def q1_pipeline(tc, T, g, sf):
    import torch
    n_li = T.LINEITEM_ROWS.get(sf, int(6_000_000 * sf))
    li = T.gen_lineitem_device(tc, n_li)
    plan = g.NativePlan(T.q1_plan(g.MemoryExec([li]), two_phase=True), tc)      # the C++ plan executor: one call per query
    times = []
    for r in range(4):
        _sync(tc)
        t0 = time.perf_counter()
        res = plan.execute(0)
        _sync(tc)
        times.append(time.perf_counter() - t0)
    del li
    torch.cuda.empty_cache()
    return {"wall_ms_best": min(times[1:]) * 1e3, "wall_ms_first": times[0] * 1e3, "result_rows": res.num_rows, "lineitem_rows": n_li,
            "lineitem_rows_per_s": n_li / min(times[1:])}


def q6_pipeline(tc, T, g, sf):
    """q6 (forecasting revenue change): one pass over four lineitem columns -- three Decimal128 (48 B) + Date32 (4 B) per row -- with the
    filter and SUM(l_extendedprice * l_discount) fused into one kernel: the plainest HBM-bound scan of the harness."""
    import torch
    n_li = T.LINEITEM_ROWS.get(sf, int(6_000_000 * sf))
    li = T.gen_lineitem_device(tc, n_li, columns=("l_quantity", "l_extendedprice", "l_discount", "l_shipdate"))
    plan = g.NativePlan(T.q6_plan(g.MemoryExec([li])), tc)
    times = []
    for r in range(5):
        _sync(tc)
        t0 = time.perf_counter()
        res = plan.execute(0)
        _sync(tc)
        times.append(time.perf_counter() - t0)
    del li
    torch.cuda.empty_cache()
    best = min(times[1:])
    return {"wall_ms_best": best * 1e3, "wall_ms_first": times[0] * 1e3, "result_rows": res.num_rows, "lineitem_rows": n_li, "lineitem_rows_per_s": n_li / best,
            "algorithmic_bytes": 52 * n_li, "GB_per_s": 52 * n_li / best / 1e9, "frac_of_8TBps": 52 * n_li / best / 8e12}


def tpch_pipelines(tc, T, g, sf):
    """q3 and q5 wall time (operator work only, inputs resident in HBM, synthetic TPC-H-shaped tables)."""
    n_li = T.LINEITEM_ROWS.get(sf, int(6_000_000 * sf))
    n_orders, n_cust, n_supp = (n_li + 3) // 4, int(150_000 * sf), int(10_000 * sf)
    li = T.gen_lineitem_device(tc, n_li, n_supp=n_supp, columns=("l_orderkey", "l_suppkey", "l_extendedprice", "l_discount", "l_shipdate"))
    od = T.gen_orders_device(tc, n_orders, n_cust)
    cu = T.gen_customer_device(tc, n_cust)
    su = T.gen_supplier_device(tc, n_supp)
    nation, region = T.nation_region_arrow()
    out = {"sf": sf, "lineitem_rows": n_li}
    for name, mk in (("q3", lambda: T.q3_plan(g.MemoryExec([cu]), g.MemoryExec([od]), g.MemoryExec([li]))),
                     ("q5", lambda: T.q5_plan(g.MemoryExec([cu]), g.MemoryExec([od]), g.MemoryExec([li]), g.MemoryExec([su]), g.MemoryExec([nation]), g.MemoryExec([region])))):
        times = []
        plan = g.NativePlan(mk(), tc)
        for r in range(4):
            _sync(tc)
            t0 = time.perf_counter()
            res = plan.execute(0)
            _sync(tc)
            times.append(time.perf_counter() - t0)
        out[name] = {"wall_ms_best": min(times[1:]) * 1e3, "wall_ms_first": times[0] * 1e3, "result_rows": res.num_rows,
                     "lineitem_rows_per_s": n_li / min(times[1:])}
    return out


def cpu_proxy_acero(T, sf):
    """CPU PROXY for q3 / q5 (SURVEY.md section 8d fallback): pyarrow Acero (multi-threaded hash join / group-by / sort) on the
    host cores over the same synthetic tables, money columns as int64 cents (cheaper for the CPU than the reference's Decimal128).
    It is NOT the reference's DataFusion path -- that cannot be built here -- and is reported only to put the GPU numbers next
    to a vectorised multi-core CPU engine on the same box.  Results are checked against the oracle's group counts."""
    import numpy as np
    import pyarrow as pa
    import pyarrow.compute as pc
    n_li = T.LINEITEM_ROWS.get(sf, int(6_000_000 * sf))
    n_orders, n_cust, n_supp = (n_li + 3) // 4, int(150_000 * sf), int(10_000 * sf)
    d = T.gen_lineitem_host(n_li, n_supp=n_supp)
    li = pa.table({"l_orderkey": d["l_orderkey"], "l_suppkey": d["l_suppkey"], "l_extendedprice": d["l_extendedprice"][0::2].astype(np.int64),
                   "l_discount": d["l_discount"][0::2].astype(np.int64), "l_shipdate": d["l_shipdate"]})
    del d
    orders, customer, supplier = T.gen_other_tables_host(n_orders, n_cust, n_supp)
    orders = orders.set_column(2, "o_orderdate", orders["o_orderdate"].cast(pa.int32()))
    nation, region = T.nation_region_arrow()

    def q3():
        c = customer.filter(pc.equal(customer["c_mktsegment"], "BUILDING")).select(["c_custkey"])
        o = orders.filter(pc.less(orders["o_orderdate"], T.Q3_DATE))
        co = o.join(c, keys="o_custkey", right_keys="c_custkey", join_type="inner").select(["o_orderkey", "o_orderdate", "o_shippriority"])
        l = li.filter(pc.greater(li["l_shipdate"], T.Q3_DATE)).select(["l_orderkey", "l_extendedprice", "l_discount"])
        j = l.join(co, keys="l_orderkey", right_keys="o_orderkey", join_type="inner")
        j = j.append_column("rev", pc.multiply(j["l_extendedprice"], pc.subtract(100, j["l_discount"])))
        g_ = j.group_by(["l_orderkey", "o_orderdate", "o_shippriority"]).aggregate([("rev", "sum")])
        return g_.sort_by([("rev_sum", "descending"), ("o_orderdate", "ascending")])

    def q5():
        r = region.filter(pc.equal(region["r_name"], "ASIA"))
        n_ = nation.join(r, keys="n_regionkey", right_keys="r_regionkey", join_type="inner").select(["n_nationkey", "n_name"])
        c = customer.join(n_, keys="c_nationkey", right_keys="n_nationkey", join_type="inner").select(["c_custkey", "c_nationkey", "n_name"])
        o = orders.filter(pc.and_(pc.greater_equal(orders["o_orderdate"], T.Q5_DATE_LO), pc.less(orders["o_orderdate"], T.Q5_DATE_HI)))
        oc = o.join(c, keys="o_custkey", right_keys="c_custkey", join_type="inner").select(["o_orderkey", "c_nationkey", "n_name"])
        l = li.select(["l_orderkey", "l_suppkey", "l_extendedprice", "l_discount"]).join(oc, keys="l_orderkey", right_keys="o_orderkey", join_type="inner")
        ls = l.join(supplier, keys=["l_suppkey", "c_nationkey"], right_keys=["s_suppkey", "s_nationkey"], join_type="inner")
        ls = ls.append_column("rev", pc.multiply(ls["l_extendedprice"], pc.subtract(100, ls["l_discount"])))
        return ls.group_by(["n_name"]).aggregate([("rev", "sum")]).sort_by([("rev_sum", "descending")])
    out = {"engine": "pyarrow %s Acero, %d threads" % (pa.__version__, pa.cpu_count()), "sf": sf, "lineitem_rows": n_li,
           "note": "CPU proxy, not the reference's DataFusion path; int64 cents instead of Decimal128"}
    for name, fn in (("q3", q3), ("q5", q5)):
        best, rows = None, 0
        for _ in range(2):
            t0 = time.perf_counter(); res = fn(); dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best; rows = res.num_rows
        out[name] = {"wall_ms_best": best * 1e3, "result_rows": rows, "lineitem_rows_per_s": n_li / best}
    return out


def dist_join(T, g, rows_per_rank, steps=5):
    """Partitioned hash join across ranks (BASELINE configs[4] shape): every rank owns a lineitem shard and the matching
    orders shard; both sides are hash-repartitioned on the join key (same partition function), exchanged with one
    variable-size all-to-all per column buffer, and joined locally.  Launch with torch.distributed.run, one rank per GPU
    (GPUQ_BENCH_BACKEND=gloo rehearses it with ranks sharing a GPU).  Weak scaling: rows per rank fixed."""
    import torch
    import torch.distributed as dist
    from arrow_ballista_amd import parallel
    from arrow_ballista_amd.expr import col
    world, rank, local = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("GPUQ_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group(backend, **({"device_id": torch.device("cuda", local)} if backend == "nccl" else {}))
    tc = g.TaskContext(device=local)
    tc.ctx.set_jit("wait")
    n_li = rows_per_rank
    n_or = (n_li + 3) // 4
    li = T.gen_lineitem_device(tc, n_li, row0=rank * n_li, columns=("l_orderkey", "l_extendedprice"))
    od = T.gen_orders_device(tc, n_or, 1_500_000, row0=rank * n_or)
    ls, os_ = li.schema(), od.schema()
    on = [(col("o_orderkey", os_), col("l_orderkey", ls))]

    def step():
        return parallel.partitioned_hash_join(tc, od, li, on, "Inner")
    out = step()
    total = torch.tensor([out.num_rows], dtype=torch.int64, device=tc.device if backend == "nccl" else "cpu")
    if world > 1:
        dist.all_reduce(total)
    times = []
    for _ in range(steps):
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        out = step()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        times.append(time.perf_counter() - t0)
    res = {"workload": "partitioned hash join lineitem x orders on orderkey, both sides exchanged", "n_gpus": world, "backend": backend,
           "probe_rows_per_rank": n_li, "build_rows_per_rank": n_or, "joined_rows_total": int(total.item()), "every_line_found_its_order": int(total.item()) == n_li * world,
           "ms_best": min(times) * 1e3, "probe_rows_per_s_all_ranks": n_li * world / min(times)}
    if world > 1:
        dist.destroy_process_group()
    return res if rank == 0 else None


def shuffle_codec(tc, T, g, rows, reps=3):
    """Shuffle sink / source codec on the q3 stage-0 shuffle columns of lineitem (l_orderkey Int64,
    l_extendedprice / l_discount Decimal128(15,2), l_shipdate Date32 = 44 B/row): one IPC RecordBatch message, LZ4_FRAME buffers.
    encode_kernels = compress + layout + pack on the device (size query: nothing copied back); encode_to_host adds the D2H of
    the body into pinned memory; decode = H2D of the message + device decompress.  CPU proxy: pyarrow (Arrow C++ + liblz4,
    its own thread pool) writing / reading the same batch in host memory."""
    import io
    import pyarrow as pa
    import torch
    from arrow_ballista_amd import shuffle as S
    t = T.gen_lineitem_device(tc, rows, columns=("l_orderkey", "l_extendedprice", "l_discount", "l_shipdate"))
    raw = rows * 44
    out = {"rows": rows, "raw_bytes": raw}

    def best(fn):
        b = None
        for _ in range(reps):
            _sync(tc); t0 = time.perf_counter(); r = fn(); _sync(tc); dt = time.perf_counter() - t0
            b = dt if b is None or dt < b else b
        return b, r
    S.encoded_size(tc, t)                                   # warm-up (pool, pinned scratch)
    dt, size = best(lambda: S.encoded_size(tc, t))
    out["encoded_bytes"] = size
    out["ratio"] = raw / size
    out["encode_kernels_ms"] = dt * 1e3
    out["encode_kernels_GBps_in"] = raw / dt / 1e9
    buf = torch.empty(size + 4096, dtype=torch.uint8, pin_memory=True)
    dt, (msg, buf) = best(lambda: S.encode_batch(tc, t, 0, buf))
    out["encode_to_host_ms"] = dt * 1e3
    out["encode_to_host_GBps_in"] = raw / dt / 1e9
    stream = io.BytesIO()
    stream.write(S._arrow_schema(t).serialize().to_pybytes()); stream.write(msg); stream.write(S.EOS)
    data = stream.getvalue()
    S.read_ipc_stream(tc, data)
    dt, _ = best(lambda: S.read_ipc_stream(tc, data))
    out["decode_from_host_ms"] = dt * 1e3
    out["decode_from_host_GBps_out"] = raw / dt / 1e9
    # CPU proxy: the same rows in the reference's configuration (8192-row batches, shuffle_writer.rs + IpcWriteOptions LZ4_FRAME)
    host = pa.ipc.open_stream(data).read_all()
    def cpu_write():
        sink = pa.BufferOutputStream()
        with pa.ipc.new_stream(sink, host.schema, options=pa.ipc.IpcWriteOptions(compression="lz4")) as w:
            w.write_table(host, max_chunksize=8192)
        return sink.getvalue()
    dt, cbuf = best(cpu_write)
    out["cpu_proxy_arrow_cpp"] = {"threads": pa.cpu_count(), "batch_rows": 8192, "write_ms": dt * 1e3, "write_GBps_in": raw / dt / 1e9, "encoded_bytes": cbuf.size}
    dt, _ = best(lambda: pa.ipc.open_stream(cbuf).read_all())
    out["cpu_proxy_arrow_cpp"].update({"read_ms": dt * 1e3, "read_GBps_out": raw / dt / 1e9})
    # the CPU-written file (2048 batches x 4 columns, linked-block frames: one wave per buffer) decoded on the device in one call
    cb = cbuf.to_pybytes()
    S.read_ipc_stream(tc, cb)
    dt, _ = best(lambda: S.read_ipc_stream(tc, cb))
    out["decode_cpu_written_file_ms"] = dt * 1e3
    out["decode_cpu_written_file_GBps_out"] = raw / dt / 1e9
    return out


def _q6_matches_numpy(np, x, d, with_stddev):
    """h2o q6 against numpy: rows sorted by (id4, id5, v3), the middles of every group (the even case is (lo + hi) / 2 in Float64,
    exactly), and -- when asked -- the groups' sample standard deviation to 1e-9 relative."""
    id4, id5, v3 = (x.column(c).to_numpy() for c in ("id4", "id5", "v3"))
    order = np.lexsort((v3, id5, id4))
    a, b, v = id4[order], id5[order], v3[order]
    starts = np.flatnonzero(np.concatenate([[True], (a[1:] != a[:-1]) | (b[1:] != b[:-1])]))
    ends = np.concatenate([starts[1:], [len(v)]])
    cnt = ends - starts
    hi = starts + cnt // 2
    med = np.where(cnt % 2 == 1, v[hi], (v[hi - 1] + v[hi]) / 2.0)
    got = d.sort_by([("id4", "ascending"), ("id5", "ascending")])
    ok = got.num_rows == len(starts) and np.array_equal(got.column("id4").to_numpy(), a[starts]) and np.array_equal(got.column("id5").to_numpy(), b[starts])
    ok = ok and np.array_equal(got.column("median_v3").to_numpy(), med)
    if ok and with_stddev:
        mean = np.add.reduceat(v, starts) / cnt
        dev = np.add.reduceat((v - np.repeat(mean, cnt)) ** 2, starts)
        sd = np.sqrt(dev / np.maximum(cnt - 1, 1))
        gsd = got.column("sd").to_numpy(zero_copy_only=False).astype(np.float64)
        many = cnt > 1
        ok = bool(np.all(np.abs(gsd[many] - sd[many]) <= 1e-9 * np.maximum(1.0, np.abs(sd[many])))) and bool(np.all(np.isnan(gsd[~many])))
    return ok


def h2o(tc, T, g, n=10_000_000, k=100, reps=3):
    """The reference's own operator micro-workloads (benchmarks/db-benchmark: groupby-datafusion.py G1_1e7_1e2_0_0 q1-q10,
    join-datafusion.py J1_1e7_NA_0_0), data regenerated with the h2o recipe (id1..id3 strings -> ints here).
    Device time per question through the native plan executor (inputs resident in HBM, best of `reps` after one warm-up), the
    same question through pyarrow Acero on the host as a labelled CPU proxy, and a check of the two results against each other.
    q6 is run three ways: its stddev half alone, its median alone, and both together -- the reference's actual q6.  Acero has no exact
    grouped median, so the two forms with a MEDIAN are checked against numpy (np.lexsort over id4, id5, v3, then the middles of every
    group) and carry no cpu_proxy_acero_ms.
    Not run: q8 (top-2 per group) -- no device operator; q10 groups by 4 of its 6 keys (MAX_KEYS = 4)."""
    import numpy as np
    import pyarrow as pa
    import pyarrow.compute as pc
    from arrow_ballista_amd.expr import col
    r = np.random.default_rng(11)
    x = pa.table({
        "id1": pa.array(r.integers(1, k + 1, n), pa.int64()), "id2": pa.array(r.integers(1, k + 1, n), pa.int64()),
        "id3": pa.array(r.integers(1, n // k + 1, n), pa.int64()), "id4": pa.array(r.integers(1, k + 1, n).astype(np.int32), pa.int32()),
        "id5": pa.array(r.integers(1, k + 1, n).astype(np.int32), pa.int32()), "id6": pa.array(r.integers(1, n // k + 1, n).astype(np.int32), pa.int32()),
        "v1": pa.array(r.integers(1, 6, n).astype(np.int32), pa.int32()), "v2": pa.array(r.integers(1, 16, n).astype(np.int32), pa.int32()),
        "v3": pa.array(np.round(r.random(n) * 100, 6), pa.float64())})
    x = x.cast(pa.schema([pa.field(f.name, f.type, nullable=False) for f in x.schema]))
    dx = g.MemoryExec([g.DeviceTable.from_arrow(x, tc.device)])
    s = dx.schema()
    A = lambda fn, c, name, c2=None: dict({"fn": fn, "expr": col(c, s), "name": name}, **({"expr2": col(c2, s)} if c2 else {}))
    questions = {
        "q1 sum(v1) by id1": (["id1"], [A("SUM", "v1", "v1")], [("v1", "sum")]),
        "q2 sum(v1) by id1,id2": (["id1", "id2"], [A("SUM", "v1", "v1")], [("v1", "sum")]),
        "q3 sum(v1) avg(v3) by id3": (["id3"], [A("SUM", "v1", "v1"), A("AVG", "v3", "v3")], [("v1", "sum"), ("v3", "mean")]),
        "q4 avg(v1..v3) by id4": (["id4"], [A("AVG", "v1", "v1"), A("AVG", "v2", "v2"), A("AVG", "v3", "v3")], [("v1", "mean"), ("v2", "mean"), ("v3", "mean")]),
        "q5 sum(v1..v3) by id6": (["id6"], [A("SUM", "v1", "v1"), A("SUM", "v2", "v2"), A("SUM", "v3", "v3")], [("v1", "sum"), ("v2", "sum"), ("v3", "sum")]),
        "q6 stddev(v3) by id4,id5": (["id4", "id5"], [A("STDDEV", "v3", "sd")], [("v3", "stddev", pc.VarianceOptions(ddof=1))]),
        "q6 median(v3) by id4,id5": (["id4", "id5"], [A("MEDIAN", "v3", "median_v3")], "numpy"),
        "q6 median(v3) stddev(v3) by id4,id5": (["id4", "id5"], [A("MEDIAN", "v3", "median_v3"), A("STDDEV", "v3", "sd")], "numpy"),
        "q7 max(v1) min(v2) by id3": (["id3"], [A("MAX", "v1", "mx"), A("MIN", "v2", "mn")], [("v1", "max"), ("v2", "min")]),
        "q9 corr(v1,v2) by id2,id4": (["id2", "id4"], [A("CORRELATION", "v1", "r", "v2")], None),
        "q10 sum(v3) count by id1..id4": (["id1", "id2", "id3", "id4"], [A("SUM", "v3", "v3"), A("COUNT", "v1", "c")], [("v3", "sum"), ("v1", "count")]),
    }
    out = {"rows": n, "groupby": {}, "join": {}}

    def timed(fn):
        fn(); best = None
        for _ in range(reps):
            _sync(tc); t0 = time.perf_counter(); res = fn(); _sync(tc); dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best
        return best, res
    for name, (keys, aggs, host_aggs) in questions.items():
        mk = lambda: g.NativePlan(g.AggregateExec("Single", [(col(c, s), c) for c in keys], aggs, dx, expected_groups=0), tc)
        plan = mk()
        dt, res = timed(lambda: plan.execute(0))
        # an operator that has never run (no remembered group count): the first execution of a fresh plan, kernels already compiled
        cold = None
        for _ in range(2):
            fresh = mk(); _sync(tc); t0 = time.perf_counter(); fresh.execute(0); _sync(tc); c = time.perf_counter() - t0
            cold = c if cold is None or c < cold else cold
        e = {"device_ms": dt * 1e3, "first_run_ms": cold * 1e3, "groups": res.num_rows, "rows_per_s": n / dt}
        if host_aggs == "numpy":
            e["cpu_proxy_acero_ms"] = None      # absent: Acero has no exact grouped median
            e["matches_cpu"] = bool(_q6_matches_numpy(np, x, res.to_arrow(), "sd" in [a["name"] for a in aggs]))
        elif host_aggs is not None:
            t0 = time.perf_counter(); h = x.group_by(keys).aggregate(host_aggs); e["cpu_proxy_acero_ms"] = (time.perf_counter() - t0) * 1e3
            e["cpu_threads"] = pa.cpu_count()
            d = res.to_arrow()
            ok = h.num_rows == d.num_rows
            for (cname, fn, *_), a in zip(host_aggs, aggs):          # order-free check: column totals agree
                hv, dv = pc.sum(h.column("%s_%s" % (cname, fn))).as_py(), pc.sum(d.column(a["name"])).as_py()
                ok = ok and abs(float(hv) - float(dv)) <= 1e-9 * max(1.0, abs(float(hv)))
            e["matches_cpu"] = bool(ok)
        out["groupby"][name] = e
    # join: x (id1 in 1..10, id2 in 1..1e4 scaled, id3 in 1..n) against small / medium / big
    jx = pa.table({"id1": pa.array(r.integers(1, 11, n), pa.int64()), "id2": pa.array(r.integers(1, n // 1000 + 1, n), pa.int64()),
                   "id3": pa.array(r.integers(1, n + 1, n), pa.int64()), "v1": pa.array(np.round(r.random(n) * 100, 6), pa.float64())})
    jx = jx.cast(pa.schema([pa.field(f.name, f.type, nullable=False) for f in jx.schema]))
    djx = g.MemoryExec([g.DeviceTable.from_arrow(jx, tc.device)])
    js = djx.schema()

    def side(m, key):
        ids = r.permutation(m)[: max(1, int(m * 0.9))] + 1          # 90 % of the key domain present, as the h2o generator leaves gaps
        t = pa.table({key: pa.array(ids, pa.int64()), "v2": pa.array(np.round(r.random(len(ids)) * 100, 6), pa.float64())})
        return t.cast(pa.schema([pa.field(f.name, f.type, nullable=False) for f in t.schema]))
    for name, m, key, jt in (("q1 small inner on id1", 10, "id1", "Inner"), ("q2 medium inner on id2", n // 1000, "id2", "Inner"), ("q3 medium left on id2", n // 1000, "id2", "Right"),
                             ("q5 big inner on id3", n, "id3", "Inner")):
        small = side(m, key).rename_columns(["r_" + key, "v2"])
        dsm = g.MemoryExec([g.DeviceTable.from_arrow(small, tc.device)])
        ss = dsm.schema()
        # build side = the smaller table (DataFusion's left input); "left join" of x keeps x's rows = Right join here
        join = g.HashJoinExec(dsm, djx, [(col("r_" + key, ss), col(key, js))], None, jt, "CollectLeft", False)
        jsch = join.schema()
        plan = g.NativePlan(g.AggregateExec("Single", [], [{"fn": "COUNT", "expr": col("v1", jsch), "name": "c"}, {"fn": "SUM", "expr": col("v2", jsch), "name": "s2"}], join), tc)
        dt, res = timed(lambda: plan.execute(0))
        cnt, s2 = (res.to_arrow().column(i)[0].as_py() for i in (0, 1))
        t0 = time.perf_counter()
        hj = jx.join(small, keys=key, right_keys="r_" + key, join_type="inner" if jt == "Inner" else "left outer")
        hc, hs = hj.num_rows, pc.sum(hj.column("v2")).as_py()
        cpu = time.perf_counter() - t0
        out["join"][name] = {"device_ms": dt * 1e3, "probe_rows_per_s": n / dt, "result_rows": cnt, "cpu_proxy_acero_ms": cpu * 1e3,
                             "matches_cpu": bool(cnt == hc and abs((s2 or 0.0) - (hs or 0.0)) <= 1e-9 * max(1.0, abs(hs or 0.0)))}
    return out


def approx_distinct(tc, T, g, log2n=28, n_grouped=10_000_000, k=100, reps=3):
    """APPROX_DISTINCT next to COUNT(DISTINCT) and to a plain streaming read of the same column (an ungrouped SUM), through the native
    plan executor, inputs resident in HBM, best of `reps` after one warm-up: (a) ungrouped over 2^log2n Int64 rows holding 2^24 different
    values -- one segment, every tile stores a partial sketch and one block merges them; (b) grouped in h2o's `id4, id5` shape
    (k x k groups) over n_grouped rows.  COUNT(DISTINCT) of the same run gives the exact counts the estimates are held against.
    Per-kernel times (the sketch pass and the merge apart) come from a kernel trace of this run, not from here."""
    import sys
    import numpy as np
    import pyarrow as pa
    from arrow_ballista_amd.expr import col

    def timed(plan):
        plan.execute(0); best = None
        for _ in range(reps):
            _sync(tc); t0 = time.perf_counter(); res = plan.execute(0); _sync(tc); dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best
        return best * 1e3, res.to_arrow()

    def three(src, keys, c, exact_rows):
        s = src.schema()
        ke = [(col(x, s), x) for x in keys]
        A = lambda fn, name, **kw: dict({"fn": fn, "expr": col(c, s), "name": name}, **kw)
        e = {}
        e["sum_ms"], _ = timed(g.NativePlan(g.AggregateExec("Single", ke, [A("SUM", "s")], src), tc))
        print("approx_distinct bench: SUM by %s done" % (keys or "nothing"), file=sys.stderr, flush=True)
        e["approx_distinct_ms"], apx = timed(g.NativePlan(g.AggregateExec("Single", ke, [A("APPROX_DISTINCT", "d")], src), tc))
        print("approx_distinct bench: APPROX_DISTINCT done", file=sys.stderr, flush=True)
        e["count_distinct_ms"], cd = timed(g.NativePlan(g.AggregateExec("Single", ke, [A("COUNT", "d", distinct=True)], src), tc))
        print("approx_distinct bench: COUNT(DISTINCT) done", file=sys.stderr, flush=True)
        e["count_distinct_over_approx"] = e["count_distinct_ms"] / e["approx_distinct_ms"]
        e["approx_over_sum"] = e["approx_distinct_ms"] / e["sum_ms"]
        by = [(x, "ascending") for x in keys]
        a, b = (apx.sort_by(by), cd.sort_by(by)) if keys else (apx, cd)
        est, exact = a.column("d").to_numpy().astype(np.float64), b.column("d").to_numpy().astype(np.float64)
        e["groups"] = int(len(exact))
        e["same_groups"] = bool(all(a.column(x).equals(b.column(x)) for x in keys)) and len(est) == len(exact)
        e["exact_is_known_count"] = None if exact_rows is None else bool(len(exact) == 1 and int(exact[0]) == exact_rows)
        e["worst_relative_error"] = float(np.max(np.abs(est - exact) / np.maximum(exact, 1.0)))
        e["mean_relative_error"] = float(np.mean(np.abs(est - exact) / np.maximum(exact, 1.0)))
        return e
    out = {}
    n = 1 << log2n
    # uniform draws, not an arithmetic sequence: the hash aggregate behind COUNT(DISTINCT) sizes itself from every (n / 2^20)-th row, and a
    # sequence i * c mod 2^24 shows such a power-of-two stride only 2^24 / stride of its values
    v = np.random.default_rng(5).integers(0, 1 << 24, n)
    known = int(np.count_nonzero(np.bincount(v, minlength=1 << 24)))
    t = pa.table({"v": pa.array(v)})
    t = t.cast(pa.schema([pa.field("v", pa.int64(), nullable=False)]))
    src = g.MemoryExec([g.DeviceTable.from_arrow(t, tc.device)])
    del v, t
    out["ungrouped"] = dict({"rows": n, "bytes": n * 8}, **three(src, [], "v", known))
    out["ungrouped"]["approx_distinct_GBps"] = n * 8 / out["ungrouped"]["approx_distinct_ms"] / 1e6
    out["ungrouped"]["sum_GBps"] = n * 8 / out["ungrouped"]["sum_ms"] / 1e6
    del src
    r = np.random.default_rng(11)
    m = n_grouped
    x = pa.table({"id4": pa.array(r.integers(1, k + 1, m).astype(np.int32)), "id5": pa.array(r.integers(1, k + 1, m).astype(np.int32)),
                  "id3": pa.array(r.integers(1, m // k + 1, m), pa.int64())})
    x = x.cast(pa.schema([pa.field(f.name, f.type, nullable=False) for f in x.schema]))
    out["by_id4_id5"] = dict({"rows": m}, **three(g.MemoryExec([g.DeviceTable.from_arrow(x, tc.device)]), ["id4", "id5"], "id3", None))
    return out


def distinct(tc, T, g, n=10_000_000, k=100, reps=3, log2big=27):
    """DISTINCT beside plain aggregates: COUNT(DISTINCT v1), SUM(v3), COUNT(DISTINCT id6) as ONE plan over n rows of the db-benchmark
    shape (v1 in 1..5, id6 in 1..n/k, v3 Float64), grouped by id4, id5 (k x k groups) and ungrouped, through the native plan executor,
    inputs resident in HBM, best of `reps` after one warm-up.  Next to the step time: the plans a user needed before for the same answers
    -- each COUNT(DISTINCT x) alone (the two-level rewrite) and the plain SUM alone, same executor, same process -- with a check that
    the answers agree; gpuq_segment_distinct alone over the id6 column sorted by (keys..., id6) (its launches between two events) with
    its rate on the algorithmic bytes, 2 x 4 per row: the value read by both passes; and a plain ungrouped SUM over id6, the one-read
    floor.  10 M Int32 rows are 40 MB, where launches weigh as much as bytes: "at_size" times the same entry point (COUNT and SUM from one
    scan) over 2^log2big sorted Int64 rows, as one segment and in segments of 1,024 rows, with its share of the 8 TB/s peak on 2 x 8
    bytes per row."""
    import ctypes as C
    import numpy as np
    import pyarrow as pa
    import torch
    from arrow_ballista_amd import binding as B
    from arrow_ballista_amd.expr import col
    r = np.random.default_rng(11)
    cols = {"id4": r.integers(1, k + 1, n).astype(np.int32), "id5": r.integers(1, k + 1, n).astype(np.int32), "id6": r.integers(1, n // k + 1, n).astype(np.int32),
            "v1": r.integers(1, 6, n).astype(np.int32), "v3": np.round(r.random(n) * 100, 6)}
    x = pa.table({c: pa.array(v) for c, v in cols.items()})
    x = x.cast(pa.schema([pa.field(f.name, f.type, nullable=False) for f in x.schema]))
    src = g.MemoryExec([g.DeviceTable.from_arrow(x, tc.device)])
    s = src.schema()

    def timed(plan):
        plan.execute(0); best = None
        for _ in range(reps):
            _sync(tc); t0 = time.perf_counter(); res = plan.execute(0); _sync(tc); dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best
        return best * 1e3, res.to_arrow()
    A = lambda fn, c, name, **kw: dict({"fn": fn, "expr": col(c, s), "name": name}, **kw)
    out = {"rows": n}
    L, ctx, stream = B.lib(), tc.ctx.h, tc.stream_ptr()
    for label, keys in (("by_id4_id5", ["id4", "id5"]), ("ungrouped", [])):
        ke = [(col(c, s), c) for c in keys]
        by = [(c, "ascending") for c in keys]
        e = {}
        e["step_ms"], one = timed(g.NativePlan(g.AggregateExec("Single", ke, [A("COUNT", "v1", "d1", distinct=True), A("SUM", "v3", "s3"), A("COUNT", "id6", "d6", distinct=True)], src), tc))
        e["count_distinct_v1_alone_ms"], d1 = timed(g.NativePlan(g.AggregateExec("Single", ke, [A("COUNT", "v1", "d1", distinct=True)], src), tc))
        e["count_distinct_id6_alone_ms"], d6 = timed(g.NativePlan(g.AggregateExec("Single", ke, [A("COUNT", "id6", "d6", distinct=True)], src), tc))
        e["sum_v3_alone_ms"], s3 = timed(g.NativePlan(g.AggregateExec("Single", ke, [A("SUM", "v3", "s3")], src), tc))
        e["three_plans_ms"] = e["count_distinct_v1_alone_ms"] + e["count_distinct_id6_alone_ms"] + e["sum_v3_alone_ms"]
        e["one_plan_over_three_plans"] = e["step_ms"] / e["three_plans_ms"]
        one, d1, d6, s3 = ((t.sort_by(by) if keys else t) for t in (one, d1, d6, s3))
        e["groups"] = one.num_rows
        e["counts_match"] = bool(one.column("d1").equals(d1.column("d1")) and one.column("d6").equals(d6.column("d6")) and all(one.column(c).equals(d1.column(c)) for c in keys))
        a, b = one.column("s3").to_numpy(), s3.column("s3").to_numpy()
        e["sum_worst_relative_difference"] = float(np.max(np.abs(a - b) / np.abs(b)))      # (two orders of a Float64 sum)
        # the reduction alone: id6 sorted by (keys..., id6) on the host, the segments from gpuq_segment_heads
        order = np.lexsort([cols["id6"]] + [cols[c] for c in keys[::-1]])
        st = pa.table({c: pa.array(cols[c][order]) for c in keys + ["id6"]})
        st = st.cast(pa.schema([pa.field(f.name, f.type, nullable=False) for f in st.schema]))
        dev = g.DeviceTable.from_arrow(st, tc.device)
        starts = torch.zeros(n + 2, dtype=torch.int32, device=tc.device); cnt = torch.zeros(2, dtype=torch.int64, device=tc.device)
        G = 1
        if keys:
            kc = (B.gpuq_column * len(keys))(*[dev.column(c).to_c() for c in keys])
            tc.ctx.check(L.gpuq_segment_heads(ctx, stream, kc, len(keys), n, None, starts.data_ptr(), n, cnt.data_ptr()))
            _sync(tc); G = int(cnt[0].item())
        else:
            starts[1] = n
        vc = dev.column("id6").to_c()
        counts = torch.empty(G + 1, dtype=torch.int64, device=tc.device)
        best = None
        for _ in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tc.ctx.check(L.gpuq_segment_distinct(ctx, stream, C.byref(vc), starts.data_ptr(), G, n, counts.data_ptr(), None, 8, None, 8, None))
            e1.record(); _sync(tc)
            ms = e0.elapsed_time(e1)
            best = ms if best is None or ms < best else best
        e["kernel_ms"] = best
        e["kernel_bytes_per_row"] = 2 * 4
        e["kernel_GBps"] = n * e["kernel_bytes_per_row"] / best / 1e6
        e["kernel_counts_match"] = bool(np.array_equal(counts[:G].cpu().numpy(), one.column("d6").to_numpy()))
        out[label] = e
        del dev, st, order
    out["plain_sum_id6_ms"], _ = timed(g.NativePlan(g.AggregateExec("Single", [], [A("SUM", "id6", "s")], src), tc))
    out["plain_sum_id6_GBps"] = n * 4 / out["plain_sum_id6_ms"] / 1e6
    for label in ("by_id4_id5", "ungrouped"):
        out[label]["kernel_over_plain_sum"] = out[label]["kernel_ms"] / out["plain_sum_id6_ms"]
    # the reduction where bytes dominate: 2^log2big sorted Int64 values (at most 2^24 different ones), COUNT and SUM from one scan -- as one
    # segment, and in segments of 1,024 rows (the values ascend across them, which the kernel neither knows nor uses)
    n2 = 1 << log2big
    big = torch.sort(torch.randint(0, 1 << 24, (n2,), dtype=torch.int64, device=tc.device))[0]
    uniq = torch.unique_consecutive(big)
    bc = B.gpuq_column()
    bc.type, bc.repr, bc.data, bc.length = B.T_INT64, B.REPR_ARROW, big.data_ptr(), n2
    torch.cuda.synchronize()
    at = {"rows": n2, "bytes_per_row": 2 * 8}
    for label, st in (("one_segment", torch.tensor([0, n2], dtype=torch.int32, device=tc.device)), ("segments_of_1024", torch.arange(0, n2 + 1, 1024, dtype=torch.int32, device=tc.device))):
        G = int(st.numel()) - 1
        counts, sums = torch.empty(G + 1, dtype=torch.int64, device=tc.device), torch.empty(G + 1, dtype=torch.int64, device=tc.device)
        torch.cuda.synchronize()
        best = None
        for _ in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tc.ctx.check(L.gpuq_segment_distinct(ctx, stream, C.byref(bc), st.data_ptr(), G, n2, counts.data_ptr(), sums.data_ptr(), 8, None, 8, None))
            e1.record(); _sync(tc)
            ms = e0.elapsed_time(e1)
            best = ms if best is None or ms < best else best
        at[label] = {"segments": G, "kernel_ms": best, "kernel_GBps": n2 * 16 / best / 1e6, "share_of_8TBps": n2 * 16 / best / 1e6 / 8000.0}
        if G == 1:
            at[label]["matches_torch_unique"] = bool(int(counts[0].item()) == int(uniq.numel()) and int(sums[0].item()) == int(uniq.sum().item()))
        else:
            at[label]["count_total"] = int(counts[:G].sum().item())      # (a value that crosses a boundary counts on both sides: >= the one segment's)
    out["at_size"] = at
    return out


def grouping_sets(tc, T, g, n=10_000_000, k=100, reps=3):
    """Grouping sets: SUM(v1), COUNT(*), AVG(v3) by ROLLUP(id4, id5) and by CUBE(id1, id4, id5), each as ONE plan over n rows of the
    db-benchmark shape (id1, id4, id5 in 1..k, v1 in 1..5, v3 Float64), through the native plan executor, inputs resident in HBM, best of
    `reps` after one warm-up.  Next to the step time: what a user had to run before for the same rows -- the S plain AggregateExec plans,
    one per set, same executor, same process -- with a check that the answers agree (COUNT and SUM exactly, AVG to a relative
    difference: two orders of a Float64 sum); and gpuq_grouping_expand alone over the columns of the plan's state table (its launches
    between two events) with its rate on the algorithmic bytes: n w read, S n w plus the validity bits written, per column."""
    import ctypes as C
    import numpy as np
    import pyarrow as pa
    import torch
    from arrow_ballista_amd import binding as B
    from arrow_ballista_amd.expr import col, lit
    r = np.random.default_rng(18)
    cols = {"id1": r.integers(1, k + 1, n).astype(np.int32), "id4": r.integers(1, k + 1, n).astype(np.int32), "id5": r.integers(1, k + 1, n).astype(np.int32),
            "v1": r.integers(1, 6, n).astype(np.int32), "v3": np.round(r.random(n) * 100, 6)}
    x = pa.table({c: pa.array(v) for c, v in cols.items()})
    x = x.cast(pa.schema([pa.field(f.name, f.type, nullable=False) for f in x.schema]))
    src = g.MemoryExec([g.DeviceTable.from_arrow(x, tc.device)])
    s = src.schema()
    aggs = [{"fn": "SUM", "expr": col("v1", s), "name": "s1"}, {"fn": "COUNT", "expr": lit(1), "name": "n"}, {"fn": "AVG", "expr": col("v3", s), "name": "a3"}]

    def timed(plan):
        plan.execute(0); best = None
        for _ in range(reps):
            _sync(tc); t0 = time.perf_counter(); res = plan.execute(0); _sync(tc); dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best
        return best * 1e3, res.to_arrow()
    L, ctx, stream = B.lib(), tc.ctx.h, tc.stream_ptr()
    out = {"rows": n}
    for label, keys, sets in (("rollup_id4_id5", ["id4", "id5"], g.plan.rollup_sets(2)), ("cube_id1_id4_id5", ["id1", "id4", "id5"], g.plan.cube_sets(3))):
        ke = [(col(c, s), c) for c in keys]
        e = {"sets": len(sets)}
        e["one_plan_ms"], one = timed(g.NativePlan(g.AggregateExec("Single", ke, aggs, src, grouping_sets=sets), tc))
        e["output_rows"] = one.num_rows
        total, agree, worst, per_set = 0.0, True, 0.0, []
        nulls = np.stack([np.asarray(one.column(c).is_null()) for c in keys], axis=1)
        for mask in sets:
            kept = [c for c, m in zip(keys, mask) if not m]
            ms, ref = timed(g.NativePlan(g.AggregateExec("Single", [(col(c, s), c) for c in kept], aggs, src), tc))
            total += ms; per_set.append(ms)
            mine = one.filter(pa.array(np.all(nulls == np.array(mask), axis=1)))      # (no NULL keys in this table: a set's rows are those NULL exactly where it masks)
            by = [(c, "ascending") for c in kept]
            mine, ref = (mine.sort_by(by), ref.sort_by(by)) if kept else (mine, ref)
            agree = agree and mine.num_rows == ref.num_rows and all(mine.column(c).equals(ref.column(c)) for c in kept + ["s1", "n"])
            if mine.num_rows == ref.num_rows:
                a, b = mine.column("a3").to_numpy(), ref.column("a3").to_numpy()
                worst = max(worst, float(np.max(np.abs(a - b) / np.abs(b))))
        e["plans_per_set_ms"] = per_set
        e["s_plans_ms"] = total
        e["one_plan_over_s_plans"] = e["one_plan_ms"] / total
        e["answers_agree"] = bool(agree)
        e["avg_worst_relative_difference"] = worst
        # the expansion alone, over columns of the state table's widths: the keys, SUM's Int64 state, COUNT's, AVG's count and Float64 sum
        fine = int(np.sum(~nulls.any(axis=1)))
        widths = [(B.T_INT32, 4, True)] * len(keys) + [(B.T_INT64, 8, False), (B.T_INT64, 8, False), (B.T_UINT64, 8, False), (B.T_FLOAT64, 8, False)]
        S = len(sets)
        bufs = []
        for ki, (tid, w, is_key) in enumerate(widths):
            c = B.gpuq_column()
            data = torch.zeros(fine * w + 16, dtype=torch.uint8, device=tc.device)
            c.type, c.repr, c.data, c.length = tid, B.REPR_ARROW, data.data_ptr(), fine
            null_sets = sum(1 << si for si, mask in enumerate(sets) if mask[ki]) if is_key else 0
            bufs.append((c, data, null_sets, torch.empty(fine * S * w + 16, dtype=torch.uint8, device=tc.device),
                         torch.empty(((fine * S + 63) // 64 + 1) * 8, dtype=torch.uint8, device=tc.device) if null_sets else None))
        best = None
        for _ in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for c, _, null_sets, o, v in bufs:
                tc.ctx.check(L.gpuq_grouping_expand(ctx, stream, C.byref(c), fine, S, null_sets, o.data_ptr(), v.data_ptr() if v is not None else None))
            e1.record(); _sync(tc)
            ms = e0.elapsed_time(e1)
            best = ms if best is None or ms < best else best
        nbytes = sum(fine * w + S * fine * w + ((S * fine + 7) // 8 if null_sets else 0) for (_, w, _), (_, _, null_sets, _, _) in zip(widths, bufs))
        e["finest_groups"] = fine
        e["expand_kernel_ms"] = best
        e["expand_algorithmic_bytes"] = int(nbytes)
        e["expand_GBps"] = nbytes / best / 1e6
        out[label] = e
        del bufs
    return out


def window(tc, T, g, log2n=28, log2p=20, reps=3):
    """BoundedWindowAggExec over 2^log2n Int64 rows that are already ordered by an Int32 partition key of about 2^log2p partitions (their
    sizes geometric) and an Int64 order key: one plan computes ROW_NUMBER, a running SUM (ROWS UNBOUNDED PRECEDING .. CURRENT ROW) and
    LAG(v, 1), through the native plan executor, inputs resident in HBM, best of `reps` after one warm-up.  Next to the step time: the
    segmented scan alone (gpuq_window_scan, its three launches between two events) with its share of the 8 TB/s peak on the algorithmic
    bytes 2 (8 + 4) + 8 + 1/8 per row -- value and segment id read twice, the cell and a validity bit written once -- and a plain
    ungrouped SUM over the same column in the same process, which is the one-read floor."""
    import ctypes as C
    import numpy as np
    import pyarrow as pa
    import torch
    from arrow_ballista_amd import binding as B
    from arrow_ballista_amd import expr as E
    from arrow_ballista_amd.expr import col
    n = 1 << log2n
    r = np.random.default_rng(9)
    k = np.cumsum(r.integers(0, 1 << (log2n - log2p), n, dtype=np.uint16 if log2n - log2p <= 16 else np.uint32) == 0, dtype=np.int32)
    t = pa.table({"k": pa.array(k), "o": pa.array(np.arange(n, dtype=np.int64)), "v": pa.array(r.integers(-1000, 1000, n))})
    t = t.cast(pa.schema([pa.field("k", pa.int32(), nullable=False), pa.field("o", pa.int64(), nullable=False), pa.field("v", pa.int64(), nullable=False)]))
    partitions = int(k[-1]) + 1
    dev = g.DeviceTable.from_arrow(t, tc.device)
    src = g.MemoryExec([dev])
    del k, t

    def timed(plan):
        plan.execute(0); best = None
        for _ in range(reps):
            _sync(tc); t0 = time.perf_counter(); res = plan.execute(0); _sync(tc); dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best
        return best * 1e3, res
    ov = dict(partition_by=[col("k")], order_by=[E.sort_expr(col("o"))])
    node = g.BoundedWindowAggExec(src, [E.window("ROW_NUMBER", [], "rn", **ov), E.window("SUM", [col("v")], "s", frame=E.rows_between(None, 0), **ov), E.lag(col("v"), "l", **ov)])
    out = {"rows": n, "partitions": partitions}
    out["step_ms"], res = timed(g.NativePlan(node, tc))
    tail = res.to_arrow().slice(n - 4, 4)
    out["last_rows"] = {c: tail[c].to_pylist() for c in ("k", "rn", "s", "l")}
    del res, tail
    s = src.schema()
    out["plain_sum_ms"], _ = timed(g.NativePlan(g.AggregateExec("Single", [], [{"fn": "SUM", "expr": col("v", s), "name": "s"}], src), tc))
    # the scan alone, on the entry point the node calls
    L, ctx, stream = B.lib(), tc.ctx.h, tc.stream_ptr()
    kc, vc = dev.column("k").to_c(), dev.column("v").to_c()
    seg = torch.empty(n, dtype=torch.int32, device=tc.device); starts = torch.empty(n + 2, dtype=torch.int32, device=tc.device)
    cnt = torch.zeros(2, dtype=torch.int64, device=tc.device)
    cells = torch.empty(n, dtype=torch.int64, device=tc.device); valid = torch.empty((n + 63) // 64 + 1, dtype=torch.int64, device=tc.device)
    tc.ctx.check(L.gpuq_segment_heads(ctx, stream, C.byref(kc), 1, n, seg.data_ptr(), starts.data_ptr(), n, cnt.data_ptr()))
    best = None
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tc.ctx.check(L.gpuq_window_scan(ctx, stream, C.byref(vc), seg.data_ptr(), n, 0, cells.data_ptr(), 8, None, valid.data_ptr(), None))
        e1.record(); _sync(tc)
        ms = e0.elapsed_time(e1)
        best = ms if best is None or ms < best else best
    out["scan_ms"] = best
    out["scan_bytes_per_row"] = 2 * (8 + 4) + 8 + 0.125
    out["scan_GBps"] = n * out["scan_bytes_per_row"] / best / 1e6
    out["scan_share_of_8TBps"] = out["scan_GBps"] / 8000.0
    out["plain_sum_GBps"] = n * 8 / out["plain_sum_ms"] / 1e6
    out["scan_over_plain_sum"] = best / out["plain_sum_ms"]
    return out


def temporal(tc, T, g, log2n=27, reps=5):
    """Interval and Duration arithmetic: a projection of `ts + interval '1' month` and one of `ts - other_ts` over 2^log2n
    Timestamp(Microsecond) rows (instants of 1950 .. 2050, required columns resident in HBM), through the native plan executor, best of
    `reps` after one warm-up.  Next to them, in the same process, `cast(cast(ts as Int64) + 1 as Timestamp)`: one column read, one
    written, one add -- the floor of a one-column projection.  ts - ts reads two columns, so its floor is 1.5 times that."""
    import numpy as np
    import pyarrow as pa
    from arrow_ballista_amd import expr as E
    from arrow_ballista_amd.expr import Operator as Op
    from arrow_ballista_amd.expr import binary, cast, col, lit
    n = 1 << log2n
    r = np.random.default_rng(11)
    lo, hi = -631152000 * 10 ** 6, 2524608000 * 10 ** 6      # 1950-01-01 .. 2050-01-01
    ts = pa.timestamp("us")
    t = pa.Table.from_arrays([pa.array(r.integers(lo, hi, n)).cast(ts), pa.array(r.integers(lo, hi, n)).cast(ts)],
                             schema=pa.schema([pa.field("a", ts, nullable=False), pa.field("b", ts, nullable=False)]))
    head = t.slice(0, 4)
    src = g.MemoryExec([g.DeviceTable.from_arrow(t, tc.device)])
    del t
    s = src.schema()

    def timed(e):
        plan = g.NativePlan(g.ProjectionExec([(e, "x")], src), tc)
        res = plan.execute(0); first = res.to_arrow().slice(0, 4)["x"].to_pylist(); del res
        best = None
        for _ in range(reps):
            _sync(tc); t0 = time.perf_counter(); res = plan.execute(0); _sync(tc); dt = time.perf_counter() - t0
            del res
            best = dt if best is None or dt < best else best
        return best * 1e3, [str(x) for x in first]
    out = {"rows": n, "first_rows": {"a": [str(x) for x in head["a"].to_pylist()], "b": [str(x) for x in head["b"].to_pylist()]}}
    out["floor_ms"], out["first_rows"]["a+1"] = timed(cast(binary(cast(col("a", s), "Int64"), Op.Plus, lit(1)), ("Timestamp", "Microsecond")))
    out["month_ms"], out["first_rows"]["a+1month"] = timed(binary(col("a", s), Op.Plus, E.interval_year_month(1)))
    out["diff_ms"], out["first_rows"]["a-b"] = timed(binary(col("a", s), Op.Minus, col("b", s)))
    out["month_over_floor"] = out["month_ms"] / out["floor_ms"]
    out["diff_over_floor"] = out["diff_ms"] / out["floor_ms"]
    out["floor_GBps"] = n * 16 / out["floor_ms"] / 1e6
    out["month_GBps"] = n * 16 / out["month_ms"] / 1e6
    out["diff_GBps"] = n * 24 / out["diff_ms"] / 1e6
    return out


def like_micro(tc, T, g, n=1 << 23, reps=5):
    """LikeExpr throughput (q13's `o_comment NOT LIKE '%special%requests%'` shape): n comment-like strings of 19-78 bytes built
    from a word list, Arrow layout in HBM; one gpuq_like_utf8 launch per pattern.  Bytes = offsets + string bytes read."""
    import ctypes as C
    import numpy as np
    import pyarrow as pa
    import pyarrow.compute as pc
    import torch
    r = np.random.default_rng(5)
    words = np.array(["special", "requests", "deposits", "pending", "furiously", "carefully", "packages", "accounts", "blithely", "ironic", "final", "express", "regular", "quickly"])
    k = 6
    parts = words[r.integers(0, len(words), (n, k))]
    col = parts[:, 0]
    for j in range(1, k):
        col = np.char.add(np.char.add(col, " "), parts[:, j])
    arr = pa.array(col, type=pa.string())
    if isinstance(arr, pa.ChunkedArray):
        arr = pa.concat_arrays(arr.chunks)
    t = g.DeviceTable.from_arrow(pa.table({"c": arr}), tc.device)
    c = t.columns[0]
    nbytes = int(arr.buffers()[2].size) + 4 * (n + 1)
    out = {"rows": n, "bytes": nbytes, "patterns": {}}
    bits = torch.zeros(((n + 63) // 64) * 8 + 8, dtype=torch.uint8, device=tc.device)
    for pat in ("%special%requests%", "furiously%", "%accounts", "%ironic%", "_pecial%"):
        best = None
        for _ in range(reps):
            _sync(tc); t0 = time.perf_counter()
            tc.ctx.check(tc.ctx.L.gpuq_like_utf8(tc.ctx.h, tc.stream_ptr(), C.byref(c.to_c()), None, n, pat.encode(), 0, 0, bits.data_ptr(), None))
            _sync(tc); dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best
        got = int(np.unpackbits(bits.cpu().numpy()[: (n + 7) // 8], bitorder="little")[:n].sum())
        t0 = time.perf_counter(); exp = pc.sum(pc.match_like(arr, pat)).as_py(); cpu = time.perf_counter() - t0
        out["patterns"][pat] = {"device_ms": best * 1e3, "GBps": nbytes / best / 1e9, "matches": got, "matches_cpu": bool(got == exp), "cpu_proxy_arrow_cpp_ms": cpu * 1e3}
    return out


def ingest_q1(tc, T, g, sf=10, batch_rows=65536, threads=(4, 8, 16), chunk_batches=64):
    """BASELINE configs[1] as the boundary hands it over: q1's 7 lineitem columns as 64 Ki-row host Arrow batches (78 B/row).
    (a) ingest alone (gpuq_ingest_push of every batch, wait for the last): H2D GB/s against the PCIe Gen5 x16 ceiling, for
    several staging-thread counts; (b) PCIe-inclusive q1: the partial aggregate consumes the landed prefix in chunks of
    `chunk_batches` batches while the staging threads keep copying, the final aggregate merges the chunks' states; wall time from
    the first push to the result, next to the HBM-resident time of the same rows."""
    import pyarrow as pa
    import torch
    from arrow_ballista_amd.ingest import Ingest
    n = T.LINEITEM_ROWS.get(sf, int(6_000_000 * sf))
    n = n // batch_rows * batch_rows                      # whole batches
    cols = ["l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag", "l_linestatus", "l_shipdate"]
    host = T.lineitem_host_to_arrow(T.gen_lineitem_host(n), n).select(cols)
    host = host.cast(pa.schema([pa.field(f.name, f.type, nullable=False) for f in host.schema])).combine_chunks()
    batches = [host.slice(i, batch_rows).to_batches()[0] for i in range(0, n, batch_rows)]
    raw = 78 * n
    out = {"rows": n, "batches": len(batches), "batch_rows": batch_rows, "bytes": raw, "pcie_gen5_x16_spec_GBps": 63.0, "ingest_only": []}
    for nt in threads:
        best = None
        for _ in range(2):
            ing = Ingest(tc, host.schema, n, 2 * n + 64, n_threads=nt)
            t0 = time.perf_counter()
            for b in batches:
                ing.push(b)
            ing.wait_rows(n)
            dt = time.perf_counter() - t0
            ing.close()
            best = dt if best is None or dt < best else best
        out["ingest_only"].append({"threads": nt, "ms": best * 1e3, "GBps": raw / best / 1e9, "frac_of_pcie_spec": raw / best / 1e9 / 63.0})
    nt = max(out["ingest_only"], key=lambda e: e["GBps"])["threads"]
    # HBM-resident reference: the same rows already on the device
    ing = Ingest(tc, host.schema, n, 2 * n + 64, n_threads=nt)
    for b in batches:
        ing.push(b)
    ing.wait_rows(n)
    resident = ing.table(0, n)
    plan = g.NativePlan(T.q1_plan(g.MemoryExec([resident]), two_phase=True), tc)
    for _ in range(3):
        plan.execute(0)
    tc.ctx.jit_wait()
    _sync(tc); t0 = time.perf_counter(); ref = plan.execute(0); _sync(tc)
    out["q1_hbm_resident_ms"] = (time.perf_counter() - t0) * 1e3
    ref_rows = ref.to_arrow().to_pylist()
    del plan, ref, resident
    ing.close()
    # pipelined: compiled plans are reused across chunks (same layout), so only data movement + kernels are timed
    chunk = chunk_batches * batch_rows
    best, rows_out = None, None
    for rep in range(3):
        ing = Ingest(tc, host.schema, n, 2 * n + 64, n_threads=nt)
        t0 = time.perf_counter()
        for b in batches:
            ing.push(b)
        states, done = [], 0
        partial = None
        while done < n:
            k = min(chunk, n - done)
            ing.wait_rows(done + k)
            view = ing.table(done, k)
            if partial is None:      # one compiled plan for every chunk: the views share a layout, only pointers and row counts change
                partial_py, full_py, final_src = T.q1_split_plan(view, 64)
                partial = g.NativePlan(partial_py, tc)
            else:
                partial.set_input(0, view)
            res = partial.execute(0)
            states.append(g.plan.materialize(tc, res.to_device_table(tc.device), force=True))
            done += k
        final_src.partitions[0] = g.plan.concat_tables(tc, states)
        res = g.NativePlan(full_py, tc).execute(0)
        _sync(tc)
        dt = time.perf_counter() - t0
        rows_out = res.to_arrow().to_pylist()
        ing.close()
        if rep > 0:
            best = dt if best is None or dt < best else best
    out["q1_pcie_inclusive"] = {"threads": nt, "chunk_batches": chunk_batches, "ms": best * 1e3, "rows_per_s": n / best, "GBps": raw / best / 1e9,
                                "equals_hbm_resident_result": rows_out == ref_rows}
    out["q1_hbm_resident_rows_per_s"] = n / (out["q1_hbm_resident_ms"] * 1e-3)
    return out


def run(tc, T, g, full=True):
    extra = {"join_probe": []}
    grid = [(20, 28, 1.0), (24, 28, 1.0), (27, 28, 1.0), (24, 28, 0.5), (24, 28, 0.1)] if full else [(20, 24, 1.0)]
    for b, p, h in grid:
        extra["join_probe"].append(join_probe_micro(tc, g, b, p, h))
    if full:
        extra["join_probe"].append(join_probe_micro(tc, g, 24, 28, 1.0, zipf=1.05))
    extra["tpch"] = tpch_pipelines(tc, T, g, 10 if full else 1)
    return extra


def sort_micro(tc, T, g, log2n=27, reps=5):
    """SortExec alone: 2^log2n generated lineitem rows, (a) by l_extendedprice (Decimal128(15,2): ~24 key bits after range
    compression -> packed 8-byte records, 3 single-read passes), (b) by (l_orderkey DESC, l_shipdate) (two-field key, one u64 word).
    Time = one execute() (min/max pass + read-back, pack, histograms, passes), best of `reps`, inputs resident in HBM."""
    from arrow_ballista_amd.expr import col
    import os
    # "SortExec alone" = the operator's permutation (gpuq_sort_run), not the materialised result: the Python restatement of the executor
    # returns the late-materialised view, the native executor (node.execute's default since round 3) would gather all three columns
    os.environ["GPUQ_PLAN_LAYER"] = "mirror"
    n = 1 << log2n
    li = T.gen_lineitem_device(tc, n, columns=("l_orderkey", "l_extendedprice", "l_shipdate"))
    src = g.MemoryExec([li])
    s = src.schema()
    out = {"rows": n}
    for name, spec in (("by_extendedprice", [("l_extendedprice", True)]), ("by_orderkey_desc_shipdate", [("l_orderkey", False), ("l_shipdate", True)])):
        plan = g.SortExec([{"expr": col(c, s), "asc": a, "nulls_first": False} for c, a in spec], src)
        for _ in range(2):
            plan.execute(0, tc)
        tc.ctx.jit_wait()
        best = None
        for _ in range(reps):
            _sync(tc); t0 = time.perf_counter(); v = plan.execute(0, tc); _sync(tc)
            dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best
        out[name] = {"ms": best * 1e3, "rows_per_s": n / best}
        del v
    os.environ.pop("GPUQ_PLAN_LAYER", None)
    return out


def sort_shard(tc, T, g, rows=224_998_637, reps=4):
    """BASELINE configs[4] on one GPU: the shard an 8-GPU SF300 `lineitem ORDER BY l_extendedprice` leaves each GPU with (1,799,989,091 / 8
    rows), key l_extendedprice Decimal128(15,2) + the l_orderkey payload, through the native executor's SortExec (deferred from the second
    execution on).  Floor = SURVEY.md section 8d: N x (K + 8) x 2 bytes with K = 16 (one read and one write of key + row id)."""
    import torch
    from arrow_ballista_amd.expr import col
    li = T.gen_lineitem_device(tc, rows, columns=("l_orderkey", "l_extendedprice"))
    src = g.MemoryExec([li]); s = src.schema()
    plan = g.NativePlan(g.SortExec([{"expr": col("l_extendedprice", s), "asc": True, "nulls_first": False}], src), tc)
    ts = []
    for r in range(reps + 1):
        if r == 1:
            plan.profile(True)
        _sync(tc); t0 = time.perf_counter(); res = plan.execute(0); _sync(tc)
        ts.append(time.perf_counter() - t0)
    ops = plan.profile_all(); plan.profile(False)
    perm_ms = sum(o.get("op_ms", 0.0) for o in ops if o["op"] == "sort") / max(1, reps)       # SortExec's own kernels: sample, pack, passes -> the permutation
    st = plan.exec_stats()
    # sortedness of the result (outside the timing): the key column of the result must be non-decreasing
    t = res.to_device_table(tc.device)
    kc = t.columns[[c.name for c in t.columns].index("l_extendedprice")]
    k = kc.data[: 16 * t.num_rows].view(torch.int64)[0::2]
    ok = bool((k[1:] >= k[:-1]).all().item()) and t.num_rows == rows
    best = min(ts[1:])
    floor = rows * (16 + 8) * 2
    del res, t, li
    torch.cuda.empty_cache()
    return {"rows": rows, "ms_best": best * 1e3, "ms_first": ts[0] * 1e3, "rows_per_s": rows / best, "sorted": ok, "deferred": st["deferred"], "host_round_trips": st["settles"] + st["host_syncs"],
            "floor_bytes": floor, "floor_GBs": floor / best / 1e9, "frac_hbm_peak": floor / best / 1e9 / 8000.0,
            "permutation_ms": perm_ms, "permutation_frac_hbm_peak": (floor / (perm_ms * 1e-3) / 1e9 / 8000.0) if perm_ms > 0 else None,
            "note": "ms_best = SortExec + the gather of key and payload into sorted order (random 8 / 16-byte reads: the larger part); permutation_ms = SortExec's own kernels"}


def merge_micro(tc, T, g, log2n=27, runs=8, reps=3):
    """Ordered fan-in alone (gpuq_merge_run behind CoalesceTasksExec with an order): `runs` partitions of 2^log2n / runs rows, each
    already sorted by l_extendedprice, merged into one order; next to it the stable sort of their concatenation (what round 1 did)."""
    from arrow_ballista_amd.expr import col
    n = (1 << log2n) // runs
    order = lambda s: [{"expr": col("l_extendedprice", s), "asc": True, "nulls_first": False}]
    parts = []
    for r in range(runs):
        li = T.gen_lineitem_device(tc, n, columns=("l_orderkey", "l_extendedprice"), row0=r * n)
        src = g.MemoryExec([li])
        parts.append(g.plan.materialize(tc, g.SortExec(order(src.schema()), src).execute(0, tc), force=True))
    src = g.MemoryExec(parts)
    s = src.schema()
    out = {"rows": n * runs, "runs": runs}
    for name, plan in (("merge", g.CoalesceTasksExec(src, list(range(runs)), order_by=order(s))),
                       ("concat_then_sort", g.SortExec(order(s), g.CoalescePartitionsExec(src)))):
        native = g.NativePlan(plan, tc)
        for _ in range(2):
            native.execute(0)
        tc.ctx.jit_wait()
        best = None
        for _ in range(reps):
            _sync(tc); t0 = time.perf_counter(); res = native.execute(0); _sync(tc)
            dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best
            del res
        out[name] = {"ms": best * 1e3, "rows_per_s": n * runs / best}
    return out


def scan_decode(tc, T, g, sf=1):
    """the CsvExec / ParquetExec leaves.  lineitem's 9 generated columns at `sf` as (a) '|' text as dbgen
    writes it, (b) Parquet as the reference's `convert --compression none` writes it (dictionary pages where they pay), both in
    host memory; timed from the host bytes to Arrow-layout columns in HBM (upload + kernels), best of 3.  Next to it pyarrow's
    own multi-threaded readers on the host cores (the decoded columns would still have to cross PCIe after that)."""
    import io
    import pyarrow as pa
    import pyarrow.csv as pacsv
    import pyarrow.parquet as pq
    from arrow_ballista_amd import scan
    n = T.LINEITEM_ROWS.get(sf, int(6_000_000 * sf))
    if hasattr(T, "gen_lineitem_host"):      # (tests/tpch_util: the oracle's host generator; same rows)
        li = T.lineitem_host_to_arrow(T.gen_lineitem_host(n), n)
    else:                                    # bench.py: the device generator's rows, copied back once
        li = T.gen_lineitem_device(tc, n, columns=("l_orderkey", "l_suppkey", "l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag", "l_linestatus", "l_shipdate")).to_arrow(tc.ctx)
    li = li.cast(pa.schema([pa.field(f.name, f.type, nullable=False) for f in li.schema]))
    arrow_bytes = sum(c.nbytes for c in li.columns)
    buf = io.BytesIO()
    pacsv.write_csv(li, buf, pacsv.WriteOptions(include_header=False, delimiter="|", quoting_style="none"))
    text = buf.getvalue()
    buf = io.BytesIO()
    pq.write_table(li, buf, compression="NONE", use_dictionary=True, data_page_size=1 << 20, row_group_size=1 << 20)
    pfile = buf.getvalue()
    tj = {"int64": "Int64", "string": "Utf8", "date32[day]": "Date32"}
    schema = [(f.name, tj.get(str(f.type), {"Decimal128": [15, 2]}), False) for f in li.schema]
    out = {"rows": n, "arrow_bytes": arrow_bytes, "text_bytes": len(text), "parquet_bytes": len(pfile)}

    def best_of(fn, reps=3):
        b = None
        for _ in range(reps):
            _sync(tc); t0 = time.perf_counter(); r = fn(); _sync(tc)
            dt = time.perf_counter() - t0
            del r
            b = dt if b is None or dt < b else b
        return b
    scan.read_csv(tc, text[:1 << 20].rsplit(b"\n", 1)[0] + b"\n", schema, delimiter="|")      # warm the allocator / staging
    dt = best_of(lambda: scan.read_csv(tc, text, schema, delimiter="|"))
    out["csv_device"] = {"ms": dt * 1e3, "file_GBps": len(text) / dt / 1e9, "rows_per_s": n / dt}
    dt = best_of(lambda: scan.read_parquet(tc, pfile))
    out["parquet_device"] = {"ms": dt * 1e3, "file_GBps": len(pfile) / dt / 1e9, "rows_per_s": n / dt}
    dt = best_of(lambda: scan.read_parquet(tc, pfile, ["l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag", "l_linestatus", "l_shipdate"]))
    out["parquet_device_q1_columns"] = {"ms": dt * 1e3, "rows_per_s": n / dt}
    buf = io.BytesIO()
    pq.write_table(li, buf, compression="SNAPPY", use_dictionary=True, data_page_size=1 << 20, row_group_size=1 << 20)
    sfile = buf.getvalue()
    dt = best_of(lambda: scan.read_parquet(tc, sfile))
    out["parquet_snappy_device"] = {"ms": dt * 1e3, "file_bytes": len(sfile), "file_GBps": len(sfile) / dt / 1e9, "rows_per_s": n / dt}
    dt = best_of(lambda: pq.read_table(pa.BufferReader(sfile)))
    out["parquet_snappy_pyarrow_host"] = {"ms": dt * 1e3, "rows_per_s": n / dt, "threads": os.cpu_count()}
    buf = io.BytesIO()
    pq.write_table(li, buf, compression="ZSTD", use_dictionary=True, data_page_size=1 << 20, row_group_size=1 << 20)      # (the reference's `tpch convert` default codec)
    zfile = buf.getvalue()
    dt = best_of(lambda: scan.read_parquet(tc, zfile))
    out["parquet_zstd_device"] = {"ms": dt * 1e3, "file_bytes": len(zfile), "file_GBps": len(zfile) / dt / 1e9, "rows_per_s": n / dt}
    dt = best_of(lambda: pq.read_table(pa.BufferReader(zfile)))
    out["parquet_zstd_pyarrow_host"] = {"ms": dt * 1e3, "rows_per_s": n / dt, "threads": os.cpu_count()}
    co = pacsv.ConvertOptions(column_types=li.schema)
    dt = best_of(lambda: pacsv.read_csv(pa.BufferReader(text), read_options=pacsv.ReadOptions(column_names=li.schema.names),
                                        parse_options=pacsv.ParseOptions(delimiter="|", quote_char=False), convert_options=co))
    out["csv_pyarrow_host"] = {"ms": dt * 1e3, "file_GBps": len(text) / dt / 1e9, "rows_per_s": n / dt, "threads": os.cpu_count()}
    dt = best_of(lambda: pq.read_table(pa.BufferReader(pfile)))
    out["parquet_pyarrow_host"] = {"ms": dt * 1e3, "file_GBps": len(pfile) / dt / 1e9, "rows_per_s": n / dt, "threads": os.cpu_count()}
    # the decoded columns feed q1 unchanged (checked against the oracle where it is at hand: the tests' T; bench.py's has none, and checks
    # the Snappy decode against the plain one instead)
    dev = scan.read_parquet(tc, pfile)
    rows = T.q1_result_to_rows(tc, T.run_q1(tc, dev))
    if hasattr(T, "q1_oracle_rows"):
        out["q1_over_decoded_columns_equals_oracle"] = rows == T.q1_oracle_rows(n) if n <= 6_100_000 else None
    rows_s = T.q1_result_to_rows(tc, T.run_q1(tc, scan.read_parquet(tc, sfile)))
    out["q1_over_snappy_equals_q1_over_plain"] = rows_s == rows and len(rows) > 0
    rows_z = T.q1_result_to_rows(tc, T.run_q1(tc, scan.read_parquet(tc, zfile)))
    out["q1_over_zstd_equals_q1_over_plain"] = rows_z == rows and len(rows) > 0
    return out


def scan_plan(tc, T, g, sf=10, reps=5):
    """q1 and q6 from Parquet FILES through ONE plan (ParquetExec leaf: footer, row-group pruning, upload of the projected chunks,
    page decode, then the query), PCIe included, next to today's two steps in the same process: scan.read_parquet of the same
    columns, then the plan over a MemoryExec.  lineitem at `sf` is written to a temporary directory as the reference's `tpch convert`
    would (ZSTD), as Snappy, and once more sorted by l_shipdate -- labelled as such: generated lineitem is not clustered by date and
    prunes little, the sorted file shows what pruning buys when it can.  Every time is a list over `reps` repetitions after one
    warm-up; "spread" is max - min of that list."""
    import json
    import shutil
    import sys
    import tempfile
    import pyarrow as pa
    import pyarrow.parquet as pq
    from arrow_ballista_amd import scan
    n = T.LINEITEM_ROWS.get(sf, int(6_000_000 * sf))
    cols = ("l_quantity", "l_extendedprice", "l_discount", "l_tax", "l_returnflag", "l_linestatus", "l_shipdate")
    if hasattr(T, "gen_lineitem_host"):
        li = T.lineitem_host_to_arrow(T.gen_lineitem_host(n), n)
    else:
        li = T.gen_lineitem_device(tc, n, columns=cols).to_arrow(tc.ctx)
    li = li.cast(pa.schema([pa.field(f.name, f.type, nullable=False) for f in li.schema]))
    tj = {"int64": "Int64", "int32": "Int32", "string": "Utf8", "date32[day]": "Date32"}
    schema = [{"name": f.name, "type": tj.get(str(f.type), {"Decimal128": [15, 2]}), "nullable": False} for f in li.schema]
    names = [f["name"] for f in schema]
    d = tempfile.mkdtemp(prefix="gpuq_scan_plan_")
    out = {"rows": n, "reps": reps, "legs": []}
    try:
        files = []
        for label, table, codec in (("zstd", li, "ZSTD"), ("snappy", li, "SNAPPY"), ("zstd, file sorted by l_shipdate", li.sort_by("l_shipdate"), "ZSTD")):
            path = os.path.join(d, "lineitem_%d.parquet" % len(files))
            pq.write_table(table, path, compression=codec, use_dictionary=True, data_page_size=1 << 20, row_group_size=1 << 20)
            files.append((label, path))
            print("scan-plan: wrote %s (%s, %d bytes)" % (path, label, os.path.getsize(path)), file=sys.stderr, flush=True)
        del li
        queries = (("q1", T.q1_plan, cols), ("q6", T.q6_plan, ("l_quantity", "l_extendedprice", "l_discount", "l_shipdate")))

        def timed(fn):
            _sync(tc); t0 = time.perf_counter(); r = fn(); _sync(tc)
            return (time.perf_counter() - t0) * 1e3, r

        def pred_of(plan):
            while not isinstance(plan, g.FilterExec):
                plan = plan.children()[0]
            return plan.predicate
        for label, path in files:
            for q, make, need in queries:
                proj = [names.index(c) for c in need]
                leaf = g.ParquetExec([[path]], schema, projection=proj)
                leaf.predicate = pred_of(make(leaf))
                one = g.NativePlan(make(leaf), tc)
                _, r = timed(lambda: one.execute(0))      # warm-up: operators compiled, staging lanes and allocator warm
                m = [x for x in one.metrics() if x["node"] == "ParquetExec"][0]
                rows_one = T.table_to_rows(tc, g.plan.materialize(tc, r.to_device_table(tc.device)))
                dev = scan.read_parquet(tc, path, list(need))
                two = g.NativePlan(make(g.MemoryExec([dev])), tc)
                rows_two = T.table_to_rows(tc, g.plan.materialize(tc, two.execute(0).to_device_table(tc.device)))
                del dev, r

                def two_step():
                    t = scan.read_parquet(tc, path, list(need))
                    two.set_input(0, t)
                    return two.execute(0), t
                t_one, t_two = [], []
                for _ in range(reps):      # interleaved: both forms see the same machine state
                    t_two.append(timed(two_step)[0])
                    t_one.append(timed(lambda: one.execute(0))[0])
                spread = lambda v: max(v) - min(v)
                out["legs"].append({"file": label, "query": q, "file_bytes": os.path.getsize(path), "one_plan_ms": [round(x, 2) for x in t_one],
                                    "two_step_ms": [round(x, 2) for x in t_two], "one_plan_best_ms": round(min(t_one), 2), "two_step_best_ms": round(min(t_two), 2),
                                    "one_plan_spread_ms": round(spread(t_one), 2), "two_step_spread_ms": round(spread(t_two), 2),
                                    "one_plan_within_spread_of_two_step": min(t_one) <= min(t_two) + max(spread(t_one), spread(t_two)),
                                    "row_groups": m["row_groups"], "row_groups_pruned": m["row_groups_pruned"], "bytes_scanned": m["bytes_scanned"],
                                    "rows_equal": rows_one == rows_two and len(rows_one) > 0})
                one.close(); two.close()
                print("scan-plan: %s" % json.dumps(out["legs"][-1]), file=sys.stderr, flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return out


if __name__ == "__main__":
    import json
    import os
    import sys
    ROOT = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tpch_util as T
    import arrow_ballista_amd as g
    if "--dist-join" in sys.argv:
        rows = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else T.LINEITEM_ROWS[10]
        r = dist_join(T, g, rows)
        if r is not None:
            print(json.dumps(r, indent=1))
        sys.exit(0)
    if "--cpu-proxy" in sys.argv:
        sf = 10 if "--sf10" in sys.argv else 1
        print(json.dumps(cpu_proxy_acero(T, sf), indent=1))
        sys.exit(0)
    tc = g.TaskContext(device=0)
    tc.ctx.set_jit("wait")      # steady-state timings: a large input waits for its specialised kernels
    if "--probe-micro" in sys.argv:      # the probe kernels alone (for rocprofv3 --pmc passes): --probe-micro 24 27 [--radix off|force|auto] [--slice N]
        i = sys.argv.index("--probe-micro")
        bits = [int(a) for a in sys.argv[i + 1:i + 4] if a.isdigit()] or [24]
        if "--radix" in sys.argv:
            tc.ctx.set_option("join_radix", sys.argv[sys.argv.index("--radix") + 1])
        if "--slice" in sys.argv:
            tc.ctx.set_option("join_radix_slice_log2", int(sys.argv[sys.argv.index("--slice") + 1]))
        if "--hash" in sys.argv:
            tc.ctx.set_option("join_dense", 0)
        print(json.dumps([join_probe_micro(tc, g, b, 28, 1.0, reps=2) for b in bits], indent=1))
        sys.exit(0)
    if "--ingest" in sys.argv:
        sf = 10 if "--sf10" in sys.argv else 1
        print(json.dumps(ingest_q1(tc, T, g, sf), indent=1))
        sys.exit(0)
    if "--sort" in sys.argv:
        i = sys.argv.index("--sort")
        bits = int(sys.argv[i + 1]) if len(sys.argv) > i + 1 and sys.argv[i + 1].isdigit() else 27
        print(json.dumps(sort_micro(tc, T, g, bits), indent=1))
        sys.exit(0)
    if "--merge" in sys.argv:
        i = sys.argv.index("--merge")
        bits = int(sys.argv[i + 1]) if len(sys.argv) > i + 1 and sys.argv[i + 1].isdigit() else 27
        print(json.dumps(merge_micro(tc, T, g, bits), indent=1))
        sys.exit(0)
    if "--scan-plan" in sys.argv:      # [--sf1]: SF10 unless told otherwise
        print(json.dumps(scan_plan(tc, T, g, 1 if "--sf1" in sys.argv else 10)))
        sys.exit(0)
    if "--scan" in sys.argv:
        sf = 10 if "--sf10" in sys.argv else 1
        print(json.dumps(scan_decode(tc, T, g, sf), indent=1))
        sys.exit(0)
    if "--temporal" in sys.argv:      # [--log2n 27]
        bits = int(sys.argv[sys.argv.index("--log2n") + 1]) if "--log2n" in sys.argv else 27
        print(json.dumps(temporal(tc, T, g, bits)))
        sys.exit(0)
    if "--like" in sys.argv:
        print(json.dumps(like_micro(tc, T, g), indent=1))
        sys.exit(0)
    if "--approx-distinct" in sys.argv:      # [--log2n 28] [--rows 10000000]
        bits = int(sys.argv[sys.argv.index("--log2n") + 1]) if "--log2n" in sys.argv else 28
        rows = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else 10_000_000
        print(json.dumps(approx_distinct(tc, T, g, bits, rows), indent=1))
        sys.exit(0)
    if "--distinct" in sys.argv:      # [--rows 10000000]
        rows = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else 10_000_000
        print(json.dumps(distinct(tc, T, g, rows)))
        sys.exit(0)
    if "--grouping-sets" in sys.argv:      # [--rows 10000000]
        rows = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else 10_000_000
        print(json.dumps(grouping_sets(tc, T, g, rows)))
        sys.exit(0)
    if "--window" in sys.argv:      # [--log2n 28] [--log2p 20]
        bits = int(sys.argv[sys.argv.index("--log2n") + 1]) if "--log2n" in sys.argv else 28
        pbits = int(sys.argv[sys.argv.index("--log2p") + 1]) if "--log2p" in sys.argv else 20
        print(json.dumps(window(tc, T, g, bits, pbits)))
        sys.exit(0)
    if "--h2o" in sys.argv:
        rows = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else 10_000_000
        print(json.dumps(h2o(tc, T, g, rows), indent=1))
        sys.exit(0)
    if "--shuffle-codec" in sys.argv:
        rows = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else 1 << 24
        print(json.dumps(shuffle_codec(tc, T, g, rows), indent=1))
        sys.exit(0)
    if "--sf100" in sys.argv:
        out = {"q1": q1_pipeline(tc, T, g, 100)}
        out.update(tpch_pipelines(tc, T, g, 100))
        print(json.dumps(out, indent=1))
    else:
        print(json.dumps(run(tc, T, g, full="--small" not in sys.argv), indent=1))
