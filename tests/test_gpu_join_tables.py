"""HashJoinExec (datafusion.proto:1346-1360) over the two join-table layouts of the device path -- the direct-addressed
array (one narrow integer key of bounded range) and the open-addressing hash table -- and the segmented, probe-ordered pair
emission of the unique-key probe, against the oracle.  The operator suite (test_gpu_operators.py) runs with the default
policy; here every join type runs under both layouts, interpreter and hiprtc-specialised kernels."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit
from oracle import oracle_np as O
import test_gpu_operators as M

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["dense", "hash", "dense+partitioned-probe"])
def layout(tc, request):
    """Join-table layout and probe strategy: direct-addressed array, hash table, or the array probed through the partitioned
    (radix) probe -- forced, with 2^10-entry slices so that small test inputs still spread over many partitions."""
    tc.ctx.set_option("join_dense", 0 if request.param == "hash" else 1)
    tc.ctx.set_option("join_radix", "force" if "partitioned" in request.param else "off")
    tc.ctx.set_option("join_radix_slice_log2", 10)
    yield request.param
    tc.ctx.set_option("join_dense", 1)
    tc.ctx.set_option("join_radix", "off")
    tc.ctx.set_option("join_radix_slice_log2", 18)


@pytest.fixture(params=["off", "force"])
def jitmode(tc, request):
    if request.param == "force" and not tc.ctx.jit_stats()["available"]:
        pytest.skip("hiprtc not available")
    tc.ctx.set_jit(request.param)
    yield request.param
    tc.ctx.set_jit("auto")


@pytest.mark.parametrize("jt", M.JOIN_TYPES)
def test_join_types_under_both_layouts(tc, layout, jitmode, jt):
    M.test_hash_join_types(tc, jt, 0.2)


def _join_rows(tc, build, probe, jt, on=("bk", "pk"), probe_pred=None):
    L, R0 = g.MemoryExec([build]), g.MemoryExec([probe])
    R = g.FilterExec(probe_pred(R0.schema()), R0) if probe_pred else R0
    ls, rs = L.schema(), R.schema()
    plan = g.HashJoinExec(L, R, [(col(on[0], ls), col(on[1], rs))], None, jt, "CollectLeft", False)
    return M.norm(M.dev_rows(tc, plan.execute(0, tc)))


def _oracle_rows(build, probe, jt, on=("bk", "pk")):
    ol, orr = O.Table.from_arrow(build), O.Table.from_arrow(probe)
    pairs = O.hash_join(ol, orr, [({"column": {"name": on[0]}}, {"column": {"name": on[1]}})], jt)
    lrows, rrows = [tuple(x) for x in ol.rows()], [tuple(x) for x in orr.rows()]
    nl, nr = len(build.schema.names), len(probe.schema.names)
    if jt in ("LeftSemi", "LeftAnti"):
        return M.norm([lrows[i] for i, _ in pairs])
    if jt in ("RightSemi", "RightAnti"):
        return M.norm([rrows[j] for _, j in pairs])
    return M.norm([(lrows[i] if i is not None else (None,) * nl) + (rrows[j] if j is not None else (None,) * nr) for i, j in pairs])


KEYSETS = {
    # name: (build keys, probe keys, arrow type)
    "negative_and_positive": (lambda r: r.permutation(np.arange(-700, 900))[:1100], lambda r: r.integers(-1000, 1200, 6000), pa.int64()),
    "int64_extremes": (lambda r: np.array([np.iinfo(np.int64).min, -1, 0, 1, np.iinfo(np.int64).max, 42], dtype=np.int64),
                       lambda r: np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0, 7, 42, -1, -2] * 40, dtype=np.int64), pa.int64()),      # range too wide: hash table
    "sparse_beyond_ratio": (lambda r: (r.permutation(4000)[:900].astype(np.int64) * 1_000_003), lambda r: (r.integers(0, 4200, 5000).astype(np.int64) * 1_000_003), pa.int64()),
    "single_key": (lambda r: np.array([123456789], dtype=np.int64), lambda r: np.array([123456789, 5, 123456789, 123456790, 123456788], dtype=np.int64), pa.int64()),
    "int32_keys": (lambda r: r.permutation(np.arange(-300, 300)).astype(np.int32)[:400], lambda r: r.integers(-400, 400, 3000).astype(np.int32), pa.int32()),
    "duplicate_build_keys": (lambda r: r.integers(100, 400, 1500), lambda r: r.integers(0, 500, 4000), pa.int64()),                # chained probe over either layout
    "sparse_domain_presence_bitmap": (lambda r: r.permutation(60_000)[:1500].astype(np.int64) - 30_000, lambda r: r.integers(-31_000, 31_000, 9000), pa.int64()),   # 1 value in 40 is a key
    "sparse_domain_with_duplicates": (lambda r: r.integers(0, 60_000, 3000), lambda r: r.integers(-100, 60_100, 9000), pa.int64()),  # bitmap build finds duplicates -> rebuilt with chains
}


@pytest.mark.parametrize("jt", ["Inner", "Left", "Right", "Full", "LeftSemi", "LeftAnti", "RightSemi", "RightAnti"])
@pytest.mark.parametrize("keyset", sorted(KEYSETS))
def test_key_domains(tc, layout, keyset, jt):
    """Key domains that steer the layout choice or sit at its edges: negative keys (index = key - min), the int64 extremes
    (range does not fit: hash table even when direct addressing is on), a sparse domain beyond the range / count ratio, a single
    key, Int32 keys, duplicate build keys (chains), probe keys below min and above max, NULL keys on both sides."""
    r = np.random.default_rng(hash(keyset) % 1000)
    mk_b, mk_p, ty = KEYSETS[keyset]
    bk, pk = np.asarray(mk_b(r)), np.asarray(mk_p(r))
    bmask = r.random(len(bk)) < 0.05 if len(bk) > 10 else None
    pmask = r.random(len(pk)) < 0.1
    build = pa.table({"bk": pa.array(bk, type=ty, mask=bmask), "bv": pa.array(np.arange(len(bk), dtype=np.int64))})
    probe = pa.table({"pk": pa.array(pk, type=ty, mask=pmask), "pid": pa.array(np.arange(len(pk), dtype=np.int64))})
    assert _join_rows(tc, build, probe, jt) == _oracle_rows(build, probe, jt)


@pytest.mark.parametrize("jt", ["Inner", "Right", "RightSemi", "RightAnti"])
def test_segments_keep_probe_order_and_cover_ragged_tails(tc, layout, jitmode, jt):
    """The unique-key probe emits its pairs in probe order through per-wave segments.  2^20 + 77 probe rows (segments of
    several waves, a ragged last word and a last segment shorter than the others), match density that varies along the input
    (empty segments, full segments), a fused probe-side filter; the C entry points directly: pair list == the oracle's
    probe-ordered list, element by element."""
    import torch
    r = np.random.default_rng(9)
    nb, n = 50_000, (1 << 20) + 77
    bkeys = r.permutation(np.arange(0, 2 * nb, 2))[:nb].astype(np.int64) + 1000          # unique even keys from 1000
    pk = r.integers(900, 2 * nb + 1200, n).astype(np.int64)
    pk[: n // 4] = 7                                                                       # a long stretch without any match
    pk[n // 4: n // 2] = np.repeat(bkeys, 8)[: n // 2 - n // 4]                            # a stretch where every row matches, clustered
    flt = r.integers(0, 10, n).astype(np.int32)
    dev = tc.device
    bt = g.DeviceTable([g.DeviceColumn("k", "Int64", torch.from_numpy(bkeys).to(dev).view(torch.uint8), nb, nullable=False)], nb)
    pt = g.DeviceTable([g.DeviceColumn("k", "Int64", torch.from_numpy(pk).to(dev).view(torch.uint8), n, nullable=False),
                        g.DeviceColumn("f", "Int32", torch.from_numpy(flt).to(dev).view(torch.uint8), n, nullable=False)], n)
    bs, ps = bt.schema(), pt.schema()
    bop = tc.op({"op": "join_build", "input": {"fields": bs}, "on": [col("k", bs)]})
    pop = tc.op({"op": "join_probe", "input": {"fields": ps}, "on": [col("k", ps)], "join_type": jt, "predicate": binary(col("f", ps), Op.Lt, lit(8, "Int32"))})
    binp, _k1 = bt.input_struct()
    pinp, _k2 = pt.input_struct()
    h = C.c_void_p()
    tc.ctx.check(tc.ctx.L.gpuq_join_build_run(bop.h, tc.stream_ptr(), C.byref(binp), 0, nb, C.byref(h)))
    ob = torch.full((n,), -2, dtype=torch.int32, device=dev)
    opb = torch.full((n,), -2, dtype=torch.int32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    tc.ctx.check(tc.ctx.L.gpuq_join_probe_run(pop.h, tc.stream_ptr(), h, C.byref(pinp), 0, ob.data_ptr(), opb.data_ptr(), n, cnt.data_ptr()))
    tc.sync()
    pop.check(tc.stream_ptr())
    k = int(cnt[0].item())
    tc.ctx.L.gpuq_join_table_free(h)
    # oracle: probe-ordered pairs
    where = {int(v): i for i, v in enumerate(bkeys)}
    passing = np.nonzero(flt < 8)[0]
    hit = np.array([where.get(int(v), -1) for v in pk[passing]])
    if jt == "Inner":
        sel = hit >= 0; exp_b, exp_p = hit[sel], passing[sel]
    elif jt == "Right":
        exp_b, exp_p = hit, passing
    elif jt == "RightSemi":
        sel = hit >= 0; exp_b, exp_p = None, passing[sel]
    else:
        sel = hit < 0; exp_b, exp_p = None, passing[sel]
    assert k == len(exp_p)
    got_p = opb[:k].cpu().numpy().astype(np.int64)
    got_b = ob[:k].cpu().numpy().astype(np.int64) if exp_b is not None else None
    if "partitioned" in layout and jt in ("Inner", "RightSemi"):
        # partition order: the same pairs, ordered by table slice; inside a slice in no particular order
        order = np.argsort(got_p, kind="stable")
        got_p = got_p[order]
        got_b = got_b[order] if got_b is not None else None
    assert np.array_equal(got_p, exp_p)
    if exp_b is not None:
        assert np.array_equal(got_b, exp_b)          # -1 == NULL_ROW (0xFFFFFFFF) for unmatched outer rows
    assert int(opb[k:].max().item() if k < n else -2) == -2                           # nothing written past the count


# hits per 64-row probe word of test_hit_queue_boundaries.  The specialised probe takes 4 words per step and resolves queued hits 64
# at a time, segments are 16 words: step 0 queues 256 hits, the first segment 448 in all (the 320-entry ring wraps); what waits after
# a step's drain is 0, 0, 63, 0 in the first segment, 0 (a step of misses only), 1, 0, 63 in the second, 5 in the ragged third
HITS_PER_WORD = [64, 64, 64, 64, 63, 1, 0, 64, 33, 0, 30, 0, 1, 0, 0, 0,
                 0, 0, 0, 0, 64, 1, 0, 0, 63, 64, 64, 64, 64, 64, 64, 63,
                 64, 5]


def hit_queue_case():
    """(build keys, probe keys, probe NULL mask, expected build row per probe row or -1): 1,024 unique build keys 8 i in shuffled row
    order, 2,048 + 77 probe rows with HITS_PER_WORD[w] matching rows in word w at shuffled lanes; the other rows miss in turn with
    an absent key inside the range (8 i + 3), a key below the minimum, a key above the maximum, and NULL (over a key that would match)."""
    r = np.random.default_rng(31)
    nb, n = 1024, 2048 + 77
    bkeys = 8 * r.permutation(nb).astype(np.int64)
    where = np.empty(nb, dtype=np.int64); where[bkeys // 8] = np.arange(nb)
    pk = np.empty(n, dtype=np.int64); null = np.zeros(n, dtype=bool); exp = np.full(n, -1, dtype=np.int64)
    assert len(HITS_PER_WORD) == (n + 63) // 64
    miss = 0
    for w, c in enumerate(HITS_PER_WORD):
        rows = np.arange(64 * w, min(64 * w + 64, n))
        hits = set(r.permutation(rows)[:c].tolist())
        assert len(hits) == c
        for p in rows:
            i = int(r.integers(0, nb))
            if p in hits:
                pk[p], exp[p] = 8 * i, where[i]
                continue
            kind, miss = miss % 4, miss + 1
            pk[p] = (8 * i + 3, -1 - 8 * i, 8 * nb + i, 8 * i)[kind]
            null[p] = kind == 3
    return bkeys, pk, null, exp


@pytest.mark.parametrize("jt", ["Inner", "RightSemi", "Right", "RightAnti"])
def test_hit_queue_boundaries(tc, jitmode, jt):
    """The specialised unique probe over a sparse key domain (presence bitmap, chosen from the data: the key range is 8 x the key
    count) queues its hits per wave and resolves them 64 at a time: hit counts per word that fill, wrap and exactly empty the
    queue, leave 0, 1 and 63 waiting across steps, a step without a hit, a ragged last segment (HITS_PER_WORD).  Inner and
    RightSemi take the queue, Right and RightAnti the same front without it; with run-time compilation off the interpreter probe
    runs over the same rows.  Pair list == the host's probe-ordered list, element by element."""
    import torch
    bkeys, pk, null, hit = hit_queue_case()
    nb, n = len(bkeys), len(pk)
    dev = tc.device
    bt = g.DeviceTable.from_arrow(pa.table({"k": pa.array(bkeys)}), dev)
    pt = g.DeviceTable.from_arrow(pa.table({"k": pa.array(pk, mask=null)}), dev)
    bs, ps = bt.schema(), pt.schema()
    bop = tc.op({"op": "join_build", "input": {"fields": bs}, "on": [col("k", bs)]})
    pop = tc.op({"op": "join_probe", "input": {"fields": ps}, "on": [col("k", ps)], "join_type": jt})
    binp, _k1 = bt.input_struct()
    pinp, _k2 = pt.input_struct()
    h = C.c_void_p()
    tc.ctx.check(tc.ctx.L.gpuq_join_build_run(bop.h, tc.stream_ptr(), C.byref(binp), 0, nb, C.byref(h)))
    ob = torch.full((n,), -2, dtype=torch.int32, device=dev)
    opb = torch.full((n,), -2, dtype=torch.int32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    tc.ctx.check(tc.ctx.L.gpuq_join_probe_run(pop.h, tc.stream_ptr(), h, C.byref(pinp), 0, ob.data_ptr(), opb.data_ptr(), n, cnt.data_ptr()))
    tc.sync()
    pop.check(tc.stream_ptr())
    k = int(cnt[0].item())
    tc.ctx.L.gpuq_join_table_free(h)
    rows = np.arange(n)
    if jt == "Inner":
        exp_b, exp_p = hit[hit >= 0], rows[hit >= 0]
    elif jt == "Right":
        exp_b, exp_p = hit, rows
    elif jt == "RightSemi":
        exp_b, exp_p = None, rows[hit >= 0]
    else:
        exp_b, exp_p = None, rows[hit < 0]
    assert k == len(exp_p)
    assert np.array_equal(opb[:k].cpu().numpy().astype(np.int64), exp_p)
    if exp_b is not None:
        assert np.array_equal(ob[:k].cpu().numpy().astype(np.int64), exp_b)          # -1 == NULL_ROW (0xFFFFFFFF) for unmatched outer rows
    assert int(opb[k:].max().item() if k < n else -2) == -2                           # nothing written past the count


def test_capacity_overflow_is_reported(tc, layout):
    """out_cap smaller than the pair count: the count is still exact, the check reports GPUQ_ERR_CAPACITY, nothing is written past out_cap."""
    import torch
    nb, n = 1000, 100_000
    dev = tc.device
    bk = torch.arange(nb, dtype=torch.int64, device=dev)
    pk = torch.arange(n, dtype=torch.int64, device=dev) % nb
    bt = g.DeviceTable([g.DeviceColumn("k", "Int64", bk.view(torch.uint8), nb, nullable=False)], nb)
    pt = g.DeviceTable([g.DeviceColumn("k", "Int64", pk.view(torch.uint8), n, nullable=False)], n)
    bs, ps = bt.schema(), pt.schema()
    bop = tc.op({"op": "join_build", "input": {"fields": bs}, "on": [col("k", bs)]})
    pop = tc.op({"op": "join_probe", "input": {"fields": ps}, "on": [col("k", ps)], "join_type": "Inner"})
    binp, _k1 = bt.input_struct()
    pinp, _k2 = pt.input_struct()
    h = C.c_void_p()
    tc.ctx.check(tc.ctx.L.gpuq_join_build_run(bop.h, tc.stream_ptr(), C.byref(binp), 0, nb, C.byref(h)))
    cap = 5000
    ob = torch.full((cap + 64,), -2, dtype=torch.int32, device=dev)
    opb = torch.full((cap + 64,), -2, dtype=torch.int32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    tc.ctx.check(tc.ctx.L.gpuq_join_probe_run(pop.h, tc.stream_ptr(), h, C.byref(pinp), 0, ob.data_ptr(), opb.data_ptr(), cap, cnt.data_ptr()))
    tc.sync()
    assert int(cnt[0].item()) == n
    with pytest.raises(g.GpuqError) as e:
        pop.check(tc.stream_ptr())
    assert e.value.status == 4
    assert int(ob[cap:].max().item()) == -2 and int(opb[cap:].max().item()) == -2
    got = opb[:cap].cpu().numpy()
    if "partitioned" in layout:       # partition order: any `cap` distinct probe rows, each paired with its own key's build row
        assert len(np.unique(got)) == cap and np.array_equal(ob[:cap].cpu().numpy(), got % nb)
    else:
        assert np.array_equal(got, np.arange(cap, dtype=np.int32))
    tc.ctx.L.gpuq_join_table_free(h)


@pytest.mark.parametrize("case", ["holds", "outlier-below", "outlier-far-above", "filtered-build"])
def test_guessed_key_range_holds_or_falls_back(tc, case):
    """From 2^21 build rows on gpuq_join_build_run sizes the direct-addressed array from a row sample (every 8th 64-row word here)
    and the build kernel checks every key against it.  The pairs must be the same whether the guess holds, an outlier in a word the
    sample skips forces the measured range (still an array), or one so far out that the table becomes a hash table."""
    nb, n = (1 << 21) + 5, 1 << 20
    BK = "bk_" + case.replace("-", "_")          # a column name of its own: operators are cached by input signature, and one that has seen a guess fail stops guessing
    r = np.random.default_rng(21)
    bk = (r.permutation(nb) + 1000).astype(np.int64)
    if case == "outlier-below":
        bk[100] = -7_000_000                      # row 100 = word 1: not sampled
    if case == "outlier-far-above":
        bk[200] = 1 << 40
    pk = r.integers(0, nb + 5000, n).astype(np.int64)
    pk[:8] = bk[[100, 200, 0, nb - 1, 64, 65, 300, 5]]
    build = pa.table({BK: bk, "brid": np.arange(nb, dtype=np.int64)})
    probe = pa.table({"pk": pk, "prid": np.arange(n, dtype=np.int64)})
    build = build.cast(pa.schema([pa.field(f.name, f.type, nullable=False) for f in build.schema]))
    probe = probe.cast(pa.schema([pa.field(f.name, f.type, nullable=False) for f in probe.schema]))
    L0, R = g.MemoryExec([build]), g.MemoryExec([probe])
    keep = np.ones(nb, bool)
    L = L0
    if case == "filtered-build":
        s0 = L0.schema()
        L = g.FilterExec(binary(binary(col(BK, s0), Op.Modulo, lit(3, "Int64")), Op.Eq, lit(0, "Int64")), L0)
        keep = bk % 3 == 0
    ls, rs = L.schema(), R.schema()
    plan = g.HashJoinExec(L, R, [(col(BK, ls), col("pk", rs))], None, "Inner", "CollectLeft", False)
    for _ in range(2):                            # second run: the operator remembers a failed guess
        out = g.plan.materialize(tc, plan.execute(0, tc)).to_arrow(tc.ctx)
        order = np.argsort(bk[keep], kind="stable")
        keys_sorted, rows_sorted = bk[keep][order], np.arange(nb)[keep][order]
        at = np.searchsorted(keys_sorted, pk)
        hit = (at < len(keys_sorted)) & (keys_sorted[np.minimum(at, len(keys_sorted) - 1)] == pk)
        assert np.array_equal(np.asarray(out.column("prid")), np.nonzero(hit)[0])
        assert np.array_equal(np.asarray(out.column("brid")), rows_sorted[at[hit]])
        assert np.array_equal(np.asarray(out.column(BK)), pk[hit])
