"""The runs aggregate's count pass runs a key-and-predicate program (csrc/expr_compile.cpp ExprCompiler::prune, csrc/capi.cpp
launch_runs_count): the scan program cut down, by liveness over its operation list, to what the group keys and the fused predicate
read -- the operands of the accumulators and the per-aggregate FILTER clauses are not loaded -- while the write pass keeps the full
program.  Both passes must find the same heads; what would show a difference is a wrong group count, a wrong key, or a sum that went
to the neighbouring row.  strategy="runs" forced at row counts whose segments (two 64-row words, csrc/kernels_hash.hip
agg_runs_geometry) make runs cross word and segment borders; the interpreter kernels (jit "off") and the generated ones ("force").
Expected values: a restatement with Python integers, and the "hash" strategy over the same plan."""
import re

import numpy as np
import pyarrow as pa
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit
from test_gpu_agg_by_build_row import native_rows

SINK_AGG_RUNS_COUNT, SINK_AGG_RUNS_WRITE = 16, 17      # csrc/gpuq_kernels.h GPUQ_SINK_*
SIZES = [1, 63, 64, 65, 129, 1000, 70_001]


@pytest.fixture(params=["off", "force"])
def jit_tc(tc, request):
    if request.param == "force" and not tc.ctx.jit_stats()["available"]:
        pytest.skip("no run-time compiler")
    tc.ctx.set_jit(request.param)
    yield tc
    tc.ctx.set_jit("auto")


def agg_path(p):
    aggs = [o for o in p.profile_all() if o["op"] == "aggregate"]
    assert len(aggs) == 1
    return aggs[0]["agg_path"]


def srt(rows):
    return sorted(rows, key=lambda r: tuple((x is None, 0 if x is None else x) for x in r))


# ------------------------------------------------------------------------------------ one table, every size
def clustered(n):
    """rows 0..63 one run whose last row (the last of word 0) the predicate drops; two runs up to row 127; word 2 (rows 128..191) dropped as
    a whole; a run of 400 rows (more than three 128-row segments); then runs of 1..200 rows; the last run has a NULL key (the packed NULL
    lies above every value: in order as the last run).  `p` (the predicate's column) and `f` (the FILTER's) are neither keys nor arguments."""
    lens = [64, 30, 34, 64, 400] + [i % 200 + 1 for i in range(n)]
    keys = np.repeat(np.arange(len(lens), dtype=np.int64) * 3 + 5, lens)[:n]
    r = np.random.default_rng(n)
    p = np.ones(n, np.int32); p[63:64] = 0; p[128:192] = 0
    mask = np.zeros(n, bool)
    if n >= 65:
        mask[keys == keys[-1]] = True
    return {"k": keys.astype(np.int32), "kmask": mask, "p": p, "v": r.integers(-10**12, 10**12, n), "w": r.integers(0, 10**6, n), "f": r.integers(-5, 6, n).astype(np.int32)}


def arrow_of(c, m):
    return pa.table({"k": pa.array(c["k"][:m], pa.int32(), mask=c["kmask"][:m]), "p": pa.array(c["p"][:m]), "v": pa.array(c["v"][:m]),
                     "w": pa.array(c["w"][:m]), "f": pa.array(c["f"][:m])})


def expected(c, m):
    """(k, SUM(v), COUNT(*), SUM(w) FILTER (WHERE f > 0)) over the rows with p = 1, Python integers"""
    acc = {}
    for i in range(m):
        if c["p"][i] != 1:
            continue
        k = None if c["kmask"][i] else int(c["k"][i])
        a = acc.setdefault(k, [0, 0, None])
        a[0] += int(c["v"][i]); a[1] += 1
        if c["f"][i] > 0:
            a[2] = (a[2] or 0) + int(c["w"][i])
    return srt([(k, a[0], a[1], a[2]) for k, a in acc.items()])


def plan_of(src, strategy):
    s = src.schema()
    aggs = [{"fn": "SUM", "expr": col("v", s), "name": "sv"}, {"fn": "COUNT", "expr": lit(1), "name": "c"},
            {"fn": "SUM", "expr": col("w", s), "name": "sw", "filter": binary(col("f", s), Op.Gt, lit(0, "Int32"))}]
    return g.AggregateExec("Single", [(col("k", s), "k")], aggs, g.FilterExec(binary(col("p", s), Op.Eq, lit(1, "Int32")), src), strategy=strategy)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_heads_of_the_count_pass_are_the_heads_of_the_write_pass(jit_tc, n):
    tc = jit_tc
    c = clustered(n)
    src = g.MemoryExec([arrow_of(c, n)])
    exp = expected(c, n)
    assert srt(native_rows(g.NativePlan(plan_of(src, "hash"), tc))) == exp
    p = g.NativePlan(plan_of(src, "runs"), tc)
    for _ in range(2):                                   # (the second run replays the first, deferred)
        assert srt(native_rows(p)) == exp
        assert len(exp) > 0 and agg_path(p) == "runs", agg_path(p)
    if n > 1:                                            # fewer rows on the same operator
        m = n * 2 // 3
        p.set_input(0, g.DeviceTable.from_arrow(arrow_of(c, m), tc.device))
        assert srt(native_rows(p)) == expected(c, m)


@pytest.mark.gpu
def test_input_that_is_not_clustered_falls_back_with_the_right_answer(jit_tc):
    tc = jit_tc
    n = 5000
    c = clustered(n)
    perm = np.random.default_rng(1).permutation(n)
    c = {name: a[perm] for name, a in c.items()}
    src = g.MemoryExec([arrow_of(c, n)])
    p = g.NativePlan(plan_of(src, "runs"), tc)
    for _ in range(2):
        assert srt(native_rows(p)) == expected(c, n)
        assert agg_path(p) == "table" and p.exec_stats()["retries"] == 0


# ------------------------------------------------------------------------------------ the q3 shape
@pytest.mark.gpu
def test_decimal_expression_of_two_columns_through_the_pair_list(jit_tc):
    """SUM(pe * (1 - pd)) GROUP BY the build row above a unique-key join: the aggregate reads pe and pd (Decimal128) through the pair
    list, the count pass reads the pair list's build rows alone"""
    tc = jit_tc
    r = np.random.default_rng(3)
    nb, npr = 3000, 30_000
    bk = np.arange(nb, dtype=np.int64) * 3 + 7
    bd = r.integers(9000, 9400, nb).astype(np.int32)
    pk = np.sort(np.where(r.random(npr) < 0.7, r.integers(0, nb, npr) * 3 + 7, -5 - r.integers(0, 1000, npr))).astype(np.int64)
    pe = r.integers(90_000, 10_494_951, npr)
    pd = r.integers(0, 11, npr)
    dec = pa.decimal128(15, 2)
    import decimal
    bt = pa.table({"bk": pa.array(bk), "bd": pa.array(bd).cast(pa.date32())})
    pt = pa.table({"pk": pa.array(pk), "pe": pa.array([decimal.Decimal(int(x)).scaleb(-2) for x in pe], dec), "pd": pa.array([decimal.Decimal(int(x)).scaleb(-2) for x in pd], dec)})
    L, R = g.MemoryExec([bt]), g.MemoryExec([pt])
    ls, rs = L.schema(), R.schema()
    j = g.HashJoinExec(L, R, [(col("bk", ls), col("pk", rs))], None, "Inner", "CollectLeft", False)
    js = j.schema()
    rev = binary(col("pe", js), Op.Multiply, binary(lit(1, ("Decimal128", 20, 0)), Op.Minus, col("pd", js)))
    date_of = dict(zip(bk.tolist(), bd.tolist()))
    acc = {}
    for k, e, d in zip(pk.tolist(), pe.tolist(), pd.tolist()):
        if k in date_of:
            a = acc.setdefault((k, date_of[k]), [0, 0])
            a[0] += e * (100 - d); a[1] += 1
    exp = srt([(k, d, a[0], a[1]) for (k, d), a in acc.items()])
    assert len(exp) > 1000
    for strategy in ("hash", "runs"):
        plan = g.AggregateExec("Single", [(col("pk", js), "pk"), (col("bd", js), "bd")], [{"fn": "SUM", "expr": rev, "name": "rev"}, {"fn": "COUNT", "expr": lit(1), "name": "c"}], j, strategy=strategy)
        p = g.NativePlan(plan, tc)
        for _ in range(3):
            assert srt(native_rows(p)) == exp
            assert p.exec_stats()["retries"] == 0
        if strategy == "runs":
            assert agg_path(p) == "runs"


# ------------------------------------------------------------------------------------ which program the count pass is given (host only)
def eval_source(descriptor, kernel):
    """the generated row function (struct JitPre .. gpuq_jit_eval) of the source handed to the run-time compiler for `kernel`"""
    text = g.compile_jit_source(descriptor, kernel)
    m = re.search(r"struct JitPre \{.*?bool gpuq_jit_eval\(", text, re.S)
    assert m, "no generated row function in the source"
    return m.group(0)


def descriptor(groups, aggs_of, with_pred):
    cols = [g.DeviceColumn(name, t, None, 0, nullable=False) for name, t in [("k", "Int32"), ("d", "Int32"), ("v", "Int64"), ("p", "Int32")]]
    src = g.MemoryExec([g.DeviceTable(cols, 0)])
    s = src.schema()
    inp = g.FilterExec(binary(col("p", s), Op.Eq, lit(1, "Int32")), src) if with_pred else src
    node = g.AggregateExec("Single", [(col(c, s), c) for c in groups], aggs_of(s), inp, strategy="runs")
    _, pred, m = g.plan._fuse(node.input)
    return node._descriptor(src.schema(), pred, m)


def test_the_count_pass_gets_a_program_of_its_own_only_when_pruning_removes_something():
    # an argument that is neither key nor predicate: the count pass's row function does not load it, the write pass's does
    d = descriptor(["k"], lambda s: [{"fn": "SUM", "expr": col("v", s), "name": "sv"}], True)
    count, write = eval_source(d, SINK_AGG_RUNS_COUNT), eval_source(d, SINK_AGG_RUNS_WRITE)
    assert count != write
    loads = lambda text: set(re.findall(r"P\.cols\[(\d+)\]", text))
    assert loads(count) < loads(write) and len(loads(write)) == 3 and len(loads(count)) == 2      # (k, p) of (k, v, p)
    # every column a key or the predicate's, COUNT(*) has no argument: nothing to remove, one program
    d = descriptor(["k", "d"], lambda s: [{"fn": "COUNT", "expr": lit(1), "name": "c"}], True)
    assert eval_source(d, SINK_AGG_RUNS_COUNT) == eval_source(d, SINK_AGG_RUNS_WRITE)
    # a FILTER clause is dropped with its aggregate's operand
    d = descriptor(["k"], lambda s: [{"fn": "COUNT", "expr": lit(1), "name": "c", "filter": binary(col("d", s), Op.Gt, lit(0, "Int32"))}], False)
    count, write = eval_source(d, SINK_AGG_RUNS_COUNT), eval_source(d, SINK_AGG_RUNS_WRITE)
    assert loads(count) < loads(write) and len(loads(count)) == 1
