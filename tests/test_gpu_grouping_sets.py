"""Grouping sets on the device: the entry point gpuq_grouping_expand alone (every width, Boolean, PACKED15, byte for byte), the Merge
mode of the aggregate operator (states in, states out), then AggregateExec with ROLLUP / CUBE / explicit sets through the native executor
-- modes Single and Partial -- against the row-by-row restatement of tests/grouping_sets_exact.py: integers, decimals and bit functions
exactly, the float functions within the bounds of tests/float_agg_exact.py, and once against pyarrow's group_by."""
import ctypes as C
import decimal
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd import binding as B
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit

import float_agg_exact as X
import grouping_sets_exact as GS

pytestmark = pytest.mark.gpu

F, T = False, True
CTX = decimal.Context(prec=60)
#        type id, bytes a row (0: a bitmap), representation
TYPES = {"Int8": (B.T_INT8, 1, B.REPR_ARROW), "Int16": (B.T_INT16, 2, B.REPR_ARROW), "Int32": (B.T_INT32, 4, B.REPR_ARROW), "Float64": (B.T_FLOAT64, 8, B.REPR_ARROW),
         "Decimal": (B.T_DECIMAL128, 16, B.REPR_ARROW), "Utf8": (B.T_UTF8, 16, B.REPR_PACKED15), "Boolean": (B.T_BOOL, 0, B.REPR_ARROW)}
N_SETS = [1, 2, 3, 5, 7, 64]
N_ROWS = [0, 1, 21, 22, 64, 65, 257, 5000]      # n_sets * n on both sides of 64, words that straddle input rows, more than one block


# ------------------------------------------------------------------------------------ the entry point on its own
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def pack_bits(bits, words):
    return np.packbits(np.concatenate([bits, np.zeros(words * 64 - len(bits), dtype=bool)]), bitorder="little")


def run_expand(tc, tname, n, n_sets, mask, valid, r):
    """One call over random bytes; the output compared byte for byte with the rule, and checked untouched beyond what the rule covers."""
    import torch
    tid, width, rep = TYPES[tname]
    total = n * n_sets
    words = (total + 63) // 64
    in_words = (n + 63) // 64
    raw = r.integers(0, 256, (max(n, 1) * width if width else (in_words + 1) * 8) + 8, dtype=np.uint8)
    data = dev(raw)
    vbuf = dev(pack_bits(valid, in_words + 1)) if valid is not None else None
    c = B.gpuq_column()
    c.type, c.repr, c.data, c.validity, c.length = tid, rep, data.data_ptr(), (vbuf.data_ptr() if vbuf is not None else None), n
    if tname == "Decimal":
        c.precision, c.scale = 38, 4
    out_bytes = total * width if width else words * 8
    out = torch.full((out_bytes + 16,), 0x77, dtype=torch.uint8, device="cuda")
    want_validity = valid is not None or mask != 0
    vout = torch.full((words * 8 + 16,), 0x77, dtype=torch.uint8, device="cuda")
    tc.ctx.check(tc.ctx.L.gpuq_grouping_expand(tc.ctx.h, tc.stream_ptr(), C.byref(c), n, n_sets, mask, out.data_ptr(), vout.data_ptr() if want_validity else None))
    tc.sync()
    out, vout = out.cpu().numpy(), vout.cpu().numpy()
    # the rule: output row o = i * n_sets + s is input row i, NULL when bit s of the mask is set or row i is NULL; a NULL row's data is zero
    o = np.arange(total)
    i, s = o // n_sets, (o % n_sets).astype(np.uint64)
    has = ((np.uint64(mask) >> s) & np.uint64(1)) == 0
    if valid is not None:
        has &= valid[i]
    if width:
        exp = np.where(has[:, None], raw[:max(n, 1) * width].reshape(-1, width)[i], 0).astype(np.uint8).reshape(-1)
    else:
        bits = np.unpackbits(raw, bitorder="little").astype(bool)
        exp = pack_bits(has & bits[i], words)      # whole words, the last one zero-padded
    assert out[:out_bytes].tobytes() == exp.tobytes(), (tname, n, n_sets, mask)
    assert set(out[out_bytes:].tolist()) == {0x77}
    if want_validity:
        assert vout[:words * 8].tobytes() == pack_bits(has, words).tobytes(), (tname, n, n_sets, mask)      # including the zero padding of the last word
        assert set(vout[words * 8:].tolist()) == {0x77}
    else:
        assert set(vout.tolist()) == {0x77}      # a NULL pointer: not written


@pytest.mark.parametrize("tname", list(TYPES))
def test_entry_point_every_width_over_the_grid(tc, tname):
    r = np.random.default_rng(len(tname))
    for n_sets in N_SETS:
        full = (1 << n_sets) - 1
        for n in N_ROWS:
            mask = [int(r.integers(0, 1 << min(n_sets, 62))) | ((1 << 63) if n_sets == 64 else 0), 1 << int(r.integers(0, n_sets)), full][(n + n_sets) % 3]
            run_expand(tc, tname, n, n_sets, mask, r.random(n) < 0.7, r)
            run_expand(tc, tname, n, n_sets, 0, None, r)      # a state column without validity: null_sets = 0, no out_validity
    run_expand(tc, tname, 65, 3, 0b101, None, r)      # masked sets over a column without validity
    run_expand(tc, tname, 65, 3, 0, r.random(65) < 0.5, r)


def test_entry_point_refusals(tc):
    L, ctx, stream = B.lib(), tc.ctx.h, tc.stream_ptr()
    import torch
    buf = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    c = B.gpuq_column()
    c.type, c.repr, c.data, c.length = B.T_INT32, B.REPR_ARROW, buf.data_ptr(), 4
    for n_sets in (0, 65, -1):
        with pytest.raises(g.GpuqError, match=r"gpuq_grouping_expand \(AggregateExec grouping sets\): n_sets is %d" % n_sets) as e:
            tc.ctx.check(L.gpuq_grouping_expand(ctx, stream, C.byref(c), 4, n_sets, 0, buf.data_ptr(), None))
        assert e.value.status == 3 and e.value.refusal == B.REFUSAL_NONE
    u = B.gpuq_column()
    u.type, u.repr, u.data, u.length = B.T_UTF8, B.REPR_ARROW, buf.data_ptr(), 4
    with pytest.raises(g.GpuqError, match=r"gpuq_grouping_expand \(AggregateExec grouping sets\): a Utf8 column must be in the fixed-width PACKED15 form") as e:
        tc.ctx.check(L.gpuq_grouping_expand(ctx, stream, C.byref(u), 4, 2, 0, buf.data_ptr(), None))
    assert e.value.status == 3 and e.value.refusal == B.REFUSAL_NONE
    # 2^31 output rows or more: refused before any pointer is looked at
    for n, n_sets in ((2 ** 31, 1), (2 ** 25, 64), (2 ** 31 // 3 + 1, 3)):
        with pytest.raises(g.GpuqError, match=r"gpuq_grouping_expand \(AggregateExec grouping sets\): .*>= 2\^31") as e:
            tc.ctx.check(L.gpuq_grouping_expand(ctx, stream, None, n, n_sets, 0, None, None))
        assert e.value.status == 3 and e.value.refusal == B.REFUSAL_NONE
    # out_validity may be left out only when nothing can be NULL
    with pytest.raises(g.GpuqError, match="out_validity may be NULL only") as e:
        tc.ctx.check(L.gpuq_grouping_expand(ctx, stream, C.byref(c), 4, 2, 1, buf.data_ptr(), None))
    assert e.value.status == 1
    run_expand(tc, "Int32", 3, 2, 1, None, np.random.default_rng(0))      # the context goes on


# ------------------------------------------------------------------------------------ tables and the restatement
WORDS = ["", "ab", "ab ", "fifteen bytes.."]


def mixed(seed, n=5000, null_c=0.1):
    r = np.random.default_rng(seed)
    big = 2 ** 62
    return {"n": n, "a": r.integers(0, 3, n).astype(np.int32), "s": np.array(WORDS, dtype=object)[r.integers(0, 4, n)], "c": r.integers(10, 15, n), "c_ok": r.random(n) >= null_c,
            "v": np.where(r.random(n) < 0.5, big - r.integers(0, 1000, n), -big + r.integers(0, 1000, n)) + r.integers(0, 2, n) * (big // 2), "v_ok": r.random(n) >= 0.15,
            "d": r.integers(-10 ** 11, 10 ** 11, n), "d_ok": r.random(n) >= 0.15, "x": r.integers(-2 ** 31, 2 ** 31, n).astype(np.int32),
            "b": r.random(n) < 0.2, "b_ok": r.random(n) >= 0.3, "f": r.integers(0, 10, n).astype(np.int32)}


def arrow_of(m, rows=None):
    t = pa.table({"a": pa.array(m["a"]), "s": pa.array(m["s"], pa.utf8()), "c": pa.array(m["c"], pa.int64(), mask=~m["c_ok"]), "v": pa.array(m["v"], pa.int64(), mask=~m["v_ok"]),
                  "d": pa.array([decimal.Decimal(int(x)).scaleb(-2, CTX) for x in m["d"]], pa.decimal128(12, 2), mask=~m["d_ok"]), "x": pa.array(m["x"]),
                  "b": pa.array(m["b"], mask=~m["b_ok"]), "f": pa.array(m["f"])})
    t = t.cast(pa.schema([pa.field(f.name, f.type, nullable=f.name in ("c", "v", "d", "b")) for f in t.schema]))
    return t if rows is None else t.take(rows)


def pylist(m, name):
    ok = m.get(name + "_ok", np.ones(m["n"], dtype=bool))
    return [(v.item() if hasattr(v, "item") else v) if o else None for v, o in zip(m[name], ok)]


def key_tuples(m, names=("a", "s", "c")):
    return list(zip(*[pylist(m, k) for k in names]))


# two nodes' worth of aggregates (an operator holds twelve accumulators): name -> (descriptor of a schema, fold of (m, rows))
def aggs_a(s):
    return [{"fn": "COUNT", "expr": lit(1), "name": "n"}, {"fn": "COUNT", "expr": col("v", s), "name": "cv"}, {"fn": "SUM", "expr": col("v", s), "name": "sv"},
            {"fn": "MIN", "expr": col("v", s), "name": "lo"}, {"fn": "MAX", "expr": col("v", s), "name": "hi"}, {"fn": "BIT_XOR", "expr": col("x", s), "name": "bx"},
            {"fn": "SUM", "expr": col("v", s), "name": "sf", "filter": binary(col("f", s), Op.Lt, lit(3, "Int32"))}]


def fold_a(m, rows):
    v, x, w = pylist(m, "v"), pylist(m, "x"), m["f"] < 3
    return (GS.count_star(rows), GS.count(v, rows), GS.total(v, rows), GS.minimum(v, rows), GS.maximum(v, rows), GS.bit_fold("XOR", x, rows, 32), GS.total(v, rows, where=w))


def aggs_b(s):
    return [{"fn": "SUM", "expr": col("d", s), "name": "sd"}, {"fn": "MIN", "expr": col("d", s), "name": "ld"}, {"fn": "MAX", "expr": col("d", s), "name": "hd"},
            {"fn": "AVG", "expr": col("d", s), "name": "ad"}, {"fn": "BOOL_OR", "expr": col("b", s), "name": "bo"}, {"fn": "COUNT", "expr": lit(1), "name": "n"}]


def fold_b(m, rows):
    d, b = pylist(m, "d"), pylist(m, "b")
    return (GS.total(d, rows, bits=128), GS.minimum(d, rows), GS.maximum(d, rows), GS.avg_decimal(d, rows), GS.bool_or(b, rows), GS.count_star(rows))


def rows_of(t, nk):
    """{key tuple: tuple of values}: decimals as their unscaled integers; no key tuple twice"""
    cols = []
    for f, c in zip(t.schema, t.columns):
        if pa.types.is_decimal128(f.type):
            cols.append([None if v is None else int(v.scaleb(f.type.scale, CTX)) for v in c.to_pylist()])
        else:
            cols.append(c.to_pylist())
    keys = list(zip(*cols[:nk]))
    assert len(set(keys)) == len(keys) == t.num_rows, "a key tuple twice"
    return dict(zip(keys, zip(*cols[nk:])))


def expected(m, sets, fold, names=("a", "s", "c"), keep=None):
    return {k: fold(m, rows) for k, rows in GS.groups(key_tuples(m, names), sets, keep).items()}


def node_of(src, mode, names, aggs, sets, strategy="auto"):
    s = src.schema()
    return g.AggregateExec(mode, [(col(k, s), k) for k in names], aggs(s), src, strategy=strategy, grouping_sets=sets)


SETS = {"rollup": GS.rollup(3), "cube": GS.cube(3), "explicit": [[F, F, T], [T, T, T], [F, F, T], [T, F, F]], "one_masking": [[F, T, F]]}


# ------------------------------------------------------------------------------------ mode Single
@pytest.mark.parametrize("strategy", ["auto", "hash"])
@pytest.mark.parametrize("which", list(SETS))
def test_single(tc, which, strategy):
    """Three keys -- Int32 of 3 values, Utf8 of 4 (the empty string and fifteen bytes among them), Int64 of 5 with 10 % NULLs -- so really
    NULL keys merge into the sets that mask `c`.  The same NativePlan twice: the second execution is the deferred replay."""
    m = mixed(1)
    t = arrow_of(m)
    sets = SETS[which]
    for aggs, fold in ((aggs_a, fold_a), (aggs_b, fold_b)):
        node = node_of(g.MemoryExec([t]), "Single", ("a", "s", "c"), aggs, sets, strategy)
        plan = g.NativePlan(node, tc)
        got = plan.execute(0).to_arrow()
        assert got.schema.names == [f["name"] for f in node.schema()] == [n for n, _, _ in plan.schema()]
        rows = rows_of(got, 3)
        exp = expected(m, sets, fold)
        assert set(rows) == set(exp), (which, sorted(set(rows) ^ set(exp), key=str)[:5])
        assert rows == exp, [(k, rows[k], exp[k]) for k in exp if rows[k] != exp[k]][:3]
        assert rows_of(plan.execute(0).to_arrow(), 3) == exp
        assert rows_of(plan.execute(0).to_arrow(), 3) == exp
    if which == "rollup":
        assert (None, None, None) in exp and exp[(None, None, None)][-1] == 5000
    if which == "explicit":      # the duplicated set counts every row twice, and the really-NULL keys land there too
        assert sum(v[-1] for k, v in exp.items() if k[0] is not None and k[1] is not None) == 2 * 5000
    if which == "one_masking":
        assert len(exp) == 3 * 6 and all(k[1] is None for k in exp)


def test_single_under_a_fused_filter_and_a_computed_projection(tc):
    m = mixed(2)
    src = g.MemoryExec([arrow_of(m)])
    s = src.schema()
    proj = g.ProjectionExec([(col("a", s), "a"), (col("s", s), "s"), (col("c", s), "c"), (binary(binary(col("c", s), Op.Multiply, lit(2)), Op.Plus, col("v", s)), "y"),
                             (col("f", s), "f")], src)
    flt = g.FilterExec(binary(col("f", proj.schema()), Op.Gt, lit(1, "Int32")), proj)
    fs = flt.schema()
    node = g.AggregateExec("Single", [(col(k, fs), k) for k in ("a", "s", "c")], [{"fn": "SUM", "expr": col("y", fs), "name": "sy"}, {"fn": "COUNT", "expr": lit(1), "name": "n"},
                                                                                 {"fn": "MAX", "expr": col("y", fs), "name": "my"}], flt, grouping_sets=GS.cube(3))
    y = [None if c is None or v is None else c * 2 + v for c, v in zip(pylist(m, "c"), pylist(m, "v"))]      # (|v| < 2^63 - 30: the sum does not wrap, the SUM of them does)
    exp = {k: (GS.total(y, rows), GS.count_star(rows), GS.maximum(y, rows)) for k, rows in GS.groups(key_tuples(m), GS.cube(3), keep=m["f"] > 1).items()}
    assert rows_of(g.NativePlan(node, tc).execute(0).to_arrow(), 3) == exp and 0 < exp[(None, None, None)][1] < m["n"]


def test_single_with_a_join_below(tc):
    m = mixed(3)
    dims = pa.table({"ka": pa.array([0, 1, 2], pa.int32()), "w": pa.array([70, 80, 80], pa.int64())})
    left, right = g.MemoryExec([dims]), g.MemoryExec([arrow_of(m)])
    join = g.HashJoinExec(left, right, [(col("ka", left.schema()), col("a", right.schema()))])
    js = join.schema()
    node = g.AggregateExec("Single", [(col("w", js), "w"), (col("s", js), "s")], [{"fn": "SUM", "expr": col("v", js), "name": "sv"}, {"fn": "COUNT", "expr": lit(1), "name": "n"}], join,
                           grouping_sets=GS.rollup(2))
    w = [70 if a == 0 else 80 for a in m["a"]]
    v = pylist(m, "v")
    exp = {k: (GS.total(v, rows), GS.count_star(rows)) for k, rows in GS.groups(list(zip(w, pylist(m, "s"))), GS.rollup(2)).items()}
    assert rows_of(g.NativePlan(node, tc).execute(0).to_arrow(), 2) == exp and len(exp) == 2 * 4 + 2 + 1


# ------------------------------------------------------------------------------------ shapes
def small_table(a, c, v):
    return pa.table({"a": pa.array(a, pa.int32()), "c": pa.array(c, pa.int64()), "v": pa.array(v, pa.int64())})


def run_small(tc, t, sets):
    src = g.MemoryExec([t])
    s = src.schema()
    node = g.AggregateExec("Single", [(col("a", s), "a"), (col("c", s), "c")], [{"fn": "SUM", "expr": col("v", s), "name": "sv"}, {"fn": "COUNT", "expr": lit(1), "name": "n"}], src,
                           grouping_sets=sets)
    plan = g.NativePlan(node, tc)
    first = plan.execute(0).to_arrow()
    assert first.schema.names == ["a", "c", "sv", "n"]
    rows = rows_of(first, 2)
    assert rows_of(plan.execute(0).to_arrow(), 2) == rows      # the same plan again
    a, c, v = (t.column(k).to_pylist() for k in ("a", "c", "v"))
    assert rows == {k: (GS.total(v, r), GS.count_star(r)) for k, r in GS.groups(list(zip(a, c)), sets).items()}
    return rows


def test_shapes(tc):
    cube = GS.cube(2)
    assert run_small(tc, small_table([], [], []), cube) == {}      # no input rows: no output rows, () among the sets or not
    assert run_small(tc, small_table([], [], []), [[T, T]]) == {}
    assert run_small(tc, small_table([7], [9], [5]), cube) == {(7, 9): (5, 1), (7, None): (5, 1), (None, 9): (5, 1), (None, None): (5, 1)}
    n = 700      # every row its own finest group
    rows = run_small(tc, small_table(list(range(n)), [i * 3 for i in range(n)], list(range(n))), GS.rollup(2))
    assert len(rows) == 2 * n + 1 and rows[(None, None)] == (n * (n - 1) // 2, n)
    rows = run_small(tc, small_table([4] * n, [6] * n, list(range(n))), cube)      # one finest group
    assert rows == {k: (n * (n - 1) // 2, n) for k in ((4, 6), (4, None), (None, 6), (None, None))}


def test_two_hundred_thousand_rows(tc):
    """About 21,000 finest groups under ROLLUP of three keys (S = 4): the state table the sets are made from is a tenth of the input."""
    n = 200_000
    r = np.random.default_rng(4)
    t = pa.table({"k1": pa.array(r.integers(0, 3, n).astype(np.int32)), "k2": pa.array(r.integers(0, 70, n).astype(np.int32)), "k3": pa.array(r.integers(0, 100, n)),
                  "v": pa.array(r.integers(-1000, 1000, n))})
    src = g.MemoryExec([t])
    s = src.schema()
    names = ["k1", "k2", "k3"]
    node = g.AggregateExec("Single", [(col(k, s), k) for k in names], [{"fn": "SUM", "expr": col("v", s), "name": "sv"}, {"fn": "COUNT", "expr": lit(1), "name": "n"}], src,
                           grouping_sets=GS.rollup(3))
    plan = g.NativePlan(node, tc)
    rows = rows_of(plan.execute(0).to_arrow(), 3)
    exp = {}
    for keep in range(3, -1, -1):      # (no NULL keys: the sets' rows do not meet)
        if keep == 0:
            exp[(None, None, None)] = (int(t["v"].to_numpy().sum()), n)
            continue
        a = t.group_by(names[:keep]).aggregate([("v", "sum"), ("v", "count")])
        for row in zip(*[a.column(k).to_pylist() for k in names[:keep] + ["v_sum", "v_count"]]):
            exp[tuple(row[:keep]) + (None,) * (3 - keep)] = (row[keep], row[keep + 1])
    assert 20_000 < sum(1 for k in exp if None not in k) <= 21_000
    assert rows == exp
    assert rows_of(plan.execute(0).to_arrow(), 3) == exp


# ------------------------------------------------------------------------------------ mode Partial, and Merge on its own
def test_partial_with_sets_then_final_partitioned(tc):
    m = mixed(5)
    pid = np.random.default_rng(6).integers(0, 3, m["n"])
    parts = [arrow_of(m, np.nonzero(pid == k)[0]) for k in range(3)]
    sets = SETS["explicit"]
    for aggs, fold in ((aggs_a, fold_a), (aggs_b, fold_b)):
        src = g.MemoryExec(parts)
        partial = node_of(src, "Partial", ("a", "s", "c"), aggs, sets)
        plain = node_of(src, "Partial", ("a", "s", "c"), aggs, None)
        assert [(f["name"], f["type"]) for f in partial.schema()] == [(f["name"], f["type"]) for f in plain.schema()]
        plan = g.NativePlan(partial, tc)
        states = [plan.execute(k).to_arrow() for k in range(3)]
        for k in range(3):
            assert states[k].schema.names == [f["name"] for f in partial.schema()]
            keys = list(zip(*[states[k].column(i).to_pylist() for i in range(3)]))
            sel = pid == k
            part_groups = GS.groups(key_tuples(m), sets, keep=sel)
            # one row per key tuple of each set, not the finest set's rows S times
            assert len(set(keys)) == len(keys) == len(part_groups) and set(keys) == set(part_groups)
        merged = g.MemoryExec([pa.concat_tables(states)])
        fs = merged.schema()
        final = g.AggregateExec("FinalPartitioned", [(col(k, fs), k) for k in ("a", "s", "c")], [{"fn": a["fn"], "name": a["name"]} for a in aggs(src.schema())], merged)
        assert rows_of(g.NativePlan(final, tc).execute(0).to_arrow(), 3) == expected(m, sets, fold)


def test_merge_between_partial_and_final(tc):
    """Final(Merge(X)) gives the rows of Final(X), X the concatenated Partial states of three partitions: exactly for integers, decimals and
    the bit functions, to the whole table's bounds for the moment functions (as the two-phase test of the float aggregates holds its Final)."""
    from test_gpu_float_agg_exact import aggs_of, check_values
    from test_gpu_agg_by_build_row import native_rows
    m = mixed(7)
    pid = np.random.default_rng(8).integers(0, 3, m["n"])
    src = g.MemoryExec([arrow_of(m, np.nonzero(pid == k)[0]) for k in range(3)])
    for aggs, fold in ((aggs_a, fold_a), (aggs_b, fold_b)):
        partial = g.NativePlan(node_of(src, "Partial", ("a", "s", "c"), aggs, None), tc)
        x = g.MemoryExec([pa.concat_tables([partial.execute(k).to_arrow() for k in range(3)])])
        xs = x.schema()
        keys = [(col(k, xs), k) for k in ("a", "s", "c")]
        fns = [{"fn": a["fn"], "name": a["name"]} for a in aggs(src.schema())]
        merge = g.AggregateExec("Merge", keys, fns, x)
        assert [(f["name"], f["type"]) for f in merge.schema()] == [(f["name"], f["type"]) for f in xs]
        merged = g.NativePlan(merge, tc).execute(0).to_arrow()
        assert merged.schema.names == [f["name"] for f in xs] and merged.num_rows == len(set(key_tuples(m))) < x.execute(0, tc).num_rows
        via_merge = g.AggregateExec("Final", keys, fns, merge)
        direct = g.AggregateExec("Final", keys, fns, x)
        a, b = rows_of(g.NativePlan(via_merge, tc).execute(0).to_arrow(), 3), rows_of(g.NativePlan(direct, tc).execute(0).to_arrow(), 3)
        assert a == b == expected(m, [[F, F, F]], fold)
    # the moment functions
    name, nulls = "f64_1e6", 0.2
    t = X.family(name, 0, nulls)
    t = t.append_column(pa.field("g32", pa.int32(), nullable=False), t["g"].cast(pa.int32()))
    part = X.partition_of(t)
    fsrc = g.MemoryExec([t.take([i for i in range(t.num_rows) if part[i] == k]) for k in range(3)])
    s = fsrc.schema()
    whole = X.reference(name, 0, nulls)
    for fn, which, finals in (("VARIANCE", "x", ["VARIANCE", "VAR_POP", "STDDEV", "STDDEV_POP"]), ("CORR", "xy", ["CORR"]), ("COVAR", "xy", ["COVAR", "COVAR_POP"])):
        partial = g.NativePlan(g.AggregateExec("Partial", [(col("g32", s), "g")], aggs_of(s, [fn]), fsrc), tc)
        x = g.MemoryExec([pa.concat_tables([partial.execute(k).to_arrow() for k in range(3)])])
        xs = x.schema()
        merge = g.AggregateExec("Merge", [(col("g", xs), "g")], [{"fn": fn, "name": fn}], x)
        assert [f["name"] for f in merge.schema()] == [f["name"] for f in xs]
        for ffn in finals:
            final = g.AggregateExec("Final", [(col("g", xs), "g")], [{"fn": ffn, "name": ffn}], merge)
            check_values(native_rows(g.NativePlan(final, tc)), whole[which], True, [ffn], False, "merge/%s/%s" % (fn, ffn))


# ------------------------------------------------------------------------------------ floats
def float_node(src, fns, sets):
    s = src.schema()
    aggs = [dict({"fn": fn, "expr": col("x", s), "name": fn}, **({"expr2": col("y", s)} if fn in ("COVAR", "COVAR_POP", "CORR") else {})) for fn in fns]
    return g.AggregateExec("Single", [(col("g", s), "g"), (col("h", s), "h")], aggs, src, grouping_sets=sets)


@pytest.mark.parametrize("name", ["f64_n1e3", "f64_1e6"])
def test_float_functions_under_rollup(tc, name):
    """Each group of each set of ROLLUP(g, h) is held to its own Tolerances with R taken over all rows that take part: the precedent of the
    two-phase runs (the states the sets are made from are a Partial's, and the Final's origin is a state mean)."""
    t = X.family(name, 0, 0.2)
    t = t.append_column(pa.field("h", pa.int32(), nullable=False), pa.array((t["p"].to_numpy() % 3).astype(np.int32)))
    xs, ys = X.f64_column(t, "x"), X.f64_column(t, "y")
    keys = list(zip(t["g"].to_pylist(), t["h"].to_pylist()))
    sets = GS.rollup(2)
    grouped = GS.groups(keys, sets)
    for fns, pair in ((["SUM", "AVG", "VARIANCE", "STDDEV"], False), (["COVAR", "CORR"], True)):
        got = g.NativePlan(float_node(g.MemoryExec([t]), fns, sets), tc).execute(0).to_arrow()
        rows = rows_of(got, 2)
        assert set(rows) == set(grouped) and len(rows) > 8 + 8 + 1
        part = [i for i in range(t.num_rows) if xs[i] is not None and (not pair or ys[i] is not None)]
        rx = Fraction(max(xs[i] for i in part)) - Fraction(min(xs[i] for i in part))
        ry = Fraction(max(ys[i] for i in part)) - Fraction(min(ys[i] for i in part)) if pair else None
        for k, grows in grouped.items():
            st = GS.stats(xs, grows, ys if pair else None)
            tol = X.Tolerances(st, rx, ry, orders=2)
            exact = st.values()
            for fn, v in zip(fns, rows[k]):
                if exact[fn] is None:
                    assert v is None, (k, fn, st.n, v)
                    continue
                err, bound = abs(Fraction(v) - exact[fn]), tol.of(fn)
                print("%s %s %s n=%d: error %.3e, bound %.3e" % (name, k, fn, st.n, float(err), float(bound)))
                assert err <= bound, (name, k, fn, st.n, v, float(exact[fn]), float(err), float(bound))


def test_float_functions_where_every_intermediate_is_exact(tc):
    """Integers below 2^10 and group sizes that are powers of two at every level of ROLLUP(g, h): every power sum, every division by n and
    every state is exactly representable, so VAR_POP and COVAR_POP come out bit for bit; the sample forms divide by n - 1 once more and are
    held within 4 u |v|, the term float_agg_exact.py grants the last division."""
    r = np.random.default_rng(12)
    gk = np.repeat(np.arange(4, dtype=np.int64), 16)
    hk = np.tile(np.repeat(np.arange(2, dtype=np.int32), 8), 4)
    o = r.permutation(64)
    x, y = r.integers(0, 1024, 64).astype(np.float64), r.integers(0, 1024, 64).astype(np.float64)
    t = pa.table({"g": pa.array(gk[o]), "h": pa.array(hk[o]), "x": pa.array(x), "y": pa.array(y)})
    grouped = GS.groups(list(zip(gk[o].tolist(), hk[o].tolist())), GS.rollup(2))
    assert sorted(len(v) for v in grouped.values()) == [8] * 8 + [16] * 4 + [64]
    for fns in (["VAR_POP", "VARIANCE"], ["COVAR_POP", "COVAR"]):      # (two nodes: a Final keeps every function's sums apart, twelve accumulators in all)
        rows = rows_of(g.NativePlan(float_node(g.MemoryExec([t]), fns, GS.rollup(2)), tc).execute(0).to_arrow(), 2)
        assert set(rows) == set(grouped)
        for k, grows in grouped.items():
            exact = GS.stats(x.tolist(), grows, y.tolist()).values()
            for fn, v in zip(fns, rows[k]):
                e = exact[fn]
                if fn.endswith("_POP"):
                    assert Fraction(v) == e, (k, fn, v, float(e))
                else:
                    assert abs(Fraction(v) - e) <= 4 * X.U * abs(e), (k, fn, v, float(e))


# ------------------------------------------------------------------------------------ a second opinion
def test_every_set_against_pyarrow_group_by(tc):
    m = mixed(9, null_c=0.0)
    t = arrow_of(m)
    names = ["a", "s", "c"]
    sets = GS.cube(3)
    src = g.MemoryExec([t])
    s = src.schema()
    node = g.AggregateExec("Single", [(col(k, s), k) for k in names], [{"fn": "COUNT", "expr": col("v", s), "name": "cv"}, {"fn": "SUM", "expr": col("d", s), "name": "sd"},
                                                                       {"fn": "MIN", "expr": col("x", s), "name": "lx"}, {"fn": "MAX", "expr": col("x", s), "name": "hx"}], src,
                           grouping_sets=sets)
    rows = rows_of(g.NativePlan(node, tc).execute(0).to_arrow(), 3)
    seen = 0
    for mask in sets:
        kept = [k for k, masked in zip(names, mask) if not masked]
        a = t.group_by(kept).aggregate([("v", "count"), ("d", "sum"), ("x", "min"), ("x", "max")])
        for row in a.to_pylist():
            key = tuple(None if masked else row[k] for k, masked in zip(names, mask))
            sd = None if row["d_sum"] is None else int(row["d_sum"].scaleb(2, CTX))
            assert rows[key] == (row["v_count"], sd, row["x_min"], row["x_max"]), (mask, key)
            seen += 1
    assert seen == len(rows)      # (no NULL keys in this table: every output row belongs to exactly one set)


# ------------------------------------------------------------------------------------ refusals and the memory budget
def test_refusals_at_run_time(tc):
    n = 300
    t = pa.table({"a": pa.array(np.arange(n, dtype=np.int32) % 3), "name": pa.array(["twenty bytes of name %02d" % (i % 7) for i in range(n)]), "v": pa.array(np.arange(n, dtype=np.int64))})
    src = g.MemoryExec([t])
    s = src.schema()
    sv = {"fn": "SUM", "expr": col("v", s), "name": "sv"}
    keys = [(col("a", s), "a"), (col("name", s), "name")]
    with pytest.raises(g.GpuqError, match=r"grouping sets: group key 'name' holds strings longer than 15 bytes") as e:
        g.NativePlan(g.AggregateExec("Single", keys, [sv], src, grouping_sets=GS.rollup(2)), tc).execute(0)
    assert e.value.status == 3 and e.value.refusal == B.REFUSAL_LONG_STRING
    # the plain node goes on grouping by long strings
    assert g.NativePlan(g.AggregateExec("Single", keys, [sv], src), tc).execute(0).num_rows == 21
    with pytest.raises(g.GpuqError, match=r"grouping sets beside COUNT\(DISTINCT") as e:
        g.NativePlan(g.AggregateExec("Single", keys[:1], [sv, {"fn": "COUNT", "expr": col("v", s), "name": "c", "distinct": True}], src, grouping_sets=[[F], [T]]), tc)
    assert e.value.status == 3 and e.value.refusal == B.REFUSAL_NONE


def test_the_expansion_counts_against_the_memory_budget(tc):
    n = 200_000      # every row its own finest group: the state table is as long as the input, the expansion eight times that
    t = pa.table({"k1": pa.array(np.arange(n, dtype=np.int64)), "k2": pa.array(np.arange(n, dtype=np.int64) * 7), "k3": pa.array((np.arange(n) % 5).astype(np.int32)),
                  "v": pa.array(np.arange(n, dtype=np.int64))})
    src = g.MemoryExec([t])
    s = src.schema()
    node = g.AggregateExec("Single", [(col(k, s), k) for k in ("k1", "k2", "k3")], [{"fn": "SUM", "expr": col("v", s), "name": "sv"}, {"fn": "COUNT", "expr": lit(1), "name": "n"}], src,
                           grouping_sets=GS.cube(3))
    plan = g.NativePlan(node, tc)      # (the table is uploaded here: it is the caller's, not the budget's)
    base = g.memory_stats(reset_peak=True)
    assert base["limit"] == 0
    got = plan.execute(0)
    total = n * (n - 1) // 2

    def grand_total(res):
        a = res.to_arrow()
        a = a.filter(pc.and_(pc.and_(pc.is_null(a["k1"]), pc.is_null(a["k2"])), pc.is_null(a["k3"])))
        return a.num_rows == 1 and (a["sv"][0].as_py(), a["n"][0].as_py())
    assert grand_total(got) == (total, n)
    del got
    held = g.memory_stats()["in_use"]      # what the plan's operators keep between executions (their tables and workspaces)
    used = g.memory_stats()["peak"] - held
    assert used > 8 * n * (8 + 8 + 4 + 8 + 8)      # an execution's own buffers: at least the expansion's five columns
    try:
        g.memory_limit(held + used // 4)
        with pytest.raises(g.GpuqError) as e:
            plan.execute(0)
        assert e.value.status == 4 and "Resources exhausted" in str(e.value) and "memory limit" in str(e.value)
        assert g.memory_stats()["in_use"] - held < (8 << 20)      # nothing leaked by the failed task
    finally:
        g.memory_limit(0)
    assert grand_total(plan.execute(0)) == (total, n)
