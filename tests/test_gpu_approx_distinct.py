"""APPROX_DISTINCT on the device (the entry point gpuq_segment_approx_distinct alone, then AggregateExec in mode Single through the
native executor) against the numpy restatement of its HyperLogLog, tests/hll_sketch.py.  A sketch is a set of maxima and the estimator
is stated in Float64 without contraction, so every comparison is exact; how far the estimate lies from the exact count is what
tests/test_cpu_approx_distinct.py settles on the restatement."""
import ctypes as C
import decimal
import os

import numpy as np
import pyarrow as pa
import pytest

import arrow_ballista_amd as g
import hll_sketch as H
import test_gpu_median as TM
from arrow_ballista_amd import binding as B
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit

pytestmark = pytest.mark.gpu

CTX = decimal.Context(prec=60)


def approx_agg(name="d", c="v", **kw):
    return lambda s: dict({"fn": "APPROX_DISTINCT", "expr": col(c, s), "name": name}, **kw)


def by_key(t, nkeys, names):
    """{key tuple: tuple of the named columns}."""
    keys = list(zip(*[t.column(i).to_pylist() for i in range(nkeys)])) if nkeys else [()] * t.num_rows
    vals = list(zip(*[t.column(n).to_pylist() for n in names]))
    assert len(set(keys)) == len(keys) == t.num_rows
    return dict(zip(keys, vals))


def expected(keys, vals, valid, tname, n):
    """{key tuple: estimate}: groups as test_gpu_median finds them, the restatement over each group's non-NULL values."""
    order, segs = TM.segments(keys, n)
    vals = np.asarray(vals, dtype=object) if tname in ("Decimal", "Utf8") else np.asarray(vals)
    return {key: H.approx_distinct(vals[order[a:b]], tname, valid[order[a:b]]) for key, a, b in segs}


# ------------------------------------------------------------------------------------ the entry point alone
def entry_shape():
    r = np.random.default_rng(21)
    n = 5000
    #         tiles 0..7, ends on an edge | 300 rows of their own | begins mid-tile, crosses three edges | empty | all NULL | | ends at n
    starts = [0, 2048] + list(range(2049, 2349)) + [3100, 3100, 3200, 4000, n]
    assert 2348 % 256 != 0 and 3100 // 256 - 2348 // 256 == 3 and n % 256 != 0 and starts[-5] == starts[-4]
    vals, valid = r.integers(-300, 300, n), r.random(n) >= 0.15
    valid[3100:3200] = False
    starts = np.array(starts, dtype=np.int32)
    exp = [H.approx_distinct(vals[a:b], "Int64", valid[a:b]) for a, b in zip(starts[:-1], starts[1:])]
    return n, vals, valid, starts, exp


def run_entry(tc, col_struct, starts_dev, n_groups, n, tile_rows, out):
    tc.ctx.check(tc.ctx.L.gpuq_segment_approx_distinct(tc.ctx.h, tc.stream_ptr(), C.byref(col_struct), starts_dev.data_ptr(), n_groups, n, tile_rows, out.data_ptr()))
    tc.sync()
    return out.cpu().numpy().view(np.uint64).tolist()


def test_entry_point_segment_shapes_and_tiles(tc):
    import torch
    n, vals, valid, starts, exp = entry_shape()
    G = len(starts) - 1
    assert exp[0] > 400 and exp[1:301] == [int(v) for v in valid[2048:2348]] and exp[-4:-2] == [0, 0] and min(exp[301], exp[-2], exp[-1]) > 300
    d, v, s = TM.to_device(vals), TM.to_device(TM.bitmap(valid)), TM.to_device(starts)
    c = TM.column_struct(B.T_INT64, d, v, n)
    guard = 0x5A5A5A5A5A5A5A5A
    got = {}
    for tile_rows in (256, 0, 1024):
        out = torch.full((G + 1,), guard, dtype=torch.int64, device="cuda")
        got[tile_rows] = run_entry(tc, c, s, G, n, tile_rows, out)
        assert got[tile_rows] == exp + [guard], tile_rows      # tiling does not show; nothing behind the last segment is written
    again = torch.full((G + 1,), guard, dtype=torch.int64, device="cuda")
    assert run_entry(tc, c, s, G, n, 256, again) == got[256]      # a second call on the same stream: the same bits
    none = torch.full((2,), guard, dtype=torch.int64, device="cuda")
    assert run_entry(tc, c, s, 0, n, 256, none) == [guard, guard]      # no segments: nothing is written
    with pytest.raises(g.GpuqError, match="tile_rows"):
        run_entry(tc, c, s, G, n, 100, again)


def test_entry_point_many_tiles_merge_in_two_levels(tc):
    """157 tiles of 256 rows, more than the 64 from which the partial sketches behind an owner are folded in 32 runs first: a segment over
    118 tiles (runs of 4, the last one short), one-row segments, a segment over 39 tiles from mid-tile to n (runs of 2)."""
    import torch
    r = np.random.default_rng(22)
    n = 40_000
    starts = np.array([0, 30_000, 30_001, 30_002, n], dtype=np.int32)
    vals, valid = r.integers(-2**40, 2**40, 6000)[r.integers(0, 6000, n)], r.random(n) >= 0.1
    exp = [H.approx_distinct(vals[a:b], "Int64", valid[a:b]) for a, b in zip(starts[:-1], starts[1:])]
    assert exp[0] > 5000 and exp[3] > 4000
    d, v, s = TM.to_device(vals), TM.to_device(TM.bitmap(valid)), TM.to_device(starts)
    c = TM.column_struct(B.T_INT64, d, v, n)
    for tile_rows in (256, 512, 0):      # 157 tiles: two levels; 79: two levels, runs of 2 and 1; one tile
        out = torch.full((5,), 77, dtype=torch.int64, device="cuda")
        assert run_entry(tc, c, s, 4, n, tile_rows, out) == exp + [77], tile_rows


# ------------------------------------------------------------------------------------ every argument type
INT_TYPES = {"Int8": pa.int8(), "Int16": pa.int16(), "Int32": pa.int32(), "Int64": pa.int64(), "UInt8": pa.uint8(), "UInt16": pa.uint16(), "UInt32": pa.uint32(),
             "UInt64": pa.uint64(), "Date32": pa.date32(), "Date64": pa.date64(), "Timestamp": pa.timestamp("ns")}
STORAGE = {"Date32": np.int32, "Date64": np.int64, "Timestamp": np.int64}
ARG_TYPES = list(INT_TYPES) + ["Float32", "Float64", "Decimal", "Utf8"]


def argument_column(r, tname, n):
    """(values for the restatement, Arrow array without its NULLs yet): about 300 different values, so every group repeats some."""
    pick = r.integers(0, 300, n)
    if tname in INT_TYPES:
        dt = np.dtype(STORAGE.get(tname, tname.lower()))
        ii = np.iinfo(dt)
        pool = r.integers(ii.min, ii.max, 300, dtype=dt, endpoint=True)
        if tname == "Date64":
            pool = pool // 86_400_000 // 1000 * 86_400_000      # whole days, in range
        vals = pool[pick]
        return vals, lambda mask: pa.array(vals, pa.from_numpy_dtype(dt), mask=mask).cast(INT_TYPES[tname])
    if tname in ("Float32", "Float64"):
        dt = np.float32 if tname == "Float32" else np.float64
        pool = (r.standard_normal(300) * 1e3).astype(dt)
        pool[:4] = [0.0, -0.0, np.inf, np.nan]
        vals = pool[pick]
        return vals, lambda mask: pa.array(vals, mask=mask)
    if tname == "Decimal":      # beyond 64 bits, both signs
        pool = [int(x) * 10**22 + int(y) for x, y in zip(r.integers(-10**15, 10**15, 300), r.integers(0, 10**18, 300))]
        vals = np.array([pool[i] for i in pick], dtype=object)
        return vals, lambda mask: pa.array([None if m else decimal.Decimal(int(v)).scaleb(-4, CTX) for v, m in zip(vals, mask)], pa.decimal128(38, 4))
    pool = ["", "a", "a ", "fifteen bytes..", "fifteen bytes.!"] + ["w%d" % i * (1 + i % 3) for i in range(295)]
    assert max(len(w.encode()) for w in pool) == 15 and len(set(pool)) == 300
    vals = np.array([pool[i] for i in pick], dtype=object)
    return vals, lambda mask: pa.array([None if m else v for v, m in zip(vals, mask)], pa.utf8())


def grouped_check(tc, tname, vals, make, valid, k):
    n = len(k)
    t = pa.table({"k": pa.array(k), "v": make(~valid)})
    got, node = TM.run_node(tc, t, ["k"], lambda s: [approx_agg()(s)])
    assert got.schema.names == ["k", "d"] and got.column("d").type == pa.uint64() and got.column("d").null_count == 0
    assert node.schema()[1] == {"name": "d", "type": "UInt64", "nullable": False}
    exp = expected([(k, np.ones(n, dtype=bool))], vals, valid, tname, n)
    assert by_key(got, 1, ["d"]) == {key: (v,) for key, v in exp.items()}
    return exp


@pytest.mark.parametrize("tname", ARG_TYPES)
def test_argument_types(tc, tname):
    r = np.random.default_rng(len(tname) + 60)
    n = 3000
    vals, make = argument_column(r, tname, n)
    valid = r.random(n) >= 0.15
    k = r.integers(0, 7, n).astype(np.int32)
    exp = grouped_check(tc, tname, vals, make, valid, k)
    assert len(exp) == 7 and all(100 < v < 320 for v in exp.values())


def test_floats_count_by_value(tc):
    """-0.0 and 0.0 are one value, two NaN patterns are one value: 2 in all; the other group holds what a bytewise count would split."""
    nans = np.array([0x7FF8000000000000, 0xFFF0000000000001], dtype=np.uint64).view(np.float64)
    vals = np.array([-0.0, 0.0, nans[0], nans[1], 1.5, -1.5, 0.0, -0.0, nans[1]])
    k = np.array([0, 0, 0, 0, 1, 1, 1, 1, 1], dtype=np.int32)
    t = pa.table({"k": pa.array(k), "v": pa.array(vals)})
    assert t.column("v").chunk(0).to_numpy().view(np.uint64).tolist() == vals.view(np.uint64).tolist()      # the payloads reach the table
    got, _ = TM.run_node(tc, t, ["k"], lambda s: [approx_agg()(s)])
    assert by_key(got, 1, ["d"]) == {(0,): (2,), (1,): (4,)}
    with np.errstate(invalid="ignore"):      # (narrowing the signalling NaN)
        f32 = pa.table({"k": pa.array(k), "v": pa.array(vals.astype(np.float32))})
    got, _ = TM.run_node(tc, f32, ["k"], lambda s: [approx_agg()(s)])
    assert by_key(got, 1, ["d"]) == {(0,): (2,), (1,): (4,)}


def test_int8_and_uint8_of_the_same_numbers_agree(tc):
    r = np.random.default_rng(5)
    n = 3000
    small, valid, k = r.integers(0, 128, n), r.random(n) >= 0.15, r.integers(0, 7, n).astype(np.int32)
    a = grouped_check(tc, "Int8", small.astype(np.int8), lambda mask: pa.array(small.astype(np.int8), mask=mask), valid, k)
    b = grouped_check(tc, "UInt8", small.astype(np.uint8), lambda mask: pa.array(small.astype(np.uint8), mask=mask), valid, k)
    assert a == b


# ------------------------------------------------------------------------------------ the node shapes
def test_ungrouped_and_no_rows(tc):
    d = TM.mixed_table(31)
    got, node = TM.run_node(tc, TM.mixed_arrow(d), [], lambda s: [approx_agg()(s)])
    assert [c.to_pylist() for c in got.columns] == [[H.approx_distinct(d["v"], "Int64", d["v_ok"])]]
    assert node.schema() == [{"name": "d", "type": "UInt64", "nullable": False}]
    empty = TM.mixed_arrow(TM.mixed_table(2, n=0))
    got, _ = TM.run_node(tc, empty, [], lambda s: [approx_agg()(s)])      # ungrouped over no rows: one row holding 0
    assert [c.to_pylist() for c in got.columns] == [[0]] and got.column("d").type == pa.uint64()
    got, _ = TM.run_node(tc, empty, ["k"], lambda s: [approx_agg()(s)])      # grouped over no rows: no rows
    assert got.num_rows == 0 and got.schema.names == ["k", "d"]


@pytest.mark.parametrize("kinds", [["Int32", "Int16?"], ["Utf8?"], ["Int64?"]], ids=lambda k: "-".join(k))
def test_keys(tc, kinds):
    r = np.random.default_rng(70 + len(kinds[0]))
    n = 3000
    cols = [TM.key_column(r, kind, n) for kind in kinds]
    vals, valid = r.integers(0, 200, n), r.random(n) >= 0.2
    t = pa.Table.from_arrays([pa.array(kv, kt, mask=~kok) for kt, kv, kok in cols] + [pa.array(vals, mask=~valid)], names=["k%d" % i for i in range(len(cols))] + ["v"])
    got, _ = TM.run_node(tc, t, ["k%d" % i for i in range(len(cols))], lambda s: [approx_agg()(s)])
    exp = expected([(kv, kok) for _, kv, kok in cols], vals, valid, "Int64", n)
    assert any(None in key for key in exp) and len(exp) > 5      # NULL is a group
    assert by_key(got, len(cols), ["d"]) == {key: (v,) for key, v in exp.items()}


def test_filter_and_the_same_argument_twice(tc):
    d = TM.mixed_table(32)
    pred = lambda s: binary(col("f", s), Op.Lt, lit(3, "Int32"))
    got, _ = TM.run_node(tc, TM.mixed_arrow(d), ["k"], lambda s: [approx_agg("a")(s), approx_agg("af", filter=pred(s))(s), approx_agg("again")(s), approx_agg("w", "w")(s)])
    keys = [(d["k"], np.ones(d["n"], dtype=bool))]
    a, w = expected(keys, d["v"], d["v_ok"], "Int64", d["n"]), expected(keys, d["w"], d["w_ok"], "Float64", d["n"])
    af = expected(keys, d["v"], d["v_ok"] & (d["f"] < 3), "Int64", d["n"])      # a row the filter does not pass counts as a NULL argument
    assert af != a and len(a) == 37
    assert by_key(got, 1, ["a", "af", "again", "w"]) == {key: (a[key], af[key], a[key], w[key]) for key in a}


def test_beside_other_aggregates_and_median(tc):
    d = TM.mixed_table(33)
    t = TM.mixed_arrow(d)
    plain = [("SUM", "v", "s"), ("COUNT", "v", "c"), ("AVG", "v", "a")]

    def aggs(s, with_new=True):
        out = [{"fn": fn, "expr": col(c, s), "name": name} for fn, c, name in plain]
        out.insert(2, TM.median_agg("mw", "w")(s))
        if with_new:      # interleaved, in declared order; one argument shared with the MEDIAN, one not
            out.insert(1, approx_agg("dv", "v")(s)); out.append(approx_agg("dw", "w")(s))
        return out
    got, node = TM.run_node(tc, t, ["k"], aggs)
    assert got.schema.names == ["k", "s", "dv", "c", "mw", "a", "dw"] and [f["name"] for f in node.schema()] == got.schema.names
    keys = [(d["k"], np.ones(d["n"], dtype=bool))]
    dv, dw = expected(keys, d["v"], d["v_ok"], "Int64", d["n"]), expected(keys, d["w"], d["w_ok"], "Float64", d["n"])
    assert by_key(got, 1, ["dv", "dw"]) == {key: (dv[key], dw[key]) for key in dv}
    mw = TM.expected_medians(keys, d["w"], d["w_ok"], "Float64", d["n"])
    rows = dict(zip(got.column("k").to_pylist(), TM.canon_column(got.column("mw"), "Float64")))
    assert rows == {key[0]: v for key, v in mw.items()}
    # the plain columns and the MEDIAN: what the same node without the new function returns
    ref, _ = TM.run_node(tc, t, ["k"], lambda s: aggs(s, False))
    names = ["s", "c", "mw", "a"]
    assert by_key(got, 1, names) == by_key(ref, 1, names) and [got.column(x).type for x in names] == [ref.column(x).type for x in names]
    # ungrouped, next to plain aggregates only
    got, _ = TM.run_node(tc, t, [], lambda s: [{"fn": "SUM", "expr": col("v", s), "name": "s"}, approx_agg("dv", "v")(s), {"fn": "COUNT", "expr": col("w", s), "name": "c"}])
    assert [c.to_pylist() for c in got.columns] == [[int(d["v"][d["v_ok"]].sum())], [H.approx_distinct(d["v"], "Int64", d["v_ok"])], [int(d["w_ok"].sum())]]


def test_fused_filter_and_computed_projection_below(tc):
    d = TM.mixed_table(34)

    def below(src):
        s = src.schema()
        proj = g.ProjectionExec([(col("k", s), "k"), (binary(binary(col("v", s), Op.Multiply, lit(2)), Op.Plus, col("f", s)), "x"), (col("f", s), "f")], src)
        return g.FilterExec(binary(col("f", proj.schema()), Op.Gt, lit(1, "Int32")), proj)
    got, _ = TM.run_node(tc, TM.mixed_arrow(d), ["k"], lambda s: [approx_agg("d", "x")(s), {"fn": "COUNT", "expr": col("x", s), "name": "c"}], below)
    sel = d["f"] > 1
    m = int(sel.sum())
    exp = expected([(d["k"][sel], np.ones(m, dtype=bool))], (d["v"] * 2 + d["f"])[sel], d["v_ok"][sel], "Int64", m)
    counts = {int(k): int((d["v_ok"] & sel & (d["k"] == k)).sum()) for k in np.unique(d["k"][sel])}
    assert by_key(got, 1, ["d", "c"]) == {key: (v, counts[key[0]]) for key, v in exp.items()}


def test_one_plan_handle_two_executions(tc):
    d = TM.mixed_table(35)
    src = g.MemoryExec([TM.mixed_arrow(d)])
    s = src.schema()
    flt = g.FilterExec(binary(col("f", s), Op.Lt, lit(8, "Int32")), src)
    agg = g.AggregateExec("Single", [(col("k", s), "k")], [approx_agg()(s), {"fn": "SUM", "expr": col("v", s), "name": "s"}], flt)
    plan = g.NativePlan(g.SortExec([{"expr": col("k", agg.schema()), "asc": True, "nulls_first": False}], agg), tc)
    sel = d["f"] < 8
    m = int(sel.sum())
    exp = expected([(d["k"][sel], np.ones(m, dtype=bool))], d["v"][sel], d["v_ok"][sel], "Int64", m)
    runs = [plan.execute(0).to_arrow() for _ in range(2)]
    assert runs[0].column("k").to_pylist() == sorted(key[0] for key in exp)
    assert runs[0].column("d").to_pylist() == [exp[(k,)] for k in runs[0].column("k").to_pylist()]
    assert runs[1].equals(runs[0])
    met = [x for x in plan.metrics() if x["node"] == "AggregateExec"][0]
    assert met["output_rows"] == 2 * len(exp) and met["elapsed_compute"] > 0


# ------------------------------------------------------------------------------------ at size
def test_fifty_thousand_values_ungrouped(tc):
    """200,000 rows, the library's own tile: several tiles, one segment, so every block stores a partial sketch and one block merges them."""
    r = np.random.default_rng(36)
    pool = r.integers(-2**62, 2**62, 50_000)
    vals = np.concatenate([pool, pool[r.integers(0, 50_000, 150_000)]])
    r.shuffle(vals)
    assert len(np.unique(vals)) == 50_000
    got, _ = TM.run_node(tc, pa.table({"v": pa.array(vals)}), [], lambda s: [approx_agg()(s)])
    e = H.approx_distinct(vals, "Int64")
    assert got.column("d").to_pylist() == [e] and abs(e - 50_000) <= 0.0325 * 50_000


def test_a_thousand_groups(tc):
    r = np.random.default_rng(37)
    n = 150_000
    k = r.integers(0, 1000, n).astype(np.int32)
    width = 1 + (np.arange(1000) * 399 // 999)      # group g draws from 1..400 different values
    vals = r.integers(0, 2**31, n) % width[k] + 1000 * k.astype(np.int64)
    got, _ = TM.run_node(tc, pa.table({"k": pa.array(k), "v": pa.array(vals)}), ["k"], lambda s: [approx_agg()(s)])
    order = np.argsort(k, kind="stable")
    cuts = np.flatnonzero(np.concatenate([[True], k[order][1:] != k[order][:-1]]))
    exp = {(int(k[order][a]),): (H.approx_distinct(x, "Int64"),) for a, x in zip(cuts, np.split(vals[order], cuts[1:]))}
    assert len(exp) == 1000 and by_key(got, 1, ["d"]) == exp
    exact = [len(np.unique(x)) for x in np.split(vals[order], cuts[1:])]
    assert min(exact) == 1 and max(exact) > 120


def test_known_answer_alltypes_plain(tc):
    """ballista/client/src/context.rs:817-829: approx_distinct(id) = 8."""
    with pa.ipc.open_file(os.path.join(os.path.dirname(__file__), "golden", "alltypes_plain.arrow")) as f:
        t = f.read_all().select(["id", "bigint_col"])
    got, _ = TM.run_node(tc, t, [], lambda s: [approx_agg("d", "id")(s)])
    assert got.column("d").to_pylist() == [8]


# ------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_function(tc):
    d = TM.mixed_table(9, n=200)
    t = TM.mixed_arrow(d).append_column("name", pa.array(["twenty bytes of name %02d" % (i % 7) for i in range(200)]))
    src = g.MemoryExec([t])
    s = src.schema()
    with pytest.raises(g.GpuqError, match="APPROX_DISTINCT.*Final"):
        g.AggregateExec("Final", [(col("k", s), "k")], [approx_agg()(s)], src).execute(0, tc)
    with pytest.raises(g.GpuqError, match="APPROX_DISTINCT.*Float64 group key"):
        g.AggregateExec("Single", [(col("w", s), "w")], [approx_agg()(s)], src).execute(0, tc)
    with pytest.raises(g.GpuqError, match="APPROX_DISTINCT.*group key.*longer than 15 bytes"):
        g.AggregateExec("Single", [(col("name", s), "name")], [approx_agg()(s)], src).execute(0, tc)
    with pytest.raises(g.GpuqError, match="APPROX_DISTINCT.*argument.*longer than 15 bytes"):
        g.AggregateExec("Single", [(col("k", s), "k")], [approx_agg("d", "name")(s)], src).execute(0, tc)
    with pytest.raises(g.GpuqError, match="APPROX_DISTINCT"):
        g.AggregateExec("Single", [(col("k", s), "k")], [approx_agg(distinct=True)(s)], src).execute(0, tc)
