"""BoundedWindowAggExec through the native executor (MemoryExec -> SortExec -> BoundedWindowAggExec unless noted) against
tests/window_exact.py, the row-by-row restatement that tests/test_cpu_window.py pins on a table with known answers.  Integers, decimals,
ranks and LAG / LEAD are compared exactly (floats by bit pattern); float sums against the exact rational with the any-order bound
(k - 1) u sum|x| of tests/float_agg_exact.py, u = 2^-53, which is derived, not measured.

The node keeps its input's order, and ties of (partition_by, order_by) may come out of the sort in any order, so every table carries a
row id `i` that is the sort's last key: the restatement then walks the node's own output columns, after they were checked to be the
input's rows."""
import ctypes as C
import decimal
import struct
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd import binding as B
from arrow_ballista_amd import expr as E
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit

import window_exact as W

pytestmark = pytest.mark.gpu

CTX = decimal.Context(prec=60)
DEC = pa.decimal128(38, 4)
SIZES = [1, 254, 1, 1, 2, 3, 63, 64, 65, 255, 256, 257, 825, 1, 1, 5000, 10, 9, 10, 11, 12, 1]      # tests/test_gpu_median.py's


# ------------------------------------------------------------------------------------ tables and results
def dec_array(vals, typ=DEC):
    return pa.array([None if v is None else decimal.Decimal(int(v)).scaleb(-typ.scale, CTX) for v in vals], typ)


def canon(c):
    """a result column as exactly comparable Python values: ints; decimals as unscaled ints (read from the buffer: a wrapped sum may hold
    more than 38 digits); dates and timestamps as their counts; floats as ("bits", pattern)"""
    c = c.combine_chunks() if isinstance(c, pa.ChunkedArray) else c
    ok = c.is_valid().to_pylist()
    t = c.type
    if pa.types.is_decimal(t):
        w = np.frombuffer(c.buffers()[1], dtype=np.uint64, count=2 * (c.offset + len(c)))[2 * c.offset:]
        return [W.wrap(int(w[2 * i]) | int(w[2 * i + 1]) << 64, 128) if o else None for i, o in enumerate(ok)]
    if pa.types.is_floating(t):
        v = c.fill_null(0).to_numpy(zero_copy_only=False)
        bits = v.view(np.uint64 if t == pa.float64() else np.uint32)
        return [("bits", int(b)) if o else None for b, o in zip(bits, ok)]
    if pa.types.is_date32(t):
        return c.cast(pa.int32()).to_pylist()
    if pa.types.is_timestamp(t):
        return c.cast(pa.int64()).to_pylist()
    return c.to_pylist()


def floats(c):
    c = c.combine_chunks() if isinstance(c, pa.ChunkedArray) else c
    return [None if x is None else float(x) for x in c.to_pylist()]


def sort_keys(names):
    return [E.sort_expr(col(n)) for n in names]


def run(tc, table, wexprs, partition_by=(), order_by=(), sort=True, below=None, plan_only=False):
    """the plan's output table.  The SortExec orders by (partition_by, order_by, i)."""
    src = g.MemoryExec([table])
    inp = below(src) if below else src
    if sort:
        inp = g.SortExec(sort_keys(list(partition_by) + list(order_by) + ["i"]), inp)
    node = g.BoundedWindowAggExec(inp, wexprs)
    if plan_only:
        return node
    return g.NativePlan(node, tc).execute(0).to_arrow()


def over(partition_by=(), order_by=()):
    return dict(partition_by=[col(c) for c in partition_by], order_by=sort_keys(order_by))


def passthrough(got, table, names):
    """the node's input columns as the restatement's table {name: canonical values}, checked to be `table`'s rows in the order the
    row ids say"""
    ids = got.column("i").to_pylist()
    assert sorted(ids) == list(range(table.num_rows))
    at = {i: j for j, i in enumerate(table.column("i").to_pylist())}      # row id -> its place in `table`
    out = {}
    for nm in names:
        src = canon(table.column(nm))
        out[nm] = canon(got.column(nm))
        assert out[nm] == [src[at[i]] for i in ids], nm
    return out


def check_sorted(t, partition_by, order_by):
    """the input really is ordered as the node's mode promises: NULLs last, ascending"""
    key = lambda r: tuple((x is None, x) for x in r)
    rows = list(zip(*[t[c] for c in list(partition_by) + list(order_by) + ["i"]]))
    assert all(key(a) <= key(b) for a, b in zip(rows, rows[1:]))


# ------------------------------------------------------------------------------------ the segment shapes, shared
@pytest.fixture(scope="module")
def shapes():
    r = np.random.default_rng(7)
    ids = np.repeat(np.arange(len(SIZES)), SIZES)
    n = len(ids)
    heads = np.concatenate([[0], np.cumsum(SIZES)[:-1]])
    assert {255, 256, 257, 2047, 2048, 2049} <= set(heads.tolist())      # heads on both sides of a 256-row block edge and a 2,048-row tile edge
    assert heads[15] == 2049 and SIZES[15] == 5000                          # rows [2049, 7049): the tiles [2048, 4096) .. [6144, 8192), two of them without a head
    assert SIZES[0] == 1 and SIZES[-1] == 1
    pos = np.arange(n) - heads[ids]
    o = (pos + 1) // 5                                                      # peer groups of five rows
    v = r.integers(-10 ** 12, 10 ** 12, n)
    vok = r.random(n) > 0.1
    vok[ids == 16] = False                                                  # an all-NULL partition
    d = [int(x) if ok else None for x, ok in zip(r.integers(-10 ** 15, 10 ** 15, n), r.random(n) > 0.1)]
    perm = r.permutation(n)                                                 # the sort below has work to do; i = the row's place in sorted order
    t = pa.table({"k": pa.array((ids * 7 - 30).astype(np.int32)), "o": pa.array(o.astype(np.int64)), "i": pa.array(np.arange(n, dtype=np.int64)),
                  "v": pa.array(v, pa.int64(), mask=~vok), "d": dec_array(d)})
    return t.take(pa.array(perm)), n


def test_segment_shapes_in_one_table(tc, shapes):
    t, n = shapes
    ov = over(["k"], ["o"])
    w = [E.window("ROW_NUMBER", [], "rn", **ov), E.window("RANK", [], "rk", **ov), E.window("DENSE_RANK", [], "dr", **ov),
         E.lag(col("v"), "lag1", **ov), E.lead(col("v"), "lead2", 2, lit(-7), **ov), E.lag(col("d"), "lagd", 70, **ov)]
    for fn in ("COUNT", "SUM", "MIN", "MAX", "AVG"):
        for c in ("v", "d"):
            w.append(E.window(fn, [col(c)], "%s_%s_range" % (fn, c), **ov))                                    # the default frame
            w.append(E.window(fn, [col(c)], "%s_%s_rows" % (fn, c), frame=E.rows_between(None, 0), **ov))
    got = run(tc, t, w, ["k"], ["o"])
    assert got.num_rows == n and got.schema.names[:5] == ["k", "o", "i", "v", "d"]
    tab = passthrough(got, t, ["k", "o", "i", "v", "d"])
    check_sorted(tab, ["k"], ["o"])
    x = W.Walk(tab, ["k"], ["o"])
    # ties straddle a block edge and a tile edge, and the long partition crosses two whole tiles
    assert all(x.qs[e] < e < x.qe[e] for e in (2560, 4096))
    assert x.ps[4096] == x.ps[6144] == 2049 and x.pe[6144] == 7049
    assert canon(got["rn"]) == x.row_number() and canon(got["rk"]) == x.rank() and canon(got["dr"]) == x.dense_rank()
    assert canon(got["lag1"]) == x.shift("v", -1) and canon(got["lead2"]) == x.shift("v", 2, -7) and canon(got["lagd"]) == x.shift("d", -70)
    for fr in ("range", "rows"):
        for c, bits, digits in (("v", 64, None), ("d", 128, 4)):
            assert canon(got["COUNT_%s_%s" % (c, fr)]) == x.count(c, fr), (c, fr)
            assert canon(got["SUM_%s_%s" % (c, fr)]) == x.sum(c, fr, bits), (c, fr)
            assert canon(got["MIN_%s_%s" % (c, fr)]) == x.minmax(c, True, fr), (c, fr)
            assert canon(got["MAX_%s_%s" % (c, fr)]) == x.minmax(c, False, fr), (c, fr)
        assert canon(got["AVG_d_" + fr]) == x.avg_decimal("d", fr, 4), fr
        check_int_avg(floats(got["AVG_v_" + fr]), x.sum_exact("v", fr))
    assert canon(got["SUM_v_range"])[-1] == tab["v"][-1] and x.ps[0] == 0 and x.pe[0] == 1      # the first and the last partition: one row


def check_int_avg(got, exact):
    """within 3 u |AVG| of the exact quotient: one rounding of the sum's conversion, one of the division"""
    for i, (a, e) in enumerate(zip(got, exact)):
        if e is None:
            assert a is None, i
            continue
        q = e[0] / e[2]
        assert a is not None and abs(Fraction(a) - q) <= 3 * W.U * abs(q), (i, a, float(q))


@pytest.mark.parametrize("k,m", [(0, 0), (1, 0), (3, 2), (None, 1), (70, 70), (10 ** 6, 10 ** 6)], ids=str)
def test_sliding_rows_frames(tc, shapes, k, m):
    t, n = shapes
    ov = over(["k"], ["o"])
    fr = E.window_frame("ROWS", E.frame_bound("PRECEDING", k), E.frame_bound("FOLLOWING", m) if m else E.frame_bound("CURRENT_ROW"))
    w = [E.window(fn, [col(c)], fn + c, frame=fr, **ov) for fn in ("SUM", "COUNT", "AVG") for c in ("v", "d")]
    got = run(tc, t, w, ["k"], ["o"])
    x = W.Walk(passthrough(got, t, ["k", "o", "i", "v", "d"]), ["k"], ["o"])
    assert canon(got["SUMv"]) == x.sum("v", (k, m), 64) and canon(got["SUMd"]) == x.sum("d", (k, m), 128)
    assert canon(got["COUNTv"]) == x.count("v", (k, m)) and canon(got["COUNTd"]) == x.count("d", (k, m))
    assert canon(got["AVGd"]) == x.avg_decimal("d", (k, m), 4)
    check_int_avg(floats(got["AVGv"]), x.sum_exact("v", (k, m)))


# ------------------------------------------------------------------------------------ small shapes
ALL_FNS = lambda ov: [E.window("ROW_NUMBER", [], "rn", **ov), E.window("RANK", [], "rk", **ov), E.window("DENSE_RANK", [], "dr", **ov), E.lag(col("v"), "lag", **ov),
                      E.lead(col("v"), "lead", 1, lit(0), **ov), E.window("COUNT", [col("v")], "c", **ov), E.window("SUM", [col("v")], "s", **ov),
                      E.window("SUM", [col("v")], "sr", frame=E.rows_between(None, 0), **ov), E.window("MIN", [col("v")], "mn", **ov),
                      E.window("MAX", [col("v")], "mx", frame=E.rows_between(None, 0), **ov), E.window("SUM", [col("v")], "sl", frame=E.rows_between(1, 1), **ov)]


def check_all_fns(got, x):
    assert canon(got["rn"]) == x.row_number() and canon(got["rk"]) == x.rank() and canon(got["dr"]) == x.dense_rank()
    assert canon(got["lag"]) == x.shift("v", -1) and canon(got["lead"]) == x.shift("v", 1, 0)
    assert canon(got["c"]) == x.count("v") and canon(got["s"]) == x.sum("v") and canon(got["sr"]) == x.sum("v", "rows")
    assert canon(got["mn"]) == x.minmax("v", True) and canon(got["mx"]) == x.minmax("v", False, "rows") and canon(got["sl"]) == x.sum("v", (1, 1))


def small_table(n, keys, seed=3):
    r = np.random.default_rng(seed)
    return pa.table({"k": pa.array(np.asarray(keys(n), dtype=np.int32)), "o": pa.array(r.integers(0, 4, n), pa.int64()), "i": pa.array(np.arange(n, dtype=np.int64)),
                     "v": pa.array(r.integers(-99, 99, n), pa.int64(), mask=r.random(n) < 0.2)})


@pytest.mark.parametrize("shape", ["n=0", "n=1", "one partition", "every row its own partition", "no partition_by", "no order_by", "neither"])
def test_small_shapes(tc, shape):
    n = {"n=0": 0, "n=1": 1}.get(shape, 300)
    keys = {"one partition": lambda n: np.zeros(n), "every row its own partition": lambda n: np.arange(n)}.get(shape, lambda n: np.arange(n) % 7)
    pb = [] if shape in ("no partition_by", "neither") else ["k"]
    ob = [] if shape in ("no order_by", "neither") else ["o"]
    t = small_table(n, keys)
    got = run(tc, t, ALL_FNS(over(pb, ob)), pb, ob)
    assert got.num_rows == n
    tab = passthrough(got, t, ["k", "o", "i", "v"])
    check_sorted(tab, pb, ob)
    check_all_fns(got, W.Walk(tab, pb, ob))


# ------------------------------------------------------------------------------------ NULLs
def test_nulls_in_arguments_and_keys(tc):
    """leading NULL arguments (NULL until the first value, COUNT 0), an all-NULL partition, NULL partition keys (one partition, sorted last),
    NULL order keys (peers of each other)"""
    k = [1] * 6 + [2] * 4 + [None] * 5 + [3] * 3
    o = [1, 1, 2, None, None, None, 1, 2, 3, 4, 5, 5, None, None, 6, 1, 2, 3]
    v = [None, None, 4, 5, None, 6, None, None, None, None, None, 7, 8, None, 9, 1, None, 2]
    n = len(k)
    t = pa.table({"k": pa.array(k, pa.int32()), "o": pa.array(o, pa.int64()), "i": pa.array(np.arange(n, dtype=np.int64)), "v": pa.array(v, pa.int64())})
    t = t.take(pa.array(np.random.default_rng(2).permutation(n)))
    ov = over(["k"], ["o"])
    got = run(tc, t, ALL_FNS(ov) + [E.window("AVG", [col("v")], "a", **ov)], ["k"], ["o"])
    tab = passthrough(got, t, ["k", "o", "i", "v"])
    check_sorted(tab, ["k"], ["o"])
    assert tab["k"] == sorted(x for x in k if x is not None) + [None] * 5
    x = W.Walk(tab, ["k"], ["o"])
    check_all_fns(got, x)
    s, c = canon(got["s"]), canon(got["c"])
    assert s[:2] == [None, None] and c[:2] == [0, 0] and canon(got["a"])[:2] == [None, None]      # before the first value
    assert s[6:10] == [None] * 4 and c[6:10] == [0] * 4 and canon(got["mn"])[6:10] == [None] * 4      # the all-NULL partition
    assert canon(got["rk"])[3:6] == [4, 4, 4] and canon(got["rn"])[10:18] == [1, 2, 3, 1, 2, 3, 4, 5]      # NULL order keys are peers; NULL keys one partition, the last
    check_int_avg(floats(got["a"]), x.sum_exact("v"))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_validity_words_of_the_result(tc, n):
    """every third argument NULL, three rows a partition: validity words that are neither all ones nor zero, a partial last word"""
    t = pa.table({"k": pa.array((np.arange(n) // 3).astype(np.int32)), "o": pa.array(np.arange(n, dtype=np.int64)), "i": pa.array(np.arange(n, dtype=np.int64)),
                  "v": pa.array(np.arange(n, dtype=np.int64) * 11 - 50, mask=np.arange(n) % 3 == 0)})
    got = run(tc, t, ALL_FNS(over(["k"], ["o"])), ["k"], ["o"])
    x = W.Walk(passthrough(got, t, ["k", "o", "i", "v"]), ["k"], ["o"])
    check_all_fns(got, x)
    assert canon(got["sr"])[0] is None and (n < 2 or canon(got["sr"])[1] is not None)


# ------------------------------------------------------------------------------------ argument types
I64MAX = 2 ** 63 - 1
TYPED = {
    "Int8": (pa.int8(), [-128, 127, 0, None, -1, 5, 5, 100]), "Int16": (pa.int16(), [-32768, 32767, None, 0, 7, -9, 300, 2]),
    "Int32": (pa.int32(), [-2 ** 31, 2 ** 31 - 1, 0, None, 12, -40, 40, 1]), "Int64": (pa.int64(), [-2 ** 63, I64MAX, None, 0, -1, 1, 10 ** 18, -10 ** 18]),
    "UInt8": (pa.uint8(), [0, 255, None, 128, 127, 1, 200, 3]), "UInt16": (pa.uint16(), [0, 65535, 32768, None, 5, 9, 1, 40000]),
    "UInt32": (pa.uint32(), [0, 2 ** 32 - 1, 2 ** 31, None, 1, 7, 2 ** 31 - 1, 9]), "UInt64": (pa.uint64(), [0, I64MAX, None, 5, 2 ** 62, 1, 77, 2]),
    "Float32": (pa.float32(), [0.0, -0.0, None, 1.5, -3.25, float("inf"), float("-inf"), 1e-30]),
    "Float64": (pa.float64(), [0.0, -0.0, None, 1.5, -3.25, float("inf"), float("-inf"), 1e-300]),
    "Decimal128(38,4)": (DEC, [0, -1, None, 10 ** 18, -10 ** 18, 5, I64MAX, -2 ** 63]),
    "Date32": (pa.date32(), [0, -719162, None, 19000, 1, 2, 40000, -5]), "Timestamp": (pa.timestamp("us"), [0, -10 ** 15, None, 10 ** 15, 1, 2, 3, -4]),
}


def typed_array(typ, vals):
    if pa.types.is_decimal(typ):
        return dec_array(vals, typ)
    if pa.types.is_date32(typ):
        return pa.array(vals, pa.int32()).cast(typ)
    if pa.types.is_timestamp(typ):
        return pa.array(vals, pa.int64()).cast(typ)
    return pa.array(vals, typ)


def total_key_of(typ):
    if not pa.types.is_floating(typ):
        return lambda x: x
    width = 64 if typ == pa.float64() else 32

    def key(x):      # x = ("bits", pattern): IEEE totalOrder
        s = W.wrap(x[1], width)
        return s ^ ((s >> (width - 1)) & ((1 << (width - 1)) - 1))
    return key


@pytest.mark.parametrize("tname", sorted(TYPED))
def test_every_argument_type_through_lag_lead_min_max(tc, tname):
    typ, vals = TYPED[tname]
    vals = vals * 3      # three partitions of eight rows, the same values in another place of the order
    n = len(vals)
    t = pa.table({"k": pa.array((np.arange(n) % 3).astype(np.int32)), "i": pa.array(np.arange(n, dtype=np.int64)), "v": typed_array(typ, vals)})
    ov = over(["k"], ["i"])
    w = [E.lag(col("v"), "lag", 2, **ov), E.lead(col("v"), "lead", 1, **ov), E.window("MIN", [col("v")], "mn", **ov), E.window("MAX", [col("v")], "mx", frame=E.rows_between(None, 0), **ov),
         E.window("COUNT", [col("v")], "c", **ov)]
    got = run(tc, t, w, ["k"], [])
    for c in ("lag", "lead", "mn", "mx"):
        assert got[c].type == typ, (c, got[c].type)
    x = W.Walk(passthrough(got, t, ["k", "i", "v"]), ["k"], ["i"])
    key = total_key_of(typ)
    assert canon(got["lag"]) == x.shift("v", -2) and canon(got["lead"]) == x.shift("v", 1) and canon(got["c"]) == x.count("v")
    assert canon(got["mn"]) == x.minmax("v", True, key=key) and canon(got["mx"]) == x.minmax("v", False, "rows", key=key)


def test_int64_sum_wraps_and_decimal_sum_holds_10_to_the_37(tc):
    big = 10 ** 37
    v = [I64MAX, 1, -5, None, -2 ** 63, -2 ** 63, 7, I64MAX]
    d = [big, big, big, None, 9 * big, 9 * big, -big, 3]      # 2.1e38 > 2^127: the running sum wraps at 128 bits
    n = len(v)
    t = pa.table({"k": pa.array(np.zeros(n, np.int32)), "i": pa.array(np.arange(n, dtype=np.int64)), "v": pa.array(v, pa.int64()), "d": dec_array(d)})
    ov = over(["k"], ["i"])
    got = run(tc, t, [E.window("SUM", [col("v")], "sv", **ov), E.window("SUM", [col("d")], "sd", frame=E.rows_between(None, 0), **ov),
                      E.window("SUM", [col("v")], "sl", frame=E.rows_between(1, 0), **ov), E.window("SUM", [col("d")], "sdl", frame=E.rows_between(2, 1), **ov)], ["k"], ["i"])
    x = W.Walk(passthrough(got, t, ["k", "i", "v", "d"]), ["k"], ["i"])
    want = x.sum("v")
    assert want[1] == -2 ** 63 and want[4] == -5 and want[5] == 2 ** 63 - 5 and canon(got["sv"]) == want      # crossed +2^63, then -2^63
    wd = x.sum("d", "rows", 128)
    assert abs(sum(e for e in d[:6] if e)) > 2 ** 127 and canon(got["sd"]) == wd
    assert canon(got["sl"]) == x.sum("v", (1, 0)) and canon(got["sdl"]) == x.sum("d", (2, 1), 128)


def test_min_max_operands_outside_int64_are_refused_as_the_aggregate_refuses_them(tc):
    """the accumulator cell of MIN / MAX holds 64 bits: a UInt64 above 2^63 - 1 and a Decimal128 beyond int64 are refused, by name"""
    n = 5
    base = {"k": pa.array(np.zeros(n, np.int32)), "i": pa.array(np.arange(n, dtype=np.int64))}
    for arr, fn in ((pa.array([1, 2, 2 ** 63 + 5, 3, 4], pa.uint64()), "MAX"), (dec_array([1, -2 ** 64, 3, 4, 5]), "MIN")):
        t = pa.table(dict(base, v=arr))
        with pytest.raises(g.GpuqError, match=fn + ".*outside int64") as e:
            run(tc, t, [E.window(fn, [col("v")], "m", **over(["k"], ["i"]))], ["k"], ["i"])
        assert e.value.status == 3
        # LAG moves the same values as bytes
        got = run(tc, t, [E.lag(col("v"), "l", **over(["k"], ["i"]))], ["k"], ["i"])
        assert canon(got["l"]) == [None] + canon(arr)[:-1]


# ------------------------------------------------------------------------------------ LAG / LEAD
def test_lag_lead_offsets_and_defaults(tc):
    sizes = [1, 63, 64, 65, 130, 2, 200]
    ids = np.repeat(np.arange(len(sizes)), sizes)
    n = len(ids)
    r = np.random.default_rng(4)
    t = pa.table({"k": pa.array(ids.astype(np.int32)), "i": pa.array(np.arange(n, dtype=np.int64)), "v": pa.array(r.integers(-1000, 1000, n), pa.int32(), mask=r.random(n) < 0.25)})
    ov = over(["k"], ["i"])
    w = []
    for off in (0, 1, 2, 63, 64, 65, 10 ** 9, 2 ** 40):
        w += [E.lag(col("v"), "lag%d" % off, off, **ov), E.lead(col("v"), "lead%d" % off, off, lit(-1, "Int32"), **ov)]
    w += [E.lag(col("v"), "lagd", 1, lit(12345, "Int32"), **ov), E.lead(col("v"), "leadn", 64, **ov), E.window("LAG", [col("v")], "lag_default_offset", **ov)]
    got = run(tc, t, w, ["k"], ["i"])
    x = W.Walk(passthrough(got, t, ["k", "i", "v"]), ["k"], ["i"])
    for off in (0, 1, 2, 63, 64, 65, 10 ** 9, 2 ** 40):
        assert canon(got["lag%d" % off]) == x.shift("v", -off), off
        assert canon(got["lead%d" % off]) == x.shift("v", off, -1), off
    assert canon(got["lagd"]) == x.shift("v", -1, 12345) and canon(got["leadn"]) == x.shift("v", 64) and canon(got["lag_default_offset"]) == x.shift("v", -1)
    lag1 = canon(got["lag1"])
    assert any(lag1[i] is None and x.ps[i] < i for i in range(n))      # a NULL value carried as a value, inside a partition


# ------------------------------------------------------------------------------------ floats
def check_float_sum(got, exact, avg=False):
    for i, (a, e) in enumerate(zip(got, exact)):
        if e is None:
            assert a is None, i
            continue
        total, mag, k = e
        bound = (k - 1) * W.U * mag
        if avg:
            bound = bound / k + W.U * abs(total / k)
            total = total / k
        assert a is not None and abs(Fraction(a) - total) <= bound, (i, a, float(total), float(bound))


@pytest.mark.parametrize("typ", [pa.float64(), pa.float32()], ids=str)
def test_float_sums_against_exact_rationals_and_bitwise_reproducible(tc, typ):
    r = np.random.default_rng(11)
    sizes = [1, 300, 2500, 3, 2048, 700]      # partitions inside one tile, across tiles, and one that is a tile
    ids = np.repeat(np.arange(len(sizes)), sizes)
    n = len(ids)
    v = (r.standard_normal(n) * 10.0 ** r.integers(-3, 9, n)).astype(np.float64 if typ == pa.float64() else np.float32)
    t = pa.table({"k": pa.array(ids.astype(np.int32)), "o": pa.array(np.arange(n, dtype=np.int64) // 4), "i": pa.array(np.arange(n, dtype=np.int64)),
                  "v": pa.array(v, typ, mask=r.random(n) < 0.05)})
    ov = over(["k"], ["o"])
    node = run(tc, t, [E.window("SUM", [col("v")], "s", **ov), E.window("SUM", [col("v")], "sr", frame=E.rows_between(None, 0), **ov), E.window("AVG", [col("v")], "a", **ov),
                       E.window("AVG", [col("v")], "ar", frame=E.rows_between(None, 0), **ov)], ["k"], ["o"], plan_only=True)
    plan = g.NativePlan(node, tc)
    got = plan.execute(0).to_arrow()
    assert got["s"].type == pa.float64() and got["a"].type == pa.float64()      # a Float32 argument sums in Float64
    ids_out = got["i"].to_pylist()
    src = floats(t["v"])
    x = W.Walk({"k": got["k"].to_pylist(), "o": got["o"].to_pylist(), "v": [src[i] for i in ids_out]}, ["k"], ["o"])
    check_float_sum(floats(got["s"]), x.sum_exact("v", "range"))
    check_float_sum(floats(got["sr"]), x.sum_exact("v", "rows"))
    check_float_sum(floats(got["a"]), x.sum_exact("v", "range"), avg=True)
    check_float_sum(floats(got["ar"]), x.sum_exact("v", "rows"), avg=True)
    again = plan.execute(0).to_arrow()      # the order of combination is fixed: the same bits
    for c in ("s", "sr", "a", "ar"):
        assert canon(again[c]) == canon(got[c]), c


# ------------------------------------------------------------------------------------ the scan beyond one step of its middle launch
def np_column(c):
    """(values with 0 under NULL, validity) as numpy arrays"""
    c = c.combine_chunks() if isinstance(c, pa.ChunkedArray) else c
    return c.fill_null(0).to_numpy(zero_copy_only=False), c.is_valid().to_numpy(zero_copy_only=False)


def numpy_reference(sizes, heads, pos, v, vok, f, fok, preceding, following):
    """{column: values}, {column: validity} of the test below, per partition with numpy: s / c / mn / sf over ROWS UNBOUNDED PRECEDING ..
    CURRENT ROW, mx / sr over the default RANGE frame (peer groups of three rows), sl over ROWS preceding PRECEDING .. following FOLLOWING"""
    n = sum(sizes)
    big = np.iinfo(np.int64)
    want = {c: np.zeros(n, np.float64 if c == "sf" else np.int64) for c in ("s", "c", "mn", "mx", "sf", "sr", "sl")}
    has = {c: np.zeros(n, bool) for c in want}
    for a, size in zip(heads, sizes):
        b = a + size
        x, ok = np.where(vok[a:b], v[a:b], 0), vok[a:b]
        P, Cn = np.cumsum(x), np.cumsum(ok)
        want["s"][a:b], want["c"][a:b] = P, Cn
        want["mn"][a:b] = np.minimum.accumulate(np.where(ok, v[a:b], big.max))
        last_peer = np.minimum((pos[a:b] // 3 + 1) * 3, size) - 1      # RANGE: up to the row's last peer
        want["mx"][a:b] = np.maximum.accumulate(np.where(ok, v[a:b], big.min))[last_peer]
        want["sr"][a:b] = P[last_peer]
        for c in ("s", "mn"):
            has[c][a:b] = Cn > 0
        has["mx"][a:b] = has["sr"][a:b] = Cn[last_peer] > 0
        want["sf"][a:b] = np.cumsum(np.where(fok[a:b], f[a:b], 0.0)); has["sf"][a:b] = np.cumsum(fok[a:b]) > 0
        P0, C0 = np.concatenate([[0], P]), np.concatenate([[0], Cn])      # P0[j] = the sum of rows [0, j)
        hi, lo = np.minimum(np.arange(size) + following, size - 1) + 1, np.maximum(np.arange(size) - preceding, 0)
        want["sl"][a:b] = P0[hi] - P0[lo]; has["sl"][a:b] = C0[hi] - C0[lo] > 0
    has["c"][:] = True
    return want, has


@pytest.mark.parametrize("sizes", [[300_000], [3, 140_000, 1, 2_101_234, 50_000, 7]], ids=["147 tiles, one partition", "1,119 tiles, six partitions"])
def test_whole_columns_across_the_waves_and_steps_of_the_tile_scan(tc, sizes):
    """The one block over the tile totals gives each of its 16 waves a contiguous share of the tiles and walks it 64 tiles a step: more
    than 64 tiles (131,072 rows) bring a second wave and the carry between waves in, more than 1,024 tiles (2,097,152 rows) a second step
    and the carry between steps.  Partitions longer than 64 tiles, and one longer than 1,024, so that those carries reach the answers;
    heads off every tile edge.  Every row of every column is compared: integers against numpy's wrapping cumsum / running minimum per
    partition, Float64 sums over whole-numbered values (exact in any order, but not in a wrong one) bit for bit."""
    r = np.random.default_rng(len(sizes))
    n = sum(sizes)
    heads = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    assert n > 131_072 and (len(sizes) == 1 or (n > 2_097_152 and max(sizes) > 2_097_152 and all(h % 2048 for h in heads[1:])))
    ids = np.repeat(np.arange(len(sizes)), sizes)
    pos = np.arange(n) - heads[ids]
    v, vok = r.integers(-10 ** 12, 10 ** 12, n), r.random(n) > 0.1
    f, fok = r.integers(-1000, 1000, n).astype(np.float64), r.random(n) > 0.1
    vok[heads] = False      # every partition starts with a NULL: no value before the first one
    t = pa.table({"k": pa.array(ids.astype(np.int32)), "o": pa.array(pos // 3), "v": pa.array(v, pa.int64(), mask=~vok), "f": pa.array(f, pa.float64(), mask=~fok)})
    ov = over(["k"], ["o"])
    rows = E.rows_between(None, 0)
    w = [E.window("SUM", [col("v")], "s", frame=rows, **ov), E.window("COUNT", [col("v")], "c", frame=rows, **ov), E.window("MIN", [col("v")], "mn", frame=rows, **ov),
         E.window("MAX", [col("v")], "mx", **ov), E.window("SUM", [col("f")], "sf", frame=rows, **ov), E.window("SUM", [col("v")], "sr", **ov),
         E.window("SUM", [col("v")], "sl", frame=E.rows_between(100_000, 5), **ov), E.window("ROW_NUMBER", [], "rn", **ov)]
    got = g.NativePlan(g.BoundedWindowAggExec(g.MemoryExec([t]), w), tc).execute(0).to_arrow()      # (already in order: no SortExec)
    assert got.num_rows == n
    want, has = numpy_reference(sizes, heads, pos, v, vok, f, fok, 100_000, 5)
    assert np.array_equal(got["rn"].to_numpy(), pos.astype(np.uint64) + 1)
    for c in want:
        vals, ok = np_column(got[c])
        assert np.array_equal(ok, has[c]), c
        w_ = np.where(has[c], want[c], 0)
        assert np.array_equal(vals.view(np.int64), w_.view(np.int64)), (c, int(np.flatnonzero(vals.view(np.int64) != w_.view(np.int64))[0]))


def test_2_to_the_31_rows_are_refused_by_every_entry_point(tc):
    """2^31 rows or more in a partition of the plan: the node makes the same test on its input's row count, and each of the four entry
    points it runs on refuses the count before it looks at a pointer -- status 3, refusal kind NONE, the node and the limit named"""
    L, ctx, stream = B.lib(), tc.ctx.h, tc.stream_ptr()
    n = 2 ** 31
    column = B.gpuq_column()
    column.type, column.length = B.T_INT64, n
    spec = (C.c_byte * 256)()      # a zeroed gpuq_window_frame_spec
    calls = {"gpuq_window_scan": lambda: L.gpuq_window_scan(ctx, stream, C.byref(column), None, n, 0, None, 8, None, None, None),
             "gpuq_window_rank": lambda: L.gpuq_window_rank(ctx, stream, None, None, None, None, n, None, None, None),
             "gpuq_window_shift": lambda: L.gpuq_window_shift(ctx, stream, C.byref(column), None, None, n, -1, None, None, None),
             "gpuq_window_frame": lambda: L.gpuq_window_frame(ctx, stream, spec, n)}
    for name, call in calls.items():
        with pytest.raises(g.GpuqError, match=name + r" \(BoundedWindowAggExec\): >= 2\^31 rows in one partition of the plan") as e:
            tc.ctx.check(call())
        assert e.value.status == 3 and e.value.refusal == B.REFUSAL_NONE, name
        assert tc.ctx.L.gpuq_window_rank(ctx, stream, None, None, None, None, 0, None, None, None) == 0      # the context goes on


# ------------------------------------------------------------------------------------ the node as a citizen of a plan
LONG = "a payload string well beyond fifteen bytes #%d"


def test_through_views_with_a_utf8_partition_key(tc):
    """the input is a hash join's output over a filter: index vectors, not dense columns.  The Utf8 partition key (<= 15 bytes) packs; the
    payload strings beyond 15 bytes travel through untouched."""
    r = np.random.default_rng(5)
    n = 3000
    fact = pa.table({"i": pa.array(np.arange(n, dtype=np.int64)), "k": pa.array(r.integers(0, 12, n), pa.int32()), "v": pa.array(r.integers(-50, 50, n), pa.int64(), mask=r.random(n) < 0.1),
                     "long": pa.array([LONG % j for j in range(n)])})
    dim = pa.table({"k2": pa.array(np.arange(10, dtype=np.int32)), "nm": pa.array(["name-%02d" % (j % 4) for j in range(10)])})      # 4 names over 10 keys; keys 10, 11 join nothing
    fsrc, dsrc = g.MemoryExec([fact]), g.MemoryExec([dim])
    flt = g.FilterExec(binary(col("v", fsrc.schema()), Op.Gt, lit(-20)), fsrc)
    join = g.HashJoinExec(dsrc, flt, [(col("k2", dsrc.schema()), col("k", fsrc.schema()))], None, "Inner", "CollectLeft", False)
    ov = over(["nm"], ["i"])
    node = g.BoundedWindowAggExec(g.SortExec(sort_keys(["nm", "i"]), join), [E.window("ROW_NUMBER", [], "rn", **ov), E.window("SUM", [col("v")], "s", frame=E.rows_between(None, 0), **ov),
                                                                               E.lag(col("v"), "l", **ov), E.window("COUNT", [col("long")], "cl", **ov)])
    got = g.NativePlan(node, tc).execute(0).to_arrow()
    keep = [j for j in range(n) if fact["v"][j].as_py() is not None and fact["v"][j].as_py() > -20 and fact["k"][j].as_py() < 10]
    assert sorted(got["i"].to_pylist()) == keep
    assert got["long"].to_pylist() == [LONG % j for j in got["i"].to_pylist()]
    assert got["nm"].to_pylist() == ["name-%02d" % (fact["k"][j].as_py() % 4) for j in got["i"].to_pylist()]
    tab = {"nm": got["nm"].to_pylist(), "i": got["i"].to_pylist(), "v": got["v"].to_pylist(), "long": got["long"].to_pylist()}
    check_sorted(tab, ["nm"], [])
    x = W.Walk(tab, ["nm"], ["i"])
    assert canon(got["rn"]) == x.row_number() and canon(got["s"]) == x.sum("v", "rows") and canon(got["l"]) == x.shift("v", -1) and canon(got["cl"]) == x.count("long")


def test_a_partition_key_beyond_15_bytes_is_refused_by_name(tc):
    n = 10
    t = pa.table({"i": pa.array(np.arange(n, dtype=np.int64)), "long": pa.array([LONG % (j // 5) for j in range(n)]), "v": pa.array(np.arange(n, dtype=np.int64))})
    for ov, what in ((over(["long"], ["i"]), "partition_by"), (over([], ["long"]), "order_by")):
        with pytest.raises(g.GpuqError, match=what + " column 'long' holds strings longer than 15 bytes") as e:
            run(tc, t, [E.window("SUM", [col("v")], "s", **ov)], sort=False)      # (already in order)
        assert e.value.status == 3


def test_two_window_nodes_stacked_and_one_under_an_aggregate(tc):
    r = np.random.default_rng(6)
    n = 2500
    t = pa.table({"a": pa.array(r.integers(0, 9, n), pa.int32()), "b": pa.array(r.integers(0, 5, n), pa.int32()), "i": pa.array(np.arange(n, dtype=np.int64)),
                  "v": pa.array(r.integers(-100, 100, n), pa.int64())})
    src = g.MemoryExec([t])
    ova, ovb = over(["a"], ["i"]), over(["b"], ["i"])
    w1 = g.BoundedWindowAggExec(g.SortExec(sort_keys(["a", "i"]), src), [E.window("SUM", [col("v")], "s1", frame=E.rows_between(None, 0), **ova), E.window("ROW_NUMBER", [], "rn", **ova)])
    w2 = g.BoundedWindowAggExec(g.SortExec(sort_keys(["b", "i"]), w1), [E.window("SUM", [col("s1")], "s2", frame=E.rows_between(None, 0), **ovb), E.window("MAX", [col("rn")], "mrn", **ovb)])
    got = g.NativePlan(w2, tc).execute(0).to_arrow()
    assert got.schema.names == ["a", "b", "i", "v", "s1", "rn", "s2", "mrn"]
    # s1 / rn by a walk over (a, i) order, carried to the output's order by the row id
    rows = sorted(range(n), key=lambda j: (t["a"][j].as_py(), j))
    x1 = W.Walk({"a": [t["a"][j].as_py() for j in rows], "v": [t["v"][j].as_py() for j in rows]}, ["a"], [])
    s1 = dict(zip(rows, x1.sum("v", "rows"))); rn = dict(zip(rows, x1.row_number()))
    ids = got["i"].to_pylist()
    assert canon(got["s1"]) == [s1[j] for j in ids] and canon(got["rn"]) == [rn[j] for j in ids]
    tab = {"b": got["b"].to_pylist(), "i": ids, "s1": canon(got["s1"]), "rn": canon(got["rn"])}
    check_sorted(tab, ["b"], [])
    x2 = W.Walk(tab, ["b"], ["i"])
    assert canon(got["s2"]) == x2.sum("s1", "rows") and canon(got["mrn"]) == x2.minmax("rn", False)
    # ... and one node under an AggregateExec
    s = w1.schema()
    agg = g.AggregateExec("Single", [(col("a", s), "a")], [{"fn": "MAX", "expr": col("rn", s), "name": "rows"}, {"fn": "MAX", "expr": col("s1", s), "name": "peak"},
                                                         {"fn": "SUM", "expr": col("rn", s), "name": "tri"}], w1)
    out = g.NativePlan(agg, tc).execute(0).to_arrow()
    want = {}
    for j in range(n):
        a = t["a"][j].as_py()
        e = want.setdefault(a, [0, -10 ** 30, 0])
        e[0] = max(e[0], rn[j]); e[1] = max(e[1], s1[j]); e[2] += rn[j]
    assert {k: list(v) for k, v in zip(out["a"].to_pylist(), zip(out["rows"].to_pylist(), out["peak"].to_pylist(), [int(z) for z in out["tri"].to_pylist()]))} == want


def test_the_workspaces_count_against_the_memory_budget(tc):
    n = 2_000_000
    r = np.random.default_rng(8)
    t = pa.table({"k": pa.array((np.arange(n) // 1000).astype(np.int32)), "i": pa.array(np.arange(n, dtype=np.int64)), "v": pa.array(r.integers(-100, 100, n), pa.int64())})
    ov = over(["k"], ["i"])
    node = g.BoundedWindowAggExec(g.MemoryExec([t]), [E.window("SUM", [col("v")], "s", **ov), E.window("AVG", [col("v")], "a", **ov), E.window("ROW_NUMBER", [], "rn", **ov), E.lag(col("v"), "l", **ov)])
    plan = g.NativePlan(node, tc)      # (the table is uploaded here: it is the caller's, not the budget's)
    base = g.memory_stats(reset_peak=True)
    assert base["limit"] == 0
    got = plan.execute(0)
    want_last = int(t["v"].to_numpy()[-1000:].sum())
    assert got.to_arrow()["s"][n - 1].as_py() == want_last
    del got
    used = g.memory_stats()["peak"] - base["in_use"]
    assert used > 8 * 4 * n      # at least the four result columns
    try:
        g.memory_limit(base["in_use"] + used // 4)
        with pytest.raises(g.GpuqError) as e:
            plan.execute(0)
        assert e.value.status == 4 and "Resources exhausted" in str(e.value) and "memory limit" in str(e.value)
        assert g.memory_stats()["in_use"] - base["in_use"] < (8 << 20)      # nothing leaked by the failed task
    finally:
        g.memory_limit(0)
    assert plan.execute(0).to_arrow()["s"][n - 1].as_py() == want_last
