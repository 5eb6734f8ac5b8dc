"""Sort keys at the edges of their types' orders (tests/sort_edge_cases.py) through every executor the row count selects, against
tests/sort_order_exact.py -- the exact order, pinned by tests/test_cpu_sort_order_exact.py -- and compared on a row-id column, so that
ties test stability.  Every plan runs twice through NativePlan: the second run takes the deferred route and the learned key layout.

  n                    executor
  2, 511, 512          k_sort_direct: (rank, value) pairs, no layout
  513, 2048            pack + k_sort_small, one block
  2049, 6144, 6145     pack + look-back passes over one-word and two-word (key, id) records; the tile is 6144
  8192, 8193, 20 011   packed 8-byte records where the key has at most 32 bits (tile 8192), several tiles of look-back

Tables tile the edge values with a seeded permutation, so every edge occurs many times: from the smallest n that holds every value twice
at least a quarter of the rows take part in ties (asserted on the input).  Comparisons are exact; floats by bit pattern."""
import decimal

import numpy as np
import pyarrow as pa
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd import expr as EX
from arrow_ballista_amd.expr import col

import sort_edge_cases as E
import sort_order_exact as X
from sort_order_exact import Key

pytestmark = pytest.mark.gpu

NS = [2, 511, 512, 513, 2048, 2049, 6144, 6145, 8192, 8193, 20_011]
ALL_ORDERS_AT = (512, 2049)      # the two mixed combinations of (direction, NULL placement) run here only


def f64_array(vals):
    """Float64 from Python floats by PATTERN (a NaN keeps its sign and payload)"""
    bits = np.array([0 if v is None else X.f64_pattern(v) for v in vals], dtype=np.uint64)
    return pa.array(bits.view(np.float64), pa.float64(), mask=np.array([v is None for v in vals], dtype=bool))


def f32_array(vals):
    data = np.array([np.float32(0) if v is None else v for v in vals], dtype=np.float32)
    return pa.array(data, pa.float32(), mask=np.array([v is None for v in vals], dtype=bool))


def dec_array(vals):
    return pa.array([None if v is None else decimal.Decimal(v) for v in vals], pa.decimal128(38, 0))


# name -> (reference kind, pool of values, arrow array of a list of them, nullable)
KINDS = {
    "int64": ("int", E.INT64_EDGES + [None], lambda v: pa.array(v, pa.int64())),                        # 64 bits and the null bit: two words
    "float64": ("float", E.F64_EDGES + [None], f64_array),
    "float32": ("float", E.F32_EDGES + [None], f32_array),
    "utf8": ("utf8", E.UTF8_EDGES + [None], lambda v: pa.array(v, pa.string())),                        # the NUL chain among them
    "decimal-128-bits": ("int", E.DECIMAL_EDGES, dec_array),                                            # the whole key, no NULL
    "decimal-129-bits": ("int", E.DECIMAL_EDGES + [None], dec_array),                                   # one bit more than a composite holds
    "all-null": ("int", [None], lambda v: pa.array(v, pa.int64())),
    "boolean": ("int", [False, True, None], lambda v: pa.array(v, pa.bool_())),
}


def tiled(pool, n, seed):
    """n rows out of pool: every entry n // len(pool) times at least, in a seeded order (n < len(pool): distinct entries)"""
    r = np.random.default_rng(seed)
    idx = r.permutation(len(pool))[:n] if n < len(pool) else r.permutation(np.arange(n) % len(pool))
    return [pool[i] for i in idx]


def table_of(columns, nullable):
    """{"k0": array, ...} + the row id"""
    n = len(next(iter(columns.values())))
    t = pa.table(dict(columns, rid=pa.array(np.arange(n, dtype=np.int64))))
    return t.cast(pa.schema([pa.field(f.name, f.type, nullable=f.name != "rid" and nullable[f.name]) for f in t.schema]))


def patterns(c):
    """a float column as (validity, bit patterns)"""
    c = c.combine_chunks() if isinstance(c, pa.ChunkedArray) else c
    dt = np.uint64 if c.type == pa.float64() else np.uint32
    bits = np.frombuffer(c.buffers()[1], dtype=dt, count=c.offset + len(c))[c.offset:]
    ok = np.asarray(c.is_valid().to_numpy(zero_copy_only=False), dtype=bool)
    return ok, np.where(ok, bits, 0)


def run_sort(tc, t, names, orders):
    """the table sorted by names under orders [(desc, nulls_first), ...], through NativePlan, twice"""
    src = g.MemoryExec([t]); s = src.schema()
    spec = [EX.sort_expr(col(nm, s), asc=not desc, nulls_first=nf) for nm, (desc, nf) in zip(names, orders)]
    p = g.NativePlan(g.SortExec(spec, g.ProjectionExec([(col("rid", s), "rid")] + [(col(nm, s), nm) for nm in names], src)), tc)
    first = p.execute(0).to_arrow()
    second = p.execute(0).to_arrow()
    assert first.column("rid").to_pylist() == second.column("rid").to_pylist(), "the deferred run orders differently"
    return second


def check_sorted(tc, t, names, spec, rows):
    """-> the device's permutation, after it was found to be the reference's"""
    want = np.array(X.stable_perm(spec, rows), dtype=np.int64)
    out = run_sort(tc, t, names, [(k.desc, k.nulls_first) for k in spec])
    got = np.asarray(out.column("rid"))
    if not np.array_equal(got, want):
        at = int(np.argmax(got != want))
        raise AssertionError("order differs from place %d on: row %d %r, expected row %d %r" % (at, got[at], rows[got[at]], want[at], rows[want[at]]))
    for nm in names:      # the key columns came along with their rows: floats bit for bit
        if pa.types.is_floating(t.column(nm).type):
            ok_in, bits_in = patterns(t.column(nm))
            ok_out, bits_out = patterns(out.column(nm))
            assert np.array_equal(ok_out, ok_in[want]) and np.array_equal(bits_out, bits_in[want]), nm
    return got


def assert_edges_present(name, kind, pool, spec, rows, n):
    if n < 2 * len(pool):
        return
    assert X.tied_rows(spec, rows) >= n / 4
    if kind == "float":
        pats = {X.f64_pattern(v[0]) for v in rows if v[0] is not None}
        nan_signs = {p >> 63 for p in pats if p & (1 << 63) - 1 > 0x7FF0000000000000}
        assert nan_signs == {0, 1} and {0, 1 << 63} <= pats, name


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", list(KINDS))
def test_single_key_at_the_type_edges(tc, name, n):
    kind, pool, make = KINDS[name]
    vals = tiled(pool, n, n)
    t = table_of({"k": make(vals)}, {"k": None in pool})
    rows = [(v,) for v in vals]
    orders = [(False, False), (True, True)] + ([(False, True), (True, False)] if n in ALL_ORDERS_AT else [])
    for desc, nf in orders:
        spec = [Key(kind, desc, nf)]
        assert_edges_present(name, kind, pool, spec, rows, n)
        check_sorted(tc, t, ["k"], spec, rows)


COMPOSITES = {
    "utf8-asc,float64-desc": (
        [Key("utf8", False, False), Key("float", True, True)],
        [(s, f) for s in ["", "a", "a\0", "a\0\0", "ab"] for f in [E.F64_EDGES[0], E.F64_EDGES[2], -0.0, 0.0, E.F64_EDGES[-3], E.F64_EDGES[-1]]],
        [lambda v: pa.array(v, pa.string()), f64_array], [False, False]),
    "float32-asc-nullable,int8-desc,utf8-asc": (
        [Key("float", False, True), Key("int", True, True), Key("utf8", False, False)],
        [(f, i, s) for f in [None, E.F32_EDGES[0], E.F32_EDGES[7], E.F32_EDGES[8], E.F32_EDGES[-1]] for i in [-128, -1, 127] for s in ["", "a", "a\0"]],
        [f32_array, lambda v: pa.array(v, pa.int8()), lambda v: pa.array(v, pa.string())], [True, False, False]),
}


@pytest.mark.parametrize("n", [512, 2048, 2049, 8193])
@pytest.mark.parametrize("name", list(COMPOSITES))
def test_composite_keys_with_ties_in_the_leading_keys(tc, name, n):
    spec, pool, makes, nullable = COMPOSITES[name]
    rows = tiled(pool, n, n + 1)
    names = ["k%d" % i for i in range(len(spec))]
    t = table_of({nm: mk([r[i] for r in rows]) for i, (nm, mk) in enumerate(zip(names, makes))}, dict(zip(names, nullable)))
    assert X.tied_rows(spec, rows) >= n / 4 and X.tied_rows(spec[:1], rows) == n
    check_sorted(tc, t, names, spec, rows)


@pytest.mark.parametrize("name", ["utf8", "float64"])
def test_the_order_does_not_depend_on_the_path_the_row_count_selects(tc, name):
    """512 rows are sorted by k_sort_direct from (rank, value) pairs, 513 by the packed composite: the same rows plus one must come out
    in the same order once the extra row is taken out.  (A string field that dropped the length tied "a" with "a\\0" on one side only.)"""
    kind, pool, make = KINDS[name]
    vals = tiled(pool, 513, 99)
    for desc, nf in [(False, False), (True, True)]:
        spec = [Key(kind, desc, nf)]
        many = check_sorted(tc, table_of({"k": make(vals)}, {"k": True}), ["k"], spec, [(v,) for v in vals])
        few = check_sorted(tc, table_of({"k": make(vals[:512])}, {"k": True}), ["k"], spec, [(v,) for v in vals[:512]])
        assert np.array_equal(many[many != 512], few)


@pytest.mark.parametrize("sizes", [[5, 0, 2049], [2048, 2049, 1]])
@pytest.mark.parametrize("name", ["utf8", "float64"])
def test_merge_of_runs_sorted_by_edge_keys(tc, name, sizes):
    """The ordered fan-in over runs that the reference sorted, through CoalesceTasksExec(order_by) and SortPreservingMergeExec.  Mode: the
    cost rule picks MERGE-PATH ROUNDS here (two or three live runs are one or two rounds, est. 1.45 ms each at most 1.9; these keys are 65
    and 125 bits wide, 9 and 16 radix passes) -- the rounds compare the same packed composites the passes would sort."""
    kind, pool, make = KINDS[name]
    spec = [Key(kind, False, False)]
    parts, rows, rid0 = [], [], 0
    for j, m in enumerate(sizes):
        vals = tiled(pool, m, 7 * m + j)
        vals = [vals[i] for i in X.stable_perm(spec, [(v,) for v in vals])]
        t = pa.table({"rid": pa.array(np.arange(rid0, rid0 + m, dtype=np.int64)), "k": make(vals)})
        parts.append(t.cast(pa.schema([pa.field("rid", pa.int64(), nullable=False), pa.field("k", t.schema.field("k").type, nullable=True)])))
        rows += [(v,) for v in vals]; rid0 += m
    want = X.stable_perm(spec, rows)
    assert X.tied_rows(spec, rows) >= len(rows) / 4
    src = g.MemoryExec(parts); s = src.schema()
    order = [EX.sort_expr(col("k", s), asc=True, nulls_first=False)]
    for plan in (g.CoalesceTasksExec(src, list(range(len(sizes))), order_by=order), g.SortPreservingMergeExec(order, src)):
        p = g.NativePlan(plan, tc)
        for _ in range(2):
            assert p.execute(0).to_arrow().column("rid").to_pylist() == want


def test_row_number_over_the_float_order(tc):
    """ROW_NUMBER() OVER (ORDER BY f64): the window operator sits on the same sort"""
    kind, pool, make = KINDS["float64"]
    n = 2049
    vals = tiled(pool, n, 5)
    t = table_of({"k": make(vals)}, {"k": True})
    spec = [Key("float", False, False)]
    src = g.MemoryExec([t]); s = src.schema()
    order = [EX.sort_expr(col("k", s), asc=True, nulls_first=False)]
    node = g.BoundedWindowAggExec(g.SortExec(order, src), [EX.window("ROW_NUMBER", [], "rn", order_by=order)])
    p = g.NativePlan(node, tc)
    for _ in range(2):
        out = p.execute(0).to_arrow()
        assert out.column("rid").to_pylist() == X.stable_perm(spec, [(v,) for v in vals])
        assert out.column("rn").to_pylist() == list(range(1, n + 1))
