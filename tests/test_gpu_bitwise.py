"""BIT_AND / BIT_OR / BIT_XOR / BOOL_AND / BOOL_OR through every aggregate kernel, and the scalar operators & | ^ through filter and
projection, on the device.  Expected values come from numpy (aggregates: the ufunc's reduce per group in the column's own dtype,
all / any for BOOL_*) and pyarrow.compute (operators) alone; every comparison is exact.

Data: a key per row, a random full-width mask M[key] per key and a random full-width r per row give x_and = M[key] | r,
x_or = M[key] & r and x_xor = r, so that a large group's BIT_AND / BIT_OR is M[key] and not 0 / all ones (asserted on the numpy side).
BIT_XOR is the sharp one: a row folded twice or dropped changes it.  The type's min, max, 0 and -1 are forced into r."""
import os

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit

pytestmark = pytest.mark.gpu

INTS = ["Int8", "Int16", "Int32", "Int64", "UInt8", "UInt16", "UInt32", "UInt64"]
NP = {"Int8": np.int8, "Int16": np.int16, "Int32": np.int32, "Int64": np.int64, "UInt8": np.uint8, "UInt16": np.uint16, "UInt32": np.uint32, "UInt64": np.uint64}
PA = {"Int8": pa.int8(), "Int16": pa.int16(), "Int32": pa.int32(), "Int64": pa.int64(), "UInt8": pa.uint8(), "UInt16": pa.uint16(), "UInt32": pa.uint32(),
      "UInt64": pa.uint64()}
ARGS = [("BIT_AND", "x_and"), ("BIT_OR", "x_or"), ("BIT_XOR", "x_xor"), ("BOOL_AND", "b_and"), ("BOOL_OR", "b_or")]
UFUNC = {"BIT_AND": np.bitwise_and, "BIT_OR": np.bitwise_or, "BIT_XOR": np.bitwise_xor, "BOOL_AND": np.logical_and, "BOOL_OR": np.logical_or}


def full_width(r, dt, n):
    ii = np.iinfo(dt)
    return r.integers(ii.min, ii.max, n, dtype=dt, endpoint=True)


class Data:
    """One table of one integer type: columns k (the key, absent when ungrouped), x_and, x_or, x_xor, b_and, b_or as numpy arrays + validity."""

    def __init__(self, seed, tname, n, key_ids=None, key_values=None, nulls=0.0, null_group=None, mask_seed=None):
        r = np.random.default_rng(seed)
        dt = NP[tname]
        ii = np.iinfo(dt)
        self.tname, self.n, self.nullable = tname, n, nulls > 0
        ngroups = 1 if key_values is None else len(key_values)
        ids = np.zeros(n, dtype=np.int64) if key_ids is None else key_ids
        m = full_width(r if mask_seed is None else np.random.default_rng(mask_seed), dt, ngroups)      # mask_seed: partitions of one table share their keys' masks
        m[(m == 0) | (m == dt(-1) if ii.min < 0 else m == ii.max)] = dt(0x5A)      # a mask that is neither 0 nor all ones
        rr = full_width(r, dt, n)
        forced = np.array([ii.min, ii.max, 0, ii.max if ii.min == 0 else -1], dtype=dt)      # -1 of an unsigned type is its max
        rr[:min(n, 4)] = forced[:min(n, 4)]
        if tname == "UInt64" and n > 6:
            rr[4:6] = [np.uint64(1) << np.uint64(63), (np.uint64(1) << np.uint64(63)) + np.uint64(12345)]
        self.ids = ids
        self.keys = None if key_values is None else key_values[ids]
        self.cols = {"x_and": m[ids] | rr, "x_or": m[ids] & rr, "x_xor": rr, "b_and": r.random(n) >= 0.02, "b_or": r.random(n) < 0.02}
        self.valid = {}
        for c in self.cols:
            v = np.ones(n, dtype=bool) if nulls <= 0 else r.random(n) >= nulls
            if null_group is not None and nulls > 0:
                v[ids == null_group] = False      # a group whose arguments are all NULL
            self.valid[c] = v

    def sorted_by_key(self):
        return self.take(np.argsort(self.keys, kind="stable"))

    def take(self, order):
        d = Data.__new__(Data)
        d.tname, d.n, d.nullable = self.tname, self.n, self.nullable
        d.ids, d.keys = self.ids[order], None if self.keys is None else self.keys[order]
        d.cols = {c: v[order] for c, v in self.cols.items()}
        d.valid = {c: v[order] for c, v in self.valid.items()}
        return d

    def arrow(self, key_type=None):
        arrays, fields = [], []
        if self.keys is not None:
            arrays.append(pa.array(self.keys, type=key_type)); fields.append(pa.field("k", key_type, nullable=False))
        for c, v in self.cols.items():
            t = pa.bool_() if c.startswith("b_") else PA[self.tname]
            arrays.append(pa.array(v, type=t, mask=~self.valid[c] if self.nullable else None)); fields.append(pa.field(c, t, nullable=self.nullable))
        return pa.Table.from_arrays(arrays, schema=pa.schema(fields))

    @staticmethod
    def concat(parts):
        d = Data.__new__(Data)
        d.tname, d.n, d.nullable = parts[0].tname, sum(p.n for p in parts), parts[0].nullable
        d.ids = np.concatenate([p.ids for p in parts])
        d.keys = None if parts[0].keys is None else np.concatenate([p.keys for p in parts])
        d.cols = {c: np.concatenate([p.cols[c] for p in parts]) for c in parts[0].cols}
        d.valid = {c: np.concatenate([p.valid[c] for p in parts]) for c in parts[0].valid}
        return d


def reduce_per_group(fn, keys, vals, valid):
    """{key: ufunc.reduce over the group's non-NULL values, in their own dtype (reduceat: reduce per run of the key-sorted values),
    or None where the group has none}."""
    out = {int(k): None for k in np.unique(keys)}
    k, v = keys[valid], vals[valid]
    if len(k):
        order = np.argsort(k, kind="stable")
        k, v = k[order], v[order]
        starts = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
        red = UFUNC[fn].reduceat(v, starts)
        assert red.dtype == vals.dtype
        out.update({int(a): (bool(b) if vals.dtype == bool else int(b)) for a, b in zip(k[starts], red)})
    return out


def expected(data):
    """{key (0 when ungrouped): (BIT_AND, BIT_OR, BIT_XOR, BOOL_AND, BOOL_OR)}; ungrouped over zero rows: one row of NULLs."""
    keys = data.keys if data.keys is not None else np.zeros(data.n, dtype=np.int64)
    per = [reduce_per_group(fn, keys, data.cols[c], data.valid[c]) for fn, c in ARGS]
    groups = sorted(per[0]) if (data.keys is not None or data.n) else [0]
    return {k: tuple(p.get(k) for p in per) for k in groups}


def data_condition(data, exp):
    """At least half the groups' BIT_AND and BIT_OR are neither 0 nor all ones (holds by construction: they are the group's mask)."""
    ones = int(np.iinfo(NP[data.tname]).max) if data.tname.startswith("U") else -1
    for i in (0, 1):
        vals = [v[i] for v in exp.values() if v[i] is not None]
        assert 2 * sum(1 for v in vals if v not in (0, ones)) >= len(vals), (data.tname, i)


def aggs_of(s, fns=ARGS):
    return [{"fn": fn, "expr": col(c, s), "name": fn.lower()} for fn, c in fns]


def rows_by_key(t, grouped, tname, suffixes=None):
    """An aggregate's result table -> {key: values}, after checking the column types: the argument's type / Boolean."""
    want = [PA[tname]] * 3 + [pa.bool_()] * 2
    vals = t.columns[1:] if grouped else t.columns
    assert [c.type for c in vals] == want, t.schema
    if suffixes is not None:
        assert t.schema.names[1 if grouped else 0:] == [fn.lower() + "[" + fn.lower() + "]" for fn, _ in ARGS]
    keys = t.column(0).to_pylist() if grouped else [0] * t.num_rows
    rows = list(zip(*[c.to_pylist() for c in vals]))
    assert len(set(keys)) == len(keys)
    return dict(zip(keys, rows))


def device_arrow(tc, dev_table):
    return g.plan.materialize(tc, dev_table).to_arrow(tc.ctx)


def run_single(tc, data, key_type, strategy, **kw):
    src = g.MemoryExec([data.arrow(key_type)])
    s = src.schema()
    groups = [(col("k", s), "k")] if data.keys is not None else []
    plan = g.AggregateExec("Single", groups, aggs_of(s), src, strategy=strategy, **kw)
    return rows_by_key(device_arrow(tc, plan.execute(0, tc)), bool(groups), data.tname)


def distinct_keys(r, n, np_type):
    ii = np.iinfo(np_type)
    k = np.unique(r.integers(ii.min, ii.max, 2 * n, dtype=np_type, endpoint=True))
    r.shuffle(k)
    assert len(k) >= n
    return k[:n]


# ------------------------------------------------------------------------------------ k_agg_tiny (+ its merge)
@pytest.mark.parametrize("nulls", [0.0, 0.15])
@pytest.mark.parametrize("tname", INTS)
def test_tiny_strategy(tc, tname, nulls):
    for n in (0, 1, 5000):
        r = np.random.default_rng(n + 11)
        ungrouped = Data(100 + n, tname, n, nulls=nulls)
        exp = expected(ungrouped)
        assert len(exp) == 1 and (n > 0 or exp[0] == (None,) * 5)      # over zero rows: one row of NULLs
        assert run_single(tc, ungrouped, None, "tiny") == exp, (tname, n)
        grouped = Data(200 + n, tname, n, key_ids=r.integers(0, 3, n), key_values=np.array([-7, 0, 2**31 - 1], dtype=np.int32), nulls=nulls, null_group=1 if n > 1 else None)
        exp = expected(grouped)
        if n == 5000:
            data_condition(ungrouped, expected(ungrouped)); data_condition(grouped, exp)
            assert len(exp) == 3 and (nulls == 0 or exp[0] == (None,) * 5)      # key value 0 is group id 1: all its arguments are NULL
        assert run_single(tc, grouped, pa.int32(), "tiny") == exp, (tname, n)


# ------------------------------------------------------------------------------------ k_agg_hash: the in-wave segmented scan, both extracts
def clustered(seed, tname, key_np, nulls, n=20_000):
    """~300 groups whose sizes run from 1 to 200 (skewed to the short ones), so that key-sorted input has runs that start and end
    anywhere in a lane / a 64-row word, with NULL arguments inside them."""
    r = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < n:
        sizes.append(1 + int(200 * r.random() ** 2.2))
    sizes[-1] -= sum(sizes) - n
    ids = np.repeat(np.arange(len(sizes)), sizes)
    r.shuffle(ids)
    return Data(seed, tname, n, key_ids=ids, key_values=distinct_keys(r, len(sizes), key_np), nulls=nulls, null_group=3)


@pytest.mark.parametrize("nulls", [0.0, 0.15])
@pytest.mark.parametrize("key", ["Int32", "Int64"])      # Int32: the key lives in the slot's state word (direct SoA extract); Int64: key words, launch_agg_emit
@pytest.mark.parametrize("tname", INTS)
def test_hash_strategy_shuffled_and_sorted(tc, tname, key, nulls):
    d = clustered(31 + len(tname), tname, NP[key], nulls)
    exp = expected(d)
    data_condition(d, exp)
    assert 200 <= len(exp) <= 450 and (nulls == 0 or any(v == (None,) * 5 for v in exp.values()))
    assert run_single(tc, d, PA[key], "hash") == exp
    s = d.sorted_by_key()
    runs = np.diff(np.flatnonzero(np.concatenate([[True], s.keys[1:] != s.keys[:-1], [True]])))
    assert runs.min() <= 2 and runs.max() >= 150
    assert run_single(tc, s, PA[key], "hash") == exp


# ------------------------------------------------------------------------------------ k_agg_lds
@pytest.mark.parametrize("nulls", [0.0, 0.15])
@pytest.mark.parametrize("tname", INTS)
def test_lds_strategy_few_groups(tc, tname, nulls):
    """Everything stays in the blocks' LDS tables; a block flushes cells no row of it touched (a NULL argument, another block's group):
    they hold the identity and must leave the global cell alone."""
    r = np.random.default_rng(5)
    n = 60_000
    d = Data(41, tname, n, key_ids=r.integers(0, 30, n), key_values=distinct_keys(r, 30, np.int32), nulls=nulls, null_group=7)
    exp = expected(d)
    data_condition(d, exp)
    assert len(exp) == 30
    assert run_single(tc, d, pa.int32(), "lds") == exp


@pytest.mark.parametrize("tname", INTS)
def test_lds_strategy_blocks_run_full(tc, tname):
    """100,000 groups: the LDS tables run full and rows fold into the global table directly."""
    r = np.random.default_rng(6)
    n = 300_000
    d = Data(43, tname, n, key_ids=r.integers(0, 100_000, n), key_values=distinct_keys(r, 100_000, np.int64), nulls=0.15, null_group=11)
    exp = expected(d)
    data_condition(d, exp)
    assert len(exp) > 90_000
    assert run_single(tc, d, pa.int64(), "lds") == exp


# ------------------------------------------------------------------------------------ k_agg_bucket
@pytest.mark.parametrize("nulls", [0.0, 0.15])
@pytest.mark.parametrize("tname", INTS)
def test_radix_strategy(tc, tname, nulls):
    r = np.random.default_rng(7)
    n = 60_000
    d = Data(47, tname, n, key_ids=r.integers(0, n // 3, n), key_values=distinct_keys(r, n // 3, np.int64), nulls=nulls, null_group=5)
    exp = expected(d)
    data_condition(d, exp)
    assert run_single(tc, d, pa.int64(), "radix", expected_groups=n // 3) == exp


# ------------------------------------------------------------------------------------ Partial -> FinalPartitioned
@pytest.mark.parametrize("strategy", ["tiny", "hash"])
@pytest.mark.parametrize("tname", INTS)
def test_partial_then_final(tc, tname, strategy):
    r = np.random.default_rng(8)
    ng = 3 if strategy == "tiny" else 300
    kv = distinct_keys(r, ng, np.int32)
    parts = [Data(51 + p, tname, 20_000, key_ids=r.integers(0, ng, 20_000), key_values=kv, nulls=0.15, null_group=2, mask_seed=50) for p in range(3)]
    src = g.MemoryExec([p.arrow(pa.int32()) for p in parts])
    s = src.schema()
    partial = g.AggregateExec("Partial", [(col("k", s), "k")], aggs_of(s), src, strategy=strategy)
    states = [device_arrow(tc, partial.execute(p, tc)) for p in range(3)]
    for p in range(3):      # the state columns have the argument's type and hold the partition's own results
        assert rows_by_key(states[p], True, tname, suffixes=True) == expected(parts[p])
    merged = g.MemoryExec([pa.concat_tables(states)])
    fs = merged.schema()
    final = g.AggregateExec("FinalPartitioned", [(col("k", fs), "k")], [{"fn": fn, "expr": None, "name": fn.lower()} for fn, _ in ARGS], merged)
    exp = expected(Data.concat(parts))
    data_condition(parts[0], exp)
    assert any(v == (None,) * 5 for v in exp.values())
    assert rows_by_key(device_arrow(tc, final.execute(0, tc)), True, tname) == exp


# ------------------------------------------------------------------------------------ the native plan: DISTINCT, FILTER, deferred runs
def native_rows(plan):
    t = plan.execute(0).to_arrow()
    return sorted(zip(*[c.to_pylist() for c in t.columns]), key=lambda row: row[0]), t


@pytest.mark.parametrize("tname", ["Int16", "UInt64"])
def test_native_plan_distinct_filter_and_deferred_runs(tc, tname):
    r = np.random.default_rng(9)
    n, ng = 20_000, 40
    dt = NP[tname]
    pool = full_width(r, dt, 25)      # few distinct values: every group sees most of them many times
    keys = r.integers(0, ng, n).astype(np.int32)
    x = pool[r.integers(0, len(pool), n)]
    valid = r.random(n) >= 0.15
    valid[keys == 4] = False
    f = r.integers(0, 10, n).astype(np.int32)
    t = pa.table({"k": pa.array(keys), "x": pa.array(x, type=PA[tname], mask=~valid), "f": pa.array(f)})
    src = g.MemoryExec([t])
    s = src.schema()
    # BIT_XOR(DISTINCT x): GROUP BY (k, x), then GROUP BY k
    plan = g.NativePlan(g.AggregateExec("Single", [(col("k", s), "k")], [{"fn": "BIT_XOR", "expr": col("x", s), "name": "dx", "distinct": True}], src), tc)
    exp = []
    for k in range(ng):
        u = np.unique(x[(keys == k) & valid])
        exp.append((k, int(np.bitwise_xor.reduce(u)) if len(u) else None))
    assert exp[4] == (4, None) and any(v not in (None, 0) for _, v in exp)
    got, tab = native_rows(plan)
    assert got == exp and tab.column(1).type == PA[tname]
    # a per-aggregate FILTER next to the unfiltered function; three executions of one handle (deferred from the second) give the same rows
    pred = binary(col("f", s), Op.Lt, lit(3, "Int32"))
    aggs = [{"fn": "BIT_OR", "expr": col("x", s), "name": "o", "filter": pred}, {"fn": "BIT_OR", "expr": col("x", s), "name": "o_all"},
            {"fn": "BIT_XOR", "expr": col("x", s), "name": "x", "filter": pred}]
    plan = g.NativePlan(g.AggregateExec("Single", [(col("k", s), "k")], aggs, src), tc)
    sel = valid & (f < 3)
    o, o_all, xs = reduce_per_group("BIT_OR", keys, x, sel), reduce_per_group("BIT_OR", keys, x, valid), reduce_per_group("BIT_XOR", keys, x, sel)
    exp = [(k, o[k], o_all[k], xs[k]) for k in range(ng)]
    assert exp[4] == (4, None, None, None)
    for run in range(3):
        assert native_rows(plan)[0] == exp, run


def test_known_answers_alltypes_plain(tc):
    """tests/golden/alltypes_plain.arrow (the reference's ballista/client/testdata/alltypes_plain.parquet): the answers are derived here
    with numpy from the file."""
    with pa.ipc.open_file(os.path.join(os.path.dirname(__file__), "golden", "alltypes_plain.arrow")) as f:
        t = f.read_all().select(["id", "bigint_col", "bool_col"])
    idc, big, boo = (t.column(c).to_numpy(zero_copy_only=False) for c in ("id", "bigint_col", "bool_col"))
    exp = (int(np.bitwise_and.reduce(idc)), int(np.bitwise_or.reduce(idc)), int(np.bitwise_xor.reduce(idc)), int(np.bitwise_or.reduce(big)), bool(boo.all()), bool(boo.any()))
    src = g.MemoryExec([t])
    s = src.schema()
    aggs = [{"fn": "BIT_AND", "expr": col("id", s), "name": "a"}, {"fn": "BIT_OR", "expr": col("id", s), "name": "o"}, {"fn": "BIT_XOR", "expr": col("id", s), "name": "x"},
            {"fn": "BIT_OR", "expr": col("bigint_col", s), "name": "ob"}, {"fn": "BOOL_AND", "expr": col("bool_col", s), "name": "ba"}, {"fn": "BOOL_OR", "expr": col("bool_col", s), "name": "bo"}]
    got = device_arrow(tc, g.AggregateExec("Single", [], aggs, src).execute(0, tc))
    assert [c.type for c in got.columns] == [pa.int32()] * 3 + [pa.int64(), pa.bool_(), pa.bool_()]
    assert [tuple(c.to_pylist()[0] for c in got.columns)] == [exp] and got.num_rows == 1


def test_mirror_layer_gives_the_same(tc, mirror_layer):
    """The Python restatement of the executor needs nothing of its own: its schema comes from the compile."""
    d = clustered(77, "UInt64", np.int32, 0.15, n=5000)
    assert run_single(tc, d, pa.int32(), "hash") == expected(d)
    t = operand_table("Int16", 5000)
    assert projected(tc, t) == projection_expected(t)


# ------------------------------------------------------------------------------------ the specialised (run-time compiled) kernels
@pytest.fixture()
def jit(tc):
    if not tc.ctx.jit_stats()["available"]:
        pytest.skip("hiprtc not available")
    tc.ctx.set_jit("force")
    before = tc.ctx.jit_stats()["launches"]
    yield tc
    tc.ctx.set_jit("auto")
    assert tc.ctx.jit_stats()["launches"] > before, "no JIT launch happened"


def test_aggregate_sinks_specialised(jit):
    """The accumulate switch of the specialised LDS-dictionary kernel folds over compile-time kinds; the hash sink's segmented scan runs
    over the generated evaluator's rows in flight; the LDS and bucket sinks fold at workgroup scope."""
    r = np.random.default_rng(12)
    d = Data(61, "UInt64", 5000, key_ids=r.integers(0, 3, 5000), key_values=np.array([5, -1, 9], dtype=np.int32), nulls=0.15, null_group=1)
    assert run_single(jit, d, pa.int32(), "tiny") == expected(d)
    s = clustered(63, "Int8", np.int64, 0.15).sorted_by_key()
    assert run_single(jit, s, pa.int64(), "hash") == expected(s)
    # the workgroup-scope folds of the block-local and the per-bucket LDS tables
    n = 60_000
    few = Data(65, "UInt16", n, key_ids=r.integers(0, 30, n), key_values=distinct_keys(r, 30, np.int32), nulls=0.15, null_group=7)
    assert run_single(jit, few, pa.int32(), "lds") == expected(few)
    many = Data(67, "Int64", n, key_ids=r.integers(0, n // 3, n), key_values=distinct_keys(r, n // 3, np.int64), nulls=0.15, null_group=5)
    assert run_single(jit, many, pa.int64(), "radix", expected_groups=n // 3) == expected(many)


# ------------------------------------------------------------------------------------ & | ^ in FilterExec and ProjectionExec
def operand_table(tname, n, seed=3):
    r = np.random.default_rng(seed + n)
    dt = NP[tname]
    ii = np.iinfo(dt)
    cols = {}
    for name in ("a", "b", "c"):
        v = full_width(r, dt, n)
        forced = np.array([ii.min, ii.max, 0, ii.max if ii.min == 0 else -1], dtype=dt)
        r.shuffle(forced)
        v[:min(n, 4)] = forced[:min(n, 4)]
        cols[name] = pa.array(v, type=PA[tname], mask=(r.random(n) < 0.15) if n > 1 else None)
    return pa.table(cols)


OPS = [(Op.BitwiseAnd, pc.bit_wise_and), (Op.BitwiseOr, pc.bit_wise_or), (Op.BitwiseXor, pc.bit_wise_xor)]


def projected(tc, t):
    src = g.MemoryExec([t])
    s = src.schema()
    plan = g.ProjectionExec([(binary(col("a", s), op, col("b", s)), "o%d" % i) for i, (op, _) in enumerate(OPS)] + [(binary(col("a", s), Op.BitwiseXor, lit(None)), "n")], src)
    out = device_arrow(tc, plan.execute(0, tc))
    assert [c.type for c in out.columns] == [t.column(0).type] * 4
    return [c.to_pylist() for c in out.columns]


def projection_expected(t):
    return [f(t["a"], t["b"]).to_pylist() for _, f in OPS] + [[None] * t.num_rows]


@pytest.mark.parametrize("tname", INTS)
def test_projection_of_bitwise_operators(tc, tname):
    for n in (1, 5000):
        t = operand_table(tname, n)
        assert projected(tc, t) == projection_expected(t), (tname, n)
    if tc.ctx.jit_stats()["available"]:      # the second run: the specialised kernel
        before = tc.ctx.jit_stats()["launches"]
        tc.ctx.set_jit("force")
        try:
            assert projected(tc, t) == projection_expected(t), tname
        finally:
            tc.ctx.set_jit("auto")
        assert tc.ctx.jit_stats()["launches"] > before


def filtered(tc, t, pred_of):
    src = g.MemoryExec([t])
    out = device_arrow(tc, g.FilterExec(pred_of(src.schema()), src).execute(0, tc))
    return [c.to_pylist() for c in out.columns]


def test_filters_on_bitwise_operators(tc):
    for n in (1, 5000):
        t = operand_table("Int32", n, seed=21)
        u = operand_table("UInt64", n, seed=22)
        top = 2**63 + 4
        cases = [
            (t, lambda s: binary(binary(col("a", s), Op.BitwiseAnd, lit(4, "Int32")), Op.Eq, lit(4, "Int32")), pc.equal(pc.bit_wise_and(t["a"], pa.scalar(4, pa.int32())), 4)),
            (t, lambda s: binary(binary(col("a", s), Op.BitwiseXor, col("b", s)), Op.Gt, col("c", s)), pc.greater(pc.bit_wise_xor(t["a"], t["b"]), t["c"])),
            (u, lambda s: binary(binary(col("a", s), Op.BitwiseAnd, lit(top, "UInt64")), Op.Eq, lit(top, "UInt64")),
             pc.equal(pc.bit_wise_and(u["a"], pa.scalar(top, pa.uint64())), pa.scalar(top, pa.uint64()))),
            (u, lambda s: binary(binary(col("a", s), Op.BitwiseOr, col("b", s)), Op.Lt, col("c", s)), pc.less(pc.bit_wise_or(u["a"], u["b"]), u["c"])),
        ]
        modes = ["auto", "force"] if (n == 5000 and tc.ctx.jit_stats()["available"]) else ["auto"]
        for mode in modes:
            tc.ctx.set_jit(mode)
            try:
                for tab, pred_of, mask in cases:
                    want = tab.filter(mask)      # a NULL predicate drops the row
                    assert n == 1 or 0 < want.num_rows < n
                    assert filtered(tc, tab, pred_of) == [c.to_pylist() for c in want.columns], (n, mode)
            finally:
                tc.ctx.set_jit("auto")
