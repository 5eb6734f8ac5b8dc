"""MEDIAN through the native executor (AggregateExec in mode Single: one sort by (keys..., argument) per distinct argument, segment heads,
one lane per segment picking the middles) against a restatement of DataFusion 34's MedianAccumulator written here: groups by sorting,
the even case's sum wrapping in fixed-width numpy integers, truncating division, Decimal128 in Python ints.  Every comparison is exact;
floats are compared by bit pattern.  (STDDEV next to a MEDIAN is the one exception: see REL_STDDEV.)"""
import ctypes as C
import decimal

import numpy as np
import pyarrow as pa
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd import binding as B
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit

pytestmark = pytest.mark.gpu

NP = {"Int8": np.int8, "Int16": np.int16, "Int32": np.int32, "Int64": np.int64, "UInt8": np.uint8, "UInt16": np.uint16, "UInt32": np.uint32, "UInt64": np.uint64,
      "Float32": np.float32, "Float64": np.float64}
PA = {"Int8": pa.int8(), "Int16": pa.int16(), "Int32": pa.int32(), "Int64": pa.int64(), "UInt8": pa.uint8(), "UInt16": pa.uint16(), "UInt32": pa.uint32(),
      "UInt64": pa.uint64(), "Float32": pa.float32(), "Float64": pa.float64(), "Decimal": pa.decimal128(38, 4)}
TYPES = list(NP) + ["Decimal"]
CTX = decimal.Context(prec=60)
# STDDEV is folded in floating point, in the order the rows arrive: the node with a MEDIAN feeds the operator key-sorted rows, the node
# without it (and numpy's two-pass formula) another order.  Float64 has 2^-53 ~ 1.1e-16 per operation; a group of at most a few thousand
# values whose variance is not small against the square of its mean loses a few thousand of those: 1e-9 relative leaves three decimal
# orders of room and is the bound bench_extras.py's h2o leg already holds the same question to.
REL_STDDEV = 1e-9


# ------------------------------------------------------------------------------------ the restatement
def is_float(tname):
    return tname in ("Float32", "Float64")


def total_order(a):
    """IEEE-754 totalOrder as an integer key: what SortExec orders floats by."""
    bits = a.view(np.int64 if a.dtype == np.float64 else np.int32)
    return bits ^ ((bits >> (bits.dtype.itemsize * 8 - 1)) & np.iinfo(bits.dtype).max)


def sort_values(vals, tname):
    if tname == "Decimal":
        return sorted(vals)
    if is_float(tname):
        return vals[np.argsort(total_order(vals), kind="stable")]
    return np.sort(vals)


def trunc_half(s):
    return -((-s) // 2) if s < 0 else s // 2      # Rust's `/`: toward zero


def median_of(vals, tname):
    """The median of the sorted non-NULL values of one group, in canonical form (canon)."""
    v = len(vals)
    if v == 0:
        return None
    if v % 2:
        return canon(vals[v // 2], tname)
    lo, hi = vals[v // 2 - 1], vals[v // 2]
    if tname == "Decimal":
        return trunc_half((int(lo) + int(hi) + 2**127) % 2**128 - 2**127)
    dt = NP[tname]
    with np.errstate(over="ignore"):
        s = np.array([lo], dt) + np.array([hi], dt)      # wraps at the declared width / rounds in the column's precision
    if is_float(tname):
        return canon((s / dt(2))[0], tname)
    return trunc_half(int(s[0]))


def canon(x, tname):
    """A value as something `==` compares exactly: a Python int; a float as its bit pattern."""
    if x is None:
        return None
    if is_float(tname):
        dt = NP[tname]
        return ("bits", int(np.array([x], dt).view(np.uint64 if dt == np.float64 else np.uint32)[0]))
    return int(x)


def segments(keys, n):
    """Group by sorting.  keys: [(values, valid)]; returns (row order, [(key tuple, first, last + 1)] over that order)."""
    if n == 0:
        return np.arange(0), []
    if not keys:
        return np.arange(n), [((), 0, n)]
    codes = []
    for vals, valid in keys:
        c = np.full(n, -1, dtype=np.int64)
        if valid.any():
            c[valid] = np.unique(np.asarray(vals)[valid], return_inverse=True)[1]
        codes.append(c)
    order = np.lexsort(codes[::-1])
    m = np.stack([c[order] for c in codes])
    head = np.concatenate([[True], (m[:, 1:] != m[:, :-1]).any(axis=0)])
    starts = list(np.flatnonzero(head)) + [n]
    out = []
    for a, b in zip(starts[:-1], starts[1:]):
        row = order[a]
        key = tuple((vals[row].item() if hasattr(vals[row], "item") else vals[row]) if valid[row] else None for vals, valid in keys)
        out.append((key, a, b))
    return order, out


def expected_medians(keys, vals, valid, tname, n, ungrouped=False):
    """{key tuple: median}; ungrouped over zero rows: one row holding NULL."""
    order, segs = segments(keys, n)
    if ungrouped and n == 0:
        return {(): None}
    vals = np.asarray(vals, dtype=object) if tname == "Decimal" else vals
    out = {}
    for key, a, b in segs:
        rows = order[a:b]
        rows = rows[valid[rows]]
        out[key] = median_of(sort_values(list(vals[rows]) if tname == "Decimal" else vals[rows], tname), tname)
    return out


# ------------------------------------------------------------------------------------ tables and results
def arrow_column(vals, valid, tname):
    if tname == "Decimal":
        return pa.array([decimal.Decimal(int(v)).scaleb(-4, CTX) if ok else None for v, ok in zip(vals, valid)], PA[tname])
    return pa.array(vals, PA[tname], mask=~valid)


def canon_column(c, tname):
    c = c.combine_chunks() if isinstance(c, pa.ChunkedArray) else c
    if tname == "Decimal":
        return [None if x is None else int(x.scaleb(4, CTX)) for x in c.to_pylist()]
    if is_float(tname):
        ok = c.is_valid().to_pylist()
        v = c.fill_null(0).to_numpy(zero_copy_only=False).astype(NP[tname], copy=False)
        return [canon(x, tname) if o else None for x, o in zip(v, ok)]
    return c.to_pylist()


def device_arrow(tc, dev_table):
    return g.plan.materialize(tc, dev_table).to_arrow(tc.ctx)


def run_node(tc, table, keys, aggs_of, below=None):
    src = g.MemoryExec([table])
    inp = below(src) if below else src
    s = inp.schema()
    node = g.AggregateExec("Single", [(col(k, s), k) for k in keys], aggs_of(s), inp)
    return device_arrow(tc, node.execute(0, tc)), node


def rows_of(t, nkeys, tnames):
    """{key tuple: tuple of the aggregate columns in canonical form}."""
    keys = list(zip(*[t.column(i).to_pylist() for i in range(nkeys)])) if nkeys else [()] * t.num_rows
    vals = list(zip(*[canon_column(t.column(nkeys + i), tn) for i, tn in enumerate(tnames)]))
    assert len(set(keys)) == len(keys) == t.num_rows
    return dict(zip(keys, vals))


def median_agg(name="m", c="v", **kw):
    return lambda s: dict({"fn": "MEDIAN", "expr": col(c, s), "name": name}, **kw)


def check_median(tc, keys, vals, valid, tname, n, key_types):
    """One MEDIAN over (vals, valid) grouped by `keys` = [(name, values, valid)]: the whole result against the restatement."""
    arrays = [pa.array(kv, kt, mask=~kok) for (_, kv, kok), kt in zip(keys, key_types)] + [arrow_column(vals, valid, tname)]
    t = pa.Table.from_arrays(arrays, names=[k[0] for k in keys] + ["v"])
    got, _ = run_node(tc, t, [k[0] for k in keys], lambda s: [median_agg()(s)])
    assert got.schema.names == [k[0] for k in keys] + ["m"] and got.column(len(keys)).type == PA[tname]
    exp = expected_medians([(kv, kok) for _, kv, kok in keys], vals, valid, tname, n, ungrouped=not keys)
    assert rows_of(got, len(keys), [tname]) == {k: (v,) for k, v in exp.items()}
    return exp


def shuffled_groups(r, sizes):
    ids = np.repeat(np.arange(len(sizes)), sizes)
    r.shuffle(ids)
    return ids


# ------------------------------------------------------------------------------------ segment shapes
def test_segment_shapes_in_one_table(tc):
    r = np.random.default_rng(1)
    #        first                                                  2047 2048 2049       all NULL  NULLs inside     last
    sizes = [1, 254, 1, 1, 2, 3, 63, 64, 65, 255, 256, 257, 825, 1, 1, 5000, 10, 9, 10, 11, 12, 1]
    heads = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    assert {255, 256, 257, 2047, 2048, 2049} <= set(heads.tolist())      # heads on both sides of a 256-row block edge and a 2,048-row scan tile edge
    ids = shuffled_groups(r, sizes)
    n = len(ids)
    vals = r.integers(-10**12, 10**12, n)
    valid = np.ones(n, dtype=bool)
    valid[ids == 16] = False
    for gid, survivors in ((17, 4), (18, 5), (19, 1), (20, 2)):      # even / odd numbers of survivors among NULLs
        rows = np.flatnonzero(ids == gid)
        valid[rows[survivors:]] = False
    exp = check_median(tc, [("k", (ids * 7 - 30).astype(np.int32), np.ones(n, dtype=bool))], vals, valid, "Int64", n, [pa.int32()])
    assert len(exp) == len(sizes) and exp[(16 * 7 - 30,)] is None and sum(v is None for v in exp.values()) == 1


@pytest.mark.parametrize("ngroups", [1, 63, 64, 65, 130])
def test_validity_words_of_the_result(tc, ngroups):
    """The result's validity is written as whole 64-bit words from a wave-wide ballot: NULL and non-NULL medians mixed, so that no
    word is 0 or all ones, and a last partial word."""
    r = np.random.default_rng(ngroups)
    ids = shuffled_groups(r, r.integers(1, 5, ngroups))
    n = len(ids)
    valid = ids % 2 == 0      # every odd group is all NULL
    exp = check_median(tc, [("k", ids.astype(np.int32), np.ones(n, dtype=bool))], r.integers(-99, 99, n).astype(np.int16), valid, "Int16", n, [pa.int32()])
    nulls = [exp[(k,)] is None for k in range(ngroups)]
    assert len(exp) == ngroups
    for w in range(0, ngroups, 64):      # a word of one segment (G = 1, 65) is that segment's bit: set
        word = nulls[w:w + 64]
        assert not all(word) and (len(word) == 1 or any(word)), w


# ------------------------------------------------------------------------------------ every argument type
def pairs_of(tname):
    """Even groups of two with their known answers [(lo, hi, median)]."""
    if tname == "Decimal":
        return [(10**30, 10**30 + 1, 10**30), (-10**30 - 3, 10**30, -1), (-10**33 - 1, -10**33, -10**33), (-3 * 10**4, 0, -15000), (-3, 0, -1)]
    dt = NP[tname]
    if tname == "Float32":      # sums that round in binary32
        return [(dt(1e-8), dt(1.0), dt(0.5)), (dt(1.0), dt(16777216.0), dt(8388608.0)), (dt(3.0e38), dt(3.0e38), dt(np.inf)), (dt(-3.0), dt(0.0), dt(-1.5))]
    if tname == "Float64":
        return [(dt(1.0), dt(9007199254740992.0), dt(4503599627370496.0)), (dt(-0.0), dt(0.0), dt(0.0)), (dt(-np.inf), dt(5.0), dt(-np.inf)), (dt(-3.0), dt(0.0), dt(-1.5))]
    ii = np.iinfo(dt)
    if ii.min < 0:
        out = [(-3, 0, -1), (ii.max, ii.max, -1), (ii.min, ii.min, 0), (ii.max - 1, ii.max, -1)]
        if tname == "Int8":
            out.append((100, 120, -18))
        if tname == "Int64":
            out.append((2**62, 2**62 + 2, -2**62 + 1))
        return out
    out = [(ii.max, ii.max, ii.max - 1 >> 1), (1, 2, 1), (0, ii.max, ii.max // 2)]
    if tname == "UInt64":
        out.append((2**63, 2**63, 0))
    return out


@pytest.mark.parametrize("tname", TYPES)
def test_argument_types(tc, tname):
    r = np.random.default_rng(len(tname) + 40)
    pairs = pairs_of(tname)
    # totalOrder inside a group: -0.0 before 0.0, a positive NaN last, infinities at the ends
    fives = [[-1.0, -0.0, 0.0, np.nan, np.nan], [-1.0, -1.0, -0.0, 0.0, np.nan], [np.inf, -np.inf, -0.0, np.nan, 7.0]] if tname == "Float64" else []
    sizes = [2] * len(pairs) + [5] * len(fives) + list(r.integers(1, 10, 40))
    ids = np.repeat(np.arange(len(sizes)), sizes)
    n = len(ids)
    if tname == "Decimal":
        vals = np.array([int(x) * 10**22 + int(y) for x, y in zip(r.integers(-10**15, 10**15, n), r.integers(0, 10**18, n))], dtype=object)
    elif is_float(tname):
        vals = (r.standard_normal(n) * 1e3).astype(NP[tname])
    else:
        ii = np.iinfo(NP[tname])
        vals = r.integers(ii.min, ii.max, n, dtype=NP[tname], endpoint=True)
    valid = r.random(n) >= 0.15
    for i, (lo, hi, _) in enumerate(pairs):
        vals[2 * i], vals[2 * i + 1], valid[2 * i], valid[2 * i + 1] = hi, lo, True, True
    for i, five in enumerate(fives):
        rows = slice(2 * len(pairs) + 5 * i, 2 * len(pairs) + 5 * i + 5)
        vals[rows], valid[rows] = five, True
    order = r.permutation(n)
    ids, vals, valid = ids[order], vals[order], valid[order]
    exp = check_median(tc, [("k", ids.astype(np.int32), np.ones(n, dtype=bool))], vals, valid, tname, n, [pa.int32()])
    for i, (_, _, want) in enumerate(pairs):      # the known answers, independent of the restatement
        assert exp[(i,)] == canon(want, tname), (tname, i)
    if tname == "Float64":
        assert [exp[(len(pairs) + i,)] for i in range(3)] == [canon(0.0, tname), canon(-0.0, tname), canon(7.0, tname)]


# ------------------------------------------------------------------------------------ keys
def key_column(r, kind, n):
    if kind == "Int32":
        return pa.int32(), r.integers(-5, 40, n).astype(np.int32), np.ones(n, dtype=bool)
    if kind == "Int64?":
        return pa.int64(), r.integers(-2**40, 2**40, 30)[r.integers(0, 30, n)], r.random(n) >= 0.1
    if kind == "Int16?":
        return pa.int16(), r.integers(-3, 4, n).astype(np.int16), r.random(n) >= 0.2
    if kind == "Int8":
        return pa.int8(), r.integers(-2, 2, n).astype(np.int8), np.ones(n, dtype=bool)
    if kind == "UInt16":
        return pa.uint16(), r.integers(65530, 65536, n).astype(np.uint16), np.ones(n, dtype=bool)
    assert kind == "Utf8?"
    words = np.array(["", "a", "ab", "ab ", "b", "fifteen bytes ok", "zz", "Zz"], dtype=object)
    words[5] = "fifteen bytes.."
    assert max(len(w) for w in words) == 15
    return pa.utf8(), words[r.integers(0, len(words), n)], r.random(n) >= 0.1


@pytest.mark.parametrize("kinds", [[], ["Int32"], ["Int64?"], ["Int32", "Int16?"], ["Utf8?"], ["Int8", "Int32", "Utf8?", "Int64?", "UInt16"]], ids=lambda k: "-".join(k) or "none")
@pytest.mark.parametrize("n", [0, 3000])
def test_keys(tc, kinds, n):
    r = np.random.default_rng(7 + len(kinds))
    cols = [key_column(r, kind, n) for kind in kinds]
    keys = [("k%d" % i, kv, kok) for i, (_, kv, kok) in enumerate(cols)]
    exp = check_median(tc, keys, r.integers(-10**6, 10**6, n), r.random(n) >= 0.2, "Int64", n, [kt for kt, _, _ in cols])
    if n == 0:
        assert exp == ({(): None} if not kinds else {})      # ungrouped over zero rows: one row holding NULL; grouped: zero rows
    else:
        assert len(exp) > (1 if kinds else 0) and (not any("?" in k for k in kinds) or any(None in k for k in exp))


# ------------------------------------------------------------------------------------ next to other aggregates
def mixed_table(seed, n=4000, ngroups=37):
    r = np.random.default_rng(seed)
    return {"k": r.integers(0, ngroups, n).astype(np.int32), "v": r.integers(-10**9, 10**9, n), "v_ok": r.random(n) >= 0.15,
            "w": (r.standard_normal(n) * 100).astype(np.float64), "w_ok": r.random(n) >= 0.15, "f": r.integers(0, 10, n).astype(np.int32), "n": n}


def mixed_arrow(d):
    return pa.table({"k": pa.array(d["k"]), "v": pa.array(d["v"], mask=~d["v_ok"]), "w": pa.array(d["w"], mask=~d["w_ok"]), "f": pa.array(d["f"])})


def test_median_beside_other_aggregates(tc):
    d = mixed_table(3)
    t = mixed_arrow(d)
    plain = [("SUM", "v", "s"), ("COUNT", "v", "c"), ("AVG", "v", "a"), ("MIN", "w", "mn"), ("STDDEV", "v", "sd")]

    def aggs(s, with_median=True):
        out = [{"fn": fn, "expr": col(c, s), "name": name} for fn, c, name in plain]
        if with_median:      # interleaved with the plain ones, in declared order
            out.insert(1, median_agg("mv", "v")(s)); out.insert(4, median_agg("mw", "w")(s)); out.append(median_agg("mv2", "v")(s))
        return out
    got, node = run_node(tc, t, ["k"], aggs)
    assert got.schema.names == ["k", "s", "mv", "c", "a", "mw", "mn", "sd", "mv2"]
    assert [f["name"] for f in node.schema()] == got.schema.names
    assert [pa.int64(), pa.float64(), pa.int64()] == [got.column(c).type for c in ("mv", "mw", "mv2")]
    keys = [(d["k"], np.ones(d["n"], dtype=bool))]
    mv, mw = expected_medians(keys, d["v"], d["v_ok"], "Int64", d["n"]), expected_medians(keys, d["w"], d["w_ok"], "Float64", d["n"])
    by_key = {k: i for i, k in enumerate(got.column("k").to_pylist())}
    assert len(by_key) == 37
    for name, exp, tn in (("mv", mv, "Int64"), ("mw", mw, "Float64"), ("mv2", mv, "Int64")):
        c = canon_column(got.column(name), tn)
        assert {k: c[i] for k, i in by_key.items()} == {k[0]: v for k, v in exp.items()}, name
    # the plain columns: what the same node without the MEDIANs returns
    ref, _ = run_node(tc, t, ["k"], lambda s: aggs(s, False))
    ref_by_key = {k: i for i, k in enumerate(ref.column("k").to_pylist())}
    worst = 0.0
    for _, _, name in plain:
        a, b = got.column(name).to_pylist(), ref.column(name).to_pylist()
        assert got.column(name).type == ref.column(name).type
        for k, i in by_key.items():
            x, y = a[i], b[ref_by_key[k]]
            if name == "sd":
                assert x is not None and y is not None
                worst = max(worst, abs(x - y) / abs(y))
            else:
                assert x == y, (name, k)
    print("stddev beside a MEDIAN against the node without it: largest relative difference %.3g" % worst)
    assert worst <= REL_STDDEV


def test_no_rows_beside_other_aggregates(tc):
    t = mixed_arrow(mixed_table(2, n=0))
    aggs = lambda s: [{"fn": "COUNT", "expr": col("v", s), "name": "c"}, median_agg("m", "v")(s), {"fn": "SUM", "expr": col("v", s), "name": "s"}]
    got, _ = run_node(tc, t, ["k"], aggs)
    assert got.num_rows == 0 and got.schema.names == ["k", "c", "m", "s"]
    got, _ = run_node(tc, t, [], aggs)      # ungrouped: one row
    assert [c.to_pylist() for c in got.columns] == [[0], [None], [None]] and got.column("m").type == pa.int64()


def test_more_columns_than_one_projection_writes(tc):
    """One key, the argument and eleven columns the SUMs read: 13 columns leave the projection, which takes two project operators."""
    r = np.random.default_rng(12)
    n = 2000
    k = r.integers(0, 9, n).astype(np.int32)
    c = [r.integers(-1000, 1000, n) for _ in range(12)]
    t = pa.table(dict({"k": pa.array(k)}, **{"c%d" % i: pa.array(v) for i, v in enumerate(c)}))
    pairs = [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 11)]
    got, _ = run_node(tc, t, ["k"], lambda s: [median_agg("m", "c0")(s)] + [{"fn": "SUM", "expr": binary(col("c%d" % a, s), Op.Plus, col("c%d" % b, s)), "name": "s%d" % a} for a, b in pairs])
    med = expected_medians([(k, np.ones(n, dtype=bool))], c[0], np.ones(n, dtype=bool), "Int64", n)
    assert rows_of(got, 1, ["Int64"] * 7) == {key: (m,) + tuple(int((c[a] + c[b])[k == key[0]].sum()) for a, b in pairs) for key, m in med.items()}


def test_two_medians_and_a_filter(tc):
    d = mixed_table(4)
    pred = lambda s: binary(col("f", s), Op.Lt, lit(3, "Int32"))
    got, _ = run_node(tc, mixed_arrow(d), ["k"], lambda s: [median_agg("mv", "v")(s), median_agg("mw", "w")(s), median_agg("mvf", "v", filter=pred(s))(s), median_agg("mv_again", "v")(s)])
    keys = [(d["k"], np.ones(d["n"], dtype=bool))]
    mv, mw = expected_medians(keys, d["v"], d["v_ok"], "Int64", d["n"]), expected_medians(keys, d["w"], d["w_ok"], "Float64", d["n"])
    mvf = expected_medians(keys, d["v"], d["v_ok"] & (d["f"] < 3), "Int64", d["n"])      # a row the filter does not pass counts as a NULL argument
    assert mvf != mv and len(mvf) == len(mv) == 37
    assert rows_of(got, 1, ["Int64", "Float64", "Int64", "Int64"]) == {k: (mv[k], mw[k], mvf[k], mv[k]) for k in mv}


def test_fused_filter_and_computed_projection_below(tc):
    d = mixed_table(5)

    def below(src):
        s = src.schema()
        proj = g.ProjectionExec([(col("k", s), "k"), (binary(binary(col("v", s), Op.Multiply, lit(2)), Op.Plus, col("f", s)), "x"), (col("f", s), "f")], src)
        ps = proj.schema()
        return g.FilterExec(binary(col("f", ps), Op.Gt, lit(1, "Int32")), proj)
    got, _ = run_node(tc, mixed_arrow(d), ["k"], lambda s: [median_agg("m", "x")(s), {"fn": "COUNT", "expr": col("x", s), "name": "c"}], below)
    sel = d["f"] > 1
    x = d["v"] * 2 + d["f"]
    exp = expected_medians([(d["k"][sel], np.ones(int(sel.sum()), dtype=bool))], x[sel], d["v_ok"][sel], "Int64", int(sel.sum()))
    counts = {int(k): int((d["v_ok"] & sel & (d["k"] == k)).sum()) for k in np.unique(d["k"][sel])}
    assert got.column("m").type == pa.int64()
    assert rows_of(got, 1, ["Int64", "Int64"]) == {k: (v, counts[k[0]]) for k, v in exp.items()}


def test_ungrouped_over_a_million_rows(tc):
    """2^20 + 3 rows, one sort key: the sort hands the key column back in order (it is then read as it lies, not through the permutation)."""
    r = np.random.default_rng(6)
    n = (1 << 20) + 3
    vals, valid = r.integers(-2**40, 2**40, n), r.random(n) >= 0.1
    exp = check_median(tc, [], vals, valid, "Int64", n, [])
    v = np.sort(vals[valid])
    assert len(v) % 2 == 0 and exp[()] == trunc_half(int(v[len(v) // 2 - 1]) + int(v[len(v) // 2]))


def test_one_plan_handle_three_executions(tc):
    """The first execution runs synchronously; later ones may defer the nodes around the MEDIAN node, never the node itself."""
    d = mixed_table(8)
    src = g.MemoryExec([mixed_arrow(d)])
    s = src.schema()
    flt = g.FilterExec(binary(col("f", s), Op.Lt, lit(8, "Int32")), src)
    agg = g.AggregateExec("Single", [(col("k", s), "k")], [median_agg("m", "v")(s), {"fn": "SUM", "expr": col("v", s), "name": "s"}], flt)
    os_ = agg.schema()
    plan = g.NativePlan(g.SortExec([{"expr": col("k", os_), "asc": True, "nulls_first": False}], agg), tc)
    sel = d["f"] < 8
    exp = expected_medians([(d["k"][sel], np.ones(int(sel.sum()), dtype=bool))], d["v"][sel], d["v_ok"][sel], "Int64", int(sel.sum()))
    runs = [plan.execute(0).to_arrow() for _ in range(3)]
    assert runs[0].column("k").to_pylist() == sorted(k[0] for k in exp)
    assert runs[0].column("m").to_pylist() == [exp[(k,)] for k in runs[0].column("k").to_pylist()]
    assert runs[1].equals(runs[0]) and runs[2].equals(runs[0])
    m = [x for x in plan.metrics() if x["node"] == "AggregateExec"][0]
    assert m["output_rows"] == 3 * len(exp) and m["elapsed_compute"] > 0


# ------------------------------------------------------------------------------------ the C entry points on their own
def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def column_struct(type_id, data, validity, n):
    c = B.gpuq_column()
    c.type, c.repr, c.data, c.validity, c.length = type_id, B.REPR_ARROW, data.data_ptr(), (validity.data_ptr() if validity is not None else None), n
    return c


def bitmap(valid):
    return np.packbits(np.concatenate([valid, np.zeros((-len(valid)) % 64 + 64, dtype=bool)]), bitorder="little")


@pytest.mark.parametrize("n", [0, 1, 65, 2049])
def test_segment_heads_entry_point(tc, n):
    import torch
    r = np.random.default_rng(n)
    k1, ok1, k2 = r.integers(0, 2, n).astype(np.int32), r.random(n) >= 0.3, r.integers(0, 2, n)
    k1[~ok1] = r.integers(-9, 9, int((~ok1).sum()))      # NULL equals NULL, whatever bytes lie under it
    d1, v1, d2 = to_device(np.concatenate([k1, np.zeros(1, k1.dtype)])), to_device(bitmap(ok1)), to_device(np.concatenate([k2, np.zeros(1, k2.dtype)]))
    cols = (B.gpuq_column * 2)(column_struct(B.T_INT32, d1, v1, n), column_struct(B.T_INT64, d2, None, n))
    seg, starts, cnt = (torch.full((n + 2,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    tc.ctx.check(tc.ctx.L.gpuq_segment_heads(tc.ctx.h, tc.stream_ptr(), cols, 2, n, seg.data_ptr(), starts.data_ptr(), n, cnt.data_ptr()))
    tc.sync()
    a = np.where(ok1, k1, -100)
    head = np.ones(n, dtype=bool)
    head[1:] = (a[1:] != a[:-1]) | (k2[1:] != k2[:-1])
    exp_starts = np.flatnonzero(head).tolist() + [n]
    assert int(cnt[0].item()) == int(head.sum())
    assert starts.cpu().numpy()[:len(exp_starts)].tolist() == exp_starts and starts.cpu().numpy()[len(exp_starts):].tolist() == [-7] * (n + 2 - len(exp_starts))
    assert seg.cpu().numpy()[:n].tolist() == (np.cumsum(head) - 1).tolist() and seg.cpu().numpy()[n:].tolist() == [-7, -7]


def test_segment_median_entry_point(tc):
    import torch
    vals = np.array([-5, 3, 9, 100, 120, 7, 8, -3, 0, 11, 1], dtype=np.int8)      # NULLs last inside every segment
    ok = np.array([1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0], dtype=bool)
    starts = np.array([0, 3, 3, 5, 7, 9, 11], dtype=np.int32)      # [-5 3 9] [] [100 120] [7 NULL] [-3 0] [NULL NULL]
    d, v, s = to_device(vals), to_device(bitmap(ok)), to_device(starts)
    c = column_struct(B.T_INT8, d, v, len(vals))
    out, out_valid = torch.full((16,), 77, dtype=torch.int8, device="cuda"), torch.full((2,), -1, dtype=torch.int64, device="cuda")
    tc.ctx.check(tc.ctx.L.gpuq_segment_median(tc.ctx.h, tc.stream_ptr(), C.byref(c), s.data_ptr(), 6, out.data_ptr(), out_valid.data_ptr()))
    tc.sync()
    assert out.cpu().numpy()[:8].tolist() == [3, 0, -18, 7, -1, 0, 77, 77]
    assert out_valid.cpu().numpy().tolist() == [0b011101, -1]      # one whole word, nothing beyond it


# ------------------------------------------------------------------------------------ refusals
def test_refusals_name_median(tc):
    d = mixed_table(9, n=200)
    t = mixed_arrow(d).append_column("name", pa.array(["twenty bytes of name %02d" % (i % 7) for i in range(200)]))
    src = g.MemoryExec([t])
    s = src.schema()
    with pytest.raises(g.GpuqError, match="MEDIAN.*Final"):
        g.AggregateExec("Final", [(col("k", s), "k")], [median_agg("m", "v")(s)], src).execute(0, tc)
    with pytest.raises(g.GpuqError, match="MEDIAN.*Float64 group key"):
        g.AggregateExec("Single", [(col("w", s), "w")], [median_agg("m", "v")(s)], src).execute(0, tc)
    with pytest.raises(g.GpuqError, match="MEDIAN.*longer than 15 bytes"):
        g.AggregateExec("Single", [(col("name", s), "name")], [median_agg("m", "v")(s)], src).execute(0, tc)
    with pytest.raises(g.GpuqError, match="MEDIAN"):
        g.AggregateExec("Single", [(col("k", s), "k")], [median_agg("m", "v", distinct=True)(s)], src).execute(0, tc)
    with pytest.raises(g.GpuqError, match="MEDIAN over Utf8"):
        g.AggregateExec("Single", [(col("k", s), "k")], [median_agg("m", "name")(s)], src).execute(0, tc)


# ------------------------------------------------------------------------------------ the reference's q6
def test_h2o_q6_shape(tc):
    """benchmarks/db-benchmark/groupby-datafusion.py q6: median(v3), stddev(v3) by id4, id5 -- at 200,000 rows."""
    r = np.random.default_rng(11)
    n = 200_000
    id4, id5, v3 = r.integers(1, 101, n).astype(np.int32), r.integers(1, 101, n).astype(np.int32), np.round(r.random(n) * 100, 6)
    t = pa.table({"id4": pa.array(id4), "id5": pa.array(id5), "v3": pa.array(v3)})
    got, _ = run_node(tc, t, ["id4", "id5"], lambda s: [median_agg("median_v3", "v3")(s), {"fn": "STDDEV", "expr": col("v3", s), "name": "sd_v3"}])
    ones = np.ones(n, dtype=bool)
    exp = expected_medians([(id4, ones), (id5, ones)], v3, ones, "Float64", n)
    assert len(exp) > 9_900
    assert rows_of(got.select(["id4", "id5", "median_v3"]), 2, ["Float64"]) == {k: (v,) for k, v in exp.items()}
    order = np.lexsort((id5, id4))
    a, b, v = id4[order], id5[order], v3[order]
    cuts = np.flatnonzero(np.concatenate([[True], (a[1:] != a[:-1]) | (b[1:] != b[:-1])]))
    sd = {(int(a[i]), int(b[i])): (float(np.std(x, ddof=1)) if len(x) > 1 else None) for i, x in zip(cuts, np.split(v, cuts[1:]))}
    worst = 0.0
    for k4, k5, x in zip(got.column("id4").to_pylist(), got.column("id5").to_pylist(), got.column("sd_v3").to_pylist()):
        y = sd[(k4, k5)]
        assert (x is None) == (y is None)
        if y is not None:
            worst = max(worst, abs(x - y) / abs(y))
    print("q6 stddev: largest relative difference %.3g" % worst)
    assert worst <= REL_STDDEV
