"""The scalar functions coalesce, nullif, nanvl, isnan, iszero, abs, signum, ceil, floor, trunc, round and sqrt on the
device: through ProjectionExec, as FilterExec predicates, as aggregate arguments and group keys; in the interpreter and in the run-time
compiled evaluator.  Expected values come from numpy and pyarrow.compute alone.  Every comparison is exact -- floats by their bit
patterns, so -0.0 is not 0.0 -- except that a NaN is matched by any NaN: IEEE-754 leaves the sign and payload of a generated NaN to the
implementation (sqrt(-1.0) is a negative NaN on x86 and a positive one here).

Rows: 0, 1, 63, 64, 65 (the wave boundaries) and 4097 (one block tail).  Each argument column exists required and with ~20 % NULLs."""
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd import expr as E
from arrow_ballista_amd.expr import Operator as Op
from arrow_ballista_amd.expr import binary, col, lit

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 4097]
INTS = {"Int8": (np.int8, pa.int8()), "Int16": (np.int16, pa.int16()), "Int32": (np.int32, pa.int32()), "Int64": (np.int64, pa.int64()),
        "UInt8": (np.uint8, pa.uint8()), "UInt16": (np.uint16, pa.uint16()), "UInt32": (np.uint32, pa.uint32()), "UInt64": (np.uint64, pa.uint64())}
FLOATS = {"Float32": (np.float32, pa.float32(), np.uint32, 23), "Float64": (np.float64, pa.float64(), np.uint64, 52)}
HALF_AWAY = "half_towards_infinity"


# ------------------------------------------------------------------------------------ running and comparing
def table_of(cols, nullable):
    """{name: (values, arrow type, validity)} -> a table whose fields are required, or nullable with the validity applied."""
    arrays, fields = [], []
    for name, (v, t, valid) in cols.items():
        arrays.append(pa.array(v, type=t, mask=~valid if nullable else None) if not isinstance(v, pa.Array) else (v if not nullable else pc.if_else(pa.array(valid), v, pa.scalar(None, t))))
        fields.append(pa.field(name, t, nullable=nullable))
    return pa.Table.from_arrays(arrays, schema=pa.schema(fields))


def run(tc, node, runs=1):
    p = g.NativePlan(node, tc)
    first = p.execute(0).to_arrow()
    for again in range(1, runs):      # deferred from the second execution on
        t = p.execute(0).to_arrow()
        assert t.schema == first.schema
        for name in first.column_names:
            same(t[name], first[name], ("execution", again, name))
    return first


def projected(tc, t, named, chunk=3):
    """{name: column} of the expressions named(schema) -> [(expr, name)], a few per ProjectionExec (the outputs of one are all live at once)."""
    src = g.MemoryExec([t])
    exprs = named(src.schema())
    out = {}
    for i in range(0, len(exprs), chunk):
        got = run(tc, g.ProjectionExec(exprs[i:i + chunk], src))
        assert got.num_rows == t.num_rows
        out.update({n: got[n] for n in got.column_names})
    return out


def filtered(tc, t, pred_of):
    src = g.MemoryExec([t])
    return run(tc, g.FilterExec(pred_of(src.schema()), src))


def evaluators(tc, n):
    """The interpreter, and for the 4097-row case the run-time compiled evaluator as well (a launch of it is asserted)."""
    yield "auto"
    if n == max(SIZES) and tc.ctx.jit_stats()["available"]:
        before = tc.ctx.jit_stats()["launches"]
        tc.ctx.set_jit("force")
        try:
            yield "force"
        finally:
            tc.ctx.set_jit("auto")
        assert tc.ctx.jit_stats()["launches"] > before, "no JIT launch happened"


def same(got, want, what=""):
    """Exact: type, NULLs, values; floats by bit pattern with NaN matching NaN."""
    got = got.combine_chunks() if isinstance(got, pa.ChunkedArray) else got
    want = want.combine_chunks() if isinstance(want, pa.ChunkedArray) else want
    if pa.types.is_timestamp(want.type):      # the engine does not carry the time zone
        assert pa.types.is_timestamp(got.type) and got.type.unit == want.type.unit, what
        got, want = got.cast(pa.int64()), want.cast(pa.int64())
    assert got.type == want.type, (what, got.type, want.type)
    assert len(got) == len(want), what
    assert got.is_null().equals(want.is_null()), (what, got.to_pylist()[:24], want.to_pylist()[:24])
    if pa.types.is_floating(want.type):
        bits = np.uint32 if want.type == pa.float32() else np.uint64
        a, b = np.asarray(got.fill_null(0)), np.asarray(want.fill_null(0))
        nan = np.isnan(b)
        bad = np.flatnonzero((a.view(bits) != b.view(bits)) & ~(nan & np.isnan(a)))
        assert len(bad) == 0, (what, bad[:8], a[bad[:8]], b[bad[:8]])
    else:
        assert got.equals(want), (what, got.to_pylist()[:24], want.to_pylist()[:24])


def arr(values, t, valid, nullable):
    return pa.array(values, type=t, mask=~valid if nullable else None)


def validity(r, n):
    return r.random(n) >= 0.2


# ------------------------------------------------------------------------------------ floats
def float_values(r, tname, n):
    dt, _, _, mant = FLOATS[tname]
    one = dt(1)
    forced = [0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, np.nextafter(dt(0.5), dt(0)), dt(2) ** mant + one, -(dt(2) ** mant + one), dt(2) ** (mant + 1), -(dt(2) ** (mant + 1)),
              1e300, -1e300, np.inf, -np.inf, np.nan, np.nextafter(dt(0), one)]      # 0.49999999999999994 for a double; 2^52 + 1 is odd with an ulp of 1
    with np.errstate(over="ignore"):
        forced = np.array(forced, dtype=np.float64).astype(dt)      # +-1e300 is +-inf as a Float32
        x = (r.standard_normal(n) * 10.0 ** r.integers(-2, 7, n)).astype(dt)
    x[:min(n, len(forced))] = forced[:min(n, len(forced))]
    if n == max(SIZES):      # otherwise floor = ceil = trunc and the test shows nothing
        rest = x[len(forced):]
        assert np.mean(rest != np.trunc(rest)) >= 0.25 and (rest < 0).any() and (rest > 0).any()
    return x


def half_away(x, dt):
    return pc.round(pa.array(x), 0, round_mode=HALF_AWAY).to_numpy(zero_copy_only=False).astype(dt, copy=False)


def round_n(x, nd, dt):
    p = dt(10.0 ** nd)
    with np.errstate(over="ignore", invalid="ignore"):
        return (half_away((x * p).astype(dt, copy=False), dt) / p).astype(dt, copy=False)


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("tname", list(FLOATS))
def test_float_functions(tc, tname, nullable):
    dt, pt, _, _ = FLOATS[tname]
    for n in SIZES:
        r = np.random.default_rng(n + len(tname))
        x, y = float_values(r, tname, n), float_values(r, tname, n)[::-1].copy()
        vx, vy = validity(r, n), validity(r, n)
        t = table_of({"x": (x, pt, vx), "y": (y, pt, vy)}, nullable)
        vxy = vx & vy

        def named(s):
            cx, cy = col("x", s), col("y", s)
            return [(E.floor(cx), "floor"), (E.ceil(cx), "ceil"), (E.trunc(cx), "trunc"), (E.round_(cx), "round"), (E.round_(cx, 0), "round0"), (E.round_(cx, 2), "round2"),
                    (E.round_(cx, 22), "round22"), (E.abs_(cx), "abs"), (E.signum(cx), "signum"), (E.sqrt(cx), "sqrt"), (E.isnan(cx), "isnan"), (E.iszero(cx), "iszero"),
                    (E.nanvl(cx, cy), "nanvl")]
        with np.errstate(invalid="ignore"):
            want = {"floor": np.floor(x), "ceil": np.ceil(x), "trunc": np.trunc(x), "round": half_away(x, dt), "round0": round_n(x, 0, dt), "round2": round_n(x, 2, dt),
                    "round22": round_n(x, 22, dt), "abs": pc.abs(pa.array(x)).to_numpy(zero_copy_only=False), "signum": np.sign(x), "sqrt": np.sqrt(x)}
        assert all(v.dtype == dt for v in want.values())
        if n > 1:
            assert np.signbit(want["round"][1]) and np.signbit(want["floor"][1]) and not np.signbit(want["signum"][1])      # x[1] is -0.0
        for mode in evaluators(tc, n):
            out = projected(tc, t, named)
            for name, w in want.items():
                same(out[name], arr(w, pt, vx, nullable), (tname, n, mode, name))
            same(out["isnan"], arr(np.isnan(x), pa.bool_(), vx, nullable), (tname, n, mode, "isnan"))
            same(out["iszero"], arr(x == 0, pa.bool_(), vx, nullable), (tname, n, mode, "iszero"))
            same(out["nanvl"], arr(np.where(np.isnan(x), y, x), pt, vxy, nullable), (tname, n, mode, "nanvl"))      # NULL if either side is
            # FilterExec: abs(x) < c, and a second predicate over the rounding and the tests (a NULL predicate drops the row)
            c = 40.0
            keep = (np.abs(x) < dt(c)) & (vx if nullable else True)
            got = filtered(tc, t, lambda s: binary(E.abs_(col("x", s)), Op.Lt, lit(c, tname)))
            same(got["x"], t["x"].filter(pa.array(keep)), (tname, n, mode, "abs(x) < c"))
            with np.errstate(invalid="ignore"):
                keep = ((np.floor(x) == half_away(x, dt)) & ~(x == 0) | np.isnan(x)) & (vx if nullable else True)
            got = filtered(tc, t, lambda s: E.or_(E.and_(binary(E.floor(col("x", s)), Op.Eq, E.round_(col("x", s))), E.not_(E.iszero(col("x", s)))), E.isnan(col("x", s))))
            if n == max(SIZES):
                assert 0 < keep.sum() < n
            same(got["y"], t["y"].filter(pa.array(keep)), (tname, n, mode, "floor(x) = round(x)"))


@pytest.mark.parametrize("tname", ["Int8", "Int32", "Int64", "UInt16", "UInt64"])
def test_integer_arguments_of_the_float_functions(tc, tname):
    """An integer argument is cast to Float64 first; abs keeps the integer type and wraps at the minimum."""
    dt, pt = INTS[tname]
    ii = np.iinfo(dt)
    for n in (65, 4097):
        r = np.random.default_rng(n)
        x = r.integers(ii.min, ii.max, n, dtype=dt, endpoint=True)
        x[:4] = [ii.min, ii.max, 0, 1]
        vx = validity(r, n)
        vx[:4] = True
        t = table_of({"x": (x, pt, vx)}, True)
        f = x.astype(np.float64)
        for mode in evaluators(tc, n):
            out = projected(tc, t, lambda s: [(E.abs_(col("x", s)), "abs"), (E.signum(col("x", s)), "signum"), (E.sqrt(col("x", s)), "sqrt"), (E.round_(col("x", s), 2), "round2"),
                                              (E.ceil(col("x", s)), "ceil")])
            same(out["abs"], pc.abs(t["x"]), (tname, n, mode, "abs"))      # pyarrow's unchecked abs wraps: abs(-128) is -128
            with np.errstate(invalid="ignore"):
                same(out["signum"], arr(np.sign(f), pa.float64(), vx, True), (tname, n, mode, "signum"))
                same(out["sqrt"], arr(np.sqrt(f), pa.float64(), vx, True), (tname, n, mode, "sqrt"))
            same(out["round2"], arr(round_n(f, 2, np.float64), pa.float64(), vx, True), (tname, n, mode, "round2"))
            same(out["ceil"], arr(f, pa.float64(), vx, True), (tname, n, mode, "ceil"))
    if ii.min < 0:
        assert out["abs"][0].as_py() == ii.min


def test_abs_of_decimals(tc):
    r = np.random.default_rng(5)
    n = 4097
    vals = [int(a) * 2**40 + int(b) for a, b in zip(r.integers(-2**62, 2**62, n), r.integers(0, 2**40, n))]      # beyond 2^64
    vals[:3] = [0, -(10**38 - 1), 10**38 - 1]
    v = validity(r, n)
    import decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        d = [decimal.Decimal(x).scaleb(-4) for x in vals]
    dec = pa.decimal128(38, 4)
    t = pa.Table.from_arrays([pc.if_else(pa.array(v), pa.array(d, dec), pa.scalar(None, dec))], schema=pa.schema([pa.field("d", dec)]))
    assert any(abs(x) > 2**64 for x in vals) and any(x < 0 for x in vals)
    for mode in evaluators(tc, n):
        out = projected(tc, t, lambda s: [(E.abs_(col("d", s)), "abs")])
        same(out["abs"], pc.if_else(pa.array(v), pa.array([x.copy_abs() for x in d], dec), pa.scalar(None, dec)), mode)


# ------------------------------------------------------------------------------------ coalesce
def column_of(r, kind, n):
    """(arrow array without NULLs, arrow type) of n random values of one of the types coalesce is tested over."""
    if kind in INTS:
        dt, pt = INTS[kind]
        ii = np.iinfo(dt)
        return pa.array(r.integers(ii.min, ii.max, n, dtype=dt, endpoint=True), pt), pt
    if kind == "Float32":
        return pa.array(float_values(r, kind, n), pa.float32()), pa.float32()
    if kind == "Decimal128":
        import decimal
        with decimal.localcontext() as ctx:
            ctx.prec = 60
            vals = [decimal.Decimal(int(a) * 2**50 + int(b)).scaleb(-4) for a, b in zip(r.integers(-2**62, 2**62, n), r.integers(0, 2**50, n))]      # beyond 2^64
        return pa.array(vals, pa.decimal128(38, 4)), pa.decimal128(38, 4)
    if kind == "Date32":
        return pa.array(r.integers(-30000, 30000, n).astype(np.int32), pa.int32()).cast(pa.date32()), pa.date32()
    if kind == "Timestamp":
        return pa.array(r.integers(-2**62, 2**62, n), pa.timestamp("ns")), pa.timestamp("ns")
    if kind == "Boolean":
        return pa.array(r.random(n) < 0.5, pa.bool_()), pa.bool_()
    words = ["", "a", "ab", "fifteen bytes ok", "fifteen_bytes_1", "x y", "NULL", "none", "zz"]
    return pa.array([words[i] if len(words[i]) <= 15 else words[i][:15] for i in r.integers(0, len(words), n)], pa.string()), pa.string()


COALESCE_KINDS = ["Int8", "Int64", "UInt64", "Float32", "Decimal128", "Date32", "Timestamp", "Boolean", "Utf8"]


@pytest.mark.parametrize("kind", COALESCE_KINDS)
def test_coalesce(tc, kind):
    for n in SIZES:
        r = np.random.default_rng(n + 3)
        cols, fields = [], []
        for i in range(4):      # a .. d with ~20 % NULLs (d with 60 %, so that all four are NULL on some rows), e required
            v, pt = column_of(r, kind, n)
            cols.append(pc.if_else(pa.array(r.random(n) >= (0.2 if i < 3 else 0.6)), v, pa.scalar(None, pt)))
            fields.append(pa.field("abcd"[i], pt, nullable=True))
        v, pt = column_of(r, kind, n)
        cols.append(v)
        fields.append(pa.field("e", pt, nullable=False))
        t = pa.Table.from_arrays(cols, schema=pa.schema(fields))
        want = {"two": pc.coalesce(t["a"], t["d"]), "four": pc.coalesce(t["d"], t["c"], t["b"], t["a"]), "two_req": pc.coalesce(t["a"], t["e"]), "four_req": pc.coalesce(t["d"], t["a"], t["e"], t["b"]),
                "one": t["c"]}
        if n == max(SIZES):
            assert want["two"].null_count > 0 and want["four"].null_count > 0 and want["four_req"].null_count == 0
        for mode in evaluators(tc, n):
            out = projected(tc, t, lambda s: [(E.coalesce(col("a", s), col("d", s)), "two"), (E.coalesce(col("d", s), col("c", s), col("b", s), col("a", s)), "four"),
                                              (E.coalesce(col("a", s), col("e", s)), "two_req"), (E.coalesce(col("d", s), col("a", s), col("e", s), col("b", s)), "four_req"),
                                              (E.coalesce(col("c", s)), "one")], chunk=2)
            for name, w in want.items():
                same(out[name], w, (kind, n, mode, name))


def test_coalesce_in_a_filter(tc):
    """abs(coalesce(a, b)) = c."""
    for n in SIZES:
        r = np.random.default_rng(n + 17)
        a, b = r.integers(-8, 8, n), r.integers(-8, 8, n)
        va, vb = validity(r, n), validity(r, n)
        t = table_of({"a": (a, pa.int64(), va), "b": (b, pa.int64(), vb)}, True)
        keep = (np.abs(np.where(va, a, b)) == 3) & (va | vb)
        if n == max(SIZES):
            assert 0 < keep.sum() < n and (keep & ~va).any()
        for mode in evaluators(tc, n):
            got = filtered(tc, t, lambda s: binary(E.abs_(E.coalesce(col("a", s), col("b", s))), Op.Eq, lit(3)))
            same(got["a"], t["a"].filter(pa.array(keep)), (n, mode))
            same(got["b"], t["b"].filter(pa.array(keep)), (n, mode))


# ------------------------------------------------------------------------------------ nullif
@pytest.mark.parametrize("nullable", [False, True])
def test_nullif(tc, nullable):
    words = np.array(["", "a", "ab", "fifteen_bytes_1", "x"], dtype=object)
    for n in SIZES:
        r = np.random.default_rng(n + 29)
        i, j = r.integers(-3, 3, n).astype(np.int32), r.integers(-3, 3, n).astype(np.int32)
        big = 2**70
        d, e = [int(k) * big for k in r.integers(-2, 2, n)], [int(k) * big for k in r.integers(-2, 2, n)]
        s, u = words[r.integers(0, len(words), n)], words[r.integers(0, len(words), n)]
        pool = np.array([np.nan, 0.0, -0.0, 1.5, -1.5, np.inf])
        f, h = pool[r.integers(0, len(pool), n)], pool[r.integers(0, len(pool), n)]
        v = {c: validity(r, n) for c in "ijdesufh"}
        dec = pa.decimal128(38, 4)
        import decimal
        with decimal.localcontext() as ctx:
            ctx.prec = 60
            dd, ee = [decimal.Decimal(x).scaleb(-4) for x in d], [decimal.Decimal(x).scaleb(-4) for x in e]
        t = table_of({"i": (i, pa.int32(), v["i"]), "j": (j, pa.int32(), v["j"]), "d": (pa.array(dd, dec), dec, v["d"]), "e": (pa.array(ee, dec), dec, v["e"]),
                      "s": (pa.array(list(s), pa.string()), pa.string(), v["s"]), "u": (pa.array(list(u), pa.string()), pa.string(), v["u"]),
                      "f": (f, pa.float64(), v["f"]), "h": (h, pa.float64(), v["h"])}, nullable)

        def want(a, b, eq, ta):
            """a where it is not NULL and not (b not NULL and a = b)."""
            va, vb = (v[a], v[b]) if nullable else (np.ones(n, bool), np.ones(n, bool))
            keep = va & ~(vb & eq)
            return pc.if_else(pa.array(keep), t[a], pa.scalar(None, ta))
        # the engine's '=' over floats is total order: NaN = NaN, -0.0 != 0.0 -- equality of the bit patterns
        feq = f.view(np.uint64) == h.view(np.uint64)
        if n == max(SIZES):
            assert (np.isnan(f) & np.isnan(h)).any() and ((f == 0) & (h == 0) & ~feq).any()
        for mode in evaluators(tc, n):
            out = projected(tc, t, lambda sc: [(E.nullif(col("i", sc), col("j", sc)), "ij"), (E.nullif(col("d", sc), col("e", sc)), "de"), (E.nullif(col("s", sc), col("u", sc)), "su"),
                                               (E.nullif(col("f", sc), col("h", sc)), "fh"), (E.nullif(col("i", sc), lit(0, "Int32")), "i0"), (E.nullif(col("i", sc), lit(None)), "in")], chunk=2)
            same(out["ij"], want("i", "j", i == j, pa.int32()), (n, mode, "ij"))
            same(out["de"], want("d", "e", np.array(d, dtype=object) == np.array(e, dtype=object), dec), (n, mode, "de"))
            same(out["su"], want("s", "u", s == u, pa.string()), (n, mode, "su"))
            same(out["fh"], want("f", "h", feq, pa.float64()), (n, mode, "fh"))
            same(out["i0"], pc.if_else(pa.array((i != 0) & (v["i"] if nullable else True)), t["i"], pa.scalar(None, pa.int32())), (n, mode, "i0"))
            same(out["in"], t["i"], (n, mode, "in"))      # a NULL b gives a


# ------------------------------------------------------------------------------------ aggregate arguments and group keys
def test_functions_as_aggregate_arguments_and_group_keys(tc):
    """GROUP BY coalesce(k, -1) and GROUP BY abs(coalesce(k, -1) - 2) with SUM(round(x, 2)), SUM(abs(i)), COUNT(nullif(i, 0)), MAX(abs(i)), against numpy.
    x = q / 4 + 0.001, so that round(x, 2) is q / 4 exactly and the sum of the group is exact in any order (without the round it is not q / 4)."""
    for n in SIZES:
        r = np.random.default_rng(n + 41)
        k = r.integers(0, 6, n).astype(np.int32)
        vk = validity(r, n)
        q = r.integers(-400, 400, n)
        x = q / 4 + 0.001
        vx = validity(r, n)
        i = r.integers(-50, 50, n)
        vi = validity(r, n)
        t = table_of({"k": (k, pa.int32(), vk), "x": (x, pa.float64(), vx), "i": (i, pa.int64(), vi)}, True)
        assert np.array_equal(round_n(x, 2, np.float64), q / 4)
        for key_name, key_of, keys in (("coalesce", lambda s: E.coalesce(col("k", s), lit(-1, "Int32")), np.where(vk, k, -1)),
                                       ("abs", lambda s: E.abs_(binary(E.coalesce(col("k", s), lit(-1, "Int32")), Op.Minus, lit(2, "Int32"))), np.abs(np.where(vk, k, -1) - 2))):
            want = {}
            for key in np.unique(keys):
                m = keys == key
                sx, si = (q / 4)[m & vx], np.abs(i)[m & vi]
                mx = np.abs(i)[m & vi]
                want[int(key)] = (float(sx.sum()) if len(sx) else None, int(si.sum()) if len(si) else None, int((m & vi & (i != 0)).sum()), int(mx.max()) if len(mx) else None)
            for mode in evaluators(tc, n):
                src = g.MemoryExec([t])
                s = src.schema()
                aggs = [{"fn": "SUM", "expr": E.round_(col("x", s), 2), "name": "sx"}, {"fn": "SUM", "expr": E.abs_(col("i", s)), "name": "si"},
                        {"fn": "COUNT", "expr": E.nullif(col("i", s), lit(0)), "name": "c"}, {"fn": "MAX", "expr": E.abs_(col("i", s)), "name": "mx"}]
                plan = g.NativePlan(g.AggregateExec("Single", [(key_of(s), "key")], aggs, src), tc)
                for again in range(2):      # the second execution is deferred; groups come in no particular order
                    out = plan.execute(0).to_arrow()
                    assert [c.type for c in out.columns] == [pa.int32(), pa.float64(), pa.int64(), pa.int64(), pa.int64()]
                    got = {row[0]: row[1:] for row in zip(*[c.to_pylist() for c in out.columns])}
                    assert len(got) == out.num_rows and got == want, (n, key_name, mode, again)


def test_deferred_runs_give_the_same_rows(tc):
    """Three executions of one plan handle (deferred from the second): a filter over a projection, both holding new functions."""
    r = np.random.default_rng(77)
    n = 4097
    x = float_values(r, "Float64", n)
    a = r.integers(-2**31, 2**31, n).astype(np.int32)
    vx, va = validity(r, n), validity(r, n)
    t = table_of({"x": (x, pa.float64(), vx), "a": (a, pa.int32(), va)}, True)
    src = g.MemoryExec([t])
    s = src.schema()
    proj = g.ProjectionExec([(E.round_(col("x", s), 2), "r"), (E.abs_(E.coalesce(col("a", s), lit(1, "Int32"))), "ab"), (col("x", s), "x")], src)
    ps = proj.schema()
    plan = g.FilterExec(E.not_(E.iszero(E.trunc(col("x", ps)))), proj)
    out = run(tc, plan, runs=3)
    with np.errstate(invalid="ignore"):
        keep = vx & (np.trunc(x) != 0)
    same(out["r"], arr(round_n(x, 2, np.float64), pa.float64(), vx, True).filter(pa.array(keep)), "round")
    same(out["ab"], pa.array(np.abs(np.where(va, a, 1).astype(np.int32)), pa.int32()).filter(pa.array(keep)), "abs")      # abs(-2^31) wraps, in numpy too
