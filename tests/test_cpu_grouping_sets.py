"""Grouping sets (GROUP BY ROLLUP / CUBE / GROUPING SETS) without a device: the restatement the GPU tests compare against
(tests/grouping_sets_exact.py) pinned on a hand-written table with the answers written out, how such a node is typed, the Merge mode of
the aggregate compile (states in, states out), what is refused and with which status, the build of the expansion kernel, and the
kernel's row rule (csrc/grouping_expand_op.h) folded by a stand-alone host program under AddressSanitizer and UBSan."""
import importlib.util
import os
import random
import re
import subprocess

import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd import binding as B
from arrow_ballista_amd.expr import col

import grouping_sets_exact as GS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arrow-ballista_amd", "csrc")
F, T = False, True


def leaf(*fields):
    """A host-only input: a schema, no data."""
    return g.MemoryExec([None], schema=[{"name": n, "type": t, "nullable": nullable} for n, t, nullable in fields])


def agg(fn, c, s, name, **kw):
    return dict({"fn": fn, "expr": col(c, s), "name": name}, **kw)


# ---------------------------------------------------------------- the restatement
#        a  b     v
ROWS = [(1, "x",  10), (1, "x",  20), (1, "y",  5), (1, None, 7), (2, "x", 1), (2, "y", 2), (2, "y", None), (2, None, 4), (2, None, 8), (1, "y", -3), (2, "x", 100),
        (1, "x",  None)]


def folded(sets):
    keys = [r[:2] for r in ROWS]
    v = [r[2] for r in ROWS]
    return {k: (GS.count_star(rows), GS.count(v, rows), GS.total(v, rows), GS.minimum(v, rows), GS.maximum(v, rows)) for k, rows in GS.groups(keys, sets).items()}


def test_the_restatement_on_a_known_table():
    # ROLLUP(a, b): the sets (a, b), (a), ().  Rows 3, 7 and 8 have a really-NULL b: they sit in the groups (1, NULL) and (2, NULL), which
    # are also where the set (a) puts every row of a = 1 and a = 2 -- one group each, there is no grouping id to tell them apart
    assert GS.rollup(2) == [[F, F], [F, T], [T, T]]
    assert folded(GS.rollup(2)) == {
        (1, "x"): (3, 2, 30, 10, 20),
        (1, "y"): (2, 2, 2, -3, 5),
        (1, None): (1 + 6, 1 + 5, 7 + 39, -3, 20),
        (2, "x"): (2, 2, 101, 1, 100),
        (2, "y"): (2, 1, 2, 2, 2),
        (2, None): (2 + 6, 2 + 5, 12 + 115, 1, 100),
        (None, None): (12, 10, 154, -3, 100),
    }
    # a duplicated set doubles its counts and sums
    assert folded([[F, T], [F, T]]) == {(1, None): (12, 10, 78, -3, 20), (2, None): (12, 10, 230, 1, 100)}
    # () alone: the grand total, one row; over no rows, none
    assert folded([[T, T]]) == {(None, None): (12, 10, 154, -3, 100)}
    assert GS.groups([], [[T, T]]) == {}
    # a fused predicate drops rows before any set sees them
    assert {k: len(r) for k, r in GS.groups([r[:2] for r in ROWS], [[T, T]], keep=[r[0] == 1 for r in ROWS]).items()} == {(None, None): 6}
    # decimal AVG truncates toward zero at four more digits; wrapping sums
    assert GS.avg_decimal([7, -7, None], [0]) == 70000 and GS.avg_decimal([1, 1, 0], [0, 1, 2]) == 6666 and GS.avg_decimal([-1, -1, 0], [0, 1, 2]) == -6666
    assert GS.avg_decimal([None], [0]) is None
    assert GS.total([2**63 - 1, 1], [0, 1]) == -2**63 and GS.total([2**63 - 1, 1], [0, 1], bits=128) == 2**63
    assert GS.bit_fold("XOR", [-1, 1], [0, 1], 32) == -2 and GS.bool_or([False, None], [0, 1]) is False and GS.bool_and([None], [0]) is None


# ---------------------------------------------------------------- typing
def test_rollup_and_cube_sets():
    assert g.plan.rollup_sets(3) == [[F, F, F], [F, F, T], [F, T, T], [T, T, T]] == GS.rollup(3)
    cube = g.plan.cube_sets(3)
    assert cube == GS.cube(3) and len(cube) == 8 and cube[0] == [F, F, F] and cube[-1] == [T, T, T]
    assert sorted(map(tuple, cube)) == sorted((a, b, c) for a in (F, T) for b in (F, T) for c in (F, T))
    assert g.plan.rollup_sets(1) == [[F], [T]] and g.plan.cube_sets(1) == [[F], [T]]


def test_schema_of_a_node_with_sets():
    src = leaf(("a", "Int32", False), ("b", "Utf8", True), ("c", "Int64", False), ("v", "Int64", True), ("d", {"Decimal128": [12, 2]}, False), ("f", "Float64", True))
    s = src.schema()
    keys = [(col(k, s), k) for k in "abc"]
    aggs = [agg("SUM", "v", s, "sv"), {"fn": "COUNT", "name": "n"}, agg("AVG", "d", s, "ad"), agg("MIN", "d", s, "md"), agg("STDDEV", "f", s, "sf"),
            agg("BIT_OR", "c", s, "oc")]      # (an operator holds twelve accumulators, and a Final shares fewer of them than a Single)
    for mode in ("Single", "Partial"):
        # (one all-false set is the plain node, typed by the native executor like every node with sets: it announces the declared form, every
        # value of a Single nullable, where the operator's own description may be tighter)
        plain = g.AggregateExec(mode, keys, aggs, src, grouping_sets=[[F, F, F]]).schema()
        assert [(f["name"], f["type"]) for f in plain] == [(f["name"], f["type"]) for f in g.AggregateExec(mode, keys, aggs, src).schema()]
        assert [f["nullable"] for f in plain[:3]] == [False, True, False]
        # a key is nullable when its expression is, or when any set masks it
        for sets, nullable in ((g.plan.rollup_sets(3), [True, True, True]), ([[F, F, F], [F, F, T]], [False, True, True]), ([[F, T, F]], [False, True, False]),
                               (g.plan.cube_sets(3), [True, True, True])):
            got = g.AggregateExec(mode, keys, aggs, src, grouping_sets=sets).schema()
            assert [(f["name"], f["type"]) for f in got[:3]] == [(f["name"], f["type"]) for f in plain[:3]]
            assert [f["nullable"] for f in got[:3]] == nullable, (mode, sets)
            # the aggregate fields (a Partial's: the state columns) are those of the same node without sets
            assert got[3:] == plain[3:], (mode, sets, got[3:], plain[3:])
        if mode == "Partial":      # states are announced as the operator types them
            assert plain == g.AggregateExec(mode, keys, aggs, src).schema()


AGG_FN_ROWS = ["COUNT", "SUM", "AVG", "MIN", "MAX", "VARIANCE", "VARIANCE_POP", "STDDEV", "STDDEV_POP", "COVARIANCE", "COVARIANCE_POP", "CORRELATION", "BIT_AND", "BIT_OR",
               "BIT_XOR", "BOOL_AND", "BOOL_OR"]      # the first name of every row of AGG_FNS (csrc/agg_compile.cpp)


def test_merge_reads_states_and_emits_them():
    """Mode Merge over a Partial's output schema gives that Partial's output again: names, types and nullability, for every function."""
    fields = [{"name": "g", "type": "Utf8", "nullable": False}, {"name": "i32", "type": "Int32", "nullable": True}, {"name": "i64", "type": "Int64", "nullable": False},
              {"name": "f64", "type": "Float64", "nullable": True}, {"name": "dec", "type": {"Decimal128": [12, 2]}, "nullable": True}, {"name": "b", "type": "Boolean", "nullable": True},
              {"name": "y", "type": "Float64", "nullable": True}]
    accepted = {}
    for fn in AGG_FN_ROWS:
        for cname in (["b"] if fn.startswith("BOOL") else ["i32", "i64", "f64", "dec"]):
            a = {"fn": fn, "expr": col(cname, fields), "name": "a"}
            if fn in ("COVARIANCE", "COVARIANCE_POP", "CORRELATION"):
                a["expr2"] = col("y", fields)
            partial_desc = {"op": "aggregate", "mode": "Partial", "input": {"fields": fields}, "group_expr": [{"expr": col("g", fields), "name": "g"}], "aggr_expr": [a]}
            try:
                partial = B.compile_check(partial_desc)
            except g.GpuqError as e:      # BIT_* over a float or a decimal: the function's own refusal, nothing of Merge's
                assert fn.startswith("BIT_") and cname in ("f64", "dec") and fn + " over" in str(e), (fn, cname, str(e))
                continue
            states = []
            for o in partial["outputs"]:
                t = o["type"]
                if t.startswith("Decimal128("):
                    p, sc = t[len("Decimal128("):-1].split(",")
                    t = {"Decimal128": [int(p), int(sc)]}
                states.append({"name": o["name"], "type": t, "nullable": bool(o["nullable"])})
            merge = B.compile_check({"op": "aggregate", "mode": "Merge", "input": {"fields": states}, "group_expr": [{"expr": col("g", states), "name": "g"}],
                                     "aggr_expr": [{"fn": fn, "name": "a"}]})
            assert merge["outputs"] == partial["outputs"], (fn, cname, merge["outputs"], partial["outputs"])
            assert len(partial["outputs"]) >= 2 and all(o["name"].startswith("a[") for o in partial["outputs"][1:])
            accepted[fn] = accepted.get(fn, 0) + 1
    assert accepted == dict({fn: 4 for fn in AGG_FN_ROWS[:12]}, **{"BIT_AND": 2, "BIT_OR": 2, "BIT_XOR": 2, "BOOL_AND": 1, "BOOL_OR": 1})
    with pytest.raises(g.GpuqError, match="unknown aggregate mode 'Merged'"):
        B.compile_check({"op": "aggregate", "mode": "Merged", "input": {"fields": fields}, "group_expr": [], "aggr_expr": []})


# ---------------------------------------------------------------- refusals
def test_refusals_by_status():
    src = leaf(("a", "Int32", False), ("b", "Utf8", True), ("v", "Int64", True))
    s = src.schema()
    keys = [(col("a", s), "a"), (col("b", s), "b")]
    sv = agg("SUM", "v", s, "sv")

    def refused(status, match, sets, aggs=(sv,), keys=keys, mode="Single"):
        with pytest.raises(g.GpuqError, match=match) as e:
            g.AggregateExec(mode, keys, list(aggs), src, grouping_sets=sets).schema()
        assert e.value.status == status and e.value.refusal == B.REFUSAL_NONE and "AggregateExec" in str(e.value), str(e.value)
    # GPUQ_ERR_INVALID
    refused(1, r"grouping set .* has 3 entries for 2 group expressions", [[F, F], [F, T, T]])
    refused(1, r"has 1 entries for 2 group expressions", [[T]])
    refused(1, r"without group expressions", [[]], keys=[])
    refused(1, r"without group expressions", [[], []], keys=[])
    refused(1, r"non-empty list", [])
    for mode in ("Final", "FinalPartitioned"):
        refused(1, r"grouping sets .*mode " + mode, GS.rollup(2), aggs=[{"fn": "SUM", "name": "sv"}], mode=mode)
    leaf_json = {"MemoryExec": {"schema": [{"name": f["name"], "type": f["type"], "nullable": f["nullable"]} for f in s], "partitions": [0]}}
    node = {"input": leaf_json, "mode": "Single", "group_expr": [{"expr": e, "name": n} for e, n in keys], "aggr_expr": [sv], "groups": GS.rollup(2)}
    with pytest.raises(g.GpuqError, match=r"AggregateExec: \"null_expr\" has 1 entries for 2 group expressions") as e:
        B.plan_schema({"AggregateExec": dict(node, null_expr=[{"literal": {"type": "Null", "value": None}}])})
    assert e.value.status == 1
    assert [f["name"] for f in B.plan_schema({"AggregateExec": node})] == ["a", "b", "sv"]      # null_expr is optional
    # GPUQ_ERR_UNSUPPORTED
    refused(3, r"65 grouping sets are not supported \(64 at most\)", [[F, bool(i & 1)] for i in range(65)])
    g.AggregateExec("Single", keys, [sv], src, grouping_sets=[[F, bool(i & 1)] for i in range(64)]).schema()
    refused(3, r"grouping sets beside MEDIAN", GS.rollup(2), aggs=[agg("MEDIAN", "v", s, "m"), sv])
    refused(3, r"grouping sets beside APPROX_DISTINCT", GS.rollup(2), aggs=[sv, agg("APPROX_DISTINCT", "v", s, "m")])
    refused(3, r"grouping sets beside COUNT\(DISTINCT", GS.rollup(2), aggs=[agg("COUNT", "v", s, "c", distinct=True)])      # (alone: before the two-level rewrite)
    refused(3, r"grouping sets beside MAX\(DISTINCT", GS.rollup(2), aggs=[sv, agg("MAX", "v", s, "c", distinct=True)])
    refused(3, r"grouping sets beside COUNT\(DISTINCT", GS.rollup(2), aggs=[sv, agg("COUNT", "v", s, "c", distinct=True)], mode="Partial")


def test_the_mirror_layer_refuses_a_node_with_sets(monkeypatch):
    src = leaf(("a", "Int32", False), ("v", "Int64", True))
    s = src.schema()
    node = g.AggregateExec("Single", [(col("a", s), "a")], [agg("SUM", "v", s, "sv")], src, grouping_sets=[[F], [T]])
    monkeypatch.setenv("GPUQ_PLAN_LAYER", "mirror")
    with pytest.raises(g.GpuqError, match="grouping sets") as e:
        node.execute(0, None)
    assert e.value.status == 3


def test_the_plan_json_carries_the_sets():
    from arrow_ballista_amd import native as N
    src = leaf(("a", "Int32", False), ("b", "Int32", False), ("v", "Int64", True))
    s = src.schema()
    keys = [(col("a", s), "a"), (col("b", s), "b")]
    d = N.plan_to_json(g.AggregateExec("Partial", keys, [agg("SUM", "v", s, "sv")], src, grouping_sets=GS.rollup(2)), None, [])["AggregateExec"]
    assert d["groups"] == [[F, F], [F, T], [T, T]] and len(d["null_expr"]) == 2
    d = N.plan_to_json(g.AggregateExec("Partial", keys, [agg("SUM", "v", s, "sv")], src), None, [])["AggregateExec"]
    assert "groups" not in d and "null_expr" not in d


# ---------------------------------------------------------------- the build
def _build_module():
    spec = importlib.util.spec_from_file_location("gpuq_build", os.path.join(ROOT, "arrow-ballista_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    return build


def test_the_expansion_kernel_builds_for_gfx950(tmp_path):
    """kernels_grouping.hip is part of the library, cross-compiles for gfx950 with the build's flags, and uses no scratch at all."""
    build = _build_module()
    assert "kernels_grouping.hip" in build.HIP_SOURCES and "kernels_grouping.hip" not in build.EMBED and "grouping_expand_op.h" in build.HEADERS
    r = subprocess.run([build._hipcc(), "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(CSRC, "kernels_grouping.hip"), "-o", os.path.join(str(tmp_path), "kernels_grouping.o"),
                        "--offload-arch=" + build.ARCH, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    build._check_scratch("kernels_grouping.hip", r.stderr)
    names = set(re.findall(r"Function Name: (\S+)", r.stderr))
    assert any("k_grouping_expand" in n for n in names), sorted(names)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert scratch and max(scratch) == 0, scratch


def test_the_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "gpuq.h")).read()
    assert re.search(r"\bint gpuq_grouping_expand\(gpuq_ctx\* ctx, void\* stream, const gpuq_column\* col, int64_t n, int n_sets, uint64_t null_sets, void\* out_data, "
                     r"uint8_t\* out_validity\);", header)
    L = B.lib()
    assert len(L.gpuq_grouping_expand.argtypes) == 8
    r = subprocess.run(["nm", "-D", "--defined-only", B.lib_path()], capture_output=True, text=True)
    assert r.returncode == 0 and re.search(r" T gpuq_grouping_expand$", r.stdout, re.M)


# ---------------------------------------------------------------- the row rule, folded on the host
@pytest.fixture(scope="module")
def expand_exe(tmp_path_factory):
    """tests/grouping_expand_host.cpp, host code only, under AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded)"""
    build = _build_module()
    exe = str(tmp_path_factory.mktemp("grouping_expand") / "grouping_expand_host")
    r = subprocess.run([build._hipcc(), "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I", build.CSRC,
                        os.path.join(ROOT, "tests", "grouping_expand_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def rule(n, n_sets, mask, valid):
    """Output row o = i * n_sets + s is input row i, NULL (-1) when bit s of mask is set or row i is NULL."""
    return [o // n_sets if not (mask >> (o % n_sets)) & 1 and (valid is None or valid[o // n_sets]) else -1 for o in range(n * n_sets)]


def words_of(bits):
    return [sum(1 << l for l, b in enumerate(bits[w:w + 64]) if b) for w in range(0, len(bits), 64)]


@pytest.mark.parametrize("n_sets", [1, 2, 3, 5, 7, 64])
def test_the_row_rule_folded_on_the_host(expand_exe, n_sets):
    rng = random.Random(n_sets)
    full = (1 << n_sets) - 1
    for n in (0, 1, 21, 22, 64, 65):
        for mask in (0, 1 << rng.randrange(n_sets), full, rng.getrandbits(n_sets)):
            for with_validity in (False, True):
                valid = [rng.random() < 0.7 for _ in range(n)]
                bits = [rng.random() < 0.5 for _ in range(n)]
                text = "%d %d %d %d\n" % (n, n_sets, mask, int(with_validity)) + "".join("%d %d\n" % (v, b) for v, b in zip(valid, bits))
                r = subprocess.run([expand_exe], input=text, capture_output=True, text=True)
                assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
                rows, vwords, dwords = [[int(x) for x in line.split()] for line in r.stdout.split("\n")[:3]]
                want = rule(n, n_sets, mask, valid if with_validity else None)
                assert rows == want, (n, n_sets, mask, with_validity)
                # whole words, the last one zero-padded
                assert vwords == words_of([x >= 0 for x in want]) and len(vwords) == (n * n_sets + 63) // 64
                assert dwords == words_of([x >= 0 and bits[x] for x in want])
