"""CPU: the aggregate compile (csrc/agg_compile.cpp) over the descriptor grid of tools/agg_compile_hashes.py, without a device.
What a Partial emits is what the Final of the same function reads; every name a function answers to compiles to the same programs;
a result projection split over several post programs is described chunk by chunk."""
import importlib.util
import json
import os

import pytest

import arrow_ballista_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("agg_compile_hashes", os.path.join(ROOT, "tools", "agg_compile_hashes.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)


def test_partial_states_are_what_the_final_reads():
    """For every (function, argument column, grouping) of the grid the Partial's output fields, given to a Final of the same
    function as its input schema, compile, and the Final's outputs equal the Single's in name, type and nullability.  A refused
    combination says which function over which type."""
    accepted, wrong = 0, []
    for fn, cname, ctype, grouped in H.single_function_grid():
        groups = ["g"] if grouped else []
        aggs = [H.agg_of(fn, cname)]
        if ctype == "Date32" and fn not in H.OVER_DATE32:
            for mode in ("Single", "Partial"):
                with pytest.raises(g.GpuqError) as e:
                    g.compile_check(H.aggregate(mode, H.FIELDS, groups, aggs))
                assert fn + " over Date32" in str(e.value), (fn, cname, mode, str(e.value))
            continue
        single = g.compile_check(H.aggregate("Single", H.FIELDS, groups, aggs))
        partial_desc = H.aggregate("Partial", H.FIELDS, groups, aggs)
        partial = g.compile_check(partial_desc)
        final = g.compile_check(H.final_of(partial_desc, partial))
        accepted += 1
        if final["outputs"] != single["outputs"]:
            wrong.append((fn, cname, grouped, final["outputs"], single["outputs"]))
        assert [o["name"] for o in single["outputs"]] == groups + ["a"]
    assert not wrong, wrong
    assert accepted == 198


def test_every_name_of_a_function_compiles_to_the_same_programs():
    for alias, fn in H.ALIASES:
        for mode in ("Single", "Partial"):
            a = g.compile_check(H.aggregate(mode, H.FIELDS, ["g"], [H.agg_of(alias, "i64n")]))
            b = g.compile_check(H.aggregate(mode, H.FIELDS, ["g"], [H.agg_of(fn, "i64n")]))
            assert json.dumps(a) == json.dumps(b), (alias, fn, mode)
            assert ("expr2" in H.agg_of(alias, "i64n")) == (fn in H.TWO_ARG)


def test_split_result_projection_is_described_chunk_by_chunk():
    d = g.compile_check(H.nine_aggregates("Single"))
    assert len(d["acc_kinds"]) == 10
    assert d["post_programs"] == len(d["posts"]) == 2
    assert sum((p["out_type"] for p in d["posts"]), []) == [o["type"] for o in d["outputs"]]
    assert d["post"] == d["posts"][0]
    one = g.compile_check(H.nine_aggregates("Partial"))      # the states are plain columns and sums: one program holds them
    assert one["post_programs"] == len(one["posts"]) == 1 and one["post"] == one["posts"][0]
