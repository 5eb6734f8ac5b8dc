"""CPU: the head / output-row arithmetic of the "runs" aggregate (csrc/gpuq_kernels.h: runs_head, runs_out_of_order, runs_out_row,
runs_piece_interior, runs_lanes_le).  tests/agg_runs_host.cpp restates the three passes around those functions on the host; it is built
here with the compiler the library's host code is built with and fed the cases the kernels must get right: row counts around a
64-row word and a segment, runs that cross a word and a segment boundary, inactive rows inside and between runs, keys out of order.
Expected: the groups of a plain walk over the rows, and which runs are stored plainly (they lie inside one word and end before its last
lane) and which are folded piece by piece (one fold per word they touch)."""
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("gpuq_build", os.path.join(ROOT, "arrow-ballista_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    exe = str(tmp_path_factory.mktemp("agg_runs") / "agg_runs_host")
    subprocess.run([build._hipcc(), "-O1", "-std=c++17", "-I", build.CSRC, os.path.join(ROOT, "tests", "agg_runs_host.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


def run(exe, rows, wps):
    """rows: [(active, key, value)] -> (out_of_order, [(key, sum, count, plain_stores, folds)])"""
    text = "%d %d\n" % (len(rows), wps) + "".join("%d %d %d\n" % r for r in rows)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    bad, total = (int(x) for x in out[0].split())
    groups = [tuple(int(x) for x in line.split()) for line in out[1:1 + total]]
    assert len(groups) == total
    return bool(bad), groups


def expected(rows):
    """the same by a plain walk: a run is a maximal stretch of consecutive active rows with one key"""
    runs, bad, prev_key = [], False, None
    for i, (active, key, value) in enumerate(rows):
        if not active:
            continue
        if runs and runs[-1][1] == i - 1 and runs[-1][2] == key:
            runs[-1][1] = i; runs[-1][3] += value; runs[-1][4] += 1
        else:
            bad = bad or (prev_key is not None and key <= prev_key)
            runs.append([i, i, key, value, 1])
        prev_key = key
    groups = []
    for a, b, key, s, c in runs:
        whole = a // 64 == b // 64 and b % 64 != 63
        groups.append((key, s, c, 1 if whole else 0, 0 if whole else b // 64 - a // 64 + 1))
    return bad, groups


def distinct(n):
    return [(1, 3 * i + 1, i - 7) for i in range(n)]


def with_run(n, a, b):
    """distinct ascending keys, rows a..b (inclusive) share one"""
    return [(1, 3 * (a if a <= i <= b else i) + 1, 5 * i + 1) for i in range(n)]


CASES = {
    "n0": [], "n1": distinct(1), "n63": distinct(63), "n64": distinct(64), "n65": distinct(65), "n255": distinct(255), "n256": distinct(256),
    "n257": distinct(257), "n3073": distinct(4 * 256 * 3 + 1),
    "one_run": [(1, 9, i) for i in range(1000)],
    "run_60_70": with_run(300, 60, 70), "run_250_260": with_run(600, 250, 260), "run_30_229": with_run(600, 30, 229),
    "run_ends_at_lane_63": with_run(200, 60, 63), "run_starts_at_lane_0": with_run(200, 64, 66), "run_0_63": with_run(200, 0, 63),
    "heavy": [(1, 10 * r + 3, r + j) for r in range(2000) for j in range(r % 7 + 1)],
    "descending": [(1, 1000 - i, i) for i in range(300)],
    "p121": [(1, 1, 10), (1, 2, 20), (1, 1, 30)],
    "p3311": [(1, 3, 1), (1, 3, 2), (1, 1, 3), (1, 1, 4)],
    "p121_far_apart": [(1, 1, 1)] * 100 + [(1, 2, 2)] * 300 + [(1, 1, 3)] * 100,
    "equal_keys_across_a_gap": [(1, 5, 1)] * 3 + [(0, 5, 0)] + [(1, 5, 1)] * 3,
    "hole_in_a_run": [(0 if i == 132 else 1, i // 5, i) for i in range(400)],
    "whole_runs_dropped": [(0 if (i // 5) % 3 == 1 else 1, i // 5, i) for i in range(1000)],
    "only_the_last_row": [(0, 7, 1)] * 700 + [(1, 3, 9)],
    "inactive_words_between": [(1, 1, 1)] * 10 + [(0, 0, 0)] * 500 + [(1, 2, 1)] * 10 + [(0, 0, 0)] * 500 + [(1, 2, 5)],
    "smaller_key_after_inactive_words": [(1, 8, 1)] * 10 + [(0, 0, 0)] * 500 + [(1, 2, 1)] * 10,
}


@pytest.mark.parametrize("wps", [1, 2, 3, 7])
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_walk_equals_plain_walk(host_program, name, wps):
    rows = CASES[name]
    bad, groups = run(host_program, rows, wps)
    exp_bad, exp_groups = expected(rows)
    assert bad == exp_bad
    assert groups == exp_groups


def test_the_cases_are_what_they_are_named_for(host_program):
    assert not expected(CASES["run_250_260"])[0] and not expected(CASES["whole_runs_dropped"])[0] and not expected(CASES["heavy"])[0]
    for name in ("descending", "p121", "p3311", "p121_far_apart", "equal_keys_across_a_gap", "hole_in_a_run", "inactive_words_between", "smaller_key_after_inactive_words"):
        assert expected(CASES[name])[0], name
    assert any(g[3] == 0 and g[4] == 2 for g in expected(CASES["run_60_70"])[1])           # one run in two pieces
    assert any(g[3] == 0 and g[4] == 4 for g in expected(CASES["run_30_229"])[1])          # rows 30..229 touch the words 0, 1, 2 and 3
