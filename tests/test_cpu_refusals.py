"""Which UNSUPPORTED it was, without a device: the refusals a caller answers by doing the work in another form carry their kind next to
the status (gpuq_last_refusal, GpuqError.refusal); every other refusal, and every other status, carries none.  The mapping itself
(csrc/status.h) runs as a host program of its own under the sanitizers."""
import ctypes as C
import importlib.util
import json
import os
import subprocess

import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd import binding as B
from arrow_ballista_amd import native as N
from arrow_ballista_amd.expr import col, substr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arrow-ballista_amd", "csrc")
FIELDS = [{"name": "s", "type": "Utf8", "nullable": True}, {"name": "v", "type": "Int64", "nullable": False}]
WINDOW = json.dumps({"WindowAggExec": {"input": {"MemoryExec": {"schema": FIELDS, "partitions": [0]}}}}).encode()


def test_the_constants_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "gpuq.h")).read()
    for name, value in [("NONE", B.REFUSAL_NONE), ("LONG_STRING", B.REFUSAL_LONG_STRING), ("WIDE_SORT_KEY", B.REFUSAL_WIDE_SORT_KEY), ("NODE_NOT_NATIVE", B.REFUSAL_NODE_NOT_NATIVE)]:
        assert "GPUQ_REFUSAL_%s = %d" % (name, value) in hdr


def test_a_node_the_executor_does_not_run_is_refused_as_such_and_the_next_failure_clears_it():
    L = B.lib()
    h = C.c_void_p()
    fake_ctx = C.c_void_p(1)      # a context handle is only dereferenced at execution time
    assert L.gpuq_plan_create(fake_ctx, WINDOW, C.byref(h)) == 3
    assert L.gpuq_last_refusal() == B.REFUSAL_NODE_NOT_NATIVE
    assert b"is not executed natively" in L.gpuq_plan_last_error()
    assert L.gpuq_plan_create(fake_ctx, b"not json", C.byref(h)) == 1
    assert L.gpuq_last_refusal() == B.REFUSAL_NONE


def test_an_unsupported_of_another_kind_carries_none():
    L = B.lib()
    h = C.c_void_p()
    assert L.gpuq_plan_create(None, WINDOW, C.byref(h)) == 3 and L.gpuq_last_refusal() == B.REFUSAL_NODE_NOT_NATIVE      # the slot holds something
    desc = {"op": "project", "input": {"fields": FIELDS}, "exprs": [{"expr": substr(col("s", FIELDS), 17), "name": "x"}]}
    buf = C.create_string_buffer(1 << 12)
    assert L.gpuq_compile_check(json.dumps(desc).encode(), buf, len(buf)) == 3
    assert L.gpuq_last_refusal() == B.REFUSAL_NONE
    assert b"substr: a start outside 1..16" in L.gpuq_last_error(None)
    with pytest.raises(g.GpuqError, match="substr: a start outside 1..16") as ei:
        B.compile_check(desc)
    assert ei.value.status == 3 and ei.value.refusal == B.REFUSAL_NONE
    with pytest.raises(g.GpuqError, match="is not executed natively") as ei:
        B.plan_schema(json.loads(WINDOW))
    assert ei.value.status == 3 and ei.value.refusal == B.REFUSAL_NODE_NOT_NATIVE


def test_the_driver_says_which_node_only_the_mirror_runs():
    leaf = g.MemoryExec([None], schema=FIELDS)      # schema only: nothing is uploaded
    with pytest.raises(g.GpuqError, match="is not executed natively") as ei:
        N.plan_to_json(g.plan.RepartitionExec(leaf, [col("v", FIELDS)], 4), None, [])
    assert ei.value.status == 3 and ei.value.refusal == B.REFUSAL_NODE_NOT_NATIVE
    assert g.GpuqError(3, "anything else").refusal == B.REFUSAL_NONE


MAIN = r"""
#include "status.h"
#include <cstdio>
using namespace gpuq;
template <class E> static void one(const char* what) {
  std::string err;
  const int rc = guarded_into(err, [&]() { throw E(what); });
  std::printf("%d %d %s\n", rc, tls_refusal(), err.c_str());
}
int main() {
  std::string err;
  std::printf("%d %d %s\n", guarded_into(err, []() {}), tls_refusal(), err.c_str());
  one<HipError>("hip");
  one<Unsupported>("plain");
  one<LongString>("long");
  one<WideSortKey>("wide");
  one<NotNative>("node");
  one<Capacity>("cap");
  one<Retry>("retry");
  std::printf("%d %d %s\n", guarded_into(err, []() { throw std::bad_alloc(); }), tls_refusal(), err.c_str());
  one<LongString>("long again");
  one<std::runtime_error>("other");
  one<NotNative>("node again");
  std::printf("%d %d %s\n", guarded_into(err, []() {}), tls_refusal(), err.c_str());      // a success leaves the slot and its text alone
  for (int k = 0; k < 5; ++k) {      // ... and back: the exception a caller of the C ABI rebuilds from (status 3, refusal k) maps to the same pair
    const int rc = guarded_into(err, [&]() { throw_unsupported(k, "back"); });
    std::printf("%d %d %s\n", rc, tls_refusal(), err.c_str());
  }
  return 0;
}
"""
TABLE = [(0, 0, ""), (2, 0, "hip"), (3, 0, "plain"), (3, 1, "long"), (3, 2, "wide"), (3, 3, "node"), (4, 0, "cap"), (7, 0, "retry"), (5, 0, "out of host memory"),
         (3, 1, "long again"), (1, 0, "other"), (3, 3, "node again"), (0, 3, "out of host memory"),      # (that line's text is main's own string: the bad_alloc's)
         (3, 0, "back"), (3, 1, "back"), (3, 2, "back"), (3, 3, "back"), (3, 0, "back")]


def test_the_mapping_as_a_host_program_under_the_sanitizers(tmp_path):
    """csrc/status.h as plain C++ with a main of its own, under AddressSanitizer and UndefinedBehaviorSanitizer: every exception type
    through guarded_into gives its status, its refusal and its message; a kind is followed by none."""
    spec = importlib.util.spec_from_file_location("gpuq_build", os.path.join(ROOT, "arrow-ballista_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    src, exe = os.path.join(str(tmp_path), "status_main.cpp"), os.path.join(str(tmp_path), "status_main")
    with open(src, "w") as f:
        f.write(MAIN)
    r = subprocess.run([build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    got = [tuple(line.split(" ", 2)) for line in out.stdout.split("\n")[:-1]]
    assert [(int(a), int(b), c) for a, b, c in got] == TABLE
