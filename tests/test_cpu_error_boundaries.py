"""CPU: every boundary to the C ABI maps what its code throws to a status code and leaves the message in a string of ITS OWN
(gpuq_last_error, gpuq_plan_last_error, gpuq_ipc_last_error, gpuq_scan_last_error; per calling thread).  Per boundary that can be
reached without a device: one malformed and one refused request -- the status code, a message in the boundary's own string, and
the strings of the other boundaries as they were.  (The status codes of the plan grammar's cases are also asserted by
test_cpu_abi_and_host.py::test_native_plan_json_is_parsed_without_a_device, those of the IPC walk by
test_ipc_peek_walks_an_arrow_cpp_stream_on_the_host; what is new here is that a failure stays inside its boundary.)"""
import ctypes as C
import io
import json

import pytest

from arrow_ballista_amd import binding as B
from arrow_ballista_amd.shuffle import gpuq_ipc_info

INVALID, UNSUPPORTED, CAPACITY = 1, 3, 4
FIELDS = [{"name": "i", "type": "Int64", "nullable": False}]
COL = {"column": {"name": "i", "index": 0}}


def _bytes(raw):
    return (C.c_uint8 * len(raw)).from_buffer_copy(raw)


def _schema_message(L):
    """A valid Arrow IPC Schema message of one Int64 field (written by the library's own host-side writer)."""
    f = (B.gpuq_field_info * 1)()
    f[0].name, f[0].type, f[0].nullable = b"k", 3, 0
    ln = C.c_int64(0)
    assert L.gpuq_ipc_schema_message(f, 1, None, 0, C.byref(ln)) == 0
    buf = (C.c_uint8 * ln.value)()
    assert L.gpuq_ipc_schema_message(f, 1, buf, ln.value, C.byref(ln)) == 0
    return buf


def _parquet_two_row_groups():
    import pyarrow as pa
    import pyarrow.parquet as pq
    buf = io.BytesIO()
    pq.write_table(pa.table({"a": pa.array(range(600), type=pa.int64())}), buf, row_group_size=300)
    return buf.getvalue()


# boundary -> (its error string, the malformed request, the refused request); a request is (call, expected status)
def _boundaries(L):
    buf = C.create_string_buffer(1 << 16)
    h, info, n = C.c_void_p(), gpuq_ipc_info(), C.c_int(0)
    junk = _bytes(bytes([7] * 64))
    schema_msg = _schema_message(L)
    pq_file = _bytes(_parquet_two_row_groups())
    rows = (C.c_int64 * 1)()
    five_keys = {"op": "sort", "input": {"fields": FIELDS}, "expr": [{"expr": COL, "asc": True}] * 5}      # MAX_SORT_KEYS is 4
    return {
        "op": (lambda: L.gpuq_last_error(None),
               (lambda: L.gpuq_compile_check(b"not json", buf, len(buf)), INVALID),
               (lambda: L.gpuq_compile_check(json.dumps(five_keys).encode(), buf, len(buf)), UNSUPPORTED)),
        "plan": (lambda: L.gpuq_plan_last_error(),
                 (lambda: L.gpuq_plan_create(None, b'{"FilterExec": {"input": 1}}', C.byref(h)), INVALID),
                 (lambda: L.gpuq_plan_create(None, json.dumps({"WindowAggExec": {"input": {"MemoryExec": {"schema": FIELDS, "partitions": [0]}}}}).encode(), C.byref(h)), UNSUPPORTED)),
        "ipc": (lambda: L.gpuq_ipc_last_error(),
                (lambda: L.gpuq_ipc_peek(C.c_void_p(C.addressof(junk)), 64, C.byref(info)), INVALID),
                (lambda: L.gpuq_ipc_peek(C.c_void_p(C.addressof(schema_msg)), 12, C.byref(info)), CAPACITY)),      # fewer bytes than the message needs
        "scan": (lambda: L.gpuq_scan_last_error(),
                 (lambda: L.gpuq_parquet_row_groups(junk, 64, None, 0, C.byref(n)), INVALID),
                 (lambda: L.gpuq_parquet_row_groups(pq_file, len(pq_file), rows, 1, C.byref(n)), CAPACITY)),       # two row groups, room for one
    }


@pytest.fixture(scope="module")
def boundaries():
    return _boundaries(B.lib())


@pytest.mark.parametrize("kind", ["malformed", "refused"])
@pytest.mark.parametrize("name", ["op", "plan", "ipc", "scan"])
def test_a_failure_stays_inside_its_boundary(boundaries, name, kind):
    # every other boundary holds the message of a failure of its own: "untouched" is then a statement about a known string
    for other, (_, (malformed, _), _) in boundaries.items():
        if other != name:
            assert malformed() == INVALID
    before = {other: b[0]() for other, b in boundaries.items() if other != name}
    assert all(before.values()), before
    last_error, malformed, refused = boundaries[name]
    call, status = malformed if kind == "malformed" else refused
    assert call() == status
    message = last_error()
    assert message, "no message behind status %d" % status
    assert {other: b[0]() for other, b in boundaries.items() if other != name} == before
    # ... and the message is this failure's, not a neighbour's
    assert message not in before.values()
