"""ParquetExec / CsvExec as leaves of the native executor, without a device: the grammar gpuq_plan_create accepts, the schema it
announces (the projected fields of the FILE schema, in projection order), what it refuses and with which words, and what the Python
driver hands over.  Nothing here opens a file: a plan is created with a context handle that is only dereferenced at execution time."""
import ctypes as C
import json

import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd import binding as B
from arrow_ballista_amd import native as N
from arrow_ballista_amd.expr import binary, col, lit

D152 = {"Decimal128": [15, 2]}
SCHEMA = [{"name": "k", "type": "Int64", "nullable": False}, {"name": "d", "type": "Date32", "nullable": False}, {"name": "p", "type": D152, "nullable": False},
          {"name": "s", "type": "Utf8", "nullable": True}, {"name": "f", "type": "Float64", "nullable": True}]
GROUPS = [[{"path": "/data/a.parquet"}, {"path": "/data/b.parquet", "range": [4, 4096]}], [], [{"path": "/data/c.parquet"}]]
PREDICATE = binary(col("d"), ">=", lit(9000, "Date32"))


def parquet(**kw):
    d = {"file_groups": GROUPS, "schema": SCHEMA}
    d.update(kw)
    return {"ParquetExec": d}


def csv(**kw):
    d = {"file_groups": GROUPS, "schema": SCHEMA, "has_header": True, "delimiter": "|"}
    d.update(kw)
    return {"CsvExec": d}


def create(plan, ctx=1):
    """(status, refusal, message, partitions) of gpuq_plan_create with a fake context, as an executor process would call it"""
    L = B.lib()
    h = C.c_void_p()
    rc = L.gpuq_plan_create(C.c_void_p(ctx) if ctx else None, json.dumps(plan).encode(), C.byref(h))
    msg = (L.gpuq_plan_last_error() or b"").decode() if rc else ""
    refusal = L.gpuq_last_refusal() if rc else B.REFUSAL_NONE
    parts = L.gpuq_plan_num_partitions(h) if rc == 0 else None
    if rc == 0:
        L.gpuq_plan_free(h)
    return rc, refusal, msg, parts


def test_both_nodes_are_accepted_and_their_partitions_are_the_file_groups():
    assert create(parquet()) == (0, B.REFUSAL_NONE, "", 3)
    assert create(parquet(projection=[2, 0], limit=10, predicate=PREDICATE, pruning=False)) == (0, B.REFUSAL_NONE, "", 3)
    assert create(csv()) == (0, B.REFUSAL_NONE, "", 3)
    assert create(csv(projection=[1], limit=0, quote="'", file_groups=[["/data/x.tbl"]])) == (0, B.REFUSAL_NONE, "", 1)
    assert create({"FilterExec": {"input": parquet(predicate=PREDICATE), "expr": PREDICATE}}) == (0, B.REFUSAL_NONE, "", 3)
    # members the reference's FileScanExecConf always carries, empty: nothing to refuse
    assert create(parquet(table_partition_cols=[], output_ordering=[]))[0] == 0


def test_the_schema_is_the_projected_file_schema_in_projection_order():
    assert B.plan_schema(parquet()) == SCHEMA
    assert B.plan_schema(parquet(projection=[3, 0, 2])) == [SCHEMA[3], SCHEMA[0], SCHEMA[2]]
    assert B.plan_schema(csv(projection=[4, 1])) == [SCHEMA[4], SCHEMA[1]]
    assert B.plan_schema(csv(projection=[])) == []
    above = {"ProjectionExec": {"input": parquet(projection=[2, 0]), "expr": [col("k")], "expr_name": ["key"]}}
    assert B.plan_schema(above) == [{"name": "key", "type": "Int64", "nullable": False}]


@pytest.mark.parametrize("plan, words", [
    (parquet(projection=[0, 5]), ["ParquetExec", "projection index 5", "5 fields"]),
    (csv(projection=[-1]), ["CsvExec", "projection index -1"]),
    (csv(delimiter="||"), ["CsvExec", "delimiter must be one byte", "'||'"]),
    (csv(delimiter=""), ["CsvExec", "delimiter must be one byte"]),
    (csv(quote="''"), ["CsvExec", "quote must be one byte"]),
    (parquet(batch_size=8192), ["ParquetExec", "unknown member 'batch_size'"]),
    (csv(predicate=PREDICATE), ["CsvExec", "unknown member 'predicate'"]),
    (parquet(has_header=True), ["ParquetExec", "unknown member 'has_header'"]),
    (parquet(file_groups=[[{"path": "/data/a.parquet", "offset": 3}]]), ["ParquetExec", "unknown member 'offset'"]),
    (parquet(file_groups=[[{"path": "/data/a.parquet", "range": [10, 4]}]]), ["ParquetExec", "range [10, 4)", "/data/a.parquet"]),
    (parquet(limit=-2), ["ParquetExec", "limit -2"]),
])
def test_malformed_nodes_are_refused_with_messages_that_name_what_is_wrong(plan, words):
    rc, refusal, msg, _ = create(plan)
    assert rc == 1 and refusal == B.REFUSAL_NONE
    for w in words:
        assert w in msg, (w, msg)


def test_missing_members_are_named():
    for plan, key in [({"CsvExec": {"file_groups": GROUPS, "schema": SCHEMA, "delimiter": ","}}, "has_header"),
                      ({"CsvExec": {"file_groups": GROUPS, "schema": SCHEMA, "has_header": False}}, "delimiter"),
                      ({"ParquetExec": {"schema": SCHEMA}}, "file_groups"), ({"ParquetExec": {"file_groups": GROUPS}}, "schema")]:
        rc, _, msg, _ = create(plan)
        assert rc == 1 and "'%s'" % key in msg, (key, msg)


@pytest.mark.parametrize("plan, what", [
    (parquet(table_partition_cols=["year"]), "table_partition_cols"), (csv(table_partition_cols=["year"]), "table_partition_cols"),
    (parquet(output_ordering=[{"expr": col("k"), "asc": True}]), "output_ordering"), (csv(escape="\\"), "escape"),
])
def test_what_stays_a_host_leaf_is_refused_as_not_native(plan, what):
    rc, refusal, msg, _ = create(plan)
    assert rc == 3 and refusal == B.REFUSAL_NODE_NOT_NATIVE and what in msg and "is not executed natively" in msg


def test_the_classes_mirror_the_reference_fields_and_know_their_schema_without_a_device():
    p = g.ParquetExec([["/data/a.parquet", {"path": "/data/b.parquet", "range": (4, 4096)}], []], SCHEMA, projection=[2, 0], limit=7, predicate=PREDICATE)
    assert p.schema() == [SCHEMA[2], SCHEMA[0]] and p.output_partition_count() == 2 and p.children() == []
    assert (p.file_groups, p.limit, p.predicate, p.projection) == ([[{"path": "/data/a.parquet"}, {"path": "/data/b.parquet", "range": (4, 4096)}], []], 7, PREDICATE, [2, 0])
    c = g.CsvExec([["/data/x.tbl"]], SCHEMA, has_header=True, delimiter="|")
    assert c.schema() == SCHEMA and c.output_partition_count() == 1 and (c.has_header, c.delimiter) == (True, "|")
    assert g.plan.ParquetExec is g.ParquetExec and g.plan.CsvExec is g.CsvExec


def test_the_driver_emits_the_nodes_the_executor_accepts():
    p = g.ParquetExec([["/data/a.parquet", {"path": "/data/b.parquet", "range": (4, 4096)}], []], SCHEMA, projection=[2, 0], limit=7, predicate=PREDICATE)
    inputs = []
    j = N.plan_to_json(g.FilterExec(PREDICATE, p), None, inputs)
    assert inputs == []
    assert j == {"FilterExec": {"input": {"ParquetExec": {"file_groups": [[{"path": "/data/a.parquet"}, {"path": "/data/b.parquet", "range": [4, 4096]}], []], "schema": SCHEMA,
                                                          "projection": [2, 0], "limit": 7, "predicate": PREDICATE}}, "expr": PREDICATE}}
    assert create(j) == (0, B.REFUSAL_NONE, "", 2) and B.plan_schema(j) == [SCHEMA[2], SCHEMA[0]]
    assert N.plan_to_json(g.ParquetExec([["/a"]], SCHEMA, pruning=False), None, []) == {"ParquetExec": {"file_groups": [[{"path": "/a"}]], "schema": SCHEMA, "pruning": False}}
    c = N.plan_to_json(g.CsvExec([["/data/x.tbl"]], SCHEMA, projection=[1], has_header=False, delimiter="|"), None, [])
    assert c == {"CsvExec": {"file_groups": [[{"path": "/data/x.tbl"}]], "schema": SCHEMA, "projection": [1], "has_header": False, "delimiter": "|", "quote": '"'}}
    assert create(c) == (0, B.REFUSAL_NONE, "", 1) and B.plan_schema(c) == [SCHEMA[1]]


@pytest.mark.parametrize("make, what", [
    (lambda: g.ParquetExec([["/a"]], SCHEMA, table_partition_cols=["year"]), "table_partition_cols"),
    (lambda: g.CsvExec([["/a"]], SCHEMA, table_partition_cols=["year"]), "table_partition_cols"),
    (lambda: g.ParquetExec([["/a"]], SCHEMA, output_ordering=[[col("k")]]), "output_ordering"),
    (lambda: g.CsvExec([["/a"]], SCHEMA, escape="\\"), "escape"),
])
def test_the_driver_refuses_what_the_native_leaf_does_not_implement(make, what):
    with pytest.raises(g.GpuqError, match="is not executed natively") as ei:
        N.plan_to_json(make(), None, [])
    assert ei.value.status == 3 and ei.value.refusal == B.REFUSAL_NODE_NOT_NATIVE and what in str(ei.value)


def test_a_plan_without_a_context_validates_and_cannot_execute():
    L = B.lib()
    h = C.c_void_p()
    assert L.gpuq_plan_create(None, json.dumps(parquet()).encode(), C.byref(h)) == 0
    out = C.c_void_p()
    assert L.gpuq_plan_execute(h, None, 0, None, 0, C.byref(out)) == 1 and b"without a context" in L.gpuq_plan_last_error()
    L.gpuq_plan_free(h)
