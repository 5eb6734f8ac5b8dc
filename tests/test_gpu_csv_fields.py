"""The device text decoder on hand-built fields and files (csv_fields.py; test_cpu_csv_fields.py proves the corpus against pyarrow
first): every valid field of every column type exact against the value plain Python recorded -- Float64 by its bits, NULLs by
position -- every field outside the grammar refused with its status and message, and whole files at the boundaries of the line
splitter against the plain reference applied line by line."""
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd import scan
import csv_fields as cf

pytestmark = pytest.mark.gpu


def _decode(tc, text, schema, **kw):
    return scan.read_csv(tc, text, schema, **kw).to_arrow(tc.ctx)


def _outcome(tc, c):
    """what the device makes of the case as a file of its own: its value (NULL as cf.NULL) or the GpuqError"""
    try:
        t = _decode(tc, cf.file_of(c), cf.field_schema(c))
    except g.GpuqError as e:
        return e
    assert t.num_rows == 3 and t.column("row").to_pylist() == [6, 7, 8], c.name
    v = cf.column_values(t.column("v"), c.ctype)[1]
    return cf.NULL if v is None else v


def _show(got):
    return "status %d (%s)" % (got.status, got) if isinstance(got, g.GpuqError) else repr(got)


@pytest.mark.parametrize("label,schema,cs,text", cf.batches(), ids=[b[0] for b in cf.batches()])
def test_valid_fields_decode_to_the_recorded_values(tc, label, schema, cs, text):
    """one file per column type, a case per line; when it fails, one file per case names the cases"""
    bad = []
    try:
        t = _decode(tc, text, schema)
        assert t.column("row").to_pylist() == list(range(len(cs)))
        assert t.column("v").null_count == sum(c.expect is cf.NULL for c in cs)
        got = cf.column_values(t.column("v"), cs[0].ctype)
        bad = ["%s: %r, expected %r" % (c.name, v, c.expect) for c, v in zip(cs, got) if not cf.same_value(v, c.expect)]
    except g.GpuqError as e:
        bad = ["%s...: %s" % (cs[0].name, _show(e))]
        for c in cs:
            got = _outcome(tc, c)
            if isinstance(got, g.GpuqError) or not cf.same_value(None if got is cf.NULL else got, c.expect):
                bad.append("%s: %s, expected %r" % (c.name, _show(got), c.expect))
    print("\n".join(bad))
    assert bad == []


def _healthy(tc):
    """a clean decode after the refusals: nothing was left behind"""
    x = cf.layout("rows/65")
    assert _layout_mismatch(tc, x) is None


REFUSED_GROUPS = ["int32/", "int64/", "date32/", "decimal_5_2/", "decimal_15_2/", "decimal_38_0/", "decimal_38_10/", "decimal_38_38/", "float64/refused",
                  "float64/outside_fast_path", "boolean/", "utf8/"]


def test_every_refused_case_is_in_a_group():
    names = [c.name for p in REFUSED_GROUPS for c in cf.cases(p, refused_only=True)]
    assert sorted(names) == sorted(c.name for c in cf.cases(refused_only=True)) and len(names) >= 350


@pytest.mark.parametrize("group", REFUSED_GROUPS)
def test_refused_fields(tc, group):
    """Each case is one field outside the grammar between two clean lines, refused by a grammar or range check with status 1
    (malformed) or 3 (well-formed, not decoded on the device) and a message that says which."""
    wrong = []
    for c in cf.cases(group, refused_only=True):
        got = _outcome(tc, c)
        if not isinstance(got, g.GpuqError):
            wrong.append("%s %r: no error, %r" % (c.name, c.field[:48], got))
        elif got.status != c.expect.status or c.expect.word not in str(got):
            wrong.append("%s %r: %s, expected status %d and '%s'" % (c.name, c.field[:48], _show(got), c.expect.status, c.expect.word))
    print("\n".join(wrong))      # (the whole list: the assertion's own report is cut short)
    assert wrong == []
    _healthy(tc)


def _layout_mismatch(tc, x):
    """None when the device decodes the layout's file to the plain reference's columns"""
    want = cf.reference_file(x.text, x.schema, x.delimiter, x.header, x.projection)
    t = _decode(tc, x.text, x.schema, delimiter=x.delimiter.decode(), has_header=x.header, projection=x.projection)
    if t.schema.names != list(want):
        return "columns %s, expected %s" % (t.schema.names, list(want))
    types = dict((s[0], s[1]) for s in x.schema)
    for name, vals in want.items():
        got = cf.column_values(t.column(name), types[name])
        if len(got) != len(vals):
            return "%s: %d rows, expected %d" % (name, len(got), len(vals))
        for r, (a, b) in enumerate(zip(got, vals)):
            if not cf.same_value(a, b):
                return "%s[%d]: %r, expected %r" % (name, r, a, b)
    return None


@pytest.mark.parametrize("x", [x for x in cf.layouts() if x.expect == "rows"], ids=[x.name for x in cf.layouts() if x.expect == "rows"])
def test_layouts_decode_as_the_plain_reference_reads_them(tc, x):
    assert _layout_mismatch(tc, x) is None


REFUSED_LAYOUTS = ["fields/", "projection/", "blank/", "cr/"]


@pytest.mark.parametrize("group", REFUSED_LAYOUTS)
def test_refused_layouts(tc, group):
    """A blank line is never a row, a carriage return inside a line never part of a value, a line never short or long of the schema's
    fields -- whatever the projection -- and a projected field never outside its grammar."""
    assert sorted(x.name for p in REFUSED_LAYOUTS for x in cf.layouts() if x.name.startswith(p) and x.expect != "rows") == sorted(x.name for x in cf.layouts() if x.expect != "rows")
    wrong = []
    for x in cf.layouts():
        if not x.name.startswith(group) or x.expect == "rows":
            continue
        try:
            t = _decode(tc, x.text, x.schema, delimiter=x.delimiter.decode(), has_header=x.header, projection=x.projection)
            wrong.append("%s: no error, %d rows" % (x.name, t.num_rows))
        except g.GpuqError as e:
            if e.status != x.expect.status or x.expect.word not in str(e):
                wrong.append("%s: %s, expected status %d and '%s'" % (x.name, _show(e), x.expect.status, x.expect.word))
    print("\n".join(wrong))      # (the whole list: the assertion's own report is cut short)
    assert wrong == []
    _healthy(tc)
