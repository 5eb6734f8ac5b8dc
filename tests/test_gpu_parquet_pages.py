"""The device Parquet page decoder on hand-assembled pages (parquet_pages.py; test_cpu_parquet_pages.py proves the corpus against
Arrow C++'s reader first): run kinds, run lengths, header widths and index widths that no writer emits, uncompressed v2 pages in
compressed chunks, every decoded type -- exact against the values the emitters recorded, Arrow types and NULL positions included;
and every targeted malformation refused with its status."""
import pyarrow as pa
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd import scan
import parquet_pages as pp

pytestmark = pytest.mark.gpu


def _decode(tc, data):
    return scan.read_parquet(tc, data).to_arrow(tc.ctx)


def _failing(tc, how, cs):
    """names (and what differs) of the cases that do not decode to their recorded values: first as one file, and only when that
    fails one file per case, to name it"""
    bad = []
    try:
        if how == "columns":
            t = _decode(tc, pp.columns_file_of(cs))
            cols = [t.column("c%d" % i) for i in range(len(cs))]
        else:
            col, at, cols = _decode(tc, pp.file_of(cs)).column("v").combine_chunks(), 0, []
            for c in cs:
                cols.append(col.slice(at, len(c.values)))
                at += len(c.values)
            if at != len(col):
                bad.append("%s...: %d rows, expected %d" % (cs[0].name, len(col), at))
        bad += ["%s: %s" % (c.name, m) for c, m in ((c, pp.mismatch(col, c.leaf, c.values)) for c, col in zip(cs, cols)) if m]
    except g.GpuqError as e:
        bad.append("%s...: %s" % (cs[0].name, e))
    if bad and len(cs) > 1:
        bad = []
        for c in cs:
            try:
                m = pp.mismatch(_decode(tc, pp.file_of([c])).column("v"), c.leaf, c.values)
                if m:
                    bad.append("%s: %s" % (c.name, m))
            except g.GpuqError as e:
                bad.append("%s: %s" % (c.name, e))
        bad = bad or ["%s...: the cases decode one by one, not as one file" % cs[0].name]
    return bad


@pytest.mark.parametrize("label,how,cs", pp.batches(), ids=[b[0] for b in pp.batches()])
def test_valid_pages_decode_to_the_recorded_values(tc, label, how, cs):
    assert _failing(tc, how, cs) == []


def _healthy(tc):
    """a clean decode after the refusals: nothing was left behind"""
    for c in (pp.cases("optional/pages_37_64_91")[0], pp.cases("kinds/v2_uncompressed_pages_in_snappy_chunk")[0]):
        assert pp.mismatch(_decode(tc, pp.file_of([c])).column("v"), c.leaf, c.values) is None, c.name


REFUSED_GROUPS = {
    "level_streams": ("refused/level", "refused/v2_repetition"),
    "index_streams": ("refused/ind",),
    "dictionary_pages": ("refused/fixed_dictionary", "refused/string_dictionary", "refused/dictionary_page"),
    "plain_pages_and_counts": ("refused/plain_page", "refused/byte_array", "refused/pages_hold"),
    "encodings_not_decoded": ("refused/bit_packed_definition_levels", "refused/delta_binary_packed_page"),
}


def test_every_refused_case_is_in_a_group():
    names = [c.name for prefixes in REFUSED_GROUPS.values() for p in prefixes for c in pp.cases(p)]
    assert sorted(names) == sorted(c.name for c in pp.cases("refused/")) and len(names) >= 40


@pytest.mark.parametrize("group", list(REFUSED_GROUPS))
def test_refused_pages(tc, group):
    """Each case is one targeted edit, refused by a check (every length in it is one the decoder compares against the end of its
    stream), with status 1 (malformed) or 3 (unsupported: BIT_PACKED levels, DELTA_BINARY_PACKED values)."""
    wrong = []
    for prefix in REFUSED_GROUPS[group]:
        for c in pp.cases(prefix):
            status = {"malformed": 1, "unsupported": 3}[c.expect]
            try:
                t = _decode(tc, pp.file_of([c]))
                wrong.append("%s: no error, %s..." % (c.name, t.column("v").to_pylist()[20:32]))
            except g.GpuqError as e:
                if e.status != status:
                    wrong.append("%s: status %d, expected %d (%s)" % (c.name, e.status, status, e))
                if c.name == "refused/bit_packed_definition_levels" and "BIT_PACKED" not in str(e):
                    wrong.append("%s: the message does not name the encoding: %s" % (c.name, e))
    assert wrong == []
    _healthy(tc)


def test_types_file_has_the_arrow_schema(tc):
    cs = pp.cases("types/", "valid")
    t = _decode(tc, pp.columns_file_of(cs))
    assert [f.type for f in t.schema] == [pp.pa_type(c.leaf) for c in cs]
    assert t.num_rows == pp.N_TYPE_ROWS and all(t.column(i).null_count == sum(v is None for v in c.values) for i, c in enumerate(cs))
