"""The hand-built text corpus of csv_fields.py is right before any kernel sees it: pyarrow's CSV reader, with the options the GPU
scan tests check against (test_gpu_scan_decode.pyarrow_csv), reads every valid case to the value plain Python recorded and refuses
every malformed one, but for the few differences named below; the grammar stated in csv_fields.reference_field agrees with every
case; the layout files reach the boundaries they are named after; and the corpus still holds what it is for.  No GPU."""
import pyarrow as pa
import pytest

import csv_fields as cf
from test_gpu_scan_decode import pyarrow_csv

# Where pyarrow and the corpus differ.  (A Float64 outside the exact fast path, a huge exponent included, is no difference: the corpus
# records float(text) beside the refusal -- inf for 1e4294967296 -- and pyarrow must read exactly that.)  Every entry is a refusal on the device side (refusing can never store a wrong value) or a
# case where the rule of the reference's reader, arrow-csv, is known; "the device returns a value neither reader returns" is never one.
PYARROW_REFUSES = {      # valid in the corpus, refused by pyarrow
    "plus_sign": "arrow-csv parses integers with a leading '+' (atoi's signed parse); Arrow C++ refuses it",
}
PYARROW_READS = {        # refused (status 1) in the corpus, read by pyarrow
    "blanks_around_numbers": "Arrow C++ trims blanks around numbers and dates; arrow-csv does not, and the device refuses them",
    "integer_hex": "Arrow C++ reads 0x10 as the integer 16; arrow-csv does not, and the device refuses it",
    "inf_nan": "Arrow C++ (and arrow-csv) read inf / nan spellings; the device decodes the exact fast path only and refuses them",
    "decimal_exponent": "Arrow C++ reads 1e2 as the decimal 100; the device refuses an exponent in a decimal",
    "decimal_beyond_precision": "Arrow C++ does not hold a decimal to its column's precision once the scale appends zeros to it, nor to 38 digits; the device refuses what does not fit",
    "zero_fraction_beyond_scale": "Arrow C++ drops fraction zeros beyond the scale; the device refuses every fraction longer than the scale",
    "year_0000": "Arrow C++ reads the year 0000; datetime has no such year and the device refuses it",
}


def _difference(c):
    """the key of PYARROW_REFUSES / PYARROW_READS a case falls under, or None"""
    n, f = c.name, c.field
    if not cf.is_refused(c):
        return "plus_sign" if f.startswith(b"+") and c.ctype in ("Int32", "Int64") else None
    if c.ctype == "Boolean" or c.ctype == "Utf8":
        return None
    if n.endswith("leading_space") or n.endswith("trailing_space"):
        return "blanks_around_numbers"
    if f == b"0x10":
        return "integer_hex"
    if c.ctype == "Float64" and f.lower().lstrip(b"-") in (b"inf", b"infinity", b"nan"):
        return "inf_nan"
    if isinstance(c.ctype, dict) and n.endswith("refused_exponent"):
        return "decimal_exponent"
    if c.ctype == "Date32" and f.startswith(b"0000-"):
        return "year_0000"
    return None


def read_field(c):
    """pyarrow's value of the case's own line in file_of(c) (NULL as cf.NULL), or the exception it raises"""
    try:
        t = pyarrow_csv(cf.file_of(c), cf.field_schema(c))
    except (pa.ArrowInvalid, pa.ArrowNotImplementedError, UnicodeError) as e:
        return e
    if t.num_rows != 3 or t.column("row").to_pylist() != [6, 7, 8]:
        return ValueError("rows %s" % t.column("row").to_pylist())
    v = cf.column_values(t.column("v"), c.ctype)[1]
    return cf.NULL if v is None else v


def test_corpus_shape():
    names = [c.name for c in cf.corpus()] + [x.name for x in cf.layouts()]
    assert len(names) == len(set(names))
    floors = {"Int32": (12, 20), "Int64": (12, 20), "Date32": (20, 50), "Float64": (45, 50), "Boolean": (8, 15), "Utf8": (10, 3),
              "Decimal128(5,2)": (15, 30), "Decimal128(15,2)": (15, 30), "Decimal128(38,0)": (8, 25), "Decimal128(38,10)": (15, 30), "Decimal128(38,38)": (10, 30)}
    for key, (n_valid, n_refused) in floors.items():
        mine = [c for c in cf.corpus() if cf.type_key(c.ctype) == key]
        assert sum(not cf.is_refused(c) for c in mine) >= n_valid and sum(cf.is_refused(c) for c in mine) >= n_refused, key
        assert any(c.expect is cf.NULL for c in mine), key
        assert key == "Utf8" or any(c.expect == cf.refused(*cf.REQUIRED) for c in mine if cf.is_refused(c)), key      # (an empty required Utf8 field is "")
    assert {cf.type_key(c.ctype) for c in cf.corpus()} == set(floors)
    known = {cf.PARSE, cf.REQUIRED, cf.COUNT, cf.FAST_PATH, cf.QUOTED, cf.BLANK, cf.BARE_CR}
    for c in cf.corpus():
        assert b"," not in c.field and b"\n" not in c.field, c.name
        if cf.is_refused(c):
            assert (c.expect.status, c.expect.word) in known and "refused" in c.name or "outside_fast_path" in c.name, c.name
            assert (c.expect.value is not None) == ((c.expect.status, c.expect.word) in (cf.FAST_PATH, cf.QUOTED)), c.name
    assert len(cf.cases("float64/outside_fast_path")) >= 20
    assert len(cf.cases("decimal_38_0/refused_wrap")) >= 9 and len(cf.cases("decimal_38_10/refused_wrap")) >= 12
    assert sum(1 for x in cf.layouts() if x.expect == "rows") >= 25 and sum(1 for x in cf.layouts() if x.expect != "rows") >= 20
    assert 10 <= len(cf.batches()) <= 30 and len(cf.cases(refused_only=True)) <= 500      # what the GPU test decodes: hundreds of tiny files, not thousands


def test_the_stated_grammar_agrees_with_every_case():
    for c in cf.corpus():
        try:
            got = cf.reference_field(c.ctype, c.nullable, c.field)
        except cf.Refused as e:
            got = e
        if c.ctype == "Utf8" and cf.is_refused(c):      # quote and carriage return are checks of the whole line
            with pytest.raises(cf.Refused) as e:
                cf.reference_file(cf.file_of(c), cf.field_schema(c))
            assert e.value == c.expect, c.name
        elif cf.is_refused(c) or isinstance(got, cf.Refused):
            assert got == c.expect, (c.name, got)
            assert c.expect.value is None or cf.same_value(got.value, c.expect.value), c.name
        else:
            assert cf.same_value(None if got is cf.NULL else got, c.expect), (c.name, got)


@pytest.mark.parametrize("label,schema,cs,text", cf.batches(), ids=[b[0] for b in cf.batches()])
def test_valid_cases_match_pyarrow(label, schema, cs, text):
    """batched as the GPU test batches them (without the lines pyarrow is known to refuse), then the known differences one by one"""
    same = [c for c in cs if _difference(c) is None]
    t = pyarrow_csv(b"".join(c.field + b",%d\n" % i for i, c in enumerate(same)), schema)
    assert t.column("row").to_pylist() == list(range(len(same)))
    for c, got in zip(same, cf.column_values(t.column("v"), cs[0].ctype)):
        assert cf.same_value(got, c.expect), (c.name, got, c.expect)
    for c in cs:
        if _difference(c) is not None:
            assert _difference(c) in PYARROW_REFUSES and isinstance(read_field(c), Exception), c.name


def test_refused_cases_are_refused_by_pyarrow():
    assert len(PYARROW_REFUSES) + len(PYARROW_READS) <= 8
    used, wrong = set(), []
    for c in cf.cases(refused_only=True):
        got, key = read_field(c), _difference(c)
        if c.expect == cf.refused(*cf.BARE_CR):      # a lone carriage return ends a record for Arrow C++ (as for csv-core): more rows, never the byte in a value
            if not (isinstance(got, (ValueError, pa.ArrowInvalid)) and ("rows" in str(got) or "columns" in str(got))):
                wrong.append((c.name, got))
        elif c.expect == cf.refused(*cf.REQUIRED):   # pyarrow knows no required column: the empty field is NULL there (arrow-csv refuses it)
            if got is not cf.NULL:
                wrong.append((c.name, got))
        elif c.expect.value is not None:             # well-formed, not decoded on the device: the host reader agrees with plain Python
            if isinstance(got, Exception) or not cf.same_value(got, c.expect.value):
                wrong.append((c.name, got))
        elif isinstance(got, Exception):
            if key is not None:
                wrong.append((c.name, "named as a difference, but refused"))
        elif key is None or key not in PYARROW_READS:
            if _unnamed_read(c) is None:
                wrong.append((c.name, got))
            else:
                used.add(_unnamed_read(c))
        else:
            used.add(key)
    assert wrong == []
    assert used == set(PYARROW_READS)


def _unnamed_read(c):
    """differences that show only in what pyarrow returns, not in the field's spelling"""
    if isinstance(c.ctype, dict) and any(w in c.name for w in ("wrap", "into_scale_10", "39_digits", "beyond_by_scale_padding")):
        return "decimal_beyond_precision"
    if isinstance(c.ctype, dict) and c.name.endswith("zero_fraction_longer_than_scale"):
        return "zero_fraction_beyond_scale"
    return None


def _pyarrow_layout(x):
    include = None if x.projection is None else [p if isinstance(p, str) else x.schema[p][0] for p in x.projection]
    return pyarrow_csv(x.text, x.schema, delimiter=x.delimiter.decode(), header=x.header, include=include)


@pytest.mark.parametrize("x", cf.layouts(), ids=[x.name for x in cf.layouts()])
def test_layouts_against_the_plain_reference_and_pyarrow(x):
    try:
        want = cf.reference_file(x.text, x.schema, x.delimiter, x.header, x.projection)
    except cf.Refused as e:
        want = e
    if x.expect == "rows":
        assert isinstance(want, dict)
        if x.pyarrow and x.text:
            t = _pyarrow_layout(x)
            assert t.schema.names == list(want)
            for name, ty, _ in x.schema:
                if name in want:
                    got = cf.column_values(t.column(name), ty)
                    assert len(got) == len(want[name]) and all(cf.same_value(g, w) for g, w in zip(got, want[name])), name
        return
    assert want == x.expect
    if not x.pyarrow:
        return
    if x.expect == cf.refused(*cf.BLANK):       # Arrow C++ skips blank lines: as many rows as lines with a byte in them
        lines = [ln for ln in x.text.replace(b"\r\n", b"\n").split(b"\n") if ln]
        assert _pyarrow_layout(x).num_rows == len(lines) - (1 if x.header else 0)
    elif x.expect == cf.refused(*cf.BARE_CR):   # ... and ends a record at a lone carriage return: the byte is in no value
        try:
            t = _pyarrow_layout(x)
            assert all("\r" not in v for v in t.column("s").to_pylist())
        except pa.ArrowInvalid:
            pass
    else:
        with pytest.raises(pa.ArrowInvalid):
            _pyarrow_layout(x)


def test_layout_files_reach_their_boundaries():
    L = cf.layout
    t = L("chunk/line_end_is_the_last_byte_of_a_chunk").text
    assert t[cf.CHUNK - 1:cf.CHUNK] == b"\n" and cf.CHUNK < len(t) < cf.CHUNK + 200
    t = L("chunk/line_end_is_the_first_byte_of_a_chunk").text
    assert t[cf.CHUNK:cf.CHUNK + 1] == b"\n" and t[cf.CHUNK - 1:cf.CHUNK] != b"\n" and cf.CHUNK < len(t) < cf.CHUNK + 200
    t = L("chunk/line_straddles_the_chunks").text
    assert b"\n" not in t[cf.CHUNK - 20:cf.CHUNK + 20] and t[cf.CHUNK + 20:cf.CHUNK + 21] == b"\n"
    t = L("chunk/crlf_split_by_the_chunks").text
    assert t[cf.CHUNK - 1:cf.CHUNK + 1] == b"\r\n" and not t.endswith(b"\n")
    assert max(len(x.text) for x in cf.layouts()) < 100_000

    def block_bytes(text, k):      # the byte range k_csv_parse looks at for lines 256k .. 256k+255: from the 16-byte boundary below the first
        starts = [0]
        for i, b in enumerate(text):
            if b == 10:
                starts.append(i + 1)
        lo, hi = starts[256 * k] & ~15, starts[min(256 * (k + 1), len(starts) - 1)]
        return hi - lo
    t = L("lds/staged_then_in_place").text
    assert cf.LDS_BYTES - 512 < block_bytes(t, 0) <= cf.LDS_BYTES < block_bytes(t, 1) < cf.LDS_BYTES + 512 and block_bytes(t, 2) < cf.LDS_BYTES
    t = L("lds/in_place_then_staged").text
    assert cf.LDS_BYTES - 512 < block_bytes(t, 1) <= cf.LDS_BYTES < block_bytes(t, 0) < cf.LDS_BYTES + 512
    t = L("lds/exactly_the_budget").text
    assert block_bytes(t, 0) == cf.LDS_BYTES
    lens = {len(ln) for ln in L("short/lines_of_1_to_3_bytes").text.split(b"\n")[:-1]}
    assert lens == {1, 2, 3}
    for n in (63, 64, 65, 255, 256, 257):
        x = L("rows/%d" % n)
        want = cf.reference_file(x.text, x.schema)
        assert len(want["i"]) == n and want["n"][0] is cf.NULL and any(v is not cf.NULL for v in want["n"])
        assert n < 65 or (want["n"][63] is cf.NULL and want["n"][64] is cf.NULL and want["b"][63] != want["b"][62])
