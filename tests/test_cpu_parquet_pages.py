"""The hand-assembled Parquet page corpus of parquet_pages.py is right before any kernel sees it: Arrow C++'s reader decodes every
valid case to the values the emitters recorded, refuses every malformed case (but for the few named in PYARROW_READS_ANYWAY), and
reads every `unsupported` case to its recorded values; a plain hybrid decoder, independent of the emitters, agrees with every level
and index stream; the host-side footer walk of the project reads the containers; and the corpus still holds what no writer emits.
No GPU."""
import io

import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import arrow_ballista_amd as g
import parquet_pages as pp


def read(data):
    return pq.read_table(io.BytesIO(data))


def as_recorded(col, leaf):
    """INT96 compares as int64 nanoseconds (whatever unit the reader maps it to); BYTE_ARRAY as text"""
    if leaf.phys == pp.INT96:
        col = col.cast(pa.timestamp("ns"))
    return col


def hybrid_decode(data, bw, n):
    """Encodings.md, RLE / bit-packed hybrid: n values of bw bits; every byte a run needs must be there"""
    out, p = [], 0
    while len(out) < n:
        h, sh = 0, 0
        while True:
            if p >= len(data):
                raise ValueError("stream ends before %d values" % n)
            c = data[p]
            p += 1
            h |= (c & 0x7F) << sh
            sh += 7
            if not c & 0x80:
                break
        if h >> 1 == 0:
            raise ValueError("empty run")
        if h & 1:
            nbytes = (h >> 1) * bw
            need = min((h >> 1) * 8, n - len(out))
            if (need * bw + 7) // 8 > len(data) - p:
                raise ValueError("bit-packed run cut short")
            word = int.from_bytes(data[p:p + nbytes], "little")
            out += [(word >> (i * bw)) & ((1 << bw) - 1) for i in range(need)]
            p += nbytes
        else:
            nb = (bw + 7) // 8
            if nb > len(data) - p:
                raise ValueError("run value cut short")
            out += [int.from_bytes(data[p:p + nb], "little")] * min(h >> 1, n - len(out))
            p += nb
    return out


def test_corpus_shape():
    names = [c.name for c in pp.corpus()]
    assert len(names) == len(set(names))
    for c in pp.corpus():
        assert c.expect in ("valid", "malformed", "unsupported"), c.name
        assert (c.values is not None) == (c.expect != "malformed"), c.name
        assert c.expect == "valid" or c.reason, c.name
        assert all(p.n <= pp.MAX_PAGE_VALUES for p in c.chunk.pages), c.name
    assert len(pp.cases("random/", "valid")) >= 100
    assert len(pp.cases("width/", "valid")) >= 35 and len(pp.cases("refused/", "malformed")) >= 35
    assert [c.name for c in pp.cases(expect="unsupported")] == ["refused/bit_packed_definition_levels", "refused/delta_binary_packed_page"]
    assert 40 <= len(pp.batches()) + len(pp.cases("refused/")) <= 200      # what the GPU test decodes: files, not thousands


def test_the_plain_decoder_agrees_with_every_emitted_stream():
    n_streams = 0
    for c in pp.corpus():
        for bw, n, data, want in c.streams:
            assert hybrid_decode(data, bw, n) == want, c.name
            n_streams += 1
    assert n_streams > 400


@pytest.mark.parametrize("label,how,cs", pp.batches(), ids=[b[0] for b in pp.batches()])
def test_valid_cases_match_arrow(label, how, cs):
    """batched exactly as the GPU test batches them, then one file per case"""
    if how == "columns":
        t = read(pp.columns_file_of(cs))
        assert t.num_rows == pp.N_TYPE_ROWS
        for i, c in enumerate(cs):
            assert pp.mismatch(as_recorded(t.column("c%d" % i), c.leaf), c.leaf, c.values) is None, c.name
    else:
        col = as_recorded(read(pp.file_of(cs)).column("v"), cs[0].leaf).combine_chunks()
        at = 0
        for c in cs:
            assert pp.mismatch(col.slice(at, len(c.values)), c.leaf, c.values) is None, c.name
            at += len(c.values)
        assert at == len(col)
    for c in cs:
        assert pp.mismatch(as_recorded(read(pp.file_of([c])).column("v"), c.leaf), c.leaf, c.values) is None, c.name


def test_malformed_cases_are_refused_by_arrow():
    assert len(pp.PYARROW_READS_ANYWAY) <= 3
    assert set(pp.PYARROW_READS_ANYWAY) <= {c.name for c in pp.cases(expect="malformed")}
    accepted = []
    for c in pp.cases(expect="malformed"):
        try:
            read(pp.file_of([c]))
            accepted.append(c.name)
        except (OSError, pa.ArrowException):
            pass
    assert sorted(accepted) == sorted(pp.PYARROW_READS_ANYWAY)


def test_unsupported_cases_are_well_formed():
    for c in pp.cases(expect="unsupported"):
        assert pp.mismatch(read(pp.file_of([c])).column("v"), c.leaf, c.values) is None, c.name


def test_the_host_footer_walk_reads_the_containers():
    from arrow_ballista_amd import scan
    L = g.lib()
    cs = pp.cases("types/", "valid")
    fields, rows = scan.parquet_schema(L, pp.columns_file_of(cs))
    assert rows == pp.N_TYPE_ROWS and len(fields) == len(cs) and [f[0] for f in fields if f[1] is None] == []
    assert [f[2] for f in fields] == [c.leaf.optional for c in cs]
    group = pp.cases("levels/", "valid")
    assert scan.parquet_row_groups(L, pp.file_of(group)) == [len(c.values) for c in group]


def _runs(data, bw):
    """(kind, count, header bytes) of every run of a valid stream"""
    p = 0
    while p < len(data):
        h, sh, p0 = 0, 0, p
        while True:
            c = data[p]
            p += 1
            h |= (c & 0x7F) << sh
            sh += 7
            if not c & 0x80:
                break
        yield ("bp" if h & 1 else "rle"), h >> 1, p - p0
        p += (h >> 1) * bw if h & 1 else (bw + 7) // 8


def test_the_corpus_still_covers_what_no_writer_emits():
    widths, long_bp, hdr_bytes = set(), 0, set()
    for c in pp.cases(expect="valid"):
        for bw, n, data, want in c.streams:
            widths.add(bw)
            for kind, count, hb in _runs(data, bw):
                long_bp += kind == "bp" and count >= 64
                hdr_bytes.add((kind, hb))
        widths |= {0} if "width/00" in c.name else set()
    assert widths >= set(range(33))
    assert long_bp >= 4 and {("rle", 3), ("rle", 5), ("bp", 2), ("bp", 3)} <= hdr_bytes
    stored_v2 = [c.name for c in pp.cases(expect="valid") if c.chunk.codec != "none" and any(p.kind == "v2" and not p.compressed for p in c.chunk.pages)
                 and any(p.compressed for p in c.chunk.pages if p.kind != "dict")]
    assert {c.chunk.codec for c in pp.cases("kinds/", "valid")} >= {"snappy", "zstd", "lz4_raw"} and len(stored_v2) >= 6
    assert any(p.kind == "index" for c in pp.cases("headers/") for p in c.chunk.pages)
    assert sum(1 for c in pp.cases("types/") if c.leaf.phys == pp.FLBA) == 16 * 4
