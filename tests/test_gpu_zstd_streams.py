"""The ZSTD page kernel (gpuq_k_zstd_pages: csrc/zstd_dec.h with 64 lanes) on hand-assembled frames (zstd_streams.py;
test_cpu_zstd_streams.py, without a GPU, proves the corpus against libzstd and runs the one-lane host build of the same text under sanitizers):
everything RFC 8878 allows and libzstd does not write, byte exact against the plaintext the builders computed by applying the
sequences; every targeted malformation refused; the launch batch crossed."""
import numpy as np
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd import scan
import compressed_streams as cs
import zstd_streams as zs

pytestmark = pytest.mark.gpu


def _values(table, tc):
    return table.to_arrow(tc.ctx).column("v").to_numpy()


def _read(tc, group):
    return _values(scan.read_parquet(tc, cs.parquet_of(group, "zstd")), tc)


def _compare(got, group, bad):
    at = 0
    for c in group:
        exp = cs.int32_of(c.plaintext)
        if not np.array_equal(got[at:at + len(exp)], exp):
            bad.append(c.name)
        at += len(exp)
    if at != len(got):
        bad.append("%s...: %d values, expected %d" % (group[0].name, len(got), at))


def failing_pages(tc, group):
    """names of the cases of `group` whose page does not decode to the plaintext: all of them as pages of one column chunk; when
    that fails, one file per case so that the page is named"""
    bad = []
    try:
        _compare(_read(tc, group), group, bad)
        if not bad:
            return bad
    except g.GpuqError:
        pass
    bad = []
    for c in group:
        try:
            _compare(_read(tc, [c]), [c], bad)
        except g.GpuqError as e:
            bad.append("%s: %s" % (c.name, e))
    return bad or ["%s...: the pages decode one by one but not as one column chunk" % group[0].name]


def test_fixed_cases_as_pages_of_one_column_chunk(tc):
    """RLE and repeat tables, accuracy logs 5 and 9/8/9, every length and offset code, one-stream and treeless Huffman literals, trees
    of depth 11, Huffman streams around the 256-byte lane window, literal runs and bitstreams around their 4096-byte windows, match
    offsets on both sides of the 64 lanes, several frames and skippable frames in a page."""
    assert failing_pages(tc, zs.cases("valid", random=False)) == []


def test_random_cases_as_pages_of_one_column_chunk(tc):
    assert failing_pages(tc, zs.cases("valid", random=True)) == []


def test_every_malformed_page_is_refused(tc):
    """All of them, one file each: each case is one targeted edit that libzstd refuses too, and its `reason` quotes the line of
    zstd_dec.h that refuses it.  A frame that names a dictionary is unsupported (status 3), not malformed.  The list is the corpus's
    own: test_cpu_zstd_streams.py, which needs no GPU and passes first, has the one-lane build refuse each of them within bounds."""
    wrong = []
    for c in zs.cases("malformed") + zs.cases("unsupported") + zs.cases("lenient"):
        try:
            got = _read(tc, [c])
            if c.expect != "lenient":
                wrong.append(c.name + ": accepted")
            elif not np.array_equal(got, cs.int32_of(c.plaintext)):
                wrong.append(c.name + ": accepted with other bytes")
        except g.GpuqError as e:
            if (e.status == 3) != (c.expect == "unsupported"):
                wrong.append("%s: status %d" % (c.name, e.status))
    assert wrong == []
    c = zs.cases("valid")[0]                 # the refusals leave nothing behind: a clean decode still succeeds
    assert np.array_equal(_read(tc, [c]), cs.int32_of(c.plaintext))


def test_pages_across_the_launch_batch(tc):
    """4096 + 5 pages of one 4-byte raw block each: the second launch of the page loop in scanfmt.cpp takes the last five."""
    n = 4096 + 5
    vals = (np.arange(n, dtype=np.int64) * 2654435761 % (1 << 31)).astype("<i4")
    pages = []
    for v in vals:
        pages.append((1, 4, zs.ZFrame(single=True).raw(v.tobytes()).frame()))
    assert len(pages[0][2]) == 13
    got = _values(scan.read_parquet(tc, cs.parquet_one_column(pages, cs.PQ_CODECS["zstd"])), tc)
    assert np.array_equal(got, vals)
