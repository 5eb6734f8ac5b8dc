"""The device decompressors on hand-assembled streams (compressed_streams.py; test_cpu_compressed_streams.py proves the corpus
against liblz4 / libsnappy first): every Snappy element kind and LZ4 frame feature that no encoder emits, byte exact against the
plaintext the emitters built; every targeted malformation refused; and the serial decoders behind GPUQ_SNAPPY_PJ=0 / GPUQ_LZ4_PJ=0."""
import os
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pytest

import arrow_ballista_amd as g
from arrow_ballista_amd import scan
from arrow_ballista_amd import shuffle as S
import compressed_streams as cs

pytestmark = pytest.mark.gpu


def _values(table, tc):
    return table.to_arrow(tc.ctx).column("v").to_numpy()


def _compare(got, group, bad):
    at = 0
    for c in group:
        exp = cs.int32_of(c.plaintext)
        if not np.array_equal(got[at:at + len(exp)], exp):
            bad.append(c.name)
        at += len(exp)
    if at != len(got):
        bad.append("%s...: %d values, expected %d" % (group[0].name, len(got), at))


def failing_parquet(tc, kind):
    """names of the valid `kind` cases whose page does not decode to the plaintext: the fixed table as pages of one column chunk,
    then the random programs as pages of another"""
    bad = []
    for group in (cs.cases(kind, "valid", random=False), cs.cases(kind, "valid", random=True)):
        try:
            _compare(_values(scan.read_parquet(tc, cs.parquet_of(group, kind)), tc), group, bad)
        except g.GpuqError:                    # name the page: one file each
            for c in group:
                try:
                    _compare(_values(scan.read_parquet(tc, cs.parquet_of([c], kind)), tc), [c], bad)
                except g.GpuqError as e:
                    bad.append("%s: %s" % (c.name, e))
    return bad


def _zeros_stream(n_bytes):
    import io
    t = pa.table({"v": pa.array(np.zeros(n_bytes // 4, np.int32))}).cast(pa.schema([pa.field("v", pa.int32(), False)]))
    sink = io.BytesIO()
    with pa.ipc.new_stream(sink, t.schema, options=pa.ipc.IpcWriteOptions(compression="lz4")) as w:
        w.write_batch(t.to_batches()[0])
    return sink.getvalue()


def failing_frames(tc):
    """names of the valid frame cases that do not decode to the plaintext: every fixed case as a stream of its own (a frame that
    sends the call to the frame-by-frame fallback must not take the others with it), the random programs as two streams"""
    bad = []
    rnd = cs.cases("lz4_frame", "valid", random=True)
    for group in [[c] for c in cs.cases("lz4_frame", "valid", random=False)] + [rnd[0::2], rnd[1::2]]:
        if "linked_stored_x" in group[0].name:
            # recycled pool memory must not equal the expected bytes by accident: the same sizes were last used for zeros
            z, _ = S.read_ipc_stream(tc, _zeros_stream(len(group[0].plaintext)))
            assert not _values(z, tc).any()
            del z
        try:
            t, _ = S.read_ipc_stream(tc, cs.ipc_of(group))
            _compare(_values(t, tc), group, bad)
        except g.GpuqError as e:
            bad.append("%s%s: %s" % (group[0].name, "..." if len(group) > 1 else "", e))
    return bad


@pytest.mark.parametrize("kind", ["snappy", "lz4_raw"])
def test_parquet_pages_of_hand_built_streams(tc, kind):
    """copy-4 elements, 3- and 4-byte literal length fields, non-minimal encodings, elements on the 4096-byte block edges, chains
    1100 copies deep: the int32 column is the plaintext, byte exact."""
    assert failing_parquet(tc, kind) == []


def test_ipc_bodies_of_hand_built_frames(tc):
    """Linked frames of stored blocks only (at the parent of this test's commit: the output was never written and the call
    returned status 0 -- launch_unpack_pages_pj left after k_sn_head when no block was compressed), matches into stored blocks,
    non-full inner blocks (the linked whole-frame walk as the fallback), block checksums, content size, content checksum,
    block-size ids 5-7."""
    assert failing_frames(tc) == []


def test_every_malformed_stream_is_refused(tc):
    """All of them, not some: each case is one targeted edit that both CPU judges reject, and its `reason` names the line of the
    kernel or the host code that refuses it."""
    accepted = []
    for c in cs.cases(expect="malformed") + cs.cases(expect="unsupported"):
        try:
            if c.kind == "lz4_frame":
                S.read_ipc_stream(tc, cs.ipc_of([c]))
            else:
                scan.read_parquet(tc, cs.parquet_of([c], c.kind))
            accepted.append(c.name)
        except g.GpuqError as e:
            if c.expect == "unsupported" and e.status != 3:
                accepted.append("%s: status %d, expected 3" % (c.name, e.status))
    assert accepted == []
    for kind in ("snappy", "lz4_raw"):       # the refusals leave nothing behind: a clean decode still succeeds
        c = cs.cases(kind, "valid")[0]
        assert np.array_equal(_values(scan.read_parquet(tc, cs.parquet_of([c], kind)), tc), cs.int32_of(c.plaintext))
    c = cs.cases("lz4_frame", "valid")[0]
    t, _ = S.read_ipc_stream(tc, cs.ipc_of([c]))
    assert np.array_equal(_values(t, tc), cs.int32_of(c.plaintext))


_SERIAL_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import arrow_ballista_amd as g
from arrow_ballista_amd import scan
import compressed_streams as cs
import test_gpu_compressed_streams as T
tc = g.TaskContext(device=0)
bad = T.failing_parquet(tc, "snappy") + T.failing_frames(tc)
try:
    scan.read_parquet(tc, cs.parquet_of(cs.cases("lz4_raw", "valid")[:3], "lz4_raw"))
    bad.append("an LZ4_RAW file was accepted by the serial decoder")
except g.GpuqError as e:
    if e.status != 3:
        bad.append("LZ4_RAW file refused with status %%d, expected 3" %% e.status)
for name in bad:
    print("FAILED " + name)
print("serial decoders done")
"""


def test_serial_decoders_behind_the_environment_switches(tc):
    """GPUQ_SNAPPY_PJ=0 selects k_unpack_pages, GPUQ_LZ4_PJ=0 the per-frame walk of k_lz4_decode for every linked frame; both are
    read once per process, so one fresh child decodes the valid Snappy and frame corpus with them.  LZ4_RAW pages have no serial
    decoder: the file is refused as unsupported."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, GPUQ_SNAPPY_PJ="0", GPUQ_LZ4_PJ="0")
    r = subprocess.run([sys.executable, "-c", _SERIAL_CHILD % (os.path.dirname(here), here)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "serial decoders done" in r.stdout
    assert [l for l in r.stdout.splitlines() if l.startswith("FAILED ")] == []
