"""The hand-assembled Snappy / LZ4 corpus of compressed_streams.py is right before any kernel sees it: the plaintext by
construction, the small reference decoders and liblz4 / libsnappy (through pyarrow) agree on every case; the Parquet and IPC
containers read back through Arrow C++ and the project's own host-side footer walk; and the corpus still holds the elements no
encoder emits; and the format parsers the kernels share (csrc/lz_elements.h), as a stand-alone program under AddressSanitizer and UBSan,
decode every valid Snappy and LZ4_RAW case byte for byte and refuse every malformed one within bounds.  No GPU."""
import io
import os
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import arrow_ballista_amd as g
import compressed_streams as cs

LIB = {"snappy": "snappy", "lz4_raw": "lz4_raw", "lz4_frame": "lz4"}
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "arrow-ballista_amd", "csrc")


def py_decode(c):
    if c.kind == "snappy":
        return cs.snappy_decode(c.stream)
    if c.kind == "lz4_raw":
        return cs.lz4_raw_decode(c.stream, len(c.plaintext))
    return cs.lz4_frame_decode(c.stream)


def lib_decode(c):
    return pa.Codec(LIB[c.kind]).decompress(c.stream, len(c.plaintext)).to_pybytes()


def test_corpus_shape():
    names = [c.name for c in cs.corpus()]
    assert len(names) == len(set(names))
    for c in cs.corpus():
        assert c.kind in LIB and c.expect in ("valid", "malformed", "unsupported") and c.reason, c.name
        assert c.name.startswith(c.kind + "/")
        assert 4 <= len(c.plaintext) <= (530_000 if c.kind == "lz4_frame" else 200_000), c.name
        if c.kind == "lz4_frame":
            assert len(c.plaintext) % 4 == 0, c.name
    for kind in LIB:
        assert len(cs.cases(kind, "valid", random=True)) >= 200 and len(cs.cases(kind, "valid", random=False)) >= 20 and len(cs.cases(kind, "malformed")) >= 5
        assert all(50 <= len(c.plaintext) <= 2004 for c in cs.cases(kind, "valid", random=True) if "full" not in c.name)
    assert [c.name for c in cs.cases(expect="unsupported")] == ["lz4_frame/bad_dictionary_id"]


def test_valid_cases_three_way():
    for c in cs.cases(expect="valid"):
        assert py_decode(c) == c.plaintext, c.name
        assert lib_decode(c) == c.plaintext, c.name


def test_malformed_cases_are_refused_by_both_judges():
    for c in cs.cases(expect="malformed"):
        with pytest.raises(cs.Malformed):
            py_decode(c)
        with pytest.raises((OSError, pa.ArrowInvalid)):
            lib_decode(c)
    for c in cs.cases(expect="unsupported"):
        with pytest.raises(cs.Unsupported):
            py_decode(c)


@pytest.mark.parametrize("kind", ["snappy", "lz4_raw"])
def test_parquet_files_read_back(kind):
    from arrow_ballista_amd import scan
    L = g.lib()
    for group in (cs.cases(kind, "valid", random=False), cs.cases(kind, "valid", random=True)):
        data = cs.parquet_of(group, kind)
        exp = np.concatenate([cs.int32_of(c.plaintext) for c in group])
        got = pq.read_table(io.BytesIO(data)).column("v").to_numpy()
        assert got.dtype == np.int32 and np.array_equal(got, exp)
        assert scan.parquet_schema(L, data) == ([("v", "Int32", False)], len(exp))
        assert scan.parquet_row_groups(L, data) == [len(exp)]
    for c in cs.cases(kind, "valid", random=False):          # one page each: a failure names the case
        assert np.array_equal(pq.read_table(io.BytesIO(cs.parquet_of([c], kind))).column("v").to_numpy(), cs.int32_of(c.plaintext)), c.name
    c = cs.cases(kind, "valid")[0]                           # the container itself, without a codec
    data = cs.parquet_one_column([(len(c.plaintext) // 4, len(c.plaintext), c.plaintext)], 0)
    assert np.array_equal(pq.read_table(io.BytesIO(data)).column("v").to_numpy(), cs.int32_of(c.plaintext))


def test_ipc_streams_read_back():
    fixed, rnd = cs.cases("lz4_frame", "valid", random=False), cs.cases("lz4_frame", "valid", random=True)
    for group in [[c] for c in fixed] + [rnd[0::2], rnd[1::2]]:
        t = pa.ipc.open_stream(cs.ipc_of(group)).read_all()
        assert t.schema == pa.schema([pa.field("v", pa.int32(), False)])
        assert np.array_equal(t.column("v").to_numpy(), np.concatenate([cs.int32_of(c.plaintext) for c in group])), group[0].name


def _snappy_elements(stream):
    """(kind, length-field width or None, offset or None) of every element of a valid stream"""
    ip = 0
    while stream[ip] & 0x80:
        ip += 1
    ip += 1
    while ip < len(stream):
        tag = stream[ip]
        k = tag & 3
        if k == 0:
            n = (tag >> 2) + 1
            nb = n - 60 if n > 60 else 0
            if nb:
                n = int.from_bytes(stream[ip + 1:ip + 1 + nb], "little") + 1
            yield "lit", nb, None, n
            ip += 1 + nb + n
        else:
            w = (1, 2, 4)[k - 1]
            off = ((tag >> 5) << 8) | stream[ip + 1] if k == 1 else int.from_bytes(stream[ip + 1:ip + 1 + w], "little")
            yield "copy%d" % w, None, off, None
            ip += 1 + w


def _frame_blocks(frame, plain_len):
    """(linked, block size, [(stored, compressed bytes)]) of a valid frame"""
    flg, bd = frame[4], frame[5]
    ip = 7 + 8 * ((flg >> 3) & 1)
    blocks = []
    while True:
        h = int.from_bytes(frame[ip:ip + 4], "little")
        ip += 4
        if h == 0:
            return not (flg >> 5) & 1, 1 << (8 + 2 * ((bd >> 4) & 7)), blocks
        blocks.append((bool(h >> 31), h & 0x7FFFFFFF))
        ip += (h & 0x7FFFFFFF) + 4 * ((flg >> 4) & 1)


def test_the_corpus_still_covers_what_no_encoder_emits():
    kinds, widths, far, three_under_four = set(), set(), 0, 0
    for c in cs.cases("snappy", "valid"):
        for kind, nb, off, n in _snappy_elements(c.stream):
            kinds.add(kind)
            if kind == "lit":
                widths.add(nb)
                three_under_four += nb == 4 and n == 3
            far += kind == "copy4" and off > 65535
    assert kinds == {"lit", "copy1", "copy2", "copy4"}
    assert widths >= {0, 1, 2, 3, 4}
    assert far >= 1 and three_under_four >= 1
    widths_seen = set()
    for c in cs.cases("snappy", "valid"):
        w = 1
        while c.stream[w - 1] & 0x80:
            w += 1
        if w > len(cs.varint(len(c.plaintext))):
            widths_seen.add(w)
    assert widths_seen >= {2, 3, 4, 5}, "no non-minimal preambles"
    stored_only, nonfull_inner, with_bchk, with_csize, with_cchk, bsids, stored_in_linked = 0, 0, 0, 0, 0, set(), 0
    for c in cs.cases("lz4_frame", "valid"):
        linked, bmax, blocks = _frame_blocks(c.stream, len(c.plaintext))
        sizes = []
        out = bytearray()          # block output sizes: re-decode block by block
        ip = 7 + 8 * ((c.stream[4] >> 3) & 1)
        for stored, bs in blocks:
            payload = c.stream[ip + 4:ip + 4 + bs]
            piece = payload if stored else cs.lz4_block_decode(payload, bytes(out[-65535:]) if linked else b"")
            out += piece
            sizes.append(len(piece))
            ip += 4 + bs + 4 * ((c.stream[4] >> 4) & 1)
        stored_only += linked and len(blocks) >= 2 and all(s for s, _ in blocks) and len(c.plaintext) > bmax
        nonfull_inner += linked and any(n < bmax for n in sizes[:-1])
        stored_in_linked += linked and any(s for s, _ in blocks) and not all(s for s, _ in blocks)
        with_bchk += (c.stream[4] >> 4) & 1
        with_csize += (c.stream[4] >> 3) & 1
        with_cchk += (c.stream[4] >> 2) & 1
        bsids.add((c.stream[5] >> 4) & 7)
    assert stored_only >= 2, "no linked frame with zero compressed blocks"
    assert nonfull_inner >= 2, "no linked frame with a non-full inner block"
    assert stored_in_linked >= 2 and with_bchk >= 3 and with_csize >= 3 and with_cchk >= 3 and bsids == {4, 5, 6, 7}


# ---- the shared parsers themselves: a plain-pointer reader, a serial expansion loop, stand-alone, under the sanitizers
HOST_PROGRAM = r"""
#include "lz_elements.h"
#include <cstdio>
#include <cstring>
#include <string>
using namespace gpuq::lz;
// the checks that depend on where the output stands are the caller's, as in the kernels
static bool snappy(const unsigned char* in, int64_t L, unsigned char* out, int64_t n) {
  const auto rd = [&](int64_t a) { return in[a]; };
  const SnHead H = sn_preamble(rd, L);
  if (!H.ok || H.ulen != n) return false;
  int64_t ip = H.start, op = 0;
  while (ip < L) {
    const SnElem e = sn_element(rd, ip, L);
    if (!e.ok || (int64_t)e.olen > n - op) return false;
    if (e.copy) {
      if (e.off == 0 || (int64_t)e.off > op) return false;
      for (uint32_t i = 0; i < e.olen; ++i) out[op + i] = out[op + i - e.off];
    } else std::memcpy(out + op, in + e.lit, e.olen);
    ip += e.size; op += e.olen;
  }
  return op == n;
}
static bool lz4_block(const unsigned char* in, int64_t L, unsigned char* out, int64_t n) {
  const auto rd = [&](int64_t a) { return in[a]; };
  int64_t ip = 0, op = 0;
  while (ip < L) {
    const Lz4Seq e = lz4_sequence(rd, ip, L, L - ip, n - op);
    if (!e.ok) return false;
    std::memcpy(out + op, in + e.lit, (size_t)e.lit_len); op += e.lit_len; ip += e.size;
    if (e.last) break;
    if (e.off == 0 || (int64_t)e.off > op || e.match_len > n - op) return false;
    for (int64_t i = 0; i < e.match_len; ++i) out[op + i] = out[op + i - e.off];
    op += e.match_len;
  }
  return op == n;
}
// corpus file: per case  u32 name length, name, u8 kind (0 snappy, 1 lz4_raw), u64 stream length, stream, u64 plaintext length, plaintext
// prints per case: name <tab> E exact, R refused, W accepted with other bytes
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  for (;;) {
    uint32_t nl; if (std::fread(&nl, 4, 1, f) != 1) break;
    std::string name(nl, ' '); uint8_t kind; uint64_t sl, pl;
    if (std::fread(&name[0], 1, nl, f) != nl || std::fread(&kind, 1, 1, f) != 1 || std::fread(&sl, 8, 1, f) != 1) return 2;
    unsigned char* in = new unsigned char[sl];      // exact-size heap buffers: an overrun is ASan's
    if (std::fread(in, 1, sl, f) != sl || std::fread(&pl, 8, 1, f) != 1) return 2;
    unsigned char* want = new unsigned char[pl];
    if (std::fread(want, 1, pl, f) != pl) return 2;
    unsigned char* out = new unsigned char[pl]; std::memset(out, 0xA5, pl);
    const bool ok = kind == 0 ? snappy(in, (int64_t)sl, out, (int64_t)pl) : lz4_block(in, (int64_t)sl, out, (int64_t)pl);
    std::printf("%s\t%c\n", name.c_str(), !ok ? 'R' : (std::memcmp(out, want, pl) == 0 ? 'E' : 'W'));
    delete[] in; delete[] want; delete[] out;
  }
  std::fclose(f);
  return 0;
}
"""


def test_host_build_of_the_parsers_under_sanitizers(tmp_path):
    """Every snappy and lz4_raw case of the corpus through csrc/lz_elements.h: valid ones byte exact, malformed ones refused, and a clean
    exit -- no read outside the exact-size buffers, no undefined behaviour.  (lz4_frame cases: their container checks are emit()'s.)"""
    todo = [c for c in cs.corpus() if c.kind in ("snappy", "lz4_raw")]
    assert len(todo) == len(cs.cases("snappy")) + len(cs.cases("lz4_raw")) and {c.expect for c in todo} == {"valid", "malformed"}
    src, exe, path = str(tmp_path / "lz_host.cpp"), str(tmp_path / "lz_host"), str(tmp_path / "corpus.bin")
    with open(src, "w") as f:
        f.write(HOST_PROGRAM)
    # the sanitizers' runtimes linked statically: the program starts in any environment, whatever that environment preloads
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                        "-I", CSRC, src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with open(path, "wb") as f:
        for c in todo:
            n = c.name.encode()
            f.write(struct.pack("<I", len(n)) + n + bytes([c.kind == "lz4_raw"]) + struct.pack("<Q", len(c.stream)) + c.stream + struct.pack("<Q", len(c.plaintext)) + c.plaintext)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "the sanitised host build stopped:\n" + r.stdout[-1500:] + r.stderr[-6000:]
    got = dict(line.split("\t") for line in r.stdout.splitlines())
    assert list(got) == [c.name for c in todo]
    assert [c.name + ": " + got[c.name] for c in todo if got[c.name] != {"valid": "E", "malformed": "R"}[c.expect]] == []
