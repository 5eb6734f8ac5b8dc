"""The hand-assembled ZSTD corpus of zstd_streams.py is right before any kernel sees it, and so is the decoder's logic on it: the
plaintext by construction and libzstd (through pyarrow) agree on every valid case; libzstd refuses every malformed and lenient one;
the Parquet containers read back through Arrow C++ and the project's own footer walk; the corpus still holds what libzstd never
writes; and the one-lane host build of csrc/zstd_dec.h, as a stand-alone program under AddressSanitizer and UBSan, decodes every
valid case byte for byte and refuses every malformed one within bounds.  No GPU."""
import io
import os
import struct
import subprocess
import time

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import arrow_ballista_amd as g
import compressed_streams as cs
import zstd_streams as zs

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "arrow-ballista_amd", "csrc")
EXPECT = {"valid": 0, "malformed": 1, "unsupported": 2, "lenient": 3}


def lib_decode(c):
    return pa.Codec("zstd").decompress(c.stream, len(c.plaintext)).to_pybytes()


def test_corpus_shape_and_build_time():
    t0 = time.process_time()      # this process's own CPU time: what a loaded machine does not stretch
    corpus = zs.corpus.__wrapped__()      # built afresh, and the copy the other tests share stays where it is
    took = time.process_time() - t0
    print("corpus: %d cases in %.2f s" % (len(corpus), took))
    assert took < 20, "building the corpus is to take seconds"
    assert corpus == zs.corpus(), "the corpus is the same every time it is built"
    names = [c.name for c in corpus]
    assert len(names) == len(set(names))
    for c in corpus:
        assert c.kind == "zstd" and c.name.startswith("zstd/") and c.expect in EXPECT and c.reason, c.name
        assert len(c.plaintext) <= 410_000, c.name
        if c.expect in ("valid", "lenient"):
            assert len(c.plaintext) >= 4 and len(c.plaintext) % 4 == 0, c.name
    assert len(zs.cases("valid", random=False)) >= 60
    rnd = zs.cases("valid", random=True)
    assert len([c for c in rnd if "full" not in c.name]) >= 200 and 3 <= len([c for c in rnd if "full" in c.name]) <= 8
    assert all(50 <= len(c.plaintext) <= 2000 for c in rnd if "full" not in c.name)
    assert all(len(c.plaintext) == 131072 for c in rnd if "full" in c.name)
    assert len(zs.cases("malformed")) >= 25
    assert 1 <= len(zs.cases("lenient")) <= 6
    assert [c.name for c in zs.cases("unsupported")] == ["zstd/bad_dictionary_id"]
    for c in zs.cases("malformed") + zs.cases("unsupported"):
        assert "`" in c.reason and any(fn in c.reason for fn in ("decode_frames", "decode_block", "seq_table", "fse_read_table", "huf_read_tree", "huf_stream", "Back::init")), c.name
    for c in zs.cases("lenient"):
        assert "section" in c.reason and '"' in c.reason, c.name


def test_valid_cases_equal_libzstd():
    for c in zs.cases("valid"):
        assert lib_decode(c) == c.plaintext, c.name


def test_libzstd_refuses_malformed_and_lenient_cases():
    for c in zs.cases("malformed") + zs.cases("lenient"):
        with pytest.raises((OSError, pa.ArrowInvalid)):
            lib_decode(c)


def test_parquet_files_read_back():
    from arrow_ballista_amd import scan
    L = g.lib()
    for group in (zs.cases("valid", random=False), zs.cases("valid", random=True)):
        data = cs.parquet_of(group, "zstd")
        exp = np.concatenate([cs.int32_of(c.plaintext) for c in group])
        got = pq.read_table(io.BytesIO(data)).column("v").to_numpy()
        assert got.dtype == np.int32 and np.array_equal(got, exp)
        assert scan.parquet_schema(L, data) == ([("v", "Int32", False)], len(exp))
        assert scan.parquet_row_groups(L, data) == [len(exp)]
    for c in zs.cases("valid", random=False)[::7]:          # one page each: the container holds a single page as well
        assert np.array_equal(pq.read_table(io.BytesIO(cs.parquet_of([c], "zstd"))).column("v").to_numpy(), cs.int32_of(c.plaintext)), c.name


# ---- a header walk: as much of the format as finding every header needs, not a decoder
def _walk(stream):
    """facts about a valid page: frame header fields, block types, literals kinds and size formats, sequence count forms, table modes"""
    F = dict(frames=0, skippable=0, fcs=set(), single=set(), checksum=0, did=set(), block_types=set(), empty_last_raw=0, lit=set(), count_forms=set(),
             modes={"ll": set(), "of": set(), "ml": set()}, mode_triples=set(), after_repeat={"ll": set(), "of": set(), "ml": set()})
    ip = 0
    while ip < len(stream):
        magic = struct.unpack_from("<I", stream, ip)[0]
        if magic & 0xFFFFFFF0 == zs.SKIP_MAGIC:
            F["skippable"] += 1
            ip += 8 + struct.unpack_from("<I", stream, ip + 4)[0]
            continue
        assert magic == zs.ZSTD_MAGIC
        fhd = stream[ip + 4]
        ip += 5
        single, did = (fhd >> 5) & 1, (0, 1, 2, 4)[fhd & 3]
        fcs = (single, 2, 4, 8)[fhd >> 6]
        F["frames"] += 1
        F["fcs"].add(fcs)
        F["single"].add(single)
        F["did"].add(did)
        F["checksum"] += (fhd >> 2) & 1
        ip += (0 if single else 1) + did + fcs
        last_mode = {}
        while True:
            bh = int.from_bytes(stream[ip:ip + 3], "little")
            ip += 3
            last, typ, size = bh & 1, (bh >> 1) & 3, bh >> 3
            F["block_types"].add(typ)
            F["empty_last_raw"] += last and typ == 0 and size == 0
            if typ == 2:
                b = stream[ip:ip + size]
                lt, sf = b[0] & 3, (b[0] >> 2) & 3
                if lt < 2:
                    h = 1 if sf & 1 == 0 else 2 if sf == 1 else 3
                    regen = int.from_bytes(b[:h], "little") >> (3 if h == 1 else 4)
                    F["lit"].add((("raw", "rle")[lt], h, regen < (32 if h == 2 else 4096 if h == 3 else 0)))
                    at = h + (regen if lt == 0 else 1)
                else:
                    h, n = (3, 10) if sf < 2 else (4, 14) if sf == 2 else (5, 18)
                    v = int.from_bytes(b[:h], "little")
                    regen, comp = (v >> 4) & ((1 << n) - 1), (v >> (4 + n)) & ((1 << n) - 1)
                    F["lit"].add((("huffman", "treeless")[lt - 2], 1 if sf == 0 else 4, n, n > 10 and max(regen, comp) < 1 << (n - 4)))
                    if lt == 2:
                        F["lit"].add(("tree", "direct" if b[h] >= 128 else "fse"))
                    at = h + comp
                c = b[at]
                form, nseq = (1, c) if c < 128 else (2, ((c - 128) << 8) + b[at + 1]) if c < 255 else (3, b[at + 1] + (b[at + 2] << 8) + 0x7F00)
                F["count_forms"].add((form, form == 2 and nseq < 128))
                if nseq:
                    m = b[at + form]
                    triple = ((m >> 6) & 3, (m >> 4) & 3, (m >> 2) & 3)
                    F["mode_triples"].add(triple)
                    for w, mode in zip(("ll", "of", "ml"), triple):
                        F["modes"][w].add(mode)
                        if mode == 3:
                            F["after_repeat"][w].add(last_mode[w])
                        else:
                            last_mode[w] = mode
            ip += 1 if typ == 1 else size
            if last:
                break
        ip += 4 * ((fhd >> 2) & 1)
    assert ip == len(stream)
    return F


def test_the_corpus_still_covers_what_libzstd_never_writes():
    fixed = zs.cases("valid", random=False)
    W = {c.name: _walk(c.stream) for c in fixed}

    def union(key, sub=None):
        out = set()
        for f in W.values():
            out |= f[key] if sub is None else f[key][sub]
        return out
    assert union("fcs") == {0, 1, 2, 4, 8} and union("single") == {0, 1} and union("did") == {0, 1, 2, 4}
    assert sum(f["checksum"] for f in W.values()) >= 2
    assert sum(f["frames"] >= 2 for f in W.values()) >= 4 and sum(f["frames"] >= 3 for f in W.values()) >= 1, "no multi-frame pages"
    assert sum(f["skippable"] for f in W.values()) >= 3, "no skippable frames"
    fcs2 = [c for c in fixed if 2 in W[c.name]["fcs"] and W[c.name]["frames"] == 1]
    assert any(len(c.plaintext) >= 65536 for c in fcs2) and any(len(c.plaintext) == 256 for c in fcs2), "2-byte content sizes at their ends"
    assert union("block_types") == {0, 1, 2} and sum(f["empty_last_raw"] for f in W.values()) >= 1
    lit = union("lit")
    for kind in ("raw", "rle"):
        assert {(kind, 1, False), (kind, 2, False), (kind, 3, False), (kind, 2, True), (kind, 3, True)} <= lit, "%s literals: a header form is gone" % kind
    assert {("huffman", 1, 10, False), ("huffman", 4, 10, False), ("huffman", 4, 14, False), ("huffman", 4, 18, False), ("huffman", 4, 14, True), ("huffman", 4, 18, True),
            ("treeless", 1, 10, False), ("treeless", 4, 14, False), ("tree", "direct"), ("tree", "fse")} <= lit
    assert union("count_forms") == {(1, False), (2, False), (2, True), (3, False)}
    for w in ("ll", "of", "ml"):
        assert union("modes", w) == {0, 1, 2, 3}, w
        assert union("after_repeat", w) == {0, 1, 2}, "Repeat_Mode after every kind of table, for " + w
    assert sum(len(set(t)) == 3 for t in union("mode_triples")) >= 3, "blocks whose three tables each have a mode of their own"
    offs = [zs.facts(c.name) for c in fixed]
    assert sum(lo < 64 for lo, hi in offs) >= 10 and sum(hi > 131072 for lo, hi in offs) >= 2, "offsets below 64 and above 128 KiB"
    rnd = [_walk(c.stream) for c in zs.cases("valid", random=True)]
    for w in ("ll", "of", "ml"):
        assert set().union(*(f["modes"][w] for f in rnd)) == {0, 1, 2, 3}
    assert {k[0] for f in rnd for k in f["lit"]} >= {"raw", "rle", "huffman", "treeless"}


# ---- the decoder itself: one lane, stand-alone, under the sanitizers
HOST_PROGRAM = r'''
#include "zstd_dec.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
// corpus file: per case  u32 name length, name, u8 class, u64 stream length, stream, u64 plaintext length, plaintext
// prints per case: name <tab> class <tab> one letter per variant -- E exact, R refused, W accepted with other bytes -- and D when every
//   refusal named a dictionary as its cause, M when some did and some did not, - when none did
//   variant 0: LDS ring + windows; 1: windows without the ring (what the kernel passes); 2: neither
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  static gpuq::zs::Shared S;
  for (;;) {
    uint32_t nl; if (std::fread(&nl, 4, 1, f) != 1) break;
    std::string name(nl, ' '); uint8_t cls; uint64_t sl, pl;
    if (std::fread(&name[0], 1, nl, f) != nl || std::fread(&cls, 1, 1, f) != 1 || std::fread(&sl, 8, 1, f) != 1) return 2;
    unsigned char* in = new unsigned char[sl];      // exact-size heap buffers: an overrun is ASan's
    if (std::fread(in, 1, sl, f) != sl || std::fread(&pl, 8, 1, f) != 1) return 2;
    unsigned char* want = new unsigned char[pl];
    if (std::fread(want, 1, pl, f) != pl) return 2;
    char res[5] = {0, 0, 0, 0, 0};
    int named = 0;
    for (int v = 0; v < 3; ++v) {
      unsigned char* out = new unsigned char[pl]; std::memset(out, 0xA5, pl);
      unsigned char* scratch = new unsigned char[gpuq::zs::BLOCK_MAX + 64];
      unsigned char* ring = new unsigned char[gpuq::zs::RING]; unsigned char* litw = new unsigned char[gpuq::zs::LITW];
      uint64_t* bitw = new uint64_t[gpuq::zs::BITW / 8 + 2]; uint64_t* hufw = new uint64_t[4 * (gpuq::zs::HUFW / 8 + 2)];
      bool dictionary = false;
      const bool ok = v < 2 ? gpuq::zs::decode_frames(in, (int64_t)sl, out, (int64_t)pl, scratch, S, gpuq::zs::Lds{v == 0 ? ring : nullptr, litw, bitw, hufw}, &dictionary)
                            : gpuq::zs::decode_frames(in, (int64_t)sl, out, (int64_t)pl, scratch, S, gpuq::zs::Lds{nullptr, nullptr, nullptr, nullptr}, &dictionary);
      named += dictionary && !ok;
      if (dictionary && ok) return 3;      // only a refusal has a cause
      res[v] = !ok ? 'R' : (std::memcmp(out, want, pl) == 0 ? 'E' : 'W');
      delete[] out; delete[] scratch; delete[] ring; delete[] litw; delete[] bitw; delete[] hufw;
    }
    res[3] = named == 3 ? 'D' : named ? 'M' : '-';
    std::printf("%s\t%d\t%s\n", name.c_str(), (int)cls, res);
    delete[] in; delete[] want;
  }
  std::fclose(f);
  return 0;
}
'''


def write_corpus_file(path, cases):
    with open(path, "wb") as f:
        for c in cases:
            n = c.name.encode()
            f.write(struct.pack("<I", len(n)) + n + bytes([EXPECT[c.expect]]) + struct.pack("<Q", len(c.stream)) + c.stream + struct.pack("<Q", len(c.plaintext)) + c.plaintext)


def build_host_program(directory, include=CSRC):
    src, exe = os.path.join(directory, "zstd_host.cpp"), os.path.join(directory, "zstd_host")
    with open(src, "w") as f:
        f.write(HOST_PROGRAM)
    # the sanitizers' runtimes linked statically: the program starts in any environment, whatever that environment preloads
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                        "-I", include, src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def host_results(directory, cases, include=CSRC):
    """{name: "EEE-" ...} from the sanitised stand-alone program: an ordinary child process in this process's own environment"""
    exe = build_host_program(directory, include)
    path = os.path.join(directory, "corpus.bin")
    write_corpus_file(path, cases)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "the sanitised host build stopped:\n" + r.stdout[-1500:] + r.stderr[-6000:]
    out = {}
    for line in r.stdout.splitlines():
        name, _, res = line.split("\t")
        out[name] = res
    assert list(out) == [c.name for c in cases]
    return out


def judge(cases, results):
    """names (with what happened) of the cases the decoder got wrong"""
    bad = []
    for c in cases:
        r = results[c.name]
        good = r == "EEE-" if c.expect == "valid" else r == "RRR-" if c.expect == "malformed" else r == "RRRD" if c.expect == "unsupported" else set(r[:3]) <= set("ER") and r[3] == "-"
        if not good:
            bad.append("%s: %s" % (c.name, r))
    return bad


def test_host_build_of_the_decoder_under_sanitizers(tmp_path):
    """Valid cases byte exact in all three variants, malformed and unsupported ones refused in all three, lenient ones refused or exact,
    and a clean exit: no access outside the exact-size buffers, no undefined behaviour."""
    assert judge(zs.corpus(), host_results(str(tmp_path), zs.corpus())) == []
