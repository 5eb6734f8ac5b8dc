// gpuq -- the Snappy and LZ4 stream formats: what an element, a sequence, a preamble and a frame's block index ARE.
//
// Format knowledge only: nothing here copies a byte, owns a buffer or knows about lanes.  Every function is a template over a byte
// reader `rd(pos) -> byte`, so each caller keeps its own way of fetching bytes -- plain global memory in the all-positions kernels,
// the LDS window of the serial Snappy decoder's preamble (kernels_lz4.hip), a host pointer in shuffle_codec.cpp and in the tests.  No function reads at or beyond the end it is given, and none reads before `p`.  What depends on where the OUTPUT
// stands (an offset of 0, an offset that reaches before the output's start, a length beyond the room that is left) stays with the caller.
// The two SERIAL decoders' loops (k_unpack_pages' element loop; lz4_decode_block and the frame walk around it in k_lz4_decode) do not
// call sn_element / lz4_sequence / lz4_frame_blocks: each is one wave's chain of dependent instructions, and an element that comes back
// as a struct to be branched on again cost them 9-10 % (profiles/README.md, round 8).  They keep their own straight-line statement of
// the format; the sanitised program and the GPU corpus hold both statements to the same streams.
//
// The same text compiles under hipcc for the device and under g++ with no HIP headers: tests/test_cpu_compressed_streams.py runs the
// whole corpus through these parsers in a sanitised stand-alone program.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LZ_FN __host__ __device__ __forceinline__
#else
#define LZ_FN inline
#endif

namespace gpuq {
namespace lz {

// ---------------------------------------------------------------- Snappy
// Raw Snappy block format [UPSTREAM-KNOWLEDGE: google/snappy format_description.txt]: varint uncompressed length, then elements --
// tag & 3 == 0 literal (length (tag >> 2) + 1, or 1-4 length bytes when that is 61-64), 1 copy with 11-bit offset and length 4-11,
// 2 copy with 16-bit offset, 3 copy with 32-bit offset (length (tag >> 2) + 1).

// the preamble of a stream [0, L): the announced length, and where the elements start.  Not ok: it runs past the end, or past 6 bytes
struct SnHead { int64_t ulen, start; bool ok; };
template <class Rd> LZ_FN SnHead sn_preamble(Rd rd, const int64_t L) {
  uint64_t ulen = 0; int sh = 0; int64_t ip = 0;
  for (;;) {
    if (ip >= L || sh > 35) return {0, ip, false};
    const uint32_t c = (uint32_t)rd(ip++); ulen |= (uint64_t)(c & 0x7F) << sh;
    if (!(c & 0x80)) return {(int64_t)ulen, ip, true};
    sh += 7;
  }
}

// the element at p of a stream [0, L), p < L: its size in the stream, the bytes it produces, and either the position of its first
// literal byte or its offset.  Not ok: it runs past L (nothing else about it means anything then)
struct SnElem { int64_t size; uint32_t olen; bool copy; uint32_t off; int64_t lit; bool ok; };
template <class Rd> LZ_FN SnElem sn_element(Rd rd, const int64_t p, const int64_t L) {
  SnElem e{1, 0u, false, 0u, 0, false};
  const uint32_t tag = (uint32_t)rd(p);
  int64_t q = p + 1;
  if ((tag & 3) == 0) {
    int64_t len = (int64_t)(tag >> 2) + 1;
    if (len > 60) {
      const int nb = (int)len - 60;
      if (q + nb > L) return e;
      uint32_t v = 0; for (int k = 0; k < nb; ++k) v |= (uint32_t)rd(q + k) << (8 * k);
      q += nb; len = (int64_t)v + 1;
    }
    e.size = q - p + len;
    if (len > L - q) return e;
    e.olen = (uint32_t)len; e.lit = q; e.ok = true;
    return e;
  }
  e.copy = true;
  if ((tag & 3) == 1) { e.size = 2; if (q + 1 > L) return e; e.olen = 4 + ((tag >> 2) & 7); e.off = ((tag >> 5) << 8) | (uint32_t)rd(q); }
  else if ((tag & 3) == 2) { e.size = 3; if (q + 2 > L) return e; e.olen = (tag >> 2) + 1; e.off = (uint32_t)rd(q) | ((uint32_t)rd(q + 1) << 8); }
  else { e.size = 5; if (q + 4 > L) return e; e.olen = (tag >> 2) + 1; e.off = (uint32_t)rd(q) | ((uint32_t)rd(q + 1) << 8) | ((uint32_t)rd(q + 2) << 16) | ((uint32_t)rd(q + 3) << 24); }
  e.ok = true;
  return e;
}

// ---------------------------------------------------------------- LZ4 block
// One sequence starting at p of a block that ends at L (p < L; both in the reader's coordinates): token, literal length (+255-runs),
// literals, then -- unless the literals end the block: `last` -- a 2-byte offset and the match length (+255-runs, + 4).
// `lit_bound` / `match_bound`: no valid literal run / match is longer (literals are bytes of the block, a match is bytes of its output
// and may be far longer than the block).  The lengths are 64-bit and checked against their bound WHILE they grow: a long run of 0xFF
// length bytes must neither wrap, nor be walked to its end from every position inside it (that keeps the all-positions pass linear).
// Not ok: the block ends inside the sequence, or a length passed its bound.
struct Lz4Seq { int64_t lit, lit_len; bool last; uint32_t off; int64_t match_len, size; bool ok; };
template <class Rd> LZ_FN bool lz4_length_run(Rd rd, int64_t& q, const int64_t L, const int64_t bound, int64_t& len) {
  if (len != 15) return true;
  uint32_t x;
  do { if (q >= L || len > bound) return false; x = (uint32_t)rd(q++); len += x; } while (x == 255);
  return true;
}
template <class Rd> LZ_FN Lz4Seq lz4_sequence(Rd rd, const int64_t p, const int64_t L, const int64_t lit_bound, const int64_t match_bound) {
  Lz4Seq e{0, 0, false, 0u, 0, 0, false};
  int64_t q = p;
  const uint32_t token = (uint32_t)rd(q++);
  int64_t lit = token >> 4;
  if (!lz4_length_run(rd, q, L, lit_bound, lit)) return e;
  e.lit = q; e.lit_len = lit;
  if (lit > L - q || lit > lit_bound) return e;
  q += lit;
  if (q == L) { e.last = true; e.size = q - p; e.ok = true; return e; }
  if (q + 2 > L) return e;
  e.off = (uint32_t)rd(q) | ((uint32_t)rd(q + 1) << 8); q += 2;
  int64_t ml = token & 15;
  if (!lz4_length_run(rd, q, L, match_bound, ml)) return e;
  e.match_len = ml + 4; e.size = q - p; e.ok = e.match_len <= match_bound;
  return e;
}

// ---------------------------------------------------------------- LZ4 frame
// The block index of a frame: [ip, iend) are the frame's bytes after its descriptor -- per block a size word (bit 31: stored), the
// block, an optional checksum; a zero word (EndMark) closes it.  `block(pos, size, stored, op, room)` is called per block with the
// output position so far and min(bmax, ulen - op), what the block decodes to when every block but the last is full (<= 0: the frame
// holds more blocks than its length allows); it returns the output position after the block, or a negative value to stop.
// -> the walk ended at the EndMark with exactly ulen bytes of output.
template <class Rd, class F> LZ_FN bool lz4_frame_blocks(Rd rd, int64_t ip, const int64_t iend, const bool block_checksums, const int64_t bmax, const int64_t ulen, F block) {
  int64_t op = 0;
  for (;;) {
    if (ip + 4 > iend) return false;      // a block header or the EndMark is expected here
    const uint32_t h = (uint32_t)rd(ip) | ((uint32_t)rd(ip + 1) << 8) | ((uint32_t)rd(ip + 2) << 16) | ((uint32_t)rd(ip + 3) << 24);
    ip += 4;
    if (h == 0) return op == ulen;
    const int64_t bs = (int64_t)(h & 0x7FFFFFFFu);
    if (bs > iend - ip) return false;
    op = block(ip, bs, (h & 0x80000000u) != 0, op, ulen - op < bmax ? ulen - op : bmax);
    if (op < 0) return false;
    ip += bs + (block_checksums ? 4 : 0);
  }
}

}  // namespace lz
}  // namespace gpuq
