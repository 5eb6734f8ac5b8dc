// APPROX_DISTINCT: one HyperLogLog sketch per segment of a column (include/gpuq.h gpuq_segment_approx_distinct; hll_estimate.h has the
// hash and the estimator).
//
// What it stands in for in the reference: DataFusion 34's ApproxDistinct accumulator, one HyperLogLog<T> per group updated row by row
// [UPSTREAM-KNOWLEDGE: datafusion physical-expr aggregate/approx_distinct.rs, hyperloglog.rs; the crate is not in the tree].  Here the
// rows of a group lie together (the plan executor sorts by the keys, or there are none), so a sketch is 16 KB of LDS that lives for one
// piece of one segment:
//   * sketch: one block per tile of tile_rows consecutive rows.  The block finds its first segment by binary search in `starts` and
//     walks the pieces of segments that lie in its tile: clear the registers, hash the rows into them (a register is read first and
//     raised by a compare-and-swap on its LDS word only when the row's rank is larger -- after a few thousand rows almost none is),
//     then either finish the segment in place (histogram of the register values, the estimator on one lane) or, when the segment
//     crosses a tile edge, store the registers to the tile's partial slot: slot 0 for a piece that began before the tile, slot 1 for
//     one that goes on behind it.
//   * merge: one block per tile.  The tile in which a crossing segment begins owns it: its slot 1 and slot 0 of the following tiles
//     are merged by bytewise max, then histogram and estimator as above.  With more than 64 tiles a first level folds the tiles behind
//     an owner in 32 runs, each into its first slot, so that no block walks more than about 1/32 of them plus 32.
// Reads n x width bytes once; no global atomics; the registers are maxima, so the result does not depend on the order of the rows.
// Nothing here is specialised at run time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpuq_kernels.h"
#include "hll_estimate.h"

namespace gpuq {

namespace {
constexpr int HLL_BLOCK = 256;
constexpr int HLL_VEC = HLL_M / 16 / HLL_BLOCK;      // 16-byte pieces of the registers per thread: 4

struct HllLds {
  uint4 regs[HLL_M / 16];      // the registers, one byte each
  uint32_t hist[HLL_BINS];
};

__device__ __forceinline__ bool hll_bit(const uint8_t* __restrict__ bits, i64 i) { return (bits[i >> 3] >> (i & 7)) & 1; }

// row i as the two words that are hashed; false: NULL
__device__ __forceinline__ bool hll_load(const HllCol& c, const i64 i, u64& lo, u64& hi) {
  if (c.valid && !hll_bit(c.valid, i)) return false;
  hi = 0;
  switch (c.width) {
    case 1: lo = c.kind == HLL_SINT ? (u64)(i64)((const int8_t*)c.data)[i] : (u64)((const uint8_t*)c.data)[i]; break;
    case 2: lo = c.kind == HLL_SINT ? (u64)(i64)((const int16_t*)c.data)[i] : (u64)((const uint16_t*)c.data)[i]; break;
    case 4: {
      const uint32_t v = ((const uint32_t*)c.data)[i];
      if (c.kind == HLL_F32) lo = (v & 0x7FFFFFFFu) > 0x7F800000u ? 0x7FC00000u : v == 0x80000000u ? 0u : v;      // every NaN is one value; -0.0 is 0.0
      else lo = c.kind == HLL_SINT ? (u64)(i64)(int32_t)v : (u64)v;
      break;
    }
    case 8: {
      const u64 v = ((const u64*)c.data)[i];
      if (c.kind == HLL_F64) lo = (v & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull ? 0x7FF8000000000000ull : v == 0x8000000000000000ull ? 0ull : v;
      else lo = v;
      break;
    }
    default: { const u64* p = (const u64*)c.data + 2 * i; lo = p[0]; hi = p[1]; break; }      // Decimal128, PACKED15: the two words as they lie
  }
  return true;
}

__device__ __forceinline__ void hll_clear(HllLds& L) {
#pragma unroll
  for (int k = 0; k < HLL_VEC; ++k) L.regs[threadIdx.x + k * HLL_BLOCK] = make_uint4(0, 0, 0, 0);
  if (threadIdx.x < HLL_BINS) L.hist[threadIdx.x] = 0;
}

__device__ __forceinline__ void hll_add(HllLds& L, const u64 lo, const u64 hi) {
  const u64 h = hll_hash(lo, hi);
  const uint32_t idx = hll_index(h), rho = hll_rho(h), sh = (idx & 3u) * 8u;
  uint32_t* w = (uint32_t*)L.regs + (idx >> 2);
  uint32_t old = *(volatile uint32_t*)w;      // (a stale word only costs a turn of the loop)
  while (((old >> sh) & 0xFFu) < rho) {
    const uint32_t prev = atomicCAS(w, old, (old & ~(0xFFu << sh)) | (rho << sh));
    if (prev == old) break;
    old = prev;
  }
}

// The registers are complete (and hist zero) behind a barrier: their histogram, then the estimate on one lane.  C[0] is what is left of m.
__device__ __forceinline__ void hll_finish(HllLds& L, u64* __restrict__ out) {
#pragma unroll
  for (int k = 0; k < HLL_VEC; ++k) {
    const uint4 v = L.regs[threadIdx.x + k * HLL_BLOCK];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (w[q] == 0) continue;
#pragma unroll
      for (int b = 0; b < 4; ++b) { const uint32_t r = (w[q] >> (8 * b)) & 0xFFu; if (r) atomicAdd(&L.hist[r < HLL_BINS ? r : HLL_BINS - 1], 1u); }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t set = 0;
    for (int k = 1; k < HLL_BINS; ++k) set += L.hist[k];
    L.hist[0] = (uint32_t)HLL_M - set;
    *out = hll_estimate(L.hist);
  }
}

// the first index in starts[0 .. n_groups] whose value is larger than `row`
__device__ __forceinline__ i64 hll_upper(const int32_t* __restrict__ starts, const i64 n_groups, const i64 row) {
  i64 lo = 0, hi = n_groups + 1;
  while (lo < hi) { const i64 m = lo + (hi - lo) / 2; if ((i64)starts[m] <= row) lo = m + 1; else hi = m; }
  return lo;
}

__device__ __forceinline__ uint4* hll_slot(uint8_t* __restrict__ partial, const i64 tile, const int slot) { return (uint4*)(partial + (size_t)(2 * tile + slot) * HLL_M); }

__global__ void __launch_bounds__(HLL_BLOCK) k_hll_sketch(const HllCol col, const int32_t* __restrict__ starts, const i64 n_groups, const i64 n_rows, const i64 tile_rows,
                                                          uint8_t* __restrict__ partial, u64* __restrict__ out) {
  __shared__ HllLds L;
  const i64 tile = blockIdx.x, row0 = tile * tile_rows, row1 = row0 + tile_rows < n_rows ? row0 + tile_rows : n_rows;
  const i64 u = hll_upper(starts, n_groups, row0);
  for (i64 g = u > 0 ? u - 1 : 0; g < n_groups; ++g) {
    const i64 s0 = starts[g], s1 = (i64)starts[g + 1] < n_rows ? (i64)starts[g + 1] : n_rows;
    if (s0 >= row1) break;
    const i64 a = s0 > row0 ? s0 : row0, b = s1 < row1 ? s1 : row1;
    if (a >= b) continue;
    hll_clear(L);
    __syncthreads();
    i64 i = a + threadIdx.x;
    for (; i + 3 * HLL_BLOCK < b; i += 4 * HLL_BLOCK) {      // four rows a lane with their loads in flight together
      u64 lo[4], hi[4]; bool ok[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) ok[k] = hll_load(col, i + k * HLL_BLOCK, lo[k], hi[k]);
#pragma unroll
      for (int k = 0; k < 4; ++k) if (ok[k]) hll_add(L, lo[k], hi[k]);
    }
    for (; i < b; i += HLL_BLOCK) {
      u64 lo, hi;
      if (hll_load(col, i, lo, hi)) hll_add(L, lo, hi);
    }
    __syncthreads();
    if (a == s0 && b == s1) hll_finish(L, out + g);
    else {
      uint4* dst = hll_slot(partial, tile, a == s0 ? 1 : 0);
#pragma unroll
      for (int k = 0; k < HLL_VEC; ++k) dst[threadIdx.x + k * HLL_BLOCK] = L.regs[threadIdx.x + k * HLL_BLOCK];
    }
    __syncthreads();      // (the next piece clears what this one still reads)
  }
}

// bytewise max of two words whose bytes are below 128 (a register holds 51 at most)
__device__ __forceinline__ uint32_t hll_max4(const uint32_t a, const uint32_t b) {
  const uint32_t ge = (((a | 0x80808080u) - b) >> 7) & 0x01010101u;      // 1 in every byte where a >= b: no byte borrows from its neighbour
  const uint32_t mask = ge * 0xFFu;
  return (a & mask) | (b & ~mask);
}

// Does a segment that goes on behind `tile` begin in it?  Then the tile owns segment g, whose partial sketches are the tile's slot 1 and
// slot 0 of the tiles behind it up to `last`.
__device__ __forceinline__ bool hll_owns(const int32_t* __restrict__ starts, const i64 n_groups, const i64 n_rows, const i64 tile_rows, const i64 tile, i64& g, i64& last) {
  const i64 row0 = tile * tile_rows, row1 = row0 + tile_rows < n_rows ? row0 + tile_rows : n_rows;
  // the segment of the tile's last row: the one segment that can begin here and go on behind the tile
  const i64 u = hll_upper(starts, n_groups, row1 - 1);
  if (u == 0 || u > n_groups) return false;
  g = u - 1;
  const i64 s0 = starts[g], s1 = (i64)starts[g + 1] < n_rows ? (i64)starts[g + 1] : n_rows;
  if (s0 < row0 || s1 <= row1) return false;
  last = (s1 - 1) / tile_rows;
  return true;
}
// the tiles behind an owner are merged in HLL_FAN runs of `step` tiles first when there are many (two_level), each run into its first tile's slot 0
constexpr int HLL_FAN = 32;
__device__ __forceinline__ i64 hll_step(const i64 tile, const i64 last, const int two_level) { return two_level ? (last - tile + HLL_FAN - 1) / HLL_FAN : 1; }

__device__ __forceinline__ void hll_max_into(uint4 (&acc)[HLL_VEC], const uint4* __restrict__ p) {
#pragma unroll
  for (int k = 0; k < HLL_VEC; ++k) {
    const uint4 v = p[threadIdx.x + k * HLL_BLOCK];
    acc[k].x = hll_max4(acc[k].x, v.x); acc[k].y = hll_max4(acc[k].y, v.y); acc[k].z = hll_max4(acc[k].z, v.z); acc[k].w = hll_max4(acc[k].w, v.w);
  }
}

// first level, grid (tiles, HLL_FAN): block (t, k) folds the k-th run of tiles behind owner t into the run's first slot 0 -- the only
// block that reads or writes those slots
__global__ void __launch_bounds__(HLL_BLOCK) k_hll_merge_runs(const int32_t* __restrict__ starts, const i64 n_groups, const i64 n_rows, const i64 tile_rows,
                                                              uint8_t* __restrict__ partial) {
  i64 g, last;
  const i64 tile = blockIdx.x;
  if (!hll_owns(starts, n_groups, n_rows, tile_rows, tile, g, last)) return;
  const i64 step = hll_step(tile, last, 1), first = tile + 1 + (i64)blockIdx.y * step, end = first + step - 1 < last ? first + step - 1 : last;
  if (step < 2 || first >= end) return;      // nothing, or one tile: it stays as it lies
  uint4* head = hll_slot(partial, first, 0);
  uint4 acc[HLL_VEC];
#pragma unroll
  for (int k = 0; k < HLL_VEC; ++k) acc[k] = head[threadIdx.x + k * HLL_BLOCK];
#pragma unroll 2
  for (i64 t = first + 1; t <= end; ++t) hll_max_into(acc, hll_slot(partial, t, 0));
#pragma unroll
  for (int k = 0; k < HLL_VEC; ++k) head[threadIdx.x + k * HLL_BLOCK] = acc[k];
}

__global__ void __launch_bounds__(HLL_BLOCK) k_hll_merge(const int32_t* __restrict__ starts, const i64 n_groups, const i64 n_rows, const i64 tile_rows,
                                                         uint8_t* __restrict__ partial, u64* __restrict__ out, const int two_level) {
  __shared__ HllLds L;
  i64 g, last;
  const i64 tile = blockIdx.x;
  if (!hll_owns(starts, n_groups, n_rows, tile_rows, tile, g, last)) return;
  const i64 step = hll_step(tile, last, two_level);
  uint4 acc[HLL_VEC];
  const uint4* own = hll_slot(partial, tile, 1);
#pragma unroll
  for (int k = 0; k < HLL_VEC; ++k) acc[k] = own[threadIdx.x + k * HLL_BLOCK];
#pragma unroll 2
  for (i64 t = tile + 1; t <= last; t += step) hll_max_into(acc, hll_slot(partial, t, 0));
#pragma unroll
  for (int k = 0; k < HLL_VEC; ++k) L.regs[threadIdx.x + k * HLL_BLOCK] = acc[k];
  if (threadIdx.x < HLL_BINS) L.hist[threadIdx.x] = 0;
  __syncthreads();
  hll_finish(L, out + g);
}
}  // namespace

i64 hll_tile_rows(i64 n_rows) {
  // about a thousand tiles at most (four blocks a CU in one round; 2 x 16 KB of partial sketch a tile), and no tile so small that
  // clearing and folding 16 KB weighs against its rows
  const i64 per = (n_rows + 1023) / 1024;
  const i64 t = (per + HLL_BLOCK - 1) / HLL_BLOCK * HLL_BLOCK;
  return t < 8192 ? 8192 : t;
}
i64 hll_tiles(i64 n_rows, i64 tile_rows) { return n_rows <= 0 ? 0 : (n_rows + tile_rows - 1) / tile_rows; }
size_t hll_partial_bytes(i64 n_rows, i64 tile_rows) { return (size_t)hll_tiles(n_rows, tile_rows) * 2 * HLL_M; }

void launch_hll_approx_distinct(hipStream_t s, const HllCol& col, const int32_t* starts, i64 n_groups, i64 n_rows, i64 tile_rows, void* partial, u64* out) {
  const i64 tiles = hll_tiles(n_rows, tile_rows);
  if (n_groups <= 0 || tiles <= 0) return;
  hipLaunchKernelGGL(k_hll_sketch, dim3((unsigned)tiles), dim3(HLL_BLOCK), 0, s, col, starts, n_groups, n_rows, tile_rows, (uint8_t*)partial, out);
  if (tiles <= 1) return;
  const int two_level = tiles > 2 * HLL_FAN ? 1 : 0;      // a segment over many tiles: its partial sketches are folded in HLL_FAN runs first
  if (two_level) hipLaunchKernelGGL(k_hll_merge_runs, dim3((unsigned)tiles, HLL_FAN), dim3(HLL_BLOCK), 0, s, starts, n_groups, n_rows, tile_rows, (uint8_t*)partial);
  hipLaunchKernelGGL(k_hll_merge, dim3((unsigned)tiles), dim3(HLL_BLOCK), 0, s, starts, n_groups, n_rows, tile_rows, (uint8_t*)partial, out, two_level);
}

}  // namespace gpuq
