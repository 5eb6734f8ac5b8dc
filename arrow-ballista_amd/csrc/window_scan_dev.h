// The device side of the segmented scan over WinElem (window_scan_op.h): the tile geometry, the loader that widens a value to a cell
// operand, the ordered wave and block scans, and the one-block scan of the tile totals.  Shared by the kernels that run the scan's three
// launches -- per-tile totals, one block over the tile totals, a downsweep from the tile's carry: kernels_window.hip (every row's running
// value) and kernels_distinct.hip (one value per segment, over the run heads of a sorted column).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "window_scan_op.h"

namespace gpuq {

namespace {
constexpr int WIN_BLOCK = 256;
constexpr int WIN_WAVES = WIN_BLOCK / 64;
constexpr int WIN_PER = 8;                          // consecutive rows per thread: one byte of a validity bitmap
constexpr int WIN_TILE = WIN_BLOCK * WIN_PER;       // 2,048

__device__ __forceinline__ bool win_bit(const uint8_t* __restrict__ bits, i64 i) { return (bits[i >> 3] >> (i & 7)) & 1; }

// a value's own bytes, zero-extended to two words (what two rows are compared by)
__device__ __forceinline__ void win_raw(const WinCol& c, const i64 i, u64& lo, u64& hi) {
  hi = 0;
  switch (c.width) {
    case 1: lo = ((const uint8_t*)c.data)[i]; break;
    case 2: lo = ((const uint16_t*)c.data)[i]; break;
    case 4: lo = ((const uint32_t*)c.data)[i]; break;
    case 8: lo = ((const u64*)c.data)[i]; break;
    default: lo = ((const u64*)c.data)[2 * i]; hi = ((const u64*)c.data)[2 * i + 1]; break;
  }
}
// those bytes widened to a cell operand, as the loaders of the other kernels widen a value: integers sign- or zero-extended to 128 bits,
// Float32 as the double of the same value, Float64 its bits
__device__ __forceinline__ void win_widen(const WinCol& c, u64& lo, u64& hi) {
  const bool sgn = c.kind == SEG_SINT;
  switch (c.width) {
    case 1: lo = sgn ? (u64)(i64)(int8_t)lo : lo; break;
    case 2: lo = sgn ? (u64)(i64)(int16_t)lo : lo; break;
    case 4: lo = c.kind == SEG_F32 ? (u64)__double_as_longlong((double)__uint_as_float((uint32_t)lo)) : sgn ? (u64)(i64)(int32_t)lo : lo; break;
    case 8: break;
    default: return;
  }
  hi = sgn ? (u64)((i64)lo >> 63) : 0;
}
__device__ __forceinline__ void win_load(const WinCol& c, const i64 i, u64& lo, u64& hi) { win_raw(c, i, lo, hi); win_widen(c, lo, hi); }

__device__ __forceinline__ WinElem win_shfl_up(const WinElem& v, const int off) {
  WinElem y;
  y.lo = __shfl_up(v.lo, off); y.hi = __shfl_up(v.hi, off); y.count = __shfl_up(v.count, off); y.head = __shfl_up(v.head, off); y.pad = 0;
  return y;
}
__device__ __forceinline__ WinElem win_shfl(const WinElem& v, const int src) {
  WinElem y;
  y.lo = __shfl(v.lo, src); y.hi = __shfl(v.hi, src); y.count = __shfl(v.count, src); y.head = __shfl(v.head, src); y.pad = 0;
  return y;
}
// Inclusive scan over the lanes in lane order (wave_incl_scan's shape; the operator is not commutative, so the earlier lanes stand left)
__device__ __forceinline__ WinElem win_wave_incl_scan(const int kind, WinElem v) {
  const int l = lane();
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const WinElem y = win_shfl_up(v, off); if (l >= off) v = win_combine(kind, y, v); }
  return v;
}
// Exclusive scan of one element per thread across the block, in thread order; *total = the block's, in every thread.  One barrier
// inside, between the stores to wtot and the reads; the kernels below call it once.
__device__ __forceinline__ WinElem win_block_excl_scan(const int kind, const WinElem& v, WinElem* wtot, WinElem* total) {
  const int w = wave(), l = lane();
  const WinElem incl = win_wave_incl_scan(kind, v);
  if (l == 63) wtot[w] = incl;
  __syncthreads();
  WinElem pre = win_identity(kind), all = win_identity(kind);
#pragma unroll
  for (int q = 0; q < WIN_WAVES; ++q) { const WinElem s = wtot[q]; if (q < w) pre = win_combine(kind, pre, s); all = win_combine(kind, all, s); }
  *total = all;
  WinElem before = win_shfl_up(incl, 1);
  if (l == 0) before = win_identity(kind);
  return win_combine(kind, pre, before);
}

// launch 2: one block of 1,024 threads turns the tile totals into the carry INTO every tile, in place.  block_walk_scan's walk -- a
// wave owns a contiguous sixteenth of the array and steps through it 64 tiles at a time -- with the ordered wave scan in place of the
// butterfly, which assumes that the operator commutes.
__global__ void __launch_bounds__(1024) k_window_tiles_scan(WinElem* __restrict__ tiles, const i64 ntiles, const int kind) {
  __shared__ WinElem wtot[16];
  const int w = wave(), l = lane();
  const i64 per = ((ntiles + 15) / 16 + 63) & ~(i64)63;
  const i64 a = (i64)w * per, b = a + per < ntiles ? a + per : ntiles;
  WinElem tot = win_identity(kind);
  for (i64 i0 = a; i0 < b; i0 += 64) {
    const i64 i = i0 + l;
    const WinElem x = win_wave_incl_scan(kind, i < b ? tiles[i] : win_identity(kind));
    tot = win_combine(kind, tot, win_shfl(x, 63));
  }
  if (l == 0) wtot[w] = tot;
  __syncthreads();
  if (threadIdx.x == 0) {
    WinElem run = win_identity(kind);
    for (int k = 0; k < 16; ++k) { const WinElem v = wtot[k]; wtot[k] = run; run = win_combine(kind, run, v); }
  }
  __syncthreads();
  WinElem carry = wtot[w];
  for (i64 i0 = a; i0 < b; i0 += 64) {
    const i64 i = i0 + l;
    const WinElem x = win_wave_incl_scan(kind, i < b ? tiles[i] : win_identity(kind));
    WinElem before = win_shfl_up(x, 1);
    if (l == 0) before = win_identity(kind);
    if (i < b) tiles[i] = win_combine(kind, carry, before);
    carry = win_combine(kind, carry, win_shfl(x, 63));
  }
}
}  // namespace

}  // namespace gpuq
