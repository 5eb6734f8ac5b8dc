// DISTINCT aggregates over a column sorted inside its segments: COUNT, SUM and BIT_XOR of every segment's distinct values
// (include/gpuq.h, gpuq_segment_distinct).
//
// What it stands in for in the reference: DataFusion 34's DistinctCount / DistinctSum / DistinctBitXor accumulators keep a hash set of
// ScalarValues per group and fold it when the group is evaluated [UPSTREAM-KNOWLEDGE: datafusion physical-expr aggregate/count_distinct.rs,
// sum_distinct.rs, bit_and_or_xor.rs; the crate is not in the tree].  Here the plan executor has sorted the input by (keys..., argument),
// so the set of a segment is its run heads (distinct_scan_op.h), and reducing them is the segmented scan of the window functions
// (window_scan_dev.h) with another row rule and another store:
//   * tile totals: a row is a scan element that restarts at a segment's first row and carries its value only when it is a run head.  The
//     test reads the row before it -- from a register, or from global memory for a thread's first row, a tile's first row included;
//   * the one-block scan of the tile totals (k_window_tiles_scan, as it is);
//   * a downsweep that stores one element per segment, at the segment's last row.
// Which segment a row lies in comes from `starts` alone: one binary search for a thread's first row, a step for each boundary after it.
// Tiles of 2,048 rows on 256 threads; one segment over all rows is spread over the device like any other input, no lane walks a
// segment, no block waits on another one, and nothing is combined by an atomic: the order of combination depends on n and the starts
// only, so a Float64 SUM is the same bits run after run.  An empty segment is met by no row: the caller zeroes the outputs first.
// Nothing here is specialised at run time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "distinct_scan_op.h"
#include "window_scan_dev.h"

namespace gpuq {

namespace {
// the last segment s of [0, G) with starts[s] <= i: of several that begin at one row, the one that holds it (the others are empty)
__device__ __forceinline__ i64 dst_segment_of(const int32_t* __restrict__ starts, const i64 G, const i64 i) {
  i64 a = 0, b = G - 1;
  while (a < b) { const i64 m = a + (b - a + 1) / 2; if ((i64)starts[m] <= i) a = m; else b = m - 1; }
  return a;
}

// the rows [r0, r0 + WIN_PER) of one thread: the operand of every run head, (take) the run heads, (heads) the segments' first rows,
// (last) their last rows, and the segment of every row; rows at and beyond n, or outside [starts[0], starts[G]), are nothing
struct DstRows { u64 lo[WIN_PER], hi[WIN_PER]; int32_t seg[WIN_PER]; uint32_t take, heads, last; };
__device__ __forceinline__ void dst_load_rows(const WinCol& c, const int32_t* __restrict__ starts, const i64 G, const i64 n, const i64 r0, DstRows& R) {
  R.take = 0; R.heads = 0; R.last = 0;
#pragma unroll
  for (int k = 0; k < WIN_PER; ++k) { R.lo[k] = 0; R.hi[k] = 0; R.seg[k] = 0; }
  if (r0 >= n) return;
  const uint32_t vbyte = c.valid ? c.valid[r0 >> 3] : 0xFFu;      // r0 is a multiple of 8
  i64 s = dst_segment_of(starts, G, r0);
  i64 beg = starts[s], end = starts[s + 1];
  u64 plo = 0, phi = 0;
  if (r0 > 0 && r0 > beg && r0 < end) win_raw(c, r0 - 1, plo, phi);      // the row before this thread's first, in its segment: from global memory
#pragma unroll
  for (int k = 0; k < WIN_PER; ++k) {
    const i64 i = r0 + k;
    if (i >= n) continue;
    if (i >= end) {      // the next segment that is not empty: usually the one that follows
      s = (s + 2 <= G && (i64)starts[s + 1] <= i && (i64)starts[s + 2] > i) ? s + 1 : dst_segment_of(starts, G, i);
      beg = starts[s]; end = starts[s + 1];
    }
    const bool inside = i >= beg && i < end, valid = inside && ((vbyte >> k) & 1u);
    u64 lo = 0, hi = 0;
    if (valid) win_raw(c, i, lo, hi);
    const bool same = lo == plo && hi == phi;
    plo = lo; phi = hi;
    R.seg[k] = (int32_t)s;
    if (inside && i == beg) R.heads |= 1u << k;
    if (inside && i + 1 == end) R.last |= 1u << k;
    if (distinct_run_head(valid, i == beg, same)) { R.take |= 1u << k; win_widen(c, lo, hi); R.lo[k] = lo; R.hi[k] = hi; }
  }
}
__device__ __forceinline__ WinElem dst_row_of(const int kind, const DstRows& R, const int k) {
  const bool take = (R.take >> k) & 1u;      // (a run head: valid, and the two other arguments no longer matter)
  return distinct_row(kind, (R.heads >> k) & 1u, take, !take, R.lo[k], R.hi[k]);
}

// launch 1: the total of every tile
__global__ void __launch_bounds__(WIN_BLOCK) k_distinct_tile_totals(const WinCol c, const int32_t* __restrict__ starts, const i64 G, const i64 n, const int kind,
                                                                    WinElem* __restrict__ tiles) {
  __shared__ WinElem wtot[WIN_WAVES];
  const i64 r0 = (i64)blockIdx.x * WIN_TILE + (i64)threadIdx.x * WIN_PER;
  DstRows R; dst_load_rows(c, starts, G, n, r0, R);
  WinElem loc = win_identity(kind);
#pragma unroll
  for (int k = 0; k < WIN_PER; ++k) loc = win_combine(kind, loc, dst_row_of(kind, R, k));
  WinElem total;
  (void)win_block_excl_scan(kind, loc, wtot, &total);
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

// launch 3: the running element at every segment's last row is the segment's: stored there, by the thread that holds the row
__global__ void __launch_bounds__(WIN_BLOCK) k_distinct_downsweep(const WinCol c, const int32_t* __restrict__ starts, const i64 G, const i64 n, const int kind,
                                                                  const WinElem* __restrict__ tiles, void* __restrict__ out_cells, const int cell_width, i64* __restrict__ out_count) {
  __shared__ WinElem wtot[WIN_WAVES];
  const i64 r0 = (i64)blockIdx.x * WIN_TILE + (i64)threadIdx.x * WIN_PER;
  DstRows R; dst_load_rows(c, starts, G, n, r0, R);
  WinElem loc = win_identity(kind);
#pragma unroll
  for (int k = 0; k < WIN_PER; ++k) loc = win_combine(kind, loc, dst_row_of(kind, R, k));
  WinElem total;
  const WinElem excl = win_block_excl_scan(kind, loc, wtot, &total);
  WinElem run = win_combine(kind, tiles[blockIdx.x], excl);
#pragma unroll
  for (int k = 0; k < WIN_PER; ++k) {
    run = win_combine(kind, run, dst_row_of(kind, R, k));
    if (!((R.last >> k) & 1u)) continue;
    const i64 s = R.seg[k];
    if (out_count) out_count[s] = run.count;
    if (!out_cells) continue;
    const u64 lo = run.count > 0 ? run.lo : 0ull, hi = run.count > 0 ? run.hi : 0ull;
    switch (cell_width) {
      case 1: ((uint8_t*)out_cells)[s] = (uint8_t)lo; break;
      case 2: ((uint16_t*)out_cells)[s] = (uint16_t)lo; break;
      case 4: ((uint32_t*)out_cells)[s] = (uint32_t)lo; break;
      case 8: ((u64*)out_cells)[s] = lo; break;
      default: ((u64*)out_cells)[2 * s] = lo; ((u64*)out_cells)[2 * s + 1] = hi; break;
    }
  }
}

// 64 consecutive segments are one wave: their validity bits (count > 0) are one word, written whole by one lane
__global__ void __launch_bounds__(WIN_BLOCK) k_distinct_valid(const i64* __restrict__ count, const i64 G, u64* __restrict__ out_valid) {
  const i64 s = (i64)blockIdx.x * WIN_BLOCK + threadIdx.x;
  const u64 word = __ballot(s < G && count[s] > 0);
  if (lane() == 0 && s < G) out_valid[s >> 6] = word;
}
}  // namespace

void launch_segment_distinct(hipStream_t s, const WinCol& c, const int32_t* starts, i64 n_groups, i64 n, int kind, void* ws, void* out_cells, int cell_width, i64* out_count) {
  if (n <= 0 || n_groups <= 0) return;
  const i64 ntiles = (n + WIN_TILE - 1) / WIN_TILE;
  WinElem* tiles = (WinElem*)ws;
  hipLaunchKernelGGL(k_distinct_tile_totals, dim3((unsigned)ntiles), dim3(WIN_BLOCK), 0, s, c, starts, n_groups, n, kind, tiles);
  hipLaunchKernelGGL(k_window_tiles_scan, dim3(1), dim3(1024), 0, s, tiles, ntiles, kind);
  hipLaunchKernelGGL(k_distinct_downsweep, dim3((unsigned)ntiles), dim3(WIN_BLOCK), 0, s, c, starts, n_groups, n, kind, (const WinElem*)tiles, out_cells, cell_width, out_count);
}
void launch_segment_distinct_valid(hipStream_t s, const i64* count, i64 n_groups, u64* out_valid) {
  if (n_groups > 0) hipLaunchKernelGGL(k_distinct_valid, dim3((unsigned)((n_groups + WIN_BLOCK - 1) / WIN_BLOCK)), dim3(WIN_BLOCK), 0, s, count, n_groups, out_valid);
}

}  // namespace gpuq
