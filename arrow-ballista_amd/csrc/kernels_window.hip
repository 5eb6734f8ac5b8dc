// Window functions over a table ordered by (partition keys, order keys): BoundedWindowAggExec (include/gpuq.h, gpuq_window_*).
//
// What it stands in for in the reference: DataFusion 34's BoundedWindowAggExec, which walks each partition row by row through a
// PartitionEvaluator / a retractable accumulator [UPSTREAM-KNOWLEDGE: datafusion physical-plan windows/bounded_window_agg_exec.rs; the
// crate is not in the tree].  Here the plan executor finds the partitions and the peer groups with gpuq_segment_heads and these kernels
// do what is left:
//   * scan: a segmented inclusive scan of one accumulator (window_scan_op.h has the element and the operator; gpuq_kernels.h what an
//     accumulator is).  The three launches of launch_exclusive_scan_i32: per-tile totals, one block over the tile totals, a downsweep
//     that starts from the tile's carry.  Tiles of 2,048 rows on 256 threads, eight consecutive rows a thread.  No block waits on
//     another one; the price is a second read of the input.  The order of combination depends on nothing but n, so a Float64 running
//     sum is the same bits run after run.
//   * rank, shift (LAG / LEAD), frame (RANGE peers, sliding ROWS, AVG, narrowing): one row a lane, from the segment ids and starts.
// Nothing here is specialised at run time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "window_scan_dev.h"

namespace gpuq {

namespace {
inline unsigned win_grid(i64 n) { return (unsigned)((n + WIN_BLOCK - 1) / WIN_BLOCK); }      // one lane per row, n < 2^31

// the rows [r0, r0 + WIN_PER) of one thread as elements; rows at and beyond n are identities
struct WinRows { u64 lo[WIN_PER], hi[WIN_PER]; uint32_t valid, heads; };
__device__ __forceinline__ void win_load_rows(const WinCol& c, const int32_t* __restrict__ seg_id, const i64 n, const i64 r0, WinRows& R) {
  R.valid = 0; R.heads = 0;
  uint32_t vbyte = 0xFFu;
  if (c.valid && r0 < n) vbyte = c.valid[r0 >> 3];      // r0 is a multiple of 8
  int32_t prev = (seg_id && r0 > 0 && r0 < n) ? seg_id[r0 - 1] : 0;
#pragma unroll
  for (int k = 0; k < WIN_PER; ++k) {
    const i64 i = r0 + k;
    R.lo[k] = 0; R.hi[k] = 0;
    if (i >= n) continue;
    const int32_t sid = seg_id ? seg_id[i] : 0;
    if (i == 0 || sid != prev) R.heads |= 1u << k;
    prev = sid;
    if ((vbyte >> k) & 1u) { R.valid |= 1u << k; win_load(c, i, R.lo[k], R.hi[k]); }
  }
}
__device__ __forceinline__ WinElem win_row_of(const int kind, const WinRows& R, const int k) {
  return win_row(kind, (R.heads >> k) & 1u, (R.valid >> k) & 1u, R.lo[k], R.hi[k]);
}

// launch 1: the total of every tile; MIN / MAX operands outside int64 are reported here (every row passes once)
__global__ void __launch_bounds__(WIN_BLOCK) k_window_tile_totals(const WinCol c, const int32_t* __restrict__ seg_id, const i64 n, const int kind, WinElem* __restrict__ tiles,
                                                                  uint32_t* __restrict__ flags) {
  __shared__ WinElem wtot[WIN_WAVES];
  const i64 r0 = (i64)blockIdx.x * WIN_TILE + (i64)threadIdx.x * WIN_PER;
  WinRows R; win_load_rows(c, seg_id, n, r0, R);
  WinElem loc = win_identity(kind);
  bool wide = false;
#pragma unroll
  for (int k = 0; k < WIN_PER; ++k) {
    loc = win_combine(kind, loc, win_row_of(kind, R, k));
    wide = wide || (((R.valid >> k) & 1u) && acc_wide_minmax(kind, R.lo[k], R.hi[k]));
  }
  if (wide && flags) atomicOr(flags, WINF_WIDE_MINMAX);
  WinElem total;
  (void)win_block_excl_scan(kind, loc, wtot, &total);
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}


// launch 2 is k_window_tiles_scan (window_scan_dev.h)
// launch 3: every row's running element = the tile's carry, the threads before it, its own rows up to and including it
__global__ void __launch_bounds__(WIN_BLOCK) k_window_downsweep(const WinCol c, const int32_t* __restrict__ seg_id, const i64 n, const int kind, const WinElem* __restrict__ tiles,
                                                                void* __restrict__ out_cells, const int cell_width, i64* __restrict__ out_count, u64* __restrict__ out_valid) {
  __shared__ WinElem wtot[WIN_WAVES];
  const i64 r0 = (i64)blockIdx.x * WIN_TILE + (i64)threadIdx.x * WIN_PER;
  WinRows R; win_load_rows(c, seg_id, n, r0, R);
  WinElem loc = win_identity(kind);
#pragma unroll
  for (int k = 0; k < WIN_PER; ++k) loc = win_combine(kind, loc, win_row_of(kind, R, k));
  WinElem total;
  const WinElem excl = win_block_excl_scan(kind, loc, wtot, &total);
  WinElem run = win_combine(kind, tiles[blockIdx.x], excl);
  uint32_t vbits = 0;
#pragma unroll
  for (int k = 0; k < WIN_PER; ++k) {
    const i64 i = r0 + k;
    run = win_combine(kind, run, win_row_of(kind, R, k));
    if (i >= n) continue;
    if (cell_width == 16) { ((u64*)out_cells)[2 * i] = run.lo; ((u64*)out_cells)[2 * i + 1] = run.hi; }
    else ((u64*)out_cells)[i] = run.lo;
    if (out_count) out_count[i] = run.count;
    if (run.count > 0) vbits |= 1u << k;
  }
  // eight threads hold the eight bytes of one validity word (r0 of the first is a multiple of 64): written whole, by that one
  if (out_valid) {
    u64 word = (u64)vbits << (8 * (lane() & 7));
    word |= __shfl_xor(word, 1); word |= __shfl_xor(word, 2); word |= __shfl_xor(word, 4);
    if ((lane() & 7) == 0 && r0 < n) out_valid[r0 >> 6] = word;
  }
}

__global__ void __launch_bounds__(WIN_BLOCK) k_window_rank(const int32_t* __restrict__ part_id, const int32_t* __restrict__ part_starts, const int32_t* __restrict__ peer_id,
                                                           const int32_t* __restrict__ peer_starts, const i64 n, u64* __restrict__ row_number, u64* __restrict__ rank,
                                                           u64* __restrict__ dense_rank) {
  const i64 i = (i64)blockIdx.x * WIN_BLOCK + threadIdx.x;
  if (i >= n) return;
  const i64 s = part_starts[part_id[i]];
  if (row_number) row_number[i] = (u64)(i - s + 1);
  const int32_t p = peer_id[i];
  if (rank) rank[i] = (u64)((i64)peer_starts[p] - s + 1);
  if (dense_rank) dense_rank[i] = (u64)((i64)p - (i64)peer_id[s] + 1);
}

__global__ void __launch_bounds__(WIN_BLOCK) k_window_shift(const void* __restrict__ data, const uint8_t* __restrict__ valid, const int width, const int32_t* __restrict__ part_id,
                                                            const int32_t* __restrict__ part_starts, const i64 n, const i64 delta, const void* __restrict__ dflt,
                                                            const uint8_t* __restrict__ dflt_valid, const int dflt_is_null, void* __restrict__ out, u64* __restrict__ out_valid) {
  const i64 i = (i64)blockIdx.x * WIN_BLOCK + threadIdx.x;
  bool has = false;
  if (i < n) {
    const int32_t p = part_id[i];
    const i64 j = i + delta;
    const bool in = j >= (i64)part_starts[p] && j < (i64)part_starts[p + 1];
    const void* src = in ? data : dflt;
    const i64 r = in ? j : i;
    has = in ? (valid ? win_bit(valid, j) : true) : (!dflt_is_null && (dflt_valid ? win_bit(dflt_valid, i) : true));
    const bool take = has && src;
    switch (width) {
      case 1: ((uint8_t*)out)[i] = take ? ((const uint8_t*)src)[r] : (uint8_t)0; break;
      case 2: ((uint16_t*)out)[i] = take ? ((const uint16_t*)src)[r] : (uint16_t)0; break;
      case 4: ((uint32_t*)out)[i] = take ? ((const uint32_t*)src)[r] : 0u; break;
      case 8: ((u64*)out)[i] = take ? ((const u64*)src)[r] : 0ull; break;
      default: ((u64*)out)[2 * i] = take ? ((const u64*)src)[2 * r] : 0ull; ((u64*)out)[2 * i + 1] = take ? ((const u64*)src)[2 * r + 1] : 0ull; break;
    }
  }
  const u64 word = __ballot(has);
  if (lane() == 0 && i < n) out_valid[i >> 6] = word;
}

__device__ __forceinline__ void win_cell_at(const WinFrame& F, const i64 r, u64& lo, u64& hi) {
  if (F.cell_width == 16) { lo = ((const u64*)F.cells)[2 * r]; hi = ((const u64*)F.cells)[2 * r + 1]; }
  else { lo = ((const u64*)F.cells)[r]; hi = 0; }
}

__global__ void __launch_bounds__(WIN_BLOCK) k_window_frame(const WinFrame F, const i64 n) {
  const i64 i = (i64)blockIdx.x * WIN_BLOCK + threadIdx.x;
  bool has = false;
  if (i < n) {
    const int32_t p = F.part_id[i];
    const i64 ps = F.part_starts[p], pe = F.part_starts[p + 1];
    i64 hi_row = i, lo_row = ps;
    if (F.mode == WFRAME_RANGE) hi_row = (i64)F.peer_starts[F.peer_id[i] + 1] - 1;
    else if (F.mode == WFRAME_SLIDING) {
      hi_row = F.following >= pe - 1 - i ? pe - 1 : i + F.following;
      lo_row = (F.preceding < 0 || F.preceding >= i - ps) ? ps : i - F.preceding;
    }
    u64 vlo, vhi; win_cell_at(F, hi_row, vlo, vhi);
    i64 cnt = F.counts ? F.counts[hi_row] : 1;
    if (lo_row > ps) {      // a difference of two running values: exact in wrapping arithmetic
      u64 blo, bhi; win_cell_at(F, lo_row - 1, blo, bhi);
      const u64 d = vlo - blo; vhi = vhi - bhi - (vlo < blo ? 1 : 0); vlo = d;
      if (F.counts) cnt -= F.counts[lo_row - 1];
    }
    has = cnt > 0;
    switch (F.out_kind) {
      case WOUT_CELL: {
        if (!has) { vlo = 0; vhi = 0; }
        else if (F.cell_width != 16) vhi = (u64)((i64)vlo >> 63);      // (an 8-byte cell stored 16 wide is a Decimal128 MIN / MAX: sign-extended, as acc_result_hi has it)
        switch (F.out_width) {
          case 1: ((uint8_t*)F.out)[i] = (uint8_t)vlo; break;
          case 2: ((uint16_t*)F.out)[i] = (uint16_t)vlo; break;
          case 4: ((uint32_t*)F.out)[i] = F.out_f32 ? __float_as_uint((float)__longlong_as_double((i64)vlo)) : (uint32_t)vlo; break;
          case 8: ((u64*)F.out)[i] = vlo; break;
          default: ((u64*)F.out)[2 * i] = vlo; ((u64*)F.out)[2 * i + 1] = vhi; break;
        }
        break;
      }
      case WOUT_AVG_INT: ((double*)F.out)[i] = has ? i128_to_f64(mk128(vlo, vhi)) / (double)cnt : 0.0; break;
      case WOUT_AVG_F64: ((double*)F.out)[i] = has ? __longlong_as_double((i64)vlo) / (double)cnt : 0.0; break;
      default: {      // WOUT_AVG_DEC: sum * 10^d / count, truncating, as the aggregate operator's result projection computes it
        i128 q = 0, r = 0;
        if (has) divmod128((i128)((u128)mk128(vlo, vhi) * (u128)mk128(F.mul_lo, F.mul_hi)), (i128)cnt, q, r);
        ((u64*)F.out)[2 * i] = (u64)q; ((u64*)F.out)[2 * i + 1] = (u64)((u128)q >> 64);
        break;
      }
    }
  }
  const u64 word = __ballot(has);
  if (F.out_valid && lane() == 0 && i < n) F.out_valid[i >> 6] = word;
}
}  // namespace

size_t window_scan_ws_bytes(i64 n) { return (size_t)((n + WIN_TILE - 1) / WIN_TILE + 1) * sizeof(WinElem); }
void launch_window_scan(hipStream_t s, const WinCol& c, const int32_t* seg_id, i64 n, int kind, void* ws, void* out_cells, int cell_width, i64* out_count, u64* out_valid,
                        uint32_t* flags) {
  if (n <= 0) return;
  const i64 ntiles = (n + WIN_TILE - 1) / WIN_TILE;
  WinElem* tiles = (WinElem*)ws;
  hipLaunchKernelGGL(k_window_tile_totals, dim3((unsigned)ntiles), dim3(WIN_BLOCK), 0, s, c, seg_id, n, kind, tiles, flags);
  hipLaunchKernelGGL(k_window_tiles_scan, dim3(1), dim3(1024), 0, s, tiles, ntiles, kind);
  hipLaunchKernelGGL(k_window_downsweep, dim3((unsigned)ntiles), dim3(WIN_BLOCK), 0, s, c, seg_id, n, kind, (const WinElem*)tiles, out_cells, cell_width, out_count, out_valid);
}
void launch_window_rank(hipStream_t s, const int32_t* part_id, const int32_t* part_starts, const int32_t* peer_id, const int32_t* peer_starts, i64 n, u64* row_number, u64* rank,
                        u64* dense_rank) {
  if (n > 0) hipLaunchKernelGGL(k_window_rank, dim3(win_grid(n)), dim3(WIN_BLOCK), 0, s, part_id, part_starts, peer_id, peer_starts, n, row_number, rank, dense_rank);
}
void launch_window_shift(hipStream_t s, const void* data, const uint8_t* valid, int width, const int32_t* part_id, const int32_t* part_starts, i64 n, i64 delta, const void* dflt,
                         const uint8_t* dflt_valid, int dflt_is_null, void* out, u64* out_valid) {
  if (n > 0) hipLaunchKernelGGL(k_window_shift, dim3(win_grid(n)), dim3(WIN_BLOCK), 0, s, data, valid, width, part_id, part_starts, n, delta, dflt, dflt_valid, dflt_is_null, out, out_valid);
}
void launch_window_frame(hipStream_t s, const WinFrame& F, i64 n) {
  if (n > 0) hipLaunchKernelGGL(k_window_frame, dim3(win_grid(n)), dim3(WIN_BLOCK), 0, s, F, n);
}

}  // namespace gpuq
