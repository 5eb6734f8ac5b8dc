// Segments of a key-sorted table and the median of each (MEDIAN aggregate, include/gpuq.h gpuq_segment_heads / gpuq_segment_median).
//
// What it stands in for in the reference: DataFusion 34's MedianAccumulator keeps every value of a group and sorts them when the
// group is evaluated [UPSTREAM-KNOWLEDGE: datafusion physical-expr aggregate/median.rs; the crate is not in the tree].  Here the
// plan executor sorts the whole input once by (keys..., argument) with the radix sort and these kernels do what is left:
//   * heads: row i starts a segment when i = 0 or any key column differs from row i - 1 (validity first, NULL equals NULL, then the
//     value's bytes) -- n x key bytes + 4 B written; an exclusive scan of the flags numbers the segments;
//   * starts: the head positions scattered by segment number, starts[G] = n;
//   * pick: one lane per segment; the argument's NULLs sort last, so the count of values is a binary search over the validity
//     bits of the segment, the middles are one or two loads: O(G log(n / G)) loads in all.
// None of this is bound by anything but the sort in front of it; nothing here is specialised at run time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpuq_kernels.h"

namespace gpuq {

namespace {
constexpr int SEG_BLOCK = 256;
inline unsigned seg_grid(i64 n) { return (unsigned)((n + SEG_BLOCK - 1) / SEG_BLOCK); }      // one lane per item, n < 2^31

__device__ __forceinline__ bool seg_bit(const uint8_t* __restrict__ bits, i64 i) { return (bits[i >> 3] >> (i & 7)) & 1; }

// does key column k differ between rows i and i - 1?
__device__ __forceinline__ bool seg_key_differs(const SegKeys& K, int k, i64 i) {
  const uint8_t* v = K.valid[k];
  if (v) {
    const bool a = seg_bit(v, i), b = seg_bit(v, i - 1);
    if (a != b) return true;
    if (!a) return false;      // NULL equals NULL, whatever bytes lie under it
  }
  const void* d = K.data[k];
  switch (K.width[k]) {
    case 0: return seg_bit((const uint8_t*)d, i) != seg_bit((const uint8_t*)d, i - 1);      // Boolean: a bitmap
    case 1: return ((const uint8_t*)d)[i] != ((const uint8_t*)d)[i - 1];
    case 2: return ((const uint16_t*)d)[i] != ((const uint16_t*)d)[i - 1];
    case 4: return ((const uint32_t*)d)[i] != ((const uint32_t*)d)[i - 1];
    case 8: return ((const u64*)d)[i] != ((const u64*)d)[i - 1];
    default: {
      const u64* p = (const u64*)d + 2 * i;
      return p[0] != p[-2] || p[1] != p[-1];
    }
  }
}

__global__ void __launch_bounds__(SEG_BLOCK) k_segment_heads(const SegKeys K, const i64 n, int32_t* __restrict__ flags) {
  const i64 i = (i64)blockIdx.x * SEG_BLOCK + threadIdx.x;
  if (i >= n) return;
  bool head = i == 0;
  for (int k = 0; k < K.n_keys && !head; ++k) head = seg_key_differs(K, k, i);
  flags[i] = head ? 1 : 0;
}

// excl[0..n]: the exclusive scan of the flags.  Row i is a head exactly when excl[i + 1] != excl[i]; its segment is excl[i + 1] - 1.
__global__ void __launch_bounds__(SEG_BLOCK) k_segment_starts(const int32_t* __restrict__ excl, const i64 n, int32_t* __restrict__ seg_id, int32_t* __restrict__ starts,
                                                              const i64 starts_cap, u64* __restrict__ n_groups) {
  const i64 i = (i64)blockIdx.x * SEG_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int32_t e0 = excl[i], e1 = excl[i + 1];
  if (seg_id) seg_id[i] = e1 - 1;
  if (e1 != e0 && (i64)e0 < starts_cap) starts[e0] = (int32_t)i;
  if (i == 0) {
    const int32_t g = excl[n];
    if ((i64)g <= starts_cap) starts[g] = (int32_t)n;
    *n_groups = (u64)g;
  }
}
__global__ void k_segment_none(int32_t* __restrict__ starts, u64* __restrict__ n_groups) { starts[0] = 0; *n_groups = 0; }

// (lo + hi) / 2 as Rust computes it on the column's own type: the sum wraps at the declared width, the division truncates toward zero
template <class U, class S> __device__ __forceinline__ U seg_mid_int(U a, U b, bool is_signed) {
  const U sum = (U)(a + b);
  return is_signed ? (U)((S)sum / 2) : (U)(sum / 2);
}

__global__ void __launch_bounds__(SEG_BLOCK) k_segment_median(const void* __restrict__ data, const uint8_t* __restrict__ valid, const int width, const int kind,
                                                              const int32_t* __restrict__ starts, const i64 n_groups, void* __restrict__ out, u64* __restrict__ out_valid) {
  const i64 s = (i64)blockIdx.x * SEG_BLOCK + threadIdx.x;
  bool has = false;
  if (s < n_groups) {
    const i64 lo = starts[s], hi = starts[s + 1];
    i64 a = lo, b = hi;      // the first NULL of the segment: the validity bits are monotone inside it (NULLs sort last)
    if (valid) { while (a < b) { const i64 m = a + (b - a) / 2; if (seg_bit(valid, m)) a = m + 1; else b = m; } }
    else a = hi;
    const i64 v = a - lo;
    has = v > 0;
    const i64 i1 = lo + v / 2, i0 = (v & 1) ? i1 : i1 - 1;      // odd: the one middle, twice
    const bool even = has && !(v & 1);
    switch (width) {
      case 1: { const uint8_t* p = (const uint8_t*)data; ((uint8_t*)out)[s] = !has ? 0 : !even ? p[i1] : seg_mid_int<uint8_t, int8_t>(p[i0], p[i1], kind == SEG_SINT); break; }
      case 2: { const uint16_t* p = (const uint16_t*)data; ((uint16_t*)out)[s] = !has ? 0 : !even ? p[i1] : seg_mid_int<uint16_t, int16_t>(p[i0], p[i1], kind == SEG_SINT); break; }
      case 4: {
        const uint32_t* p = (const uint32_t*)data; uint32_t r = 0;
        if (has && !even) r = p[i1];
        else if (even && kind == SEG_F32) { const float m = (__uint_as_float(p[i0]) + __uint_as_float(p[i1])) / 2.0f; r = __float_as_uint(m); }
        else if (even) r = seg_mid_int<uint32_t, int32_t>(p[i0], p[i1], kind == SEG_SINT);
        ((uint32_t*)out)[s] = r; break;
      }
      case 8: {
        const u64* p = (const u64*)data; u64 r = 0;
        if (has && !even) r = p[i1];
        else if (even && kind == SEG_F64) { const double m = (__longlong_as_double((i64)p[i0]) + __longlong_as_double((i64)p[i1])) / 2.0; r = (u64)__double_as_longlong(m); }
        else if (even) r = seg_mid_int<u64, i64>(p[i0], p[i1], kind == SEG_SINT);
        ((u64*)out)[s] = r; break;
      }
      default: {      // Decimal128: a signed 128-bit integer as (lo, hi) words
        const u64* p = (const u64*)data; u64 rl = 0, rh = 0;
        if (has && !even) { rl = p[2 * i1]; rh = p[2 * i1 + 1]; }
        else if (even) {
          const u64 al = p[2 * i0], ah = p[2 * i0 + 1], bl = p[2 * i1], bh = p[2 * i1 + 1];
          u64 sl = al + bl, sh = ah + bh + (sl < al ? 1 : 0);      // wraps at 128 bits
          const u64 neg = sh >> 63;                                 // truncation toward zero: a negative sum is rounded up before the shift
          const u64 tl = sl + neg; sh += (tl < sl ? 1 : 0); sl = tl;
          rl = (sl >> 1) | (sh << 63); rh = (u64)((i64)sh >> 1);
        }
        ((u64*)out)[2 * s] = rl; ((u64*)out)[2 * s + 1] = rh; break;
      }
    }
  }
  // 64 consecutive segments are one wave: their validity bits are one word, written whole by one lane
  const u64 word = __ballot(has);
  if (lane() == 0 && s < n_groups) out_valid[s >> 6] = word;
}
}  // namespace

void launch_segment_heads(hipStream_t s, const SegKeys& K, i64 n, int32_t* scan /* n + 1 */, void* scan_ws, size_t scan_ws_bytes, int32_t* seg_id, int32_t* starts, i64 starts_cap,
                          u64* n_groups) {
  if (n <= 0) { hipLaunchKernelGGL(k_segment_none, dim3(1), dim3(1), 0, s, starts, n_groups); return; }
  hipLaunchKernelGGL(k_segment_heads, dim3(seg_grid(n)), dim3(SEG_BLOCK), 0, s, K, n, scan);
  launch_exclusive_scan_i32(s, scan, n, scan_ws, scan_ws_bytes);
  hipLaunchKernelGGL(k_segment_starts, dim3(seg_grid(n)), dim3(SEG_BLOCK), 0, s, (const int32_t*)scan, n, seg_id, starts, starts_cap, n_groups);
}

void launch_segment_median(hipStream_t s, const void* data, const uint8_t* valid, int width, int kind, const int32_t* starts, i64 n_groups, void* out, u64* out_valid) {
  if (n_groups > 0) hipLaunchKernelGGL(k_segment_median, dim3(seg_grid(n_groups)), dim3(SEG_BLOCK), 0, s, data, valid, width, kind, starts, n_groups, out, out_valid);
}

}  // namespace gpuq
