// The HyperLogLog of APPROX_DISTINCT (include/gpuq.h, gpuq_segment_approx_distinct): the hash, a value's register and rank, and the
// estimator -- stated once for the device (kernels_hll.hip), for a host build and as the text tests/hll_sketch.py restates.
//
// DataFusion's sketch: precision p = 14, m = 16384 one-byte registers, q = 50 [UPSTREAM-KNOWLEDGE: physical-expr
// aggregate/hyperloglog.rs; the crate is not in the tree].  Its ahash is CPU-feature dependent, so the hash is gpuq's own (the value
// half of hash_combine, gpuq_dev.h).  The estimator is Ertl's improved one over the histogram C[0..51] of the register values; all of
// it is Float64 with contraction off and nothing in it is transcendental beyond a constant, so every build gives the same bits.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPUQ_HLL_HD __host__ __device__
#else
#define GPUQ_HLL_HD
#endif

namespace gpuq {

constexpr int HLL_P = 14, HLL_M = 1 << HLL_P, HLL_Q = 64 - HLL_P, HLL_BINS = HLL_Q + 2;      // register values 0..51

GPUQ_HLL_HD inline uint64_t hll_mix64(uint64_t x) {      // splitmix64's finaliser: mix64 of gpuq_dev.h
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31; return x;
}
GPUQ_HLL_HD inline uint64_t hll_hash(uint64_t lo, uint64_t hi) { return hll_mix64(lo ^ hll_mix64(hi + 0x632BE59BD9B4E019ull)); }
GPUQ_HLL_HD inline uint32_t hll_index(uint64_t h) { return (uint32_t)(h & (uint64_t)(HLL_M - 1)); }
GPUQ_HLL_HD inline uint32_t hll_rho(uint64_t h) {      // 1..51
  return (uint32_t)__builtin_ctzll((h >> HLL_P) | (1ull << HLL_Q)) + 1;
}

GPUQ_HLL_HD inline double hll_sigma(double x) {
#pragma clang fp contract(off)
  if (x == 1.0) return INFINITY;
  double y = 1.0, z = x, prev;
  do { x *= x; prev = z; z += x * y; y += y; } while (z != prev);
  return z;
}
GPUQ_HLL_HD inline double hll_tau(double x) {
#pragma clang fp contract(off)
  if (x == 0.0 || x == 1.0) return 0.0;
  double y = 1.0, z = 1.0 - x, prev;
  do { x = sqrt(x); prev = z; y *= 0.5; z -= (1.0 - x) * (1.0 - x) * y; } while (z != prev);
  return z / 3.0;
}
// C[k]: how many of the m registers hold k.  0.5 / ln 2 = 0.72134752044448170...
GPUQ_HLL_HD inline uint64_t hll_estimate(const uint32_t* C) {
#pragma clang fp contract(off)
  const double m = (double)HLL_M;
  double z = m * hll_tau((m - (double)C[HLL_Q + 1]) / m);
  for (int k = HLL_Q; k >= 1; --k) z = 0.5 * (z + (double)C[k]);
  z += m * hll_sigma((double)C[0] / m);
  if (!(z < INFINITY)) return 0;      // every register 0
  const double e = floor(0.7213475204444817 * m * m / z + 0.5);
  return e >= 18446744073709551616.0 ? UINT64_MAX : (uint64_t)e;      // (z = 0, every register at q + 1: the conversion saturates, as Rust's does)
}

}  // namespace gpuq
