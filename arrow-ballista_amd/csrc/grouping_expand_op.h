// The row rule of the grouping-set expansion (kernels_grouping.hip, gpuq_grouping_expand), as plain functions: the kernel calls them
// lane by lane, tests/grouping_expand_host.cpp folds output rows with them on the host.
//
// A column of n rows is written n_sets times over, row-interleaved: output row o = i * n_sets + s is input row i as grouping set s sees
// it -- NULL when bit s of null_sets is set (the set masks this key), the input row otherwise.  No output position depends on n.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gpuq {

// output row o -> (input row, set)
__host__ __device__ __forceinline__ int64_t gexp_row(const int64_t o, const int n_sets) { return (int64_t)((uint32_t)o / (uint32_t)n_sets); }      // o < 2^31
__host__ __device__ __forceinline__ int gexp_set(const int64_t o, const int n_sets) { return (int)((uint32_t)o % (uint32_t)n_sets); }
__host__ __device__ __forceinline__ bool gexp_masked(const uint64_t null_sets, const int s) { return (null_sets >> s) & 1ull; }
__host__ __device__ __forceinline__ bool gexp_bit(const uint8_t* bits, const int64_t i) { return (bits[i >> 3] >> (i & 7)) & 1; }
// is output row o a value?  Not masked by its set, and valid in the input (validity == nullptr: every input row is)
__host__ __device__ __forceinline__ bool gexp_valid(const int64_t o, const int n_sets, const uint64_t null_sets, const uint8_t* validity) {
  if (gexp_masked(null_sets, gexp_set(o, n_sets))) return false;
  return validity ? gexp_bit(validity, gexp_row(o, n_sets)) : true;
}
// the value bit of output row o of a Boolean column (a bitmap): a NULL row's data is zero
__host__ __device__ __forceinline__ bool gexp_bool(const int64_t o, const int n_sets, const uint64_t null_sets, const uint8_t* validity, const uint8_t* bits) {
  return gexp_valid(o, n_sets, null_sets, validity) && gexp_bit(bits, gexp_row(o, n_sets));
}
// The 64-bit word w of a bitmap over the output rows [0, total): bit l is `pred(64 * w + l)`, rows at and beyond `total` give 0 (the
// last word is zero-padded).  On the device a wave assembles it by one ballot -- lane l holds row 64 * w + l -- and one lane stores it
// whole; this is the same word folded bit by bit.
template <class Pred> __host__ __forceinline__ uint64_t gexp_word(const int64_t w, const int64_t total, Pred&& pred) {
  uint64_t word = 0;
  for (int l = 0; l < 64; ++l) { const int64_t o = 64 * w + l; if (o < total && pred(o)) word |= 1ull << l; }
  return word;
}

}  // namespace gpuq
