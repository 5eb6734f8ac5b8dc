// Grouping sets (GROUP BY ROLLUP / CUBE / GROUPING SETS): the expansion of a Partial aggregate's output, one copy of every row per set
// (include/gpuq.h, gpuq_grouping_expand).
//
// What it stands in for in the reference: DataFusion 34's AggregateExec evaluates the group expressions once per grouping set over every
// input batch and feeds all key tuples to one table [UPSTREAM-KNOWLEDGE: datafusion physical-plan aggregates/mod.rs evaluate_group_by; the
// crate is not in the tree].  Here the input is aggregated once, at the finest grain, and the plan executor makes the sets from that much
// smaller state table (plan_exec.cpp, GroupingExpand): this kernel writes every column S times over, row-interleaved, with the keys a
// set masks as NULLs, and a Final / Merge aggregate groups the result again.
//
// One lane per OUTPUT row; grouping_expand_op.h has the row rule.  Validity (and the data of a Boolean column, a bitmap) is assembled by
// a ballot and stored as whole 64-bit words by one lane of the wave that holds the word's rows: no atomics, no scratch, nothing zeroed
// beforehand.  Nothing here is specialised at run time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpuq_kernels.h"
#include "grouping_expand_op.h"

namespace gpuq {

namespace {
constexpr int GEXP_BLOCK = 256;      // four waves: a block's first row is a multiple of 64, so every wave holds the rows of one word

// width: 1, 2, 4, 8 or 16 bytes a row, or 0 -- a Boolean column, data and out are bitmaps
__global__ void __launch_bounds__(GEXP_BLOCK) k_grouping_expand(const void* __restrict__ data, const uint8_t* __restrict__ valid, const int width, const i64 total, const int n_sets,
                                                                const u64 null_sets, void* __restrict__ out, u64* __restrict__ out_valid) {
  const i64 o = (i64)blockIdx.x * GEXP_BLOCK + threadIdx.x;
  bool has = false, bit = false;
  if (o < total) {
    has = gexp_valid(o, n_sets, null_sets, valid);
    const i64 r = gexp_row(o, n_sets);
    switch (width) {
      case 0: bit = has && gexp_bit((const uint8_t*)data, r); break;
      case 1: ((uint8_t*)out)[o] = has ? ((const uint8_t*)data)[r] : (uint8_t)0; break;
      case 2: ((uint16_t*)out)[o] = has ? ((const uint16_t*)data)[r] : (uint16_t)0; break;
      case 4: ((uint32_t*)out)[o] = has ? ((const uint32_t*)data)[r] : 0u; break;
      case 8: ((u64*)out)[o] = has ? ((const u64*)data)[r] : 0ull; break;
      default: ((u64*)out)[2 * o] = has ? ((const u64*)data)[2 * r] : 0ull; ((u64*)out)[2 * o + 1] = has ? ((const u64*)data)[2 * r + 1] : 0ull; break;
    }
  }
  // lanes at and beyond `total` vote 0: the last word is zero-padded
  const u64 vword = __ballot(has);
  if (width == 0) { const u64 dword = __ballot(bit); if (lane() == 0 && o < total) ((u64*)out)[o >> 6] = dword; }
  if (out_valid && lane() == 0 && o < total) out_valid[o >> 6] = vword;
}
}  // namespace

void launch_grouping_expand(hipStream_t s, const void* data, const uint8_t* valid, int width, i64 n, int n_sets, u64 null_sets, void* out, u64* out_valid) {
  const i64 total = n * n_sets;      // < 2^31: the entry point refuses more
  if (total <= 0) return;
  hipLaunchKernelGGL(k_grouping_expand, dim3((unsigned)((total + GEXP_BLOCK - 1) / GEXP_BLOCK)), dim3(GEXP_BLOCK), 0, s, data, valid, width, total, n_sets, null_sets, out, out_valid);
}

}  // namespace gpuq
