// The row rule of the grouping-set expansion (csrc/grouping_expand_op.h: gexp_row / gexp_set / gexp_masked / gexp_valid / gexp_bool and
// the word a wave writes, gexp_word) folded on the host.  The header's functions are the code under test; the kernel of
// csrc/kernels_grouping.hip calls the same ones, one lane per output row, and stores what a ballot gives.  tests/test_cpu_grouping_sets.py
// builds and drives it.
//   stdin:  "n n_sets null_sets has_validity", then n rows "valid bit" (bit: the row's value in a Boolean column)
//   stdout: line 1: for every output row the input row it copies, or -1 where it is NULL
//           line 2: the validity bitmap's 64-bit words, (n * n_sets + 63) / 64 of them
//           line 3: the data words of the column taken as a Boolean one
#include <cstdint>
#include <cstdio>
#include <vector>

#include "grouping_expand_op.h"

using namespace gpuq;

int main() {
  long long n = 0; int n_sets = 0, has_validity = 0; unsigned long long null_sets = 0;
  if (std::scanf("%lld %d %llu %d", &n, &n_sets, &null_sets, &has_validity) != 4 || n < 0 || n_sets < 1 || n_sets > 64) return 2;
  // the bitmaps as the column holds them: exactly the bytes n rows need, so that a read beyond row n - 1 is a read beyond the buffer
  std::vector<uint8_t> valid((size_t)(n + 7) / 8, 0), bits((size_t)(n + 7) / 8, 0);
  for (long long i = 0; i < n; ++i) {
    int v = 0, b = 0;
    if (std::scanf("%d %d", &v, &b) != 2) return 2;
    if (v) valid[(size_t)(i >> 3)] |= (uint8_t)(1u << (i & 7));
    if (b) bits[(size_t)(i >> 3)] |= (uint8_t)(1u << (i & 7));
  }
  const uint8_t* vp = has_validity ? valid.data() : nullptr;
  const int64_t total = (int64_t)n * n_sets;
  for (int64_t o = 0; o < total; ++o) {
    const bool has = gexp_valid(o, n_sets, (uint64_t)null_sets, vp);
    if (gexp_masked((uint64_t)null_sets, gexp_set(o, n_sets)) && has) return 3;
    std::printf("%lld ", has ? (long long)gexp_row(o, n_sets) : -1ll);
  }
  std::printf("\n");
  const int64_t words = (total + 63) / 64;
  for (int64_t w = 0; w < words; ++w) std::printf("%llu ", (unsigned long long)gexp_word(w, total, [&](int64_t o) { return gexp_valid(o, n_sets, (uint64_t)null_sets, vp); }));
  std::printf("\n");
  for (int64_t w = 0; w < words; ++w)
    std::printf("%llu ", (unsigned long long)gexp_word(w, total, [&](int64_t o) { return gexp_bool(o, n_sets, (uint64_t)null_sets, vp, bits.data()); }));
  std::printf("\n");
  return 0;
}
