// The key encoding of the sort (csrc/sort_key_op.h: sort_view / mm_value / sort_key_layout / sort_pack_key / sort_direct_key) run on the
// host.  The header's functions are the code under test; k_sort_minmax, k_sort_pack and k_sort_direct of csrc/kernels_sort.hip call the
// same row rules lane by lane, and sort_key_plan of csrc/capi.cpp the same layout.  tests/test_cpu_sort_order_exact.py builds and drives it.
//   stdin:  "mode n_keys n stride", then per key "kind desc nulls_first", then n rows of n_keys x "isnull lo hi" (the key register's two
//           words, unsigned: an integer sign-extended to 128 bits, a float its Float64 pattern, a string packed as CC_STR is)
//   mode 1: min / max / flags of all rows (in blocks of 7, folded as the read-back is) -> the layout -> every row packed
//           stdout: "total T", per key "key k vbits null_bit shift rshift len_bits", then -- unless T > 128, which prints "wide" and
//           packs nothing -- per row "bad hi lo": the composite's two words
//   mode 2: per row, per key "rank hi lo": what the one-block sort compares
//   mode 3: as mode 1, but the layout is GUESSED from every stride-th row and the last one, and every row is packed with check = 1
#include <cstdio>
#include <vector>

#include "sort_key_op.h"

using namespace gpuq;

struct Cell { int isn; unsigned long long lo, hi; };

int main() {
  int mode = 0, n_keys = 0; long long n = 0, stride = 1;
  if (std::scanf("%d %d %lld %lld", &mode, &n_keys, &n, &stride) != 4 || mode < 1 || mode > 3 || n_keys < 1 || n_keys > MAX_SORT_KEYS || n < 0 || stride < 1) return 2;
  SortSpec S{}; S.n_keys = n_keys;
  for (int k = 0; k < n_keys; ++k) { S.reg[k] = k; if (std::scanf("%d %d %d", &S.kind[k], &S.desc[k], &S.nulls_first[k]) != 3) return 2; }
  std::vector<Cell> rows((size_t)n * n_keys);
  for (auto& c : rows) if (std::scanf("%d %llu %llu", &c.isn, &c.lo, &c.hi) != 3) return 2;
  auto cell = [&](long long i, int k) -> const Cell& { return rows[(size_t)i * n_keys + k]; };

  if (mode == 2) {
    for (long long i = 0; i < n; ++i) {
      for (int k = 0; k < n_keys; ++k) {
        const Cell& c = cell(i, k); u128 u;
        const uint32_t rank = sort_direct_key(c.lo, c.hi, c.isn != 0, S.kind[k], S.desc[k] != 0, S.nulls_first[k] != 0, u);
        std::printf("%u %llu %llu ", rank, (unsigned long long)(u >> 64), (unsigned long long)u);
      }
      std::printf("\n");
    }
    return 0;
  }

  // the min/max pass: blocks of 7 rows, one {min_lo, min_hi, max_lo, max_hi, flags} per block and key
  const long long BLOCK = 7;
  const int n_blocks = (int)((n + BLOCK - 1) / BLOCK) + 1;      // (+ one block that saw no row)
  std::vector<u64> hmm((size_t)n_blocks * MAX_SORT_KEYS * 5, 0);
  for (int b = 0; b < n_blocks; ++b) {
    for (int k = 0; k < n_keys; ++k) {
      MinMax m; mm_init(m);
      for (long long i = b * BLOCK; i < n && i < (b + 1) * BLOCK; ++i) {
        if (mode == 3 && i % stride != 0 && i != n - 1) continue;
        const Cell& c = cell(i, k);
        mm_value(m, c.lo, c.hi, c.isn != 0, S.kind[k]);
      }
      u64* o = &hmm[((size_t)b * MAX_SORT_KEYS + k) * 5];
      o[0] = m.mn_lo; o[1] = m.mn_hi; o[2] = m.mx_lo; o[3] = m.mx_hi; o[4] = m.fl;
    }
  }
  SortPack K{};
  const int total = sort_key_layout(S, hmm.data(), n_blocks, mode == 3, K);
  std::printf("total %d\n", total);
  for (int k = 0; k < n_keys; ++k) std::printf("key %d %d %d %d %d %d\n", k, K.vbits[k], K.null_bit[k], K.shift[k], K.rshift[k], K.len_bits[k]);
  if (total > 128) { std::printf("wide\n"); return 0; }
  K.total_bits = total;
  if (K.check != (mode == 3 ? 1 : 0)) return 3;
  for (long long i = 0; i < n; ++i) {
    u128 comp = 0; bool bad = false;
    for (int k = 0; k < n_keys; ++k) { const Cell& c = cell(i, k); comp |= sort_pack_key(c.lo, c.hi, c.isn != 0, S, K, k, bad); }
    if (!bad && total < 128 && (comp >> total) != 0) return 4;      // a composite beyond its own width
    std::printf("%d %llu %llu\n", bad ? 1 : 0, (unsigned long long)(comp >> 64), (unsigned long long)comp);
  }
  return 0;
}
