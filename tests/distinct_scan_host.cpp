// The row rule of the DISTINCT reduction (csrc/distinct_scan_op.h: distinct_run_head / distinct_row over win_row / win_combine of
// csrc/window_scan_op.h and acc_identity / acc_combine of csrc/gpuq_kernels.h) folded on the host in three groupings.  The headers'
// functions are the code under test; the kernels of csrc/kernels_distinct.hip combine rows with the same calls, grouped by thread, wave
// and tile, and keep the element at every segment's last row.  tests/test_cpu_distinct.py builds and drives it.
//   stdin:  "kind n", then n rows "seg_head valid lo hi" (kind: an AccKind; lo, hi: the value's two words, unsigned -- its bytes and its
//           operand; a float its bit pattern).  A NULL row's bytes are zeroes, as the kernel's loader leaves them.
//   stdout: three blocks of n lines "count lo hi" -- every row's running element, folded left to right, in tiles of 7 with a carry, and
//           as a balanced tree -- each block closed by a line "-"
#include <cstdio>
#include <vector>

#include "distinct_scan_op.h"

using namespace gpuq;

static void tree(const int kind, const std::vector<WinElem>& rows, std::vector<WinElem>& out, const size_t a, const size_t b, WinElem& total) {
  if (b - a == 1) { out[a] = rows[a]; total = rows[a]; return; }
  const size_t mid = a + (b - a) / 2;
  WinElem tl, tr;
  tree(kind, rows, out, a, mid, tl);
  tree(kind, rows, out, mid, b, tr);
  for (size_t i = mid; i < b; ++i) out[i] = win_combine(kind, tl, out[i]);
  total = win_combine(kind, tl, tr);
}

static void print(const std::vector<WinElem>& v) {
  for (const WinElem& e : v) std::printf("%lld %llu %llu\n", e.count, e.lo, e.hi);
  std::printf("-\n");
}

int main() {
  int kind = 0; long long n = 0;
  if (std::scanf("%d %lld", &kind, &n) != 2 || n < 0) return 2;
  std::vector<WinElem> rows((size_t)n);
  unsigned long long plo = 0, phi = 0;
  for (auto& r : rows) {
    int head = 0, valid = 0; unsigned long long lo = 0, hi = 0;
    if (std::scanf("%d %d %llu %llu", &head, &valid, &lo, &hi) != 4) return 2;
    if (!valid) { lo = 0; hi = 0; }
    r = distinct_row(kind, head != 0, valid != 0, lo == plo && hi == phi, lo, hi);
    plo = lo; phi = hi;
  }
  // left to right
  std::vector<WinElem> a((size_t)n);
  WinElem run = win_identity(kind);
  for (size_t i = 0; i < rows.size(); ++i) { run = win_combine(kind, run, rows[i]); a[i] = run; }
  print(a);
  // tiles of 7: totals, the carry into every tile, a second walk from the carry
  constexpr size_t TILE = 7;
  const size_t ntiles = (rows.size() + TILE - 1) / TILE;
  std::vector<WinElem> carry(ntiles + 1), b((size_t)n);
  for (size_t t = 0; t < ntiles; ++t) {
    WinElem tot = win_identity(kind);
    for (size_t i = t * TILE; i < rows.size() && i < (t + 1) * TILE; ++i) tot = win_combine(kind, tot, rows[i]);
    carry[t] = tot;
  }
  WinElem before = win_identity(kind);
  for (size_t t = 0; t < ntiles; ++t) { const WinElem tot = carry[t]; carry[t] = before; before = win_combine(kind, before, tot); }
  for (size_t t = 0; t < ntiles; ++t) {
    WinElem r = carry[t];
    for (size_t i = t * TILE; i < rows.size() && i < (t + 1) * TILE; ++i) { r = win_combine(kind, r, rows[i]); b[i] = r; }
  }
  print(b);
  // a balanced tree
  std::vector<WinElem> c((size_t)n);
  WinElem total;
  if (n > 0) tree(kind, rows, c, 0, rows.size(), total);
  print(c);
  return 0;
}
