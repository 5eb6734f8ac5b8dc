// Host restatement of the "runs" aggregate (csrc/kernels_hash.hip k_agg_runs_count / k_agg_runs_order / k_agg_runs_write) around the
// head / output-row functions of csrc/gpuq_kernels.h, which are the code under test: the walk below does with loops what a wave does
// with ballots and shuffles and calls the same functions for every decision.  tests/test_cpu_agg_runs.py builds and drives it.
//   stdin:  n wps, then n rows "active key value"
//   stdout: "out_of_order groups", then per result row "key sum count plain_stores folds"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpuq_kernels.h"

using namespace gpuq;

struct Row { int active; u64 key; long long value; };
struct Lane { bool head; u64 prev_p1; };

// one segment's walk: lane views of the words [ws, ws + wps), the state seeded from the last row of the word before
template <class Body>
static u64 walk(const std::vector<Row>& rows, const i64 ws, const i64 wps, Body body) {
  const i64 n = (i64)rows.size(), nwords = (n + 63) >> 6;
  bool below63 = false; u64 last_p1 = 0;
  if (ws > 0 && ws * 64 - 1 < n && rows[(size_t)(ws * 64 - 1)].active) { below63 = true; last_p1 = rows[(size_t)(ws * 64 - 1)].key + 1; }
  for (i64 w = ws; w < ws + wps && w < nwords; ++w) {
    u64 active_mask = 0;
    for (int l = 0; l < 64; ++l) if (w * 64 + l < n && rows[(size_t)(w * 64 + l)].active) active_mask |= 1ull << l;
    Lane lanes[64];
    for (int l = 0; l < 64; ++l) {
      const bool active = (active_mask >> l) & 1;
      const u64 key = active ? rows[(size_t)(w * 64 + l)].key : 0;
      const u64 under = l ? runs_lanes_le(active_mask, l - 1) : 0;
      const u64 prev_p1 = under ? rows[(size_t)(w * 64 + 63 - __builtin_clzll(under))].key + 1 : last_p1;
      const bool below = l ? ((active_mask >> (l - 1)) & 1) != 0 : below63;
      lanes[l] = Lane{runs_head(active, below, prev_p1, key), prev_p1};
    }
    if (active_mask) last_p1 = rows[(size_t)(w * 64 + 63 - __builtin_clzll(active_mask))].key + 1;
    below63 = (active_mask >> 63) != 0;
    body(w, active_mask, lanes);
  }
  return last_p1;
}

int main() {
  long long n = 0, wps = 0;
  if (std::scanf("%lld %lld", &n, &wps) != 2 || n < 0 || wps < 1) return 2;
  std::vector<Row> rows((size_t)n);
  for (auto& r : rows) { unsigned long long k; if (std::scanf("%d %llu %lld", &r.active, &k, &r.value) != 3) return 2; r.key = k; }
  const i64 nwords = (n + 63) >> 6, nsegs = (nwords + wps - 1) / wps;
  // count
  std::vector<uint32_t> counts((size_t)nsegs); std::vector<u64> seg_last((size_t)nsegs), seg_first((size_t)nsegs);
  bool bad = false;
  for (i64 s = 0; s < nsegs; ++s) {
    uint32_t heads = 0; u64 first_p1 = 0;
    seg_last[(size_t)s] = walk(rows, s * wps, wps, [&](i64 w, u64, const Lane* lanes) {
      for (int l = 0; l < 64; ++l) {
        const u64 key = lanes[l].head ? rows[(size_t)(w * 64 + l)].key : 0;
        heads += lanes[l].head;
        bad = bad || runs_out_of_order(lanes[l].head, lanes[l].prev_p1, key);
        if (lanes[l].head && lanes[l].prev_p1 == 0) first_p1 = key + 1;
      }
    });
    counts[(size_t)s] = heads; seg_first[(size_t)s] = first_p1;
  }
  // scan + order
  uint32_t total = 0; u64 before = 0;
  for (i64 s = 0; s < nsegs; ++s) {
    const uint32_t c = counts[(size_t)s]; counts[(size_t)s] = total; total += c;
    if (seg_first[(size_t)s] != 0 && seg_first[(size_t)s] <= before) bad = true;
    if (seg_last[(size_t)s] > before) before = seg_last[(size_t)s];
  }
  // write
  std::vector<u64> okey(total, 0); std::vector<long long> osum(total, 0), ocnt(total, 0); std::vector<int> plain(total, 0), folds(total, 0);
  for (i64 s = 0; s < nsegs; ++s) {
    uint32_t heads = 0;
    walk(rows, s * wps, wps, [&](i64 w, u64 active_mask, const Lane* lanes) {
      u64 head_mask = 0, start_mask = 0;
      for (int l = 0; l < 64; ++l) {
        const bool active = (active_mask >> l) & 1;
        if (lanes[l].head) head_mask |= 1ull << l;
        if (lanes[l].head || !active || l == 0) start_mask |= 1ull << l;
      }
      long long sum = 0, cnt = 0;
      for (int l = 0; l < 64; ++l) {
        const bool active = (active_mask >> l) & 1;
        if ((start_mask >> l) & 1) { sum = 0; cnt = 0; }
        if (!active) continue;
        const Row& r = rows[(size_t)(w * 64 + l)];
        sum += r.value; cnt += 1;
        const uint32_t g = runs_out_row(counts[(size_t)s], heads, head_mask, l);
        if (g >= total) { std::printf("row %lld: output row %u of %u\n", (long long)(w * 64 + l), g, total); std::exit(3); }
        if (lanes[l].head) okey[g] = r.key;
        const bool tail = l == 63 || ((start_mask >> (l + 1)) & 1);
        if (!tail) continue;
        if (runs_piece_interior(head_mask, start_mask, l)) { osum[g] = sum; ocnt[g] = cnt; plain[g] += 1; }
        else { osum[g] += sum; ocnt[g] += cnt; folds[g] += 1; }
      }
      heads += (uint32_t)__builtin_popcountll(head_mask);
    });
  }
  std::printf("%d %u\n", bad ? 1 : 0, total);
  for (uint32_t g = 0; g < total; ++g) std::printf("%llu %lld %lld %d %d\n", okey[g], osum[g], ocnt[g], plain[g], folds[g]);
  return 0;
}
