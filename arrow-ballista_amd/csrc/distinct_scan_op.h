// One row of a column sorted inside its segments, as an element of the segmented scan (window_scan_op.h): what a DISTINCT aggregate
// reduces (kernels_distinct.hip, gpuq_segment_distinct).  Plain functions: the kernels call them row by row, tests/distinct_scan_host.cpp
// folds rows with them on the host.
//
// The distinct values of a segment are its run heads: a row that is not NULL and either opens the segment or differs, byte for byte, from
// the row before it.  A segment's first row restarts the element, every other row that is no run head contributes nothing -- so the
// element at a segment's last row holds (the number of run heads, their accumulator cell).
#pragma once
#include "window_scan_op.h"

namespace gpuq {

__host__ __device__ __forceinline__ bool distinct_run_head(const bool valid, const bool seg_head, const bool same_as_prev) { return valid && (seg_head || !same_as_prev); }
__host__ __device__ __forceinline__ WinElem distinct_row(const int kind, const bool seg_head, const bool valid, const bool same_as_prev, const u64 lo, const u64 hi) {
  return win_row(kind, seg_head, distinct_run_head(valid, seg_head, same_as_prev), lo, hi);
}

}  // namespace gpuq
