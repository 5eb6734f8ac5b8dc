// The element and the operator of the segmented window scan (kernels_window.hip, gpuq_window_scan), as plain functions: the kernels
// call them lane by lane, tests/window_scan_host.cpp folds rows with them on the host.
//
// An element stands for a run of adjacent rows: (a partition head was seen in the run, the non-NULL values since the last head -- or
// since the run's first row when it holds none --, their accumulator cell).  What an accumulator is stays where it is stated:
// acc_identity / acc_combine in gpuq_kernels.h.
#pragma once
#include "gpuq_kernels.h"

namespace gpuq {

struct WinElem { u64 lo, hi; i64 count; uint32_t head; uint32_t pad; };

// no rows.  Its cell is the accumulator's identity, but nothing below relies on that value being neutral: an element without values is
// skipped by its count (acc_identity's +inf is not neutral for a MIN over NaNs in total order, nor 0.0 for a sum of -0.0).
__host__ __device__ __forceinline__ WinElem win_identity(const int kind) { return WinElem{acc_identity(kind, 0), acc_identity(kind, 1), 0, 0u, 0u}; }
// one row: its value is its cell (COUNT: 1); a NULL value contributes nothing but may still start a partition
__host__ __device__ __forceinline__ WinElem win_row(const int kind, const bool head, const bool valid, const u64 lo, const u64 hi) {
  WinElem e = win_identity(kind);
  e.head = head ? 1u : 0u;
  if (valid) { e.count = 1; e.lo = kind == ACC_COUNT ? 1ull : lo; e.hi = kind == ACC_COUNT ? 0ull : hi; }
  return e;
}
// a then b (b's rows follow a's): (f1, c1, v1) o (f2, c2, v2) = f2 ? (1, c2, v2) : (f1, c1 + c2, acc_combine(v1, v2)).  Associative, not commutative.
__host__ __device__ __forceinline__ WinElem win_combine(const int kind, const WinElem& a, const WinElem& b) {
  if (b.head) return b;
  WinElem r = a;
  if (b.count == 0) return r;
  if (a.count == 0) { r.lo = b.lo; r.hi = b.hi; r.count = b.count; return r; }
  r.count += b.count;
  acc_combine(kind, r.lo, r.hi, b.lo, b.hi);
  return r;
}

}  // namespace gpuq
