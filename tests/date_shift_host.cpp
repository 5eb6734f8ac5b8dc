// The calendar arithmetic of csrc/date_shift_op.h run on the host (the header is plain C++ there), under AddressSanitizer / UBSan:
// one line "day k shifted" for every day of 1600-01-01 .. 2400-12-31 stepped by 7 and for every month end of those years, times every
// k below.  tests/test_cpu_temporal_arith.py compares the lines with dateutil.  The day numbers of the range's ends and the month ends
// come from the header's own civil_to_days / days_in_month: the test builds the same list from datetime.date, so a wrong one shows as
// a differing line.
#include <cstdio>

#include "date_shift_op.h"

int main() {
  typedef long long i64;
  static const i64 ks[] = {-25, -13, -12, -1, 0, 1, 11, 12, 13, 1200};
  const i64 first = gpuq::civil_to_days<i64>(1600, 1u, 1u), last = gpuq::civil_to_days<i64>(2400, 12u, 31u);
  int bad = 0;
  auto emit = [&](const i64 day) {
    i64 y; unsigned m, d;
    gpuq::civil_of_days<i64>(day, y, m, d);
    if (gpuq::civil_to_days<i64>(y, m, d) != day || m < 1u || m > 12u || d < 1u || d > gpuq::days_in_month<i64>(y, m)) ++bad;
    for (const i64 k : ks) std::printf("%lld %lld %lld\n", day, k, gpuq::month_shift_days<i64>(day, k));
  };
  for (i64 day = first; day <= last; day += 7) emit(day);
  for (i64 y = 1600; y <= 2400; ++y)
    for (unsigned m = 1; m <= 12; ++m) emit(gpuq::civil_to_days<i64>(y, m, gpuq::days_in_month<i64>(y, m)));
  // the narrow instantiation the CSV parser uses agrees with the wide one
  for (int y = 1; y <= 9999; y += 7)
    for (unsigned m = 1; m <= 12; ++m)
      if ((i64)gpuq::civil_to_days<int>(y, m, 1u) != gpuq::civil_to_days<i64>(y, m, 1u)) ++bad;
  if (bad) { std::fprintf(stderr, "%d self-check failures\n", bad); return 1; }
  return 0;
}
