// The calendar arithmetic of the engine, each rule stated once, as plain functions: the interpreter and the generated code call them
// lane by lane (gpuq_dev.h: OP_DATEPART, OP_MONTHSHIFT), the CSV date parser calls civil_to_days (kernels_scanfmt.hip), and
// tests/date_shift_host.cpp runs them on the host against dateutil.
//
//   civil_of_days      day number (days since 1970-01-01) -> (year, month 1-12, day 1-31)
//   civil_to_days      the inverse
//   days_in_month      28 / 29 / 30 / 31
//   month_shift_days   the day number k months later: the day of the month clamped to the target month's length
//   month_shift_fwd    the same for 0 <= k < 4800, which is what the device runs
//
// Proleptic Gregorian throughout [UPSTREAM-KNOWLEDGE: chrono's NaiveDate as arrow-arith 49 uses it -- Date32Type::add_year_months is
// shift_months(date, k): month index y * 12 + (m - 1) + k, day = min(day, days in the target month); the two conversions are Howard
// Hinnant's civil_from_days / days_from_civil].  Integer divisions by constants only, and only the era, the year and the month index
// are as wide as I: what lies inside one 400-year era is 32-bit (run_program pays every case's registers in every interpreter kernel).
// No headers: the file is read by hipcc, by hiprtc and by a plain C++ compiler alike.
#pragma once

#if defined(__HIPCC__) || defined(__HIPCC_RTC__) || defined(__CUDACC__)
#define GPUQ_CAL_HD __host__ __device__ __forceinline__
#else
#define GPUQ_CAL_HD inline
#endif

namespace gpuq {

// I: int for a four-digit year (the CSV parser), long long wherever the day number comes from a column: every intermediate of a
// Timestamp(Second)'s day (|days| < 2^47) and of a shift by |k| < 2^32 months stays far inside 64 bits.

// floor(a / b) and the remainder in [0, b) for a constant b > 0
template <class I> GPUQ_CAL_HD I cal_floor_div(const I a, const int b, unsigned& rem) {
  const I q = (a >= 0 ? a : a - (b - 1)) / b;
  rem = (unsigned)(a - q * b);
  return q;
}
// the day number of day d of month m in year `yoe` (0-399, counted from 1 March) of a 400-year era
template <class I> GPUQ_CAL_HD I cal_era_days(const I era, const unsigned yoe, const unsigned m, const unsigned d) {
  const unsigned doy = (153u * (m > 2u ? m - 3u : m + 9u) + 2u) / 5u + d - 1u;      // [0, 365]
  const unsigned doe = yoe * 365u + yoe / 4u - yoe / 100u + doy;                    // [0, 146096]
  return era * 146097 + (I)doe - 719468;
}
template <class I> GPUQ_CAL_HD I civil_to_days(I y, const unsigned m, const unsigned d) {
  y -= m <= 2u ? 1 : 0;
  unsigned yoe;
  const I era = cal_floor_div<I>(y, 400, yoe);
  return cal_era_days<I>(era, yoe, m, d);
}
// era, year of the era counted from 1 March (0-399), month and day of a day number
template <class I> GPUQ_CAL_HD I cal_split(const I days, unsigned& yoe, unsigned& m, unsigned& d) {
  unsigned doe;                                                                     // [0, 146096]
  const I era = cal_floor_div<I>(days + 719468, 146097, doe);
  yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;                  // [0, 399]
  const unsigned doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);                  // [0, 365]
  const unsigned mp = (5u * doy + 2u) / 153u;                                       // [0, 11]
  d = doy - (153u * mp + 2u) / 5u + 1u;
  m = mp < 10u ? mp + 3u : mp - 9u;
  return era;
}
template <class I> GPUQ_CAL_HD void civil_of_days(const I days, I& y, unsigned& m, unsigned& d) {
  unsigned yoe;
  const I era = cal_split<I>(days, yoe, m, d);
  y = (I)yoe + era * 400 + (m <= 2u ? 1 : 0);
}
// r: the year modulo 400, in [0, 399]
GPUQ_CAL_HD unsigned cal_month_length(const unsigned r, const unsigned m) {
  if (m == 2u) return (r % 4u == 0u && (r % 100u != 0u || r == 0u)) ? 29u : 28u;
  return 30u + ((m + (m >> 3)) & 1u);                                               // 31 for 1 3 5 7 8 10 12
}
template <class I> GPUQ_CAL_HD unsigned days_in_month(const I y, const unsigned m) {
  unsigned r;
  (void)cal_floor_div<I>(y, 400, r);
  return cal_month_length(r, m);
}
// The day number r months LATER, 0 <= r < 4800.  Whole 400-year eras are 146,097 days each and shift nothing else, so a shift by any k
// is this one by k mod 4800 plus floor(k / 4800) eras (month_shift_days; the expression compiler folds the eras into a constant it
// adds anyway).  Inside one era everything but the era itself is 32-bit: the one wide division is cal_split's.
template <class I> GPUQ_CAL_HD I month_shift_fwd(const I days, const unsigned r) {
  unsigned yoe, m, d;
  I era = cal_split<I>(days, yoe, m, d);
  const unsigned mi = (yoe + (m <= 2u ? 1u : 0u)) * 12u + (m - 1u) + r;             // months since January of the era's year 0: < 9612
  const unsigned y2 = mi / 12u, m2 = mi - y2 * 12u + 1u;                            // y2 <= 800
  const unsigned e2 = y2 / 400u, r400 = y2 - e2 * 400u;
  era += (I)e2;
  const unsigned len = cal_month_length(r400, m2), d2 = d < len ? d : len;
  // January and February count to the year before (civil_to_days), which for r400 = 0 is the last year of the era before
  unsigned yoe2 = r400;
  if (m2 <= 2u) { if (r400 == 0u) { era -= 1; yoe2 = 399u; } else yoe2 = r400 - 1u; }
  return cal_era_days<I>(era, yoe2, m2, d2);
}
template <class I> GPUQ_CAL_HD I month_shift_days(const I days, const I k) {
  unsigned r;
  const I eras = cal_floor_div<I>(k, 4800, r);
  return month_shift_fwd<I>(days, r) + eras * 146097;
}

}  // namespace gpuq
