"""Interval and Duration arithmetic restated on Python ints: the second opinion the temporal tests compare the engine with.

It shares nothing with csrc/: dates go through datetime.date and dateutil.relativedelta (whose months=k is the rule arrow-arith 49 /
chrono apply: month index shifted, day of the month clamped), timestamps are (day, time of day) pairs split by Python's floor division,
and the sub-day part is added as an exact count of nanoseconds and floored back to the unit.

An interval is the triple (months, days, nanoseconds) whatever its IntervalUnit; sign is +1 for `+` and -1 for `-`.
"""
import datetime
import functools

from dateutil.relativedelta import relativedelta

EPOCH = datetime.date(1970, 1, 1)
UNITS = ["Second", "Millisecond", "Microsecond", "Nanosecond"]
PER_SECOND = {"Second": 1, "Millisecond": 10 ** 3, "Microsecond": 10 ** 6, "Nanosecond": 10 ** 9}
DAY_NS = 86400 * 10 ** 9
MIN_DAYS = (datetime.date(1, 1, 1) - EPOCH).days          # what datetime.date can hold
MAX_DAYS = (datetime.date(9999, 12, 31) - EPOCH).days


class OutOfRange(Exception):
    """The result leaves int32 days / the int64 count: an error of the run."""


def year_month(months):
    return (int(months), 0, 0)


def day_time(days, milliseconds):
    return (0, int(days), int(milliseconds) * 10 ** 6)


def month_day_nano(months, days, nanoseconds):
    return (int(months), int(days), int(nanoseconds))


def days_of(y, m, d):
    return (datetime.date(y, m, d) - EPOCH).days


@functools.lru_cache(maxsize=None)
def shift_months(days, k):
    """The day number k months later (k < 0: earlier), the day of the month clamped to the target month's length."""
    return ((EPOCH + datetime.timedelta(days=days)) + relativedelta(months=k) - EPOCH).days


def _trunc_div(a, b):
    q = abs(a) // b
    return q if a >= 0 else -q


def date32_add(days, interval, sign=1):
    """Date32 +- interval: months first, then the days, then the sub-day part as whole days truncated toward zero."""
    if days is None or interval is None:
        return None
    months, d, ns = (sign * x for x in interval)
    x = shift_months(days, months) if months else days
    x = x + d + _trunc_div(ns, DAY_NS)
    if not -2 ** 31 <= x < 2 ** 31:
        raise OutOfRange(x)
    return x


def timestamp_add(count, unit, interval, sign=1):
    """Timestamp(unit) +- interval: (day, time of day) by floor division, the day shifted by the months, days of 86,400 s, the sub-day
    part exactly, and the exact instant floored to the unit."""
    if count is None or interval is None:
        return None
    months, d, ns = (sign * x for x in interval)
    per_day = PER_SECOND[unit] * 86400
    ns_per_unit = 10 ** 9 // PER_SECOND[unit]
    day, tod = divmod(count, per_day)
    if months:
        day = shift_months(day, months)
    exact_ns = (day * per_day + tod) * ns_per_unit + d * DAY_NS + ns
    x = exact_ns // ns_per_unit
    if not -2 ** 63 <= x < 2 ** 63:
        raise OutOfRange(x)
    return x


def wrap64(x):
    return None if x is None else (x + 2 ** 63) % 2 ** 64 - 2 ** 63


def sub64(a, b):
    """Timestamp - Timestamp, Timestamp - Duration, Duration - Duration: 64-bit wrapping."""
    return None if a is None or b is None else wrap64(a - b)


def add64(a, b):
    return None if a is None or b is None else wrap64(a + b)
