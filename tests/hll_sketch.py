"""A numpy restatement of APPROX_DISTINCT's HyperLogLog (include/gpuq.h, gpuq_segment_approx_distinct): the canonical words of a value
per type, the hash, the registers and Ertl's estimator.  A helper for the tests, not a test; it states the rules a second time, in
another language, and shares no code with csrc/hll_estimate.h."""
import math

import numpy as np

P, M, Q = 14, 1 << 14, 50
MASK64 = (1 << 64) - 1
ALPHA = 0.7213475204444817      # 0.5 / ln 2
SIGNED = ("Int8", "Int16", "Int32", "Int64", "Date32", "Date64", "Timestamp")
UNSIGNED = ("UInt8", "UInt16", "UInt32", "UInt64")


def mix64(x):
    x = np.array(x, dtype=np.uint64)
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def hash64(lo, hi):
    with np.errstate(over="ignore"):
        return mix64(lo ^ mix64(hi + np.uint64(0x632BE59BD9B4E019)))


def words(values, tname):
    """(lo, hi): the two 64-bit words of every value that are hashed."""
    n = len(values)
    hi = np.zeros(n, dtype=np.uint64)
    if tname in SIGNED:
        return np.asarray(values).astype(np.int64).view(np.uint64), hi
    if tname in UNSIGNED:
        return np.asarray(values).astype(np.uint64), hi
    if tname == "Float64":
        bits = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64).copy()
        bits[np.isnan(values)] = 0x7FF8000000000000      # every NaN is one value
        bits[bits == np.uint64(0x8000000000000000)] = 0      # -0.0 is 0.0
        return bits, hi
    if tname == "Float32":
        bits = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32).copy()
        bits[np.isnan(values)] = 0x7FC00000
        bits[bits == np.uint32(0x80000000)] = 0
        return bits.astype(np.uint64), hi
    if tname == "Decimal":      # unscaled Python ints: 128-bit two's complement
        v = [int(x) % (1 << 128) for x in values]
    else:      # Utf8 of 15 bytes or fewer: the bytes big-endian in bits 127..8, the length in bits 7..0
        assert tname == "Utf8"
        b = [x.encode() for x in values]
        assert all(len(x) <= 15 for x in b)
        v = [int.from_bytes(x.ljust(15, b"\0"), "big") << 8 | len(x) for x in b]
    return np.array([x & MASK64 for x in v], dtype=np.uint64), np.array([x >> 64 for x in v], dtype=np.uint64)


def registers(lo, hi):
    h = hash64(np.asarray(lo, dtype=np.uint64), np.asarray(hi, dtype=np.uint64))
    idx = (h & np.uint64(M - 1)).astype(np.int64)
    w = (h >> np.uint64(P)) | np.uint64(1 << Q)
    low = w & (~w + np.uint64(1))      # the lowest set bit: a power of two, exact in Float64
    rho = np.frexp(low.astype(np.float64))[1].astype(np.uint8)      # 2^k = 0.5 * 2^(k + 1): ctz + 1
    reg = np.zeros(M, dtype=np.uint8)
    np.maximum.at(reg, idx, rho)
    return reg


def sigma(x):
    if x == 1.0:
        return math.inf
    y, z = 1.0, x
    while True:
        x *= x
        prev = z
        z += x * y
        y += y
        if z == prev:
            return z


def tau(x):
    if x == 0.0 or x == 1.0:
        return 0.0
    y, z = 1.0, 1.0 - x
    while True:
        x = math.sqrt(x)
        prev = z
        y *= 0.5
        z -= (1.0 - x) * (1.0 - x) * y
        if z == prev:
            return z / 3.0


def estimate_histogram(c):
    """c[k], k = 0..51: how many registers hold k."""
    m = float(M)
    z = m * tau((m - float(c[Q + 1])) / m)
    for k in range(Q, 0, -1):
        z = 0.5 * (z + float(c[k]))
    z += m * sigma(float(c[0]) / m)
    if math.isinf(z):
        return 0
    if z == 0.0:      # every register at q + 1: the conversion saturates
        return MASK64
    return min(int(math.floor(ALPHA * m * m / z + 0.5)), MASK64)


def estimate_registers(reg):
    return estimate_histogram(np.bincount(reg, minlength=Q + 2))


def approx_distinct(values, tname, valid=None):
    """The estimate over the non-NULL values."""
    if valid is not None:
        valid = np.asarray(valid, dtype=bool)
        values = [v for v, ok in zip(values, valid) if ok] if tname in ("Decimal", "Utf8") else np.asarray(values)[valid]
    if len(values) == 0:
        return 0
    return estimate_registers(registers(*words(values, tname)))
