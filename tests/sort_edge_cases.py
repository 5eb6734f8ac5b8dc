"""Sort keys at the edges of their types' orders, shared by tests/test_cpu_sort_order_exact.py (the encoding, on the host) and
tests/test_gpu_sort_key_edges.py (every executor of the sort, on the device).  Values are plain Python: ints, floats made from their bit
patterns (a NaN keeps its sign and payload), str.  Each list is in ascending order as tests/sort_order_exact.py states it."""
import struct

import numpy as np


def f64_from_pattern(p):
    return struct.unpack("<d", struct.pack("<Q", p))[0]


I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
INT64_EDGES = [I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX]

DEC38_MAX = 10**38 - 1
DECIMAL_EDGES = [-DEC38_MAX, -(1 << 126), -(1 << 64), -(1 << 63), -1, 0, 1, 1 << 63, 1 << 64, 1 << 126, DEC38_MAX]      # Decimal128(38, 0), unscaled

_F64_POS = [0x0000000000000000, 0x0000000000000001, 0x0010000000000000, 0x3FF0000000000000, 0x7FEFFFFFFFFFFFFF, 0x7FF0000000000000,
            0x7FF8000000000000, 0x7FF8000000000123]      # +0, smallest subnormal, smallest normal, 1, largest, inf, two quiet NaNs
F64_EDGE_PATTERNS = [p | 1 << 63 for p in reversed(_F64_POS)] + _F64_POS
F64_EDGES = [f64_from_pattern(p) for p in F64_EDGE_PATTERNS]

_F32_POS = [0x00000000, 0x00000001, 0x00800000, 0x3F800000, 0x7F7FFFFF, 0x7F800000, 0x7FC00000, 0x7FC00123]
F32_EDGE_PATTERNS = [p | 1 << 31 for p in reversed(_F32_POS)] + _F32_POS
F32_EDGES = list(np.array(F32_EDGE_PATTERNS, dtype=np.uint32).view(np.float32))      # numpy float32 scalars: float() widens them

UTF8_EDGES = ["", "a", "a\0", "a\0\0", "ab", "abcdefghijklmn", "abcdefghijklmno", "\x7f", "\u0080", "é", "\U0001F600"]      # bytewise: 7F < C2 80 < C3 A9 < F0 ..
