// The key encoding of the sort (kernels_sort.hip, sort_key_plan in capi.cpp), as plain functions: the kernels call the row rules lane by
// lane, the host plans the layout with sort_key_layout, and tests/sort_key_host.cpp runs all of it on the host against an exact order.
//
//   sort_view          a key register as a signed 128-bit value whose order is the key's order
//   mm_value           one row of the per-key min / max / flags pass (k_sort_minmax)
//   sort_direct_key    the (2-bit rank, unsigned value) pair the one-block sort compares (k_sort_direct)
//   sort_pack_key      one key's field of the composite, placed, with the verdict of a checked layout (k_sort_pack)
//   sort_key_layout    per-block (min, max, flags) -> the bit layout of the composite key and its width
//
// The packed string field: the bytes up to the longest value, zero-padded.  Zero padding ties s with s + "\0", so when any value of the
// column ENDS in a 0x00 byte (flag bit 2 of the min/max pass) the 4-bit length is appended below the bytes; no other column pays for it.
// All differences are taken in u128: a Decimal128(38) range spans more than an i128 difference holds.
#pragma once
#include "gpuq_kernels.h"

namespace gpuq {

// ordered 128-bit view of a key register: signed integers as is; f64 through the total-order map;
// packed strings with the top bit flipped so that signed compare == bytewise compare
__host__ __device__ __forceinline__ i128 sort_view(u64 lo, u64 hi, int kind) {
  if (kind == 1) { const i64 k = f64_total_key(lo); return (i128)k; }
  if (kind == 2) hi ^= 0x8000000000000000ull;
  return mk128(lo, hi);
}
// a packed string (bytes big-endian in bits 127..8, length in bits 7..0): its length, and whether its last byte is 0x00
__host__ __device__ __forceinline__ uint32_t sort_str_len(u64 lo) { return (uint32_t)(lo & 0xFFu); }
__host__ __device__ __forceinline__ bool sort_str_ends_nul(u64 lo, u64 hi) {
  const uint32_t len = sort_str_len(lo);
  // byte len - 1: bits 63 - 8 (len - 1) .. of hi for len <= 8, of lo beyond (one 64-bit shift: the min/max kernel has no registers to spare)
  return len != 0 && (((len <= 8 ? hi : lo) >> ((64 - 8 * len) & 63)) & 0xFFu) == 0;      // (a length beyond 15 is refused elsewhere)
}

// ------------------------------------------------------------------ min / max per key
// flags: bit 0 any non-null, bit 1 any NULL, bit 2 a string that ends in a 0x00 byte, bit 8 + l a string of l bytes (l <= 15).  Bits only,
// so that parts of the input merge by OR and a row costs no compare: k_sort_minmax<8> sits two registers below losing a wave.
struct MinMax { u64 mn_lo, mn_hi, mx_lo, mx_hi; uint32_t fl; };
constexpr uint32_t MM_ANY_VALUE = 1u, MM_ANY_NULL = 2u, MM_TAIL_NUL = 4u;
__host__ __device__ __forceinline__ void mm_init(MinMax& m) { m.mn_lo = ~0ull; m.mn_hi = 0x7FFFFFFFFFFFFFFFull; m.mx_lo = 0; m.mx_hi = 0x8000000000000000ull; m.fl = 0; }
__host__ __device__ __forceinline__ void mm_update(MinMax& m, i128 v) {
  if (v < mk128(m.mn_lo, m.mn_hi)) { m.mn_lo = (u64)v; m.mn_hi = (u64)((u128)v >> 64); }
  if (v > mk128(m.mx_lo, m.mx_hi)) { m.mx_lo = (u64)v; m.mx_hi = (u64)((u128)v >> 64); }
}
// the flags of two parts of the input as the flags of both
__host__ __device__ __forceinline__ u64 mm_flags_merge(u64 a, u64 b) { return a | b; }
__host__ __device__ __forceinline__ void mm_value(MinMax& m, u64 lo, u64 hi, bool isn, int kind) {
  if (isn) { m.fl |= MM_ANY_NULL; return; }
  m.fl |= MM_ANY_VALUE; mm_update(m, sort_view(lo, hi, kind));
  if (kind == 2) m.fl |= (0x100u << (sort_str_len(lo) & 15u)) | (sort_str_ends_nul(lo, hi) ? MM_TAIL_NUL : 0u);      // the lengths that occur: bit 8 + len
}

// ------------------------------------------------------------------ the one-block sort's comparator input
// The key normalised to an unsigned 128-bit value whose order is the requested order (ASC / DESC), and its 2-bit rank for NULL placement
// (0 NULL first, 1 value, 2 NULL last; 3 is padding).  Rows compare by (rank_0, value_0, rank_1, value_1, ..., row id).
__host__ __device__ __forceinline__ uint32_t sort_direct_key(u64 lo, u64 hi, bool isn, int kind, bool desc, bool nulls_first, u128& u) {
  u = 0;
  if (isn) return nulls_first ? 0u : 2u;
  u = (u128)sort_view(lo, hi, kind) ^ ((u128)1 << 127);     // signed order -> unsigned order
  if (desc) u = ~u;
  return 1u;
}

// ------------------------------------------------------------------ the composite key's fields
// the value a field holds before the base is taken off: the view without what the layout drops (strings: the length byte and the bytes
// beyond the longest value; arithmetic shift keeps the order), with the string's length below it when the layout asks for it
__host__ __device__ __forceinline__ i128 sort_field_value(u64 lo, u64 hi, int kind, const SortPack& K, int k) {
  const i128 v = sort_view(lo, hi, kind) >> K.rshift[k];
  if (K.len_bits[k] == 0) return v;
  return (i128)(((u128)v << K.len_bits[k]) | (u128)(sort_str_len(lo) & ((1u << K.len_bits[k]) - 1u)));
}
// Key k of a row as its field of the composite, in place.  bad (only ever set, and only when K.check): the layout does not hold this
// row -- a value outside its field (below the base wraps to a huge field: caught too), a NULL where there is no null bit, a string
// beyond the longest one the layout keeps, or one that ends in 0x00 where the layout keeps no length.
__host__ __device__ __forceinline__ u128 sort_pack_key(u64 lo, u64 hi, bool isn, const SortSpec& S, const SortPack& K, int k, bool& bad) {
  u128 field = 0;
  if (!isn) {
    const u128 v = (u128)sort_field_value(lo, hi, S.kind[k], K, k);
    const u128 base = ((u128)K.base_hi[k] << 64) | (u128)K.base_lo[k];
    field = S.desc[k] ? base - v : v - base;
    if (K.check) {
      if (K.vbits[k] < 128 && (field >> K.vbits[k]) != 0) bad = true;
      if (S.kind[k] == 2 && ((int)sort_str_len(lo) > 16 - (K.rshift[k] + 7) / 8 || (K.len_bits[k] == 0 && sort_str_ends_nul(lo, hi)))) bad = true;
    }
  } else if (K.check && K.null_bit[k] < 0) bad = true;
  if (K.null_bit[k] >= 0) {
    // nulls_first: NULL -> 0, value -> 1 in the bit above the value field
    const u128 flag = (isn != (bool)S.nulls_first[k]) ? 1 : 0;
    field |= flag << K.null_bit[k];
  }
  return K.shift[k] < 128 ? field << K.shift[k] : (u128)0;      // (an empty field above 128 bits of others)
}

#ifndef GPUQ_JIT
// ------------------------------------------------------------------ the layout
inline int bitlen128(u128 v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }
// hmm: the read-back of the min/max pass, [block][MAX_SORT_KEYS] x {min_lo, min_hi, max_lo, max_hi, flags} in the ordered view.
// Returns the width of the composite key; beyond 128 bits K is not to be used (WideSortKey).
// guess: the ranges are those of a SAMPLE, widened into a layout that the pack kernel then verifies row by row (K.check = 1).  The guess
// keeps the cost class of the sample's own layout (number of passes, packed 8-byte records or not): it is widened by 1/64 of the range on
// both sides if that is free, by 1/4096 if not, and always spread over the whole 2^bits its width has anyway.
// Ranges are handled as offset-binary u128 (x ^ 2^127: the order of the signed view, without its overflow).
inline int sort_key_layout(const SortSpec& S, const u64* hmm, int n_blocks, bool guess, SortPack& K_out) {
  const u128 TOP = (u128)1 << 127, UMAX = ~(u128)0;
  u128 mn[MAX_SORT_KEYS], mx[MAX_SORT_KEYS]; u64 fl[MAX_SORT_KEYS] = {0, 0, 0, 0}; int rshift[MAX_SORT_KEYS] = {0, 0, 0, 0}, len_bits[MAX_SORT_KEYS] = {0, 0, 0, 0};
  for (int k = 0; k < S.n_keys; ++k) {
    i128 a = (i128)(UMAX >> 1), c = -a - 1;
    for (int b = 0; b < n_blocks; ++b) {
      const u64* o = &hmm[((size_t)b * MAX_SORT_KEYS + k) * 5];
      if (!(o[4] & MM_ANY_VALUE)) { fl[k] |= (o[4] & 0xFF); continue; }
      const i128 oa = mk128(o[0], o[1]), oc = mk128(o[2], o[3]);
      if (oa < a) a = oa;
      if (oc > c) c = oc;
      fl[k] = mm_flags_merge(fl[k], o[4]);
    }
    if (S.kind[k] == 2) {
      int maxlen = 0; for (int l = 1; l <= 15; ++l) if ((fl[k] >> (8 + l)) & 1) maxlen = l;      // the longest string
      rshift[k] = maxlen > 0 ? 8 * (15 - maxlen) + 8 : 127;      // (only empty strings: nothing but the view's sign is left -- a shift by 128 is undefined)
      if (fl[k] & MM_TAIL_NUL) len_bits[k] = 4;
    }
    if (fl[k] & MM_ANY_VALUE) {
      a >>= rshift[k]; c >>= rshift[k];
      if (len_bits[k]) { a = (i128)((u128)a << 4); c = (i128)(((u128)c << 4) | 15u); }      // every length the field can hold
    }
    mn[k] = (u128)a ^ TOP; mx[k] = (u128)c ^ TOP;
  }
  // layout for the ranges [mn - range >> mshift, mx + range >> mshift] (mshift < 0: the ranges as they are)
  auto layout = [&](int mshift, bool spread, SortPack& K) {
    int width[MAX_SORT_KEYS] = {0, 0, 0, 0}; int total = 0;
    K = SortPack{};
    for (int k = 0; k < S.n_keys; ++k) {
      int vb = 0; K.rshift[k] = rshift[k]; K.len_bits[k] = len_bits[k];
      if (fl[k] & MM_ANY_VALUE) {
        u128 lo = mn[k], hi = mx[k];
        if (mshift >= 0) {
          const u128 m = ((hi - lo) >> mshift) + 1;
          lo = lo > m ? lo - m : 0;
          hi = UMAX - hi > m ? hi + m : UMAX;
        }
        vb = bitlen128(hi - lo);
        if (spread && vb < 127) {      // the field holds 2^vb values whatever the range: centre the range in it
          const u128 full = ((u128)1 << vb) - 1, spare = full - (hi - lo), down = spare / 2;
          lo = lo > down ? lo - down : 0;
          hi = UMAX - lo > full ? lo + full : UMAX;
        }
        const u128 base = (S.desc[k] ? hi : lo) ^ TOP; K.base_lo[k] = (u64)base; K.base_hi[k] = (u64)(base >> 64);
      }
      K.vbits[k] = vb;
      K.null_bit[k] = (fl[k] & MM_ANY_NULL) ? vb : -1;
      width[k] = vb + ((fl[k] & MM_ANY_NULL) ? 1 : 0);
      total += width[k];
    }
    int sh = 0; for (int k = S.n_keys - 1; k >= 0; --k) { K.shift[k] = sh; sh += width[k]; }
    return total;
  };
  auto cost_class = [](int total) { return ((total + 7) / 8) * 4 + (total <= 32 ? 0 : total <= 64 ? 1 : 2); };
  int total = layout(-1, false, K_out);
  if (guess) {
    const int cls = cost_class(total);
    SortPack G{}; int t = layout(6, true, G);
    if (cost_class(t) != cls) t = layout(12, true, G);
    if (cost_class(t) != cls) t = layout(-1, true, G);
    K_out = G; total = t; K_out.check = 1;
  }
  return total;
}
#endif  // GPUQ_JIT

}  // namespace gpuq
