// Internal C++ launch interface between the C ABI (capi.cpp) and the HIP kernels.
#pragma once
#include "gpuq_dev.h"
#ifndef GPUQ_JIT
#include <type_traits>
#include "devbuf.h"      // HIPCHECK (launch_sink)
#endif

namespace gpuq {

// ----- project / materialise
constexpr int MAX_OUTS = 16;
struct OutCol {
  void* data;          // fixed-width destination (4/8/16 B per row by cls; CC_STR stores the 16-B packed form)
  u64* validity;       // optional validity bitmap as 64-bit words (bit i of word w = row 64*w+i); nullptr = not written
  int32_t reg;
  int32_t cls;         // CC_I32 / CC_U32 / CC_I64 / CC_I128 / CC_STR / CC_BIT(data = u64 bitmap words)
};
struct OutSpec { int32_t n_out; int32_t pad; OutCol cols[MAX_OUTS]; };

// ----- aggregate
constexpr int MAX_ACCS = 12;
constexpr int MAX_KEYS = 4;
enum AccKind : int32_t { ACC_SUM = 0, ACC_COUNT = 1, ACC_COUNT_STAR = 2, ACC_MIN = 3, ACC_MAX = 4, ACC_FSUM = 5, ACC_FMIN = 6, ACC_FMAX = 7,
                         ACC_BAND = 8, ACC_BOR = 9, ACC_BXOR = 10 /* bitwise: the low 64 bits of the argument's two's-complement pattern */ };
struct AggSpec {
  int32_t n_keys, n_accs;
  int32_t key_reg[MAX_KEYS];
  int32_t acc_kind[MAX_ACCS];
  int32_t acc_reg[MAX_ACCS];
};

// The origins of the moment aggregates (agg_compile.cpp, Moments): origin k is register reg[k] of the pick program on the lowest
// row that passes its predicate and is not NULL there -- 0.0 when there is no such row or the value is not finite.  It is stored
// to every dst[i] with dst_origin[i] == k: the immediate slots of the uploaded programs that read it.  Built once per operator
// and kept in device memory.
constexpr int MAX_ORIGINS = 8;
constexpr int MAX_ORIGIN_DSTS = 40;
struct OriginPick {
  int32_t n_origins, n_dsts;
  int32_t reg[MAX_ORIGINS];
  int32_t dst_origin[MAX_ORIGIN_DSTS];
  u64* dst[MAX_ORIGIN_DSTS];
};

// Result layout shared by the tiny and hash aggregates (device memory, caller allocated):
//   keys  [cap][n_keys] as (lo,hi) u64 pairs      key_nulls[cap] bitmask over keys
//   cells [cap][n_accs] as (lo,hi) u64 pairs      n_groups (device u32)
struct AggOut {
  u64* keys; uint32_t* key_nulls; u64* cells; uint32_t* n_groups; int32_t cap; int32_t pad;
};

// scan kernels (kernels_scan.hip)


// hash kernels (kernels_hash.hip)
constexpr int MAX_KW = 2 * MAX_KEYS + 1;
struct KeySpec {
  int32_t n_keys;
  int32_t key_reg[MAX_KEYS];
  int32_t key_wide[MAX_KEYS];  // 1: key needs both 64-bit halves (Decimal128, packed Utf8); 0: hi is the sign extension
  int32_t null_word;           // 1: append the key null-mask as a key word (group-by keys, null_equals_null joins)
  int32_t key_words;           // total u64 key words per slot
  int32_t word_reg[MAX_KW];    // key word q comes from register word_reg[q] ...
  int32_t word_half[MAX_KW];   // ... half 0 = lo, 1 = hi, 2 = the key null mask
  // Hash aggregate only.  state_key = 1: the whole key, NULL flags included, packs into one word of at most 62 bits and lives in the
  // slot's state word (HashTable below): key k is the low sk_bits[k] bits of its register (its type's width; sk_signed[k]: sign-extended
  // on the way out) and, when sk_null[k], one bit above them that says NULL; the fields follow each other from bit 0.
  int32_t state_key;
  int32_t sk_bits[MAX_KEYS], sk_signed[MAX_KEYS], sk_null[MAX_KEYS];
};
// Open-addressing table, linear probing, one slot = slot_words u64:
//   [0]            low 32 bits state (0 empty, 1 locked, else hash tag|2); high 32 bits payload (join: chain head row)
//   [1..key_words] key words
//   [1+key_words..] aggregate cells, two u64 (lo,hi) per accumulator
// A hash aggregate whose key fits the state word (KeySpec::state_key) has key_words = 0 and slots of 1 + 2 * n_accs words:
//   [0]            0 empty, else (packed key << 2) | 2 -- one compare-and-swap claims the slot and publishes the key
//   [1..]          aggregate cells
// Join tables over ONE narrow (<= 64-bit) integer key whose values span a bounded range use direct addressing instead:
// dense[key - dense_min] = chain head row (0xFFFFFFFF = no such key), dense_range entries.  One load per probe, no probing
// loop, and a probe side that is clustered / sorted by the key (fact-table foreign keys) walks the table sequentially.
struct HashTable {
  u64* slots;
  u64 n_slots;         // power of two
  int32_t slot_words;
  int32_t key_words;
  uint32_t* dense;     // nullptr = open addressing (slots)
  i64 dense_min;
  u64 dense_range;
  // Sparse domains (few keys in a wide range: a filtered dimension table) add a presence bitmap, one bit per key value, and leave
  // the row array uninitialised: only bits are cleared at build time (range / 8 bytes instead of 4 x range), a probe that misses
  // touches the bitmap alone (32 x denser than the array: L2- or Infinity-Cache-resident), a hit reads bitmap + array.
  // Only for unique build keys (duplicates need the chain heads initialised).  nullptr = the array alone (NIL = no key).
  uint32_t* dense_bits;
};
// Membership in the direct-addressed table, in three steps that stay separate because callers with several rows in flight issue every
// load before they test any: the index of a key (false: outside the table), the presence word of an index, the index's bit in that word.
__device__ __forceinline__ bool dense_index(const HashTable& T, const u64 key, u64& idx) { idx = key - (u64)T.dense_min; return idx < T.dense_range; }
__device__ __forceinline__ uint32_t dense_presence_word(const uint32_t* __restrict__ dense_bits, const u64 idx) { return dense_bits[idx >> 5]; }
__device__ __forceinline__ bool dense_present(const uint32_t word, const u64 idx) { return (word >> (idx & 31)) & 1u; }
// chain fusion: the build kernel first looks its rows up in ANOTHER join's table (kernels_hash.hip k_join_build_body)
struct SemiProbe { HashTable T; KeySpec K; int32_t null_eq; int32_t on; uint32_t* hit_out; u64* rows_out; };
enum JoinType : int32_t { JT_INNER = 0, JT_LEFT = 1, JT_RIGHT = 2, JT_FULL = 3, JT_LEFT_SEMI = 4, JT_LEFT_ANTI = 5, JT_RIGHT_SEMI = 6, JT_RIGHT_ANTI = 7 };

// build: payload = payload_via ? via[payload_via-1][pos] : pos.  next == nullptr => unique keys only (FLAG_DUP_BUILD_KEY on a duplicate)

// ----- accumulator algebra: what an AccKind IS, stated once for every aggregate kernel (k_agg_tiny + k_agg_tiny_merge, k_agg_hash,
// k_agg_lds, k_agg_bucket).  A cell is two u64 words (lo, hi): SUM is a 128-bit integer, COUNT / MIN / MAX a 64-bit one in lo, the
// float kinds a double's bit pattern in lo, the bitwise kinds (BAND / BOR / BXOR) the low 64 bits of the argument's pattern in lo, hi 0
// (the result projection re-extends them to the argument's type).  A new kind is added here; a new aggregate kernel is a loop around these helpers.
// (k_agg_tiny's per-row accumulate into lane-private slots is its own algorithm and stays in kernels_scan.hip.)
constexpr uint32_t NIL = 0xFFFFFFFFu;      // no row / no slot
__device__ __forceinline__ uint32_t tag_of(u64 h) { return (uint32_t)(h >> 32) | 2u; }

// identity of a cell, word `half` (this and acc_combine are plain arithmetic: host code may call them too, tests/window_scan_host.cpp does)
__host__ __device__ __forceinline__ u64 acc_identity(const int kind, const int half) {
  switch (kind) {
    case ACC_MIN: return half ? 0 : 0x7FFFFFFFFFFFFFFFull;
    case ACC_MAX: return half ? ~0ull : 0x8000000000000000ull;
    case ACC_FMIN: return half ? 0 : 0x7FF0000000000000ull;  // +inf
    case ACC_FMAX: return half ? 0 : 0xFFF0000000000000ull;  // -inf
    case ACC_BAND: return half ? 0 : ~0ull;
    default: return 0;      // (BOR, BXOR: 0)
  }
}
// initial value of word w of a table slot whose cells start at word cell0: state, hash and key words are 0
__device__ __forceinline__ u64 slot_word_identity(const AggSpec& A, const int w, const int cell0) {
  const int a = (w - cell0) >> 1;
  return (w >= cell0 && a < A.n_accs) ? acc_identity(A.acc_kind[a], (w - cell0) & 1) : 0;
}
// a block of `nthreads` empties its LDS table
__device__ __forceinline__ void lds_table_init(u64* slots, const uint32_t cap, const int slot_words, const int cell0, const AggSpec& A, const uint32_t nthreads) {
  for (uint32_t i = threadIdx.x; i < cap * (uint32_t)slot_words; i += nthreads) slots[i] = slot_word_identity(A, (int)(i % (uint32_t)slot_words), cell0);
}
// What accumulator a takes from the current row: its argument register (COUNT and COUNT(*): 1 -- a count is a sum of ones).
// false: the row does not contribute (the argument is NULL).
__device__ __forceinline__ bool acc_operand(const AggSpec& A, const int a, GPUQ_REGS_CPARAM, u64& vlo, u64& vhi) {
  const int kind = A.acc_kind[a];
  vlo = 1; vhi = 0;
  if (kind == ACC_COUNT_STAR) return true;
  const int r = __builtin_amdgcn_readfirstlane(A.acc_reg[a]);
  if (kind != ACC_COUNT) { vlo = rlo[r]; vhi = rhi[r]; }
  return !((rnulls >> r) & 1);
}
// MIN / MAX keep 64 bits: an operand outside int64 has to be refused (FLAG_WIDE_MINMAX), never folded
__device__ __forceinline__ bool acc_wide_minmax(const int kind, const u64 vlo, const u64 vhi) {
  return (kind == ACC_MIN || kind == ACC_MAX) && (i64)vhi != ((i64)vlo >> 63);
}
// partial (olo, ohi) combined into partial (lo, hi), no atomics (registers, or memory one thread owns)
__host__ __device__ __forceinline__ void acc_combine(const int kind, u64& lo, u64& hi, const u64 olo, const u64 ohi) {
  switch (kind) {
    case ACC_SUM: case ACC_COUNT: case ACC_COUNT_STAR: { const u64 s = lo + olo; hi = hi + ohi + (s < lo ? 1 : 0); lo = s; break; }
    case ACC_MIN: if ((i64)olo < (i64)lo) lo = olo; break;
    case ACC_MAX: if ((i64)olo > (i64)lo) lo = olo; break;
    case ACC_FSUM: lo = __builtin_bit_cast(u64, __builtin_bit_cast(double, lo) + __builtin_bit_cast(double, olo)); break;
    case ACC_FMIN: if (f64_total_key(olo) < f64_total_key(lo)) lo = olo; break;
    case ACC_FMAX: if (f64_total_key(olo) > f64_total_key(lo)) lo = olo; break;
    case ACC_BAND: lo &= olo; break;
    case ACC_BOR: lo |= olo; break;
    case ACC_BXOR: lo ^= olo; break;
    default: break;
  }
}
// (vlo, vhi) folded into a cell other threads fold into too: SCOPE = __HIP_MEMORY_SCOPE_AGENT for a cell in device memory,
// __HIP_MEMORY_SCOPE_WORKGROUP for one in LDS.  Integer adds commute, so SUM's carry can trail; adding zero is skipped, and so is
// a bitwise operand that is its kind's identity (the untouched cells of a flushed LDS table).
template <int SCOPE>
__device__ __forceinline__ void acc_fold(u64* c, const int kind, const u64 vlo, const u64 vhi) {
  switch (kind) {
    case ACC_COUNT: case ACC_COUNT_STAR: if (vlo) __hip_atomic_fetch_add(c, vlo, __ATOMIC_RELAXED, SCOPE); break;
    case ACC_SUM: {
      if (!(vlo | vhi)) break;
      const u64 old = __hip_atomic_fetch_add(c, vlo, __ATOMIC_RELAXED, SCOPE);
      const u64 carry = (old + vlo < old) ? 1 : 0;
      if (vhi + carry) __hip_atomic_fetch_add(c + 1, vhi + carry, __ATOMIC_RELAXED, SCOPE);
      break;
    }
    case ACC_MIN: __hip_atomic_fetch_min((i64*)c, (i64)vlo, __ATOMIC_RELAXED, SCOPE); break;
    case ACC_MAX: __hip_atomic_fetch_max((i64*)c, (i64)vlo, __ATOMIC_RELAXED, SCOPE); break;
    case ACC_FSUM: unsafeAtomicAdd((double*)c, __longlong_as_double((i64)vlo)); break;      // (a CAS loop or a fetch_add cost the same: measured)
    case ACC_FMIN: case ACC_FMAX: {
      // total-order min/max through a CAS loop on the bit pattern
      u64 cur = __hip_atomic_load(c, __ATOMIC_RELAXED, SCOPE);
      for (;;) {
        const bool better = (kind == ACC_FMIN) ? (f64_total_key(vlo) < f64_total_key(cur)) : (f64_total_key(vlo) > f64_total_key(cur));
        if (!better || __hip_atomic_compare_exchange_strong(c, &cur, vlo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE)) break;
      }
      break;
    }
    case ACC_BAND: if (~vlo) __hip_atomic_fetch_and(c, vlo, __ATOMIC_RELAXED, SCOPE); break;
    case ACC_BOR: if (vlo) __hip_atomic_fetch_or(c, vlo, __ATOMIC_RELAXED, SCOPE); break;
    case ACC_BXOR: if (vlo) __hip_atomic_fetch_xor(c, vlo, __ATOMIC_RELAXED, SCOPE); break;
    default: break;
  }
}
// high word of a finished cell as the result carries it: MIN / MAX are sign-extended to 128 bits (the bitwise kinds never write hi: 0)
__device__ __forceinline__ u64 acc_result_hi(const int kind, const u64 lo, const u64 hi) {
  return (kind == ACC_MIN || kind == ACC_MAX) ? (u64)((i64)lo >> 63) : hi;
}

// ----- aggregate over key-clustered input ("runs", kernels_hash.hip k_agg_runs_count / k_agg_runs_write): the head / output-row arithmetic,
// plain functions so that a host program can call them too.  Rows are looked at 64 at a time (one wave-word); a key is the packed
// state-word key (< 2^62) and travels as key + 1 where 0 has to mean "no row".
//   active      the row exists and passes the fused predicate
//   below       row pos - 1 is active (lane 0: the last row of the word before)
//   prev_p1     key + 1 of the nearest active row before this one, as far back as the wave's segment reaches (0: none there)
// A row starts a run (is a head) when it is active and does not continue the run of the row directly below it.
__host__ __device__ inline bool runs_head(const bool active, const bool below, const u64 prev_p1, const u64 key) { return active && !(below && prev_p1 == key + 1); }
// A head must exceed every key before it; rows before it are non-decreasing unless an earlier head already failed this test, so the
// nearest active row stands for all of them.  (Equal keys around an inactive row are two runs of one key: out of order, by this rule.)
__host__ __device__ inline bool runs_out_of_order(const bool head, const u64 prev_p1, const u64 key) { return head && prev_p1 != 0 && key + 1 <= prev_p1; }
// the lanes 0..lane of a 64-bit lane mask
__host__ __device__ inline u64 runs_lanes_le(const u64 mask, const int lane) { return mask & (~0ull >> (63 - lane)); }
// Output row of the active row in `lane`: (heads up to and including the row) - 1 = heads of the earlier segments (base) + of this
// segment's earlier words + of this word's lanes 0..lane, - 1.  A row that continues a run from before the word gets that run's row.
__host__ __device__ inline uint32_t runs_out_row(const uint32_t base, const uint32_t heads_before_word, const u64 head_mask, const int lane) {
  return base + heads_before_word + (uint32_t)__builtin_popcountll(runs_lanes_le(head_mask, lane)) - 1u;
}
// A piece is a run's share of one word; it ends in `tail_lane` and starts in the nearest lane at or below it that does not continue
// the lane below (start_mask: those lanes; lane 0 always is one).  It is the whole run -- interior, its cells are stored plainly --
// when it starts with a head and ends before lane 63 (what follows is then another run, an inactive row or the end of the input).
// Any other piece may share its run with a neighbouring word and folds into the run's cells atomically.
__host__ __device__ inline bool runs_piece_interior(const u64 head_mask, const u64 start_mask, const int tail_lane) {
  const int start = 63 - __builtin_clzll(runs_lanes_le(start_mask, tail_lane) | 1ull);
  return tail_lane < 63 && ((head_mask >> start) & 1ull);
}
// How the rows are dealt out: wave-segment s (one wave of a block, segments of a block are neighbours) owns the 64-row words
// [s * wps, (s + 1) * wps); per segment the count kernel leaves its number of heads (scanned into the segment's first output row),
// key + 1 of its last active row and of the one head it could not test (nothing active before it inside the segment): 0 = none.
struct RunsGeom { i64 wps; int32_t nsegs; int32_t pad; uint32_t* counts; u64* seg_last; u64* seg_first; };

// LDS open-addressing table of one block: slot = [state (0 empty, 1 being written, else tag), hash if STORE_HASH, key words, cells].
// Finds the key's slot or claims one, starting at slot `start & (cap - 1)` and giving up (NIL) after max_probes occupied slots.
template <bool STORE_HASH>
__device__ __forceinline__ uint32_t lds_find_or_insert(u64* slots, const uint32_t cap, const int slot_words, const int key_words, const u64 (&kw)[MAX_KW], const u64 h,
                                                       const uint32_t start, const uint32_t max_probes) {
  constexpr int key0 = STORE_HASH ? 2 : 1;
  const uint32_t mask = cap - 1;
  uint32_t s = start & mask;
  const u64 tag = (u64)tag_of(h);
  for (uint32_t probes = 0; probes < max_probes;) {
    u64* slot = slots + (size_t)s * slot_words;
    u64 st = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (st == 0) {
      u64 expected = 0;
      if (__hip_atomic_compare_exchange_strong(slot, &expected, 1ull, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
        if (STORE_HASH) __hip_atomic_store(slot + 1, h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
        for (int q = 0; q < MAX_KW; ++q) if (q < key_words) __hip_atomic_store(slot + key0 + q, kw[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __hip_atomic_store(slot, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return s;
      }
      st = expected;
    }
    if (st == 1) continue;                           // being published by another lane: look again
    if (st == tag) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
      bool eq = !STORE_HASH || __hip_atomic_load(slot + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == h;
#pragma unroll
      for (int q = 0; q < MAX_KW; ++q) if (q < key_words) eq = eq && (__hip_atomic_load(slot + key0 + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == kw[q]);
      if (eq) return s;
    }
    s = (s + 1) & mask; ++probes;
  }
  return NIL;
}

// a finished table slot ([state, key words, cells from word cell0]) written as row g of the result
__device__ __forceinline__ void emit_group(const u64* slot, const int cell0, const KeySpec& K, const AggSpec& A, const AggOut& out, const uint32_t g) {
  const int kstride = K.n_keys > 0 ? K.n_keys : 1;
  int w = 0;
  for (int k = 0; k < K.n_keys; ++k) {
    const u64 lo = slot[1 + w]; ++w;
    u64 hi = (u64)((i64)lo >> 63);
    if (K.key_wide[k]) { hi = slot[1 + w]; ++w; }
    out.keys[((size_t)g * kstride + k) * 2] = lo;
    out.keys[((size_t)g * kstride + k) * 2 + 1] = hi;
  }
  out.key_nulls[g] = K.null_word ? (uint32_t)slot[1 + w] : 0u;
  for (int a = 0; a < A.n_accs; ++a) {
    const u64 lo = slot[cell0 + 2 * a];
    out.cells[((size_t)g * A.n_accs + a) * 2] = lo;
    out.cells[((size_t)g * A.n_accs + a) * 2 + 1] = acc_result_hi(A.acc_kind[a], lo, slot[cell0 + 2 * a + 1]);
  }
}

// sort / partition (kernels_sort.hip)
constexpr int MAX_SORT_KEYS = 4;
struct SortSpec {
  int32_t n_keys;
  int32_t reg[MAX_SORT_KEYS];
  int32_t desc[MAX_SORT_KEYS];
  int32_t nulls_first[MAX_SORT_KEYS];
  int32_t kind[MAX_SORT_KEYS];     // 0 integer/decimal/date, 1 float64 (total order), 2 packed Utf8
};
constexpr int SORT_MAX_PASSES = 16;  // 8-bit digits of a composite key of up to 128 bits
struct SortPack {                   // computed on the host from the per-key min/max
  u64 base_lo[MAX_SORT_KEYS], base_hi[MAX_SORT_KEYS];   // min (ASC) or max (DESC) in the ordered view
  int32_t shift[MAX_SORT_KEYS];     // bit position of the key's field in the composite
  int32_t null_bit[MAX_SORT_KEYS];  // bit (inside the field) of the null flag, -1 = none
  int32_t rshift[MAX_SORT_KEYS];    // packed Utf8: drop the length byte and the bytes beyond the longest string
  int32_t len_bits[MAX_SORT_KEYS];  // packed Utf8: 4 when the length goes below the bytes (a value of the column ends in 0x00: sort_key_op.h), else 0
  int32_t vbits[MAX_SORT_KEYS];     // width of the value field (without the null flag)
  int32_t check;                    // 1: the layout was GUESSED from a sample -- the pack kernel verifies every row against it and raises
                                    // hist[SORT_MAX_PASSES * 256] when a value falls outside its field or a NULL meets a key without a null bit
                                    // 2: the same, reported as FLAG_SORT_LAYOUT in the operator's status word (deferred execution: nobody reads hist)
  int32_t total_bits;               // width of the composite key: padding records (rows beyond a device-side row count) hold all ones in it
};

// aggregate post-processing (kernels_scan.hip): AoS result -> one (lo,hi) column per key / accumulator
struct AggSoA {
  ulonglong2* key_col[MAX_KEYS]; u64* key_valid[MAX_KEYS];   // validity words, bit g of word g/64
  ulonglong2* acc_col[MAX_ACCS];
};

// generator (kernels_gen.hip)


// deferred execution: up to 64 device words gathered into one contiguous block (gpuq_ops_settle)
struct GatherWords { int32_t n; int32_t pad; const u64* src[64]; };

// ----- sinks: the kernels that evaluate a compiled expression program.  Each exists as the AOT template k_X<MAXC> and as a
// hiprtc-specialised gpuq_jit_entry (the same .hip text under GPUQ_JIT_KERNEL == id).  The ids are ABI (gpuq_compile_jit_source,
// gpuq_op_jit_source); GPUQ_SINKS below gives each its source file and entry-point name.
#define GPUQ_SINK_FILTER_BITMAP 1
#define GPUQ_SINK_PROJECT 2
#define GPUQ_SINK_AGG_TINY 3
#define GPUQ_SINK_AGG_HASH 4
#define GPUQ_SINK_JOIN_BUILD 5
#define GPUQ_SINK_JOIN_PROBE 6
#define GPUQ_SINK_JOIN_PROBE_UNIQUE 7
#define GPUQ_SINK_SORT_MINMAX 8
#define GPUQ_SINK_SORT_PACK 9
#define GPUQ_SINK_PART_PID 10
#define GPUQ_SINK_AGG_BUCKET_ID 11
#define GPUQ_SINK_AGG_BUCKET 12
#define GPUQ_SINK_AGG_LDS 13
#define GPUQ_SINK_JOIN_KEYRANGE 14
#define GPUQ_SINK_RJ_PACK 15
#define GPUQ_SINK_AGG_RUNS_COUNT 16
#define GPUQ_SINK_AGG_RUNS_WRITE 17

#ifndef GPUQ_JIT
// ---- host launch interface (AOT build only)
struct SinkInfo { int id; const char* file; const char* entry; };
constexpr SinkInfo GPUQ_SINKS[] = {
    {GPUQ_SINK_FILTER_BITMAP, "kernels_scan.hip", "gpuq_jit_filter_bitmap"},
    {GPUQ_SINK_PROJECT, "kernels_scan.hip", "gpuq_jit_project"},
    {GPUQ_SINK_AGG_TINY, "kernels_scan.hip", "gpuq_jit_agg_tiny"},
    {GPUQ_SINK_AGG_HASH, "kernels_hash.hip", "gpuq_jit_agg_hash"},
    {GPUQ_SINK_JOIN_BUILD, "kernels_hash.hip", "gpuq_jit_join_build"},
    {GPUQ_SINK_JOIN_PROBE, "kernels_hash.hip", "gpuq_jit_join_probe"},
    {GPUQ_SINK_JOIN_PROBE_UNIQUE, "kernels_hash.hip", "gpuq_jit_join_probe_unique"},
    {GPUQ_SINK_SORT_MINMAX, "kernels_sort.hip", "gpuq_jit_sort_minmax"},
    {GPUQ_SINK_SORT_PACK, "kernels_sort.hip", "gpuq_jit_sort_pack"},
    {GPUQ_SINK_PART_PID, "kernels_sort.hip", "gpuq_jit_part_pid"},
    {GPUQ_SINK_AGG_BUCKET_ID, "kernels_hash.hip", "gpuq_jit_agg_bucket_id"},
    {GPUQ_SINK_AGG_BUCKET, "kernels_hash.hip", "gpuq_jit_agg_bucket"},
    {GPUQ_SINK_AGG_LDS, "kernels_hash.hip", "gpuq_jit_agg_lds"},
    {GPUQ_SINK_JOIN_KEYRANGE, "kernels_hash.hip", "gpuq_jit_join_keyrange"},
    {GPUQ_SINK_RJ_PACK, "kernels_hash.hip", "gpuq_jit_rj_pack"},
    {GPUQ_SINK_AGG_RUNS_COUNT, "kernels_hash.hip", "gpuq_jit_agg_runs_count"},
    {GPUQ_SINK_AGG_RUNS_WRITE, "kernels_hash.hip", "gpuq_jit_agg_runs_write"},
};
// The launchers of the sinks take `jit_fn`: the specialised function to run (capi.cpp's SinkJit resolves it), or nullptr for the AOT kernel.
void launch_gather_words(hipStream_t s, const GatherWords& g, u64* out);
void set_num_cus(int n);
int num_cus();
// blocks for n rows at one 64-row word per wave, at least one, capped at blocks_per_cu per compute unit
int grid_for_words(i64 n, int waves_per_block, int blocks_per_cu);
void launch_filter_bitmap(hipStream_t s, void* jit_fn, const DevProgram& P, i64 n, u64* bitmap, uint32_t* block_counts, int nblocks, i64 words_per_block);
void launch_scan_block_counts(hipStream_t s, uint32_t* block_counts, int nblocks, u64* total_out);
void launch_compact(hipStream_t s, const u64* bitmap, const uint32_t* block_offsets, int nblocks, i64 words_per_block, i64 n,
                    const uint32_t* sel_in, uint32_t* sel_out);
void launch_project(hipStream_t s, void* jit_fn, const DevProgram& P, i64 n, const OutSpec& O);
int agg_tiny_max_groups(int n_accs);
size_t agg_tiny_workspace_bytes(int gmax, int n_keys, int n_accs, int* nblocks_out);
void launch_agg_tiny(hipStream_t s, void* jit_fn, const DevProgram& P, i64 n, const AggSpec& A, int gmax, void* workspace);
void launch_agg_tiny_merge(hipStream_t s, const DevProgram& P, i64 n, const AggSpec& A, int gmax, void* workspace, const AggOut& out);
void launch_ht_init(hipStream_t s, const HashTable& T, const AggSpec* A);
void launch_agg_hash(hipStream_t s, void* jit_fn, const DevProgram& P, i64 n, const KeySpec& K, const AggSpec& A, const HashTable& T);
void launch_key_sample(hipStream_t s, const DevProgram& P, i64 n, const KeySpec& K, i64 stride, i64 nsample, uint32_t* bitmap, u64 nbits, unsigned long long* passed);
// origins_dev: device memory; first_row: MAX_ORIGINS device words of scratch (the lowest row that takes part, per origin)
void launch_agg_origin_pick(hipStream_t s, const DevProgram& pick, i64 n, const OriginPick* origins_dev, unsigned int* first_row);
uint32_t agg_lds_slots(const HashTable& T);
int agg_lds_grid(i64 n);
void launch_agg_lds(hipStream_t s, void* jit_fn, const DevProgram& P, i64 n, const KeySpec& K, const AggSpec& A, const HashTable& T, u64* fstage, int n_fsum);
void launch_agg_bucket_id(hipStream_t s, void* jit_fn, const DevProgram& P, i64 n, const KeySpec& K, u64 bucket_mask, u64* bid, uint32_t* ids);
void launch_bucket_bounds(hipStream_t s, const u64* sorted_bid, i64 n, u64 nbuckets, uint32_t* bounds, int shift);
void launch_agg_bucket(hipStream_t s, void* jit_fn, const DevProgram& P, const KeySpec& K, const AggSpec& A, const uint32_t* ids, const uint32_t* bounds, uint32_t nbuckets,
                       uint32_t cap, int slot_words, const AggOut& out);
// soa: state-word keys only (K.state_key): the groups are written as result columns directly (out gives the capacity and the count word)
void launch_agg_hash_extract(hipStream_t s, const KeySpec& K, const AggSpec& A, const HashTable& T, const AggOut& out, uint32_t* flags, const AggSoA* soa = nullptr);
// aggregate over key-clustered input (state-word keys): the segments of `n` rows (arrays not set), then the launches in their order --
// heads per segment; one block that scans the counts (in place; n_groups_out: the group count word and its pad) and tests the order
// across segments (FLAG_AGG_RUNS); one result row per run, written into columns whose accumulator cells hold their identities (cap rows)
RunsGeom agg_runs_geometry(i64 n);
void launch_agg_runs_count(hipStream_t s, void* jit_fn, const DevProgram& P, i64 n, const KeySpec& K, const RunsGeom& G);
void launch_agg_runs_scan_order(hipStream_t s, const RunsGeom& G, u64* n_groups_out, uint32_t* flags);
void launch_agg_runs_write(hipStream_t s, void* jit_fn, const DevProgram& P, i64 n, const KeySpec& K, const AggSpec& A, const RunsGeom& G, const AggSoA& soa, uint32_t cap);
void launch_fill_cells(hipStream_t s, ulonglong2* cells, i64 n, u64 lo, u64 hi);
// false: no interpreter kernel for this shape (chain fusion over more than 8 input columns)
bool launch_join_build(hipStream_t s, void* jit_fn, const DevProgram& P, i64 n, const KeySpec& K, const HashTable& T, uint32_t* next, uint32_t* present,
                       int payload_via, int null_equals_null, const SemiProbe* semi = nullptr);
// key range of the rows a join build would insert: out = {min (i64), max (i64), count (u64)}, pre-set by the caller to {INT64_MAX, INT64_MIN, 0}
void launch_join_keyrange(hipStream_t s, void* jit_fn, const DevProgram& P, i64 n, const KeySpec& K, int null_equals_null, u64* out, i64 wstep = 1);   // wstep > 1: every wstep-th 64-row word
// unique build keys: every wave owns `wpw` consecutive 64-row words (segment g = words [g*wpw, (g+1)*wpw)) and writes its pairs, in probe
// order, to seg_build / seg_probe starting at row g*wpw*64; seg_counts[g] = pairs of the segment.  launch_copy_segments then moves
// the segments to their final places (seg_counts already scanned to exclusive offsets).
void launch_join_probe_unique(hipStream_t s, void* jit_fn, const DevProgram& P, i64 n, const KeySpec& K, const HashTable& T, int join_type, int null_equals_null, int payload_via,
                              uint32_t* seg_build, uint32_t* seg_probe, uint32_t* seg_counts, int nsegs, i64 wpw, uint32_t* visited);
void launch_copy_segments(hipStream_t s, const uint32_t* seg_build, const uint32_t* seg_probe, const uint32_t* seg_offsets, int nsegs, i64 wpw, i64 n,
                          const u64* total, uint32_t* out_build, uint32_t* out_probe, u64 out_cap, uint32_t* flags);
// partitioned probe over a direct-addressed table (kernels_hash.hip): records = (table index << 32 | probe row), one scatter pass on
// the high index bits; offsets of the dropped-rows digit (hist[nparts * nblocks]) = number of live records after the scan
void launch_join_locality(hipStream_t s, const DevProgram& P, i64 n, const KeySpec& K, const HashTable& T, i64 stride, i64 nsample, u64* out);
struct RjGeomHost { uint32_t nparts, shift; i64 tile; int32_t nblocks; };
void rj_geometry(i64 n, u64 range, int slice_log2, RjGeomHost* g);
size_t rj_hist_entries(const RjGeomHost& g);
void launch_rj_partition(hipStream_t s, void* jit_fn, const DevProgram& P, i64 n, const KeySpec& K, const HashTable& T, int payload_via, const RjGeomHost& g,
                         u64* rec, u64* rec_out, int32_t* hist, void* scan_ws, size_t scan_ws_bytes);
int rj_probe_geometry(i64 n, i64* wpw_out);
void launch_rj_probe(hipStream_t s, const u64* rec, const int32_t* n_live, const HashTable& T, int join_type, uint32_t* seg_build, uint32_t* seg_probe,
                     uint32_t* seg_counts, int nblocks, i64 wpw);
void launch_bitmap_select(hipStream_t s, const u64* present, const u64* visited, int matched, i64 nwords, i64 n, u64* bitmap,
                          uint32_t* block_counts, int nblocks, i64 wpb);
void launch_join_probe(hipStream_t s, void* jit_fn, const DevProgram& P, i64 n, const KeySpec& K, const HashTable& T, const uint32_t* next,
                       int join_type, int payload_via, int null_equals_null, uint32_t* out_build, uint32_t* out_probe,
                       u64 out_cap, u64* out_count, uint32_t* visited);
int sort_minmax_blocks(i64 n);
void launch_sort_minmax(hipStream_t s, void* jit_fn, const DevProgram& P, i64 n, const SortSpec& S, u64* out, int nblocks, i64 wstep = 1);   // wstep > 1: every wstep-th 64-row word only (a sample)
int sort_max_passes();
void launch_sort_pack(hipStream_t s, void* jit_fn, const DevProgram& P, i64 n, const SortSpec& S, const SortPack& K, u64* key_lo, u64* key_hi, uint32_t* ids, u64* hist, int hist_passes);
void launch_part_pid(hipStream_t s, void* jit_fn, const DevProgram& P, i64 n, const KeySpec& K, uint32_t nparts, u64* pid_out, uint32_t* ids);
void launch_part_offsets(hipStream_t s, const u64* pid, i64 n, uint32_t nparts, uint32_t* counts_ws, u64* offsets_out, int shift);
void launch_counts_to_ghist(hipStream_t s, const uint32_t* counts, uint32_t np, u64* ghist);
void launch_gather_u64(hipStream_t s, const u64* src, const uint32_t* idx, i64 n, u64* dst);
int sort_small_max();
int sort_direct_max();
void launch_sort_direct(hipStream_t s, const DevProgram& P, i64 n, const SortSpec& S, uint32_t* perm);
void launch_sort_small(hipStream_t s, const u64* klo, const u64* khi, const uint32_t* ids, i64 n, uint32_t* out);
size_t onesweep_ws_bytes(i64 n);
int onesweep_max_passes();
size_t merge_splits_entries(i64 max_len, int n_pairs);
void launch_merge_pairs(hipStream_t s, const u64* klo, const u64* khi, const uint32_t* ids, const i64* pairs, int n_pairs, i64 max_len, i64* splits,
                        u64* klo_out, u64* khi_out, uint32_t* ids_out);
void launch_radix_ghist(hipStream_t s, const u64* keys, i64 n, int shift0, int npasses, u64* ghist);
void launch_radix_ghist_scan(hipStream_t s, u64* ghist, int npasses);      // counts -> bases, all passes in one launch
// np stable 8-bit passes from bit shift0 (kernels_sort.hip); (keys, vals) <-> (keys2, vals2) change roles pass by pass
void launch_onesweep_passes(hipStream_t s, u64*& keys, uint32_t*& vals, u64*& keys2, uint32_t*& vals2, i64 n, int shift0, int np, const u64* gexcl,
                            void* ws, size_t ws_bytes, uint32_t* final_vals_out, int final_mode /* 0 records, 1 row ids only, 2 packed records + row ids */);
void launch_agg_emit(hipStream_t s, const AggOut& raw, int n_keys, int n_accs, uint32_t n_groups, const AggSoA& soa, const uint32_t* n_groups_dev = nullptr);
void launch_concat_bitmap(hipStream_t s, u64* dst, i64 dst_bit_offset, const uint8_t* src, i64 src_bit_offset, i64 n_bits);
void launch_unpack_utf8_lengths(hipStream_t s, const ulonglong2* packed, i64 n, int32_t* lens_out, uint32_t* too_long);
constexpr int LIKE_MAX_TOKENS = 256;
constexpr int LIKE_MAX_SEGS = 8;
struct LikePattern {
  int32_t n; int32_t regex_mode; uint16_t tok[LIKE_MAX_TOKENS];     // 0..255 literal byte, 256 '_', 257 '%'
  // the pattern as literal segments between '%' (n_seg < 0: it holds '_' or too many segments: the general matcher runs)
  int32_t n_seg, anchored_start, anchored_end, pad;
  int32_t seg_off[LIKE_MAX_SEGS], seg_len[LIKE_MAX_SEGS];
  unsigned long long seg_first8[LIKE_MAX_SEGS], seg_mask8[LIKE_MAX_SEGS];
};
void launch_like_utf8(hipStream_t s, const uint8_t* data, const int32_t* offsets, const uint8_t* validity, const uint32_t* idx, i64 n, const LikePattern& pat, int negated,
                      u64* bits_out, u64* valid_out);
void launch_mark_rows(hipStream_t s, const uint32_t* rows, i64 n, uint8_t* bitmap);
void launch_utf8_compare(hipStream_t s, const uint8_t* adata, const int32_t* aoffs, const uint8_t* avalid, const uint32_t* aidx, const uint8_t* bdata, const int32_t* boffs,
                         const uint8_t* bvalid, const uint32_t* bidx, int32_t blen, i64 n, int op, u64* bits_out, u64* valid_out);
void launch_sort_decode(hipStream_t s, const u64* recs, int rec_shift, i64 n, const SortPack& K, int desc, int nulls_first, int width, void* out, u64* valid_out);
void launch_cross_pairs(hipStream_t s, i64 n_left, i64 n_right, uint32_t* left_rows, uint32_t* right_rows);
void launch_offsets_rebase(hipStream_t s, const int32_t* src, i64 n, int32_t delta, int32_t* dst);
void launch_take_utf8_lengths(hipStream_t s, const int32_t* offsets, const uint8_t* validity, const uint32_t* idx, i64 n, int32_t* lens, u64* valid_out);
void launch_take_utf8_bytes(hipStream_t s, const uint8_t* data, const int32_t* offsets, const uint32_t* idx, i64 n, const int32_t* out_offsets, uint8_t* out, i64 total_bytes);
void launch_unpack_utf8_bytes(hipStream_t s, const ulonglong2* packed, i64 n, const int32_t* offsets, uint8_t* data_out);
void launch_exclusive_scan_i32(hipStream_t s, int32_t* data, i64 n, void* workspace, size_t ws_bytes);   // in place, n+1 entries out
size_t exclusive_scan_ws_bytes(i64 n);
// ----- LZ4 block codec (shuffle sink / source, kernels_lz4.hip)
struct Lz4Block { int64_t src; int64_t slot; int32_t len; int32_t pad; };     // compress: one <= 64 KiB input block and its worst-case output slot
constexpr int LZ4_UNIT_BLOCK = 0, LZ4_UNIT_STORED = 1, LZ4_UNIT_FRAME_BLOCKS = 2;
constexpr int LZ4_UNIT_BLOCK_CHECKSUM = 1;
struct Lz4Unit { int64_t src, dst, src_len, dst_len; int32_t mode, flags; };  // decompress: one independent block, or the blocks of one linked frame
constexpr int64_t LZ4_BLOCK_BYTES = 65536;
inline int64_t lz4_slot_bytes(int64_t len) { return ((len + len / 255 + 16) + 15) & ~(int64_t)15; }
void launch_lz4_compress(hipStream_t s, const uint8_t* src, uint8_t* slots, const Lz4Block* blocks, int n_blocks, int32_t* csize);
void launch_lz4_layout(hipStream_t s, const Lz4Block* blocks, const int32_t* csize, const int32_t* buf_first_block, int n_buffers, int64_t* buf_off, int64_t* buf_len,
                       int64_t* blk_dst);
void launch_lz4_pack(hipStream_t s, const uint8_t* src, const uint8_t* slots, const Lz4Block* blocks, int n_blocks, const int32_t* csize, const int32_t* blk_buffer,
                     const int32_t* buf_first_block, const int64_t* buf_off, const int64_t* buf_len, const int64_t* blk_dst, uint8_t* body);
void launch_lz4_decode(hipStream_t s, const uint8_t* src, int64_t src_bytes, uint8_t* dst, const Lz4Unit* units, int n_units, uint32_t* status);
struct Utf8Piece { const int32_t* tmp; int64_t n; int32_t* dst; int64_t at, dl, start, used; int32_t first, pad; };   // one batch of a Utf8 column (kernels_lz4.hip)
void launch_utf8_piece_starts(hipStream_t s, Utf8Piece* pieces, int n_pieces, uint32_t* gap);
void launch_utf8_piece_offsets(hipStream_t s, const Utf8Piece* pieces, int n_pieces, int64_t max_rows);
void launch_utf8_piece_validate(hipStream_t s, const Utf8Piece* pieces, int n_pieces, int64_t max_rows, uint32_t* status);
void launch_utf8_piece_compact(hipStream_t s, const Utf8Piece* pieces, int n_pieces, int64_t max_bytes, const uint8_t* from, uint8_t* to);
// ----- page / shuffle-block decompression (kernels_lz4.hip, kernels_zstd_dev.hip; host side: unpack_launch.cpp)
// One job: a Parquet page, or one block of a linked LZ4 frame.  [src, +src_len) -> [dst, +dst_len); the first `raw_prefix` bytes of both are
// copied verbatim (a v2 data page's levels) and `mode` says what the rest is:
//   UNPACK_STORED         the bytes themselves
//   UNPACK_SNAPPY         one raw Snappy stream
//   UNPACK_LZ4_BLOCK      one LZ4 block: an LZ4_RAW page, or a compressed block of a linked frame
//   UNPACK_LINKED_STORED  a stored block of a linked frame (its bytes can be the source of later blocks' matches)
//   UNPACK_ZSTD           ZSTD frames: the unpack kernels copy the prefix and leave the rest to launch_zstd_pages
// The four placement fields are read by the parallel decoder only.  s_off: the job's place in the resolve array (one 32-bit word per output
// byte behind the prefix, a multiple of 4); c_off: its place in the per-position arrays (one slot per compressed byte behind the prefix, + 1),
// the compressed jobs of a call back to back in job order.  Copies point into a FRAME: f_off is the frame's place in the resolve array and
// p_base the job's position in the frame's output (s_off = f_off + p_base); a page is its own frame (f_off = s_off, p_base = 0).
enum UnpackMode : int32_t { UNPACK_STORED = 0, UNPACK_SNAPPY = 1, UNPACK_LZ4_BLOCK = 2, UNPACK_LINKED_STORED = 3, UNPACK_ZSTD = 4 };
// the status word of these kernels (Snappy, LZ4, ZSTD): a job whose compressed bytes are damaged, and a ZSTD frame that names a dictionary,
// which the device does not decode (unsupported).  Callers treat every bit but the second as damage.
constexpr uint32_t UNPACKF_MALFORMED = 1u, UNPACKF_ZSTD_DICTIONARY = 8u;
struct UnpackJob { int64_t src, dst, src_len, dst_len, raw_prefix; int32_t mode, pad; int64_t s_off, c_off, f_off, p_base; };
// The serial decoder: one wave per job walks the elements and moves the bytes (stored, Snappy and -- prefix only -- ZSTD jobs)
void launch_unpack_pages(hipStream_t s, const uint8_t* src, uint8_t* dst, const UnpackJob* jobs, int n_jobs, uint32_t* status);
// `which`: indices of the UNPACK_ZSTD jobs, `scratch`: zstd_scratch_bytes(n) bytes
size_t zstd_scratch_bytes(int n_pages);
void launch_zstd_pages(hipStream_t s, const uint8_t* src, uint8_t* dst, const UnpackJob* jobs, const int32_t* which, int n, uint8_t* scratch, uint32_t* status);
// The parallel decoder (no serial element walk; every mode but UNPACK_ZSTD's body).  `jobs`: n HOST jobs with their placement fields set;
// everything else -- the block maps, the round counts, the scratch, what is zeroed, the launches -- follows from the jobs.  Synchronises the
// stream before it returns.  `X` is reused from call to call (the batches of one file); nothing in it outlives a call.
struct UnpackScratch { DevBuf jobs, resolve, blkmap, cmap, counts, jump_a, jump_b, olen, mark, scan; };
inline bool unpack_job_is_compressed(const UnpackJob& j) { return j.mode == UNPACK_SNAPPY || j.mode == UNPACK_LZ4_BLOCK; }
void unpack_pages_parallel(hipStream_t s, const uint8_t* src, uint8_t* dst, const UnpackJob* jobs, int n, UnpackScratch& X, uint32_t* status);
// its kernels, one launch each (unpack_launch.cpp holds the order and the scratch contract).  The maps name (job, first byte) per
// PJ_BLOCK_BYTES of output (blkmap) / of compressed positions (cmap); cnt_prev / cnt_cur: one zeroed word per job and round
constexpr int PJ_BLOCK_BYTES = 4096;
void launch_sn_head(hipStream_t s, const uint8_t* src, uint8_t* dst, const UnpackJob* jobs, int n_jobs, uint8_t* mark, uint32_t* resolve, uint32_t* status);
void launch_sn_next(hipStream_t s, const uint8_t* src, const uint2* cmap, int n_cblocks, const UnpackJob* jobs, uint32_t* jump, uint32_t* olen);
void launch_sn_mark(hipStream_t s, const uint2* cmap, int n_cblocks, const UnpackJob* jobs, const uint32_t* jump_in, uint32_t* jump_out, uint8_t* mark, const uint32_t* cnt_prev,
                    uint32_t* cnt_cur, bool first);
void launch_sn_lens(hipStream_t s, const uint2* cmap, int n_cblocks, const UnpackJob* jobs, const uint8_t* mark, const uint32_t* olen, int32_t* pos, uint32_t* status);
void launch_sn_fill(hipStream_t s, const uint8_t* src, const uint2* cmap, int n_cblocks, const UnpackJob* jobs, const uint8_t* mark, const int32_t* pos, uint32_t* resolve,
                    uint32_t* status);
void launch_snappy_round(hipStream_t s, uint32_t* resolve, const uint2* blkmap, int n_blocks, const UnpackJob* jobs, const uint32_t* cnt_prev, uint32_t* cnt_cur, bool first);
void launch_snappy_emit(hipStream_t s, const uint32_t* resolve, const uint2* blkmap, int n_blocks, const UnpackJob* jobs, uint8_t* dst, uint32_t* status);
void launch_utf8_code_rows(hipStream_t s, const void* codes, int width, const uint8_t* validity, i64 n, uint32_t* rows);      // width 8 (Int64) or 4 (UInt32)
void launch_utf8_sort_piece(hipStream_t s, const uint8_t* data, const int32_t* offsets, const uint8_t* validity, const uint32_t* idx, i64 n, int piece, void* out, u64* valid_out);
void launch_utf8_max_len(hipStream_t s, const int32_t* offsets, const uint8_t* validity, const uint32_t* idx, i64 n, int32_t* out);
void launch_utf8_intern(hipStream_t s, const uint8_t* ddata, const int32_t* doffs, const uint8_t* data, const int32_t* offsets, const uint8_t* validity, const uint32_t* idx, i64 n,
                        u64* table, u64 mask, int insert, i64* codes, u64* valid_out, uint32_t* flags);
void launch_popcount_bits(hipStream_t s, const uint8_t* bits, int64_t n_bits, unsigned long long* out);
// ----- segments of a key-sorted table and their medians (kernels_segment.hip)
constexpr int SEG_MAX_KEYS = 16;
struct SegKeys { int32_t n_keys; int32_t width[SEG_MAX_KEYS]; const void* data[SEG_MAX_KEYS]; const uint8_t* valid[SEG_MAX_KEYS]; };      // width: bytes per value, 0 = a bitmap (Boolean)
enum SegKind : int32_t { SEG_SINT = 0, SEG_UINT = 1, SEG_F32 = 2, SEG_F64 = 3 };      // how two middles are combined (width 16 is always a signed integer)
// scan: n + 1 words of scratch (the flags, then their exclusive scan); seg_id (n, or nullptr), starts (starts_cap + 1), n_groups as gpuq_segment_heads
void launch_segment_heads(hipStream_t s, const SegKeys& K, i64 n, int32_t* scan, void* scan_ws, size_t scan_ws_bytes, int32_t* seg_id, int32_t* starts, i64 starts_cap, u64* n_groups);
void launch_segment_median(hipStream_t s, const void* data, const uint8_t* valid, int width, int kind, const int32_t* starts, i64 n_groups, void* out, u64* out_valid);
// ----- window functions over a table ordered by (partition keys, order keys) (kernels_window.hip; window_scan_op.h has the scan's operator)
struct WinCol { const void* data; const uint8_t* valid; int32_t width; int32_t kind; };      // kind: a SegKind, how a value of 8 bytes or fewer is widened
constexpr uint32_t WINF_WIDE_MINMAX = 1u;      // the scan's status word: a MIN / MAX operand outside int64 (what FLAG_WIDE_MINMAX is to the aggregate operator)
size_t window_scan_ws_bytes(i64 n);            // one scan element per tile of 2,048 rows
// segmented inclusive scan of accumulator `kind` (an AccKind) over rows [0, n): seg_id (or nullptr: one partition) restarts it.  out_cells:
// cell_width 8 (the low word) or 16 bytes a row; out_count (i64 a row: the non-NULL values so far) and out_valid (bit = count > 0, whole
// 64-bit words) may be nullptr.
void launch_window_scan(hipStream_t s, const WinCol& c, const int32_t* seg_id, i64 n, int kind, void* ws, void* out_cells, int cell_width, i64* out_count, u64* out_valid,
                        uint32_t* flags);
void launch_window_rank(hipStream_t s, const int32_t* part_id, const int32_t* part_starts, const int32_t* peer_id, const int32_t* peer_starts, i64 n, u64* row_number, u64* rank,
                        u64* dense_rank);
// out[i] = data[i + delta] inside row i's partition, else dflt[i] (dflt_is_null, or dflt == nullptr: NULL); width 1, 2, 4, 8 or 16 bytes
void launch_window_shift(hipStream_t s, const void* data, const uint8_t* valid, int width, const int32_t* part_id, const int32_t* part_starts, i64 n, i64 delta, const void* dflt,
                         const uint8_t* dflt_valid, int dflt_is_null, void* out, u64* out_valid);
// Frames over the scan's running cells P (and counts C, or nullptr: never NULL): the value of row i is P[hi] - P[lo - 1] over
//   WFRAME_ROWS     lo = part_start, hi = i            WFRAME_RANGE    lo = part_start, hi = peer_end(i) - 1
//   WFRAME_SLIDING  lo = max(part_start, i - preceding) (preceding < 0: unbounded), hi = min(part_end - 1, i + following)
// with P[part_start - 1] = 0, stored as out_kind says: the cell in out_width bytes (out_f32: a double stored as a float), or an AVG --
// of an exact 128-bit integer sum in Float64, of a Float64 sum, of a decimal sum times mul, truncating.  out_valid: bit = count > 0.
enum WinFrameMode : int32_t { WFRAME_ROWS = 0, WFRAME_RANGE = 1, WFRAME_SLIDING = 2 };
enum WinOutKind : int32_t { WOUT_CELL = 0, WOUT_AVG_INT = 1, WOUT_AVG_F64 = 2, WOUT_AVG_DEC = 3 };
struct WinFrame {
  const void* cells; const i64* counts; const int32_t* part_id; const int32_t* part_starts; const int32_t* peer_id; const int32_t* peer_starts;
  i64 preceding, following; u64 mul_lo, mul_hi;
  int32_t cell_width, mode, out_kind, out_width, out_f32, pad;
  void* out; u64* out_valid;
};
void launch_window_frame(hipStream_t s, const WinFrame& F, i64 n);
// ----- DISTINCT aggregates over a column sorted inside its segments (kernels_distinct.hip; distinct_scan_op.h has the row rule)
// accumulator `kind` (ACC_COUNT, ACC_SUM, ACC_FSUM or ACC_BXOR) over the run heads of every segment of rows [0, n): out_cells[g] in cell_width
// bytes (1, 2, 4, 8: the low bytes of the cell; 16: both words) and out_count[g], either may be nullptr.  ws: window_scan_ws_bytes(n).  A
// segment without rows is met by no tile: the caller zeroes the outputs.
void launch_segment_distinct(hipStream_t s, const WinCol& c, const int32_t* starts, i64 n_groups, i64 n, int kind, void* ws, void* out_cells, int cell_width, i64* out_count);
void launch_segment_distinct_valid(hipStream_t s, const i64* count, i64 n_groups, u64* out_valid);      // bit g = count[g] > 0, whole 64-bit words
// ----- grouping sets: every row of a column n_sets times over, row-interleaved (kernels_grouping.hip; grouping_expand_op.h has the row rule)
// out row i * n_sets + s = row i, NULL (and zero) when bit s of null_sets is set or the row is NULL; width 1, 2, 4, 8 or 16 bytes, or 0: a
// Boolean column, data and out are bitmaps.  out_valid (whole 64-bit words, the last zero-padded) may be nullptr.  n * n_sets < 2^31.
void launch_grouping_expand(hipStream_t s, const void* data, const uint8_t* valid, int width, i64 n, int n_sets, u64 null_sets, void* out, u64* out_valid);
// ----- one HyperLogLog estimate per segment of a column (kernels_hll.hip; hll_estimate.h has the hash and the estimator)
enum HllKind : int32_t { HLL_SINT = 0, HLL_UINT = 1, HLL_F32 = 2, HLL_F64 = 3 };      // how a value of 8 bytes or fewer is widened to 64 bits (width 16: both words as they lie)
struct HllCol { const void* data; const uint8_t* valid; int32_t width; int32_t kind; };
i64 hll_tile_rows(i64 n_rows);                              // the library's choice of tile_rows: a multiple of 256
size_t hll_partial_bytes(i64 n_rows, i64 tile_rows);        // two 16 KB sketches per tile
// out[g] for every non-empty segment g (the caller zeroes `out`: an empty segment is met by no tile); rows [0, n_rows) of `col` are read
void launch_hll_approx_distinct(hipStream_t s, const HllCol& col, const int32_t* starts, i64 n_groups, i64 n_rows, i64 tile_rows, void* partial, u64* out);

// ----- scan-side decode (kernels_scanfmt.hip): delimited text and Parquet pages
enum CsvKind : int32_t { CSV_SKIP = 0, CSV_I32 = 1, CSV_I64 = 2, CSV_DATE32 = 3, CSV_DEC128 = 4, CSV_F64 = 5, CSV_BOOL = 6, CSV_UTF8 = 7 };
constexpr int CSV_MAX_FIELDS = 64;
struct CsvSpec {
  int32_t n_fields; int32_t kind[CSV_MAX_FIELDS]; int32_t out[CSV_MAX_FIELDS]; int32_t scale[CSV_MAX_FIELDS]; int32_t nullable[CSV_MAX_FIELDS];
  int32_t prec[CSV_MAX_FIELDS];
  uint8_t delim, quote; uint8_t pad[2];
};
struct CsvOut { void* data[CSV_MAX_FIELDS]; u64* valid[CSV_MAX_FIELDS]; uint32_t* str_start[CSV_MAX_FIELDS]; int32_t* str_len[CSV_MAX_FIELDS]; };
constexpr uint32_t CSVF_BAD_NUMBER = 1u, CSVF_FIELD_COUNT = 2u, CSVF_QUOTE = 4u, CSVF_NULL_IN_REQUIRED = 8u, CSVF_FLOAT_PRECISION = 16u, CSVF_BLANK_LINE = 32u, CSVF_BARE_CR = 64u;
void launch_csv_count_lines(hipStream_t s, const uint8_t* text, i64 n, i64 chunk, int nblocks, uint32_t* counts);
void launch_csv_line_starts(hipStream_t s, const uint8_t* text, i64 n, i64 chunk, int nblocks, const uint32_t* block_offsets, i64* starts);
void launch_csv_parse(hipStream_t s, const uint8_t* text, i64 n_bytes, const i64* starts, i64 row0, i64 n_rows, const CsvSpec& S, const CsvOut& O, uint32_t* flags);
void launch_csv_copy_strings(hipStream_t s, const uint8_t* text, const uint32_t* start, const int32_t* offsets, i64 n, uint8_t* out);
enum PqPhys : int32_t { PQ_BOOL = 0, PQ_I32 = 1, PQ_I64 = 2, PQ_I96 = 3 /* nanoseconds of the day + Julian day -> Timestamp(ns) */, PQ_F32 = 4, PQ_F64 = 5, PQ_BYTE_ARRAY = 6, PQ_FLBA = 7 };
enum PqEnc : int32_t { PQE_PLAIN = 0, PQE_DICT = 2, PQE_RLE = 3 };
struct PqPage { i64 src; int32_t bytes; int32_t n_values; i64 row0; int32_t enc; int32_t def_bytes; int32_t def_v2; int32_t dict; };
struct PqDict { i64 values; i64 str_offsets; int32_t n; int32_t pad; };
struct PqCol { int32_t phys, width; int32_t flba_len, optional; void* data; u64* valid; int32_t* str_len; i64* str_src; };
constexpr uint32_t PQF_MALFORMED = 1u, PQF_UNSUPPORTED = 2u;
void launch_pq_decode(hipStream_t s, const uint8_t* file, i64 file_bytes, const PqPage* pages, int n_pages, const PqCol& C, const PqDict* dicts, const uint8_t* dict_values,
                      const int32_t* dict_str_offsets, uint32_t* scratch, i64 scratch_stride, uint32_t* flags);
void launch_pq_copy_strings(hipStream_t s, const uint8_t* file, const uint8_t* dict_values, const i64* src, const int32_t* offsets, i64 n, uint8_t* out);
void launch_pq_dict_strings(hipStream_t s, const uint8_t* file, i64 src, int32_t bytes, int32_t n, int32_t* offsets, uint8_t* out, uint32_t* flags);
void launch_pq_dict_fixed(hipStream_t s, const uint8_t* file, i64 src, int32_t n, int32_t phys, int32_t flba_len, int32_t width, uint8_t* out);

// Launch a kernel that exists once per column-slot count: `pick(MaxC<M>{})` returns &k_X<M> (GPUQ_PICK(k_X) is that function), and
// the instantiation is chosen from the program's n_cols.  With `jit_fn` the hiprtc-specialised entry of the same sink runs instead,
// on the same arguments: it reads them as raw bytes, so they must have exactly the kernel's parameter types (the caller casts, once).
template <int M> using MaxC = std::integral_constant<int, M>;
#define GPUQ_PICK(KERNEL) [](auto M) { return &KERNEL<decltype(M)::value>; }
template <class Pick, class... Args>
inline void launch_sink(void* jit_fn, int n_cols, Pick pick, dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
  static_assert(std::is_same_v<decltype(pick(MaxC<2>{})), void (*)(Args...)>, "launch_sink: argument types differ from the kernel's parameter types");
  if (jit_fn) {
    void* a[] = {(void*)&args...};
    HIPCHECK(hipModuleLaunchKernel((hipFunction_t)jit_fn, grid.x, grid.y, grid.z, block.x, block.y, block.z, (unsigned)lds, s, a, nullptr));
  } else if (n_cols <= 2) hipLaunchKernelGGL(pick(MaxC<2>{}), grid, block, lds, s, args...);
  else if (n_cols <= 4) hipLaunchKernelGGL(pick(MaxC<4>{}), grid, block, lds, s, args...);
  else if (n_cols <= 8) hipLaunchKernelGGL(pick(MaxC<8>{}), grid, block, lds, s, args...);
  else hipLaunchKernelGGL(pick(MaxC<16>{}), grid, block, lds, s, args...);
}
#endif  // GPUQ_JIT

}  // namespace gpuq
