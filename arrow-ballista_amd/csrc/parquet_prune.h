// Row-group pruning from footer statistics, on the host (where the reference's ParquetExec does it).  Plain C++17, no HIP header.
//
// may_be_true(predicate, row group) is a three-valued walk collapsed to one bit: "false" only when the chunk statistics PROVE that
// no row of the group makes the predicate true, "true" for everything else -- in particular for everything this file does not
// understand.  The predicate is NOT applied to rows by a scan; the FilterExec above the leaf does that.  The rules:
//   comparisons   `column op literal` / `literal op column`, op in = < <= > >=; the literal has EXACTLY the column's type (for a decimal
//                 the same precision and scale); anything under a cast is not understood.  `column != literal` never prunes.
//                 `column IN (literals)` (not negated) may be true if any element lies in [min, max].  IS NULL may be true unless
//                 null_count is present and 0; IS NOT NULL unless null_count is present and equals the chunk's num_values.
//   structure     AND: both sides may be true.  OR: either side.  NOT over a supported comparison negates the operator, any other NOT
//                 answers true.  A NULL literal in a comparison answers false (the comparison is NULL for every row).
//   all-NULL      a comparison over a column with null_count == num_values answers false whatever min and max hold; with null_count
//                 absent the group is not known to be all-NULL.
//   bounds        min and max are BOUNDS, never attained values (writers may truncate a string min, and truncate and increment a
//                 string max): `>` against a max equal to the literal prunes, `>=` keeps, and `=` never concludes "every row equals".
//   trusted       min_value / max_value for every supported type; the deprecated min / max only where the signed order they were
//                 written in is the column's own: INT32 / INT64 physical columns that are signed integers, dates, timestamps or
//                 decimals.  They are ignored for BYTE_ARRAY, FIXED_LEN_BYTE_ARRAY and unsigned integers.
//   bytes         Int8..Int64, Date32, Timestamp, decimals on INT32 / INT64: little-endian, signed.  UInt8..UInt64: unsigned.  Decimals
//                 on FIXED_LEN_BYTE_ARRAY / BYTE_ARRAY: big-endian two's complement, 1..16 bytes, sign-extended.  Utf8: bytewise
//                 unsigned, a proper prefix first (gpuq_utf8_compare's order).  Boolean: one byte.  INT96 has no usable statistics.
//   floats        Float32 / Float64 columns are NEVER pruned on.  Writers leave NaN out of min / max, and whether a NaN row satisfies
//                 `x > c` depends on the comparison kernel's ordering of NaN; the executor's NaN semantics were not checked when this
//                 was written, so correctness is not staked on them.
//   unusable      a value whose length does not fit the physical type, min > max in the column's order, a column that is not in the
//                 file: the group is kept, and the call still succeeds.
//   byte ranges   a row group belongs to the range [start, end) that contains the file offset of its first column chunk's first page
//                 (the dictionary page offset if there is one, else the data page offset) -- DataFusion's rule [UPSTREAM-KNOWLEDGE].
//                 Ranges that tile [0, file size) select every row group exactly once.
#pragma once
#include "json.h"
#include "parquet_meta.h"
#include <string>
#include <vector>

namespace gpuq {

typedef __int128 pq_i128;
struct PqTypeId { int id = -1, p = 0, s = 0; bool operator==(const PqTypeId& o) const { return id == o.id && p == o.p && s == o.s; } };
struct PqValue { bool is_str = false; pq_i128 i = 0; std::string s; };      // integers, dates, timestamps, decimals, booleans | Utf8 bytes
inline int pq_cmp(const PqValue& a, const PqValue& b) {
  if (a.is_str) { const int c = a.s.compare(b.s); return c < 0 ? -1 : (c > 0 ? 1 : 0); }      // char_traits<char>: unsigned bytes, a proper prefix first
  return a.i < b.i ? -1 : (a.i > b.i ? 1 : 0);
}
inline bool pq_type_signed(int id) { return id == GPUQ_INT8 || id == GPUQ_INT16 || id == GPUQ_INT32 || id == GPUQ_INT64 || id == GPUQ_DATE32 || id == GPUQ_TIMESTAMP || id == GPUQ_DECIMAL128; }
inline bool pq_type_unsigned(int id) { return id == GPUQ_UINT8 || id == GPUQ_UINT16 || id == GPUQ_UINT32 || id == GPUQ_UINT64; }

// the type a predicate literal declares; false = a type this file does not compare
inline bool pq_type_of_json(const Json& j, PqTypeId& t) {
  static const struct { const char* n; int id; } names[] = {{"Int8", GPUQ_INT8}, {"Int16", GPUQ_INT16}, {"Int32", GPUQ_INT32}, {"Int64", GPUQ_INT64}, {"UInt8", GPUQ_UINT8},
    {"UInt16", GPUQ_UINT16}, {"UInt32", GPUQ_UINT32}, {"UInt64", GPUQ_UINT64}, {"Date32", GPUQ_DATE32}, {"Utf8", GPUQ_UTF8}, {"Boolean", GPUQ_BOOL}, {"Null", GPUQ_NULL}};
  t = PqTypeId();
  if (j.is_str()) { for (auto& n : names) if (j.s == n.n) { t.id = n.id; return true; } return false; }
  if (!j.is_obj()) return false;
  if (const Json* d = j.find("Decimal128")) {
    if (!d->is_arr() || d->a.size() != 2 || !d->a[0].is_num() || !d->a[1].is_num()) return false;
    t.id = GPUQ_DECIMAL128; t.p = (int)d->a[0].i64(); t.s = (int)d->a[1].i64(); return true;
  }
  if (const Json* ts = j.find("Timestamp")) {
    const Json* u = ts->is_arr() ? (ts->a.empty() ? nullptr : &ts->a[0]) : ts;
    if (!u || !u->is_str()) return false;
    t.id = GPUQ_TIMESTAMP;
    if (u->s == "Second" || u->s == "s") t.p = 0; else if (u->s == "Millisecond" || u->s == "ms") t.p = 1; else if (u->s == "Microsecond" || u->s == "us") t.p = 2;
    else if (u->s == "Nanosecond" || u->s == "ns") t.p = 3; else return false;
    return true;
  }
  return false;
}
// decimal text of an integer of up to 38 digits
inline bool pq_parse_i128(const std::string& s, pq_i128& out) {
  size_t k = 0; bool neg = false;
  if (k < s.size() && (s[k] == '-' || s[k] == '+')) { neg = s[k] == '-'; ++k; }
  if (k >= s.size() || s.size() - k > 38) return false;
  unsigned __int128 v = 0;
  for (; k < s.size(); ++k) { if (s[k] < '0' || s[k] > '9') return false; v = v * 10 + (unsigned)(s[k] - '0'); }
  out = neg ? -(pq_i128)v : (pq_i128)v;      // < 10^38 < 2^127
  return true;
}
inline bool pq_in_range(int id, pq_i128 v) {
  switch (id) {
    case GPUQ_INT8: return v >= -128 && v <= 127; case GPUQ_INT16: return v >= -32768 && v <= 32767;
    case GPUQ_INT32: case GPUQ_DATE32: return v >= INT32_MIN && v <= INT32_MAX;
    case GPUQ_INT64: case GPUQ_TIMESTAMP: return v >= INT64_MIN && v <= INT64_MAX;
    case GPUQ_UINT8: return v >= 0 && v <= 255; case GPUQ_UINT16: return v >= 0 && v <= 65535; case GPUQ_UINT32: return v >= 0 && v <= (pq_i128)UINT32_MAX;
    case GPUQ_UINT64: return v >= 0 && v <= (pq_i128)UINT64_MAX;
    case GPUQ_BOOL: return v == 0 || v == 1;
    default: return true;
  }
}
// {"literal": {"type", "value"}}: 0 = not a literal this file compares, 1 = a value, 2 = a NULL of any type
inline int pq_literal(const Json& e, PqTypeId& t, PqValue& v) {
  if (!(e.is_obj() && e.o.size() == 1 && e.o[0].first == "literal" && e.o[0].second.is_obj())) return 0;
  const Json& l = e.o[0].second; const Json* ty = l.find("type"); const Json* val = l.find("value");
  if (!ty) return 0;
  if (!val || val->is_null()) return 2;
  if (!pq_type_of_json(*ty, t) || t.id == GPUQ_NULL) return 0;
  v = PqValue();
  if (t.id == GPUQ_UTF8) { if (!val->is_str()) return 0; v.is_str = true; v.s = val->s; return 1; }
  if (t.id == GPUQ_BOOL) { if (val->kind != Json::BOOL) return 0; v.i = val->b ? 1 : 0; return 1; }
  if (!(val->is_str() || val->is_num()) || !pq_parse_i128(val->s, v.i) || !pq_in_range(t.id, v.i)) return 0;
  return 1;
}

// One column of one row group, ready to compare against: its type, whether min / max could be used, the null count.
struct PqColStats { PqTypeId type; bool has_min = false, has_max = false, has_null_count = false; PqValue min, max; int64_t null_count = 0, num_values = 0; };

inline bool pq_decode_stat(const PqSchemaElem& L, int gt, const std::string& b, PqValue& out) {
  out = PqValue();
  const size_t n = b.size(); const uint8_t* p = (const uint8_t*)b.data();
  const bool dec = L.logical_decimal || L.converted == 5;
  switch (L.type) {
    case 0: if (n != 1 || p[0] > 1) return false; out.i = p[0]; return true;
    case 1: { if (n != 4) return false; uint32_t u; std::memcpy(&u, p, 4); out.i = pq_type_unsigned(gt) ? (pq_i128)u : (pq_i128)(int32_t)u; return pq_in_range(gt, out.i); }
    case 2: { if (n != 8) return false; uint64_t u; std::memcpy(&u, p, 8); out.i = pq_type_unsigned(gt) ? (pq_i128)u : (pq_i128)(int64_t)u; return true; }
    case 6: case 7:
      if (dec) {
        if (n < 1 || n > 16 || (L.type == 7 && (int64_t)n != L.type_length)) return false;
        unsigned __int128 u = (p[0] & 0x80) ? ~(unsigned __int128)0 : 0;      // sign extension
        for (size_t k = 0; k < n; ++k) u = (u << 8) | p[k];
        out.i = (pq_i128)u; return true;
      }
      if (L.type == 6 && gt == GPUQ_UTF8) { out.is_str = true; out.s = b; return true; }
      return false;
    default: return false;      // INT96, FLOAT, DOUBLE
  }
}
// (little-endian hosts: the device's, and every host this library is built for)
inline PqColStats pq_col_stats(const PqSchemaElem& L, const PqChunk& K) {
  PqColStats c; int gt = -1, gp = 0, gs = 0, w = 0;
  const bool dec = L.logical_decimal || L.converted == 5;
  if (L.type == 6 && dec) { gt = GPUQ_DECIMAL128; gp = L.precision; gs = L.scale; }      // (not decoded on the device; its statistics still bound it)
  else if (!pq_leaf_type(L, gt, gp, gs, w)) return c;
  c.num_values = K.num_values;
  if (K.stats.has_null_count && K.stats.null_count >= 0 && K.stats.null_count <= K.num_values) { c.has_null_count = true; c.null_count = K.stats.null_count; }
  if (gt == GPUQ_FLOAT32 || gt == GPUQ_FLOAT64 || L.type == 3 || L.num_children > 0 || L.repetition == 2) { c.type.id = gt; c.type.p = gp; c.type.s = gs; return c; }
  c.type.id = gt; c.type.p = gp; c.type.s = gs;
  const bool deprecated_ok = (L.type == 1 || L.type == 2) && pq_type_signed(gt);
  const PqStats& S = K.stats;
  if (S.has_min_value) c.has_min = pq_decode_stat(L, gt, S.min_value, c.min);
  else if (deprecated_ok && S.has_min_deprecated) c.has_min = pq_decode_stat(L, gt, S.min_deprecated, c.min);
  if (S.has_max_value) c.has_max = pq_decode_stat(L, gt, S.max_value, c.max);
  else if (deprecated_ok && S.has_max_deprecated) c.has_max = pq_decode_stat(L, gt, S.max_deprecated, c.max);
  // a member that was present but unusable taints the other: the writer is not one to trust.  So does min > max.
  const bool any_bad = ((S.has_min_value || (deprecated_ok && S.has_min_deprecated)) && !c.has_min) || ((S.has_max_value || (deprecated_ok && S.has_max_deprecated)) && !c.has_max);
  if (any_bad || (c.has_min && c.has_max && pq_cmp(c.min, c.max) > 0)) c.has_min = c.has_max = false;
  return c;
}

struct PqPruner {
  const PqFileMeta& M; const gpuq_field_info* fields; int n_fields;
  const std::string* column(const Json& e) const {
    if (!(e.is_obj() && e.o.size() == 1 && e.o[0].first == "column" && e.o[0].second.is_obj())) return nullptr;
    const Json* n = e.o[0].second.find("name");
    return n && n->is_str() ? &n->s : nullptr;
  }
  // statistics of the named column in group g; false = nothing is known (not in the file or the declared schema, declared with another type, nested)
  bool stats(const std::string& name, size_t g, PqColStats& out) const {
    int declared = -1; for (int i = 0; i < n_fields; ++i) if (name == fields[i].name) declared = i;
    if (declared < 0 || M.schema.empty()) return false;
    int leaf = -1; for (size_t k = 1; k < M.schema.size(); ++k) if (M.schema[k].name == name) leaf = (int)k - 1;
    for (size_t k = 1; k < M.schema.size(); ++k) if (M.schema[k].num_children > 0) return false;      // flat schemas only: leaf k is chunk k
    if (leaf < 0 || (size_t)leaf >= M.groups[g].cols.size()) return false;
    out = pq_col_stats(M.schema[(size_t)leaf + 1], M.groups[g].cols[(size_t)leaf]);
    const gpuq_field_info& f = fields[declared];
    if (out.type.id != f.type) return false;
    if ((f.type == GPUQ_DECIMAL128 || f.type == GPUQ_TIMESTAMP) && out.type.p != f.precision) return false;
    if (f.type == GPUQ_DECIMAL128 && out.type.s != f.scale) return false;
    return true;
  }
  static int op_of(const std::string& s) {      // 0 = 1 < 2 <= 3 > 4 >= 5 != ; -1 other
    if (s == "=" || s == "Eq") return 0; if (s == "<" || s == "Lt") return 1; if (s == "<=" || s == "LtEq") return 2;
    if (s == ">" || s == "Gt") return 3; if (s == ">=" || s == "GtEq") return 4; if (s == "!=" || s == "NotEq") return 5;
    return -1;
  }
  static int flip(int op) { static const int f[6] = {0, 3, 4, 1, 2, 5}; return f[op]; }        // literal op column -> column op' literal
  static int negate(int op) { static const int n[6] = {5, 4, 3, 2, 1, 0}; return n[op]; }      // NOT (a op b) = a op' b where neither is NULL; NULL rows make neither true
  // `column op literal` over group g
  bool compare(const std::string& name, int op, int lit_kind, const PqTypeId& lt, const PqValue& lv, size_t g) const {
    if (lit_kind == 2) return false;      // NULL literal: the comparison is NULL for every row
    PqColStats c;
    if (!stats(name, g, c)) return true;
    if (c.type.id == GPUQ_FLOAT32 || c.type.id == GPUQ_FLOAT64) return true;
    if (!(lt == c.type)) return true;      // (the plan would carry a cast; a comparison across types is not understood)
    if (c.has_null_count && c.null_count == c.num_values) return false;      // all NULL (an empty chunk included): no row compares true
    switch (op) {
      case 0: return !((c.has_min && pq_cmp(lv, c.min) < 0) || (c.has_max && pq_cmp(lv, c.max) > 0));
      case 1: return !(c.has_min && pq_cmp(c.min, lv) >= 0);
      case 2: return !(c.has_min && pq_cmp(c.min, lv) > 0);
      case 3: return !(c.has_max && pq_cmp(c.max, lv) <= 0);
      case 4: return !(c.has_max && pq_cmp(c.max, lv) < 0);
      default: return true;      // !=: min and max are bounds, "every row equals the literal" is never known
    }
  }
  // the comparison `e` is, if it is one this file supports: column name, operator (as column op literal), literal
  bool comparison(const Json& e, const std::string*& name, int& op, int& kind, PqTypeId& lt, PqValue& lv) const {
    if (!(e.is_obj() && e.o.size() == 1 && e.o[0].first == "binary_expr" && e.o[0].second.is_obj())) return false;
    const Json& b = e.o[0].second; const Json* l = b.find("l"); const Json* r = b.find("r"); const Json* o = b.find("op");
    if (!l || !r || !o || !o->is_str()) return false;
    op = op_of(o->s); if (op < 0) return false;
    if ((name = column(*l)) && (kind = pq_literal(*r, lt, lv))) return true;
    if ((name = column(*r)) && (kind = pq_literal(*l, lt, lv))) { op = flip(op); return true; }
    return false;
  }
  bool may_be_true(const Json& e, size_t g, int depth = 0) const {
    if (depth > 256 || !e.is_obj() || e.o.size() != 1 || !e.o[0].second.is_obj()) return true;
    const std::string& kind = e.o[0].first; const Json& v = e.o[0].second;
    if (kind == "binary_expr") {
      const Json* o = v.find("op"); const Json* l = v.find("l"); const Json* r = v.find("r");
      if (!o || !o->is_str() || !l || !r) return true;
      if (o->s == "AND" || o->s == "And") return may_be_true(*l, g, depth + 1) && may_be_true(*r, g, depth + 1);
      if (o->s == "OR" || o->s == "Or") return may_be_true(*l, g, depth + 1) || may_be_true(*r, g, depth + 1);
      const std::string* name; int op, lk; PqTypeId lt; PqValue lv;
      if (!comparison(e, name, op, lk, lt, lv)) return true;
      return compare(*name, op, lk, lt, lv, g);
    }
    if (kind == "not_expr") {
      const Json* in = v.find("expr");
      const std::string* name; int op, lk; PqTypeId lt; PqValue lv;
      if (!in || !comparison(*in, name, op, lk, lt, lv)) return true;
      return compare(*name, negate(op), lk, lt, lv, g);
    }
    if (kind == "is_null_expr" || kind == "is_not_null_expr") {
      const Json* in = v.find("expr"); const std::string* name = in ? column(*in) : nullptr; PqColStats c;
      if (!name || !stats(*name, g, c) || !c.has_null_count) return true;
      return kind == "is_null_expr" ? c.null_count != 0 : c.null_count != c.num_values;
    }
    if (kind == "in_list") {
      const Json* in = v.find("expr"); const Json* list = v.find("list"); const std::string* name = in ? column(*in) : nullptr;
      if (!name || !list || !list->is_arr() || v.get_bool("negated", false)) return true;
      for (auto& el : list->a) {
        PqTypeId lt; PqValue lv; const int lk = pq_literal(el, lt, lv);
        if (lk == 0 || compare(*name, 0, lk, lt, lv, g)) return true;      // (a NULL element makes no row true)
      }
      return false;
    }
    return true;
  }
};

// The row groups of `M` in [range_start, range_end) (range_end < 0: all of them), ascending; *n_in_range = their number; then, with a
// predicate, those of them it may be true in.
inline std::vector<int32_t> pq_prune(const PqFileMeta& M, const Json* predicate, const gpuq_field_info* fields, int n_fields, int64_t range_start, int64_t range_end, int* n_in_range) {
  std::vector<int32_t> keep; int in_range = 0;
  PqPruner P{M, fields, n_fields};
  for (size_t g = 0; g < M.groups.size(); ++g) {
    if (range_end >= 0) {
      // a group without column chunks has no offset: it goes to the range that holds offset 0, so that a tiling still sees it once
      const int64_t at = M.groups[g].cols.empty() ? 0 : pq_chunk_start(M.groups[g].cols[0]);
      if (at < range_start || at >= range_end) continue;
    }
    ++in_range;
    if (predicate && !P.may_be_true(*predicate, g)) continue;
    keep.push_back((int32_t)g);
  }
  if (n_in_range) *n_in_range = in_range;
  return keep;
}

}  // namespace gpuq
