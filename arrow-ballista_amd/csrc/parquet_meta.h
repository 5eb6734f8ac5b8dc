// The metadata of a Parquet file as the host reads it: the Thrift compact protocol (the parts the format uses), the footer --
// schema, row groups, column chunks and their Statistics -- and the mapping of a leaf to a gpuq type.  Plain C++17, no HIP header
// (zstd_dec.h, lz_elements.h and hll_estimate.h are the precedent): scanfmt.cpp includes it for the device decode, plan_exec.cpp for
// the scan leaf, parquet_prune.h for row-group pruning, and a stand-alone host program can be built from it alone.
#pragma once
#include "../../include/gpuq.h"
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace gpuq {

struct TReader {
  const uint8_t* p; const uint8_t* e;
  void need(size_t n) const { if ((size_t)(e - p) < n) throw std::runtime_error("parquet: metadata ends inside a Thrift value"); }
  uint64_t varint() { uint64_t v = 0; int sh = 0; for (;;) { need(1); const uint8_t c = *p++; v |= (uint64_t)(c & 0x7F) << sh; if (!(c & 0x80)) return v; sh += 7; if (sh > 63) throw std::runtime_error("parquet: varint too long"); } }
  int64_t zigzag() { const uint64_t v = varint(); return (int64_t)((v >> 1) ^ (~(v & 1) + 1)); }
  std::string binary() { const uint64_t n = varint(); need(n); std::string s((const char*)p, (size_t)n); p += n; return s; }
  // field header: returns false at STOP; type in the low nibble, id by delta or explicit
  bool field(int& type, int& id, int& last) {
    need(1); const uint8_t b = *p++;
    if (b == 0) return false;
    type = b & 0x0F; const int delta = b >> 4;
    id = delta ? (int)((unsigned)last + (unsigned)delta) : (int)zigzag();
    last = id; return true;
  }
  int depth = 0;      // nesting of the value being skipped: a crafted footer of struct headers must not walk the host stack down
  struct Nest { int& d; Nest(int& d_) : d(d_) { if (++d > 64) throw std::runtime_error("parquet: Thrift metadata nested deeper than 64 levels"); } ~Nest() { --d; } };
  void skip(int type) {
    Nest nest(depth);
    switch (type) {
      case 1: case 2: break;                                   // bool true / false (value in the type)
      case 3: need(1); ++p; break;                             // i8
      case 4: case 5: case 6: (void)zigzag(); break;           // i16 / i32 / i64
      case 7: need(8); p += 8; break;                          // double
      case 8: { const uint64_t n = varint(); need(n); p += n; break; }     // binary
      case 9: case 10: { need(1); const uint8_t h = *p++; uint64_t n = h >> 4; const int et = h & 0x0F; if (n == 15) n = varint(); for (uint64_t i = 0; i < n; ++i) skip_elem(et); break; }
      case 11: { const uint64_t n = varint(); if (n) { need(1); const uint8_t kv = *p++; for (uint64_t i = 0; i < n; ++i) { skip_elem(kv >> 4); skip_elem(kv & 0x0F); } } break; }
      case 12: { int t, id, last = 0; while (field(t, id, last)) skip(t); break; }
      default: throw std::runtime_error("parquet: unknown Thrift type " + std::to_string(type));
    }
  }
  void skip_elem(int et) { if (et == 1 || et == 2) { need(1); ++p; } else skip(et); }      // booleans inside collections take a byte
  uint64_t list_header(int& elem_type) { need(1); const uint8_t h = *p++; uint64_t n = h >> 4; elem_type = h & 0x0F; if (n == 15) n = varint(); return n; }
};

struct PqSchemaElem { int type = -1, type_length = 0, repetition = 0, num_children = 0, converted = -1, scale = 0, precision = 0; std::string name; bool logical_decimal = false, logical_date = false, logical_string = false;
                      int int_bits = 0; bool int_signed = true; int ts_unit = -1; };      // LogicalType INTEGER {bitWidth, isSigned}, TIMESTAMP {unit}: gpuq TimeUnit 1 ms / 2 us / 3 ns
// Statistics (parquet.thrift, ColumnMetaData field 12) of one column chunk, as written: a "present" bit for each member.  Nothing is
// interpreted here; parquet_prune.h decides which members it trusts.  A Statistics struct whose members have unexpected Thrift types is
// dropped whole (has_* all false), never an error: a file that decodes without statistics decodes with bad ones.
struct PqStats {
  std::string max_deprecated, min_deprecated, max_value, min_value;      // fields 1, 2, 5, 6
  int64_t null_count = 0;                                                // field 3
  bool is_max_exact = false, is_min_exact = false;                       // fields 7, 8
  bool has_max_deprecated = false, has_min_deprecated = false, has_null_count = false, has_max_value = false, has_min_value = false,
       has_is_max_exact = false, has_is_min_exact = false;
};
struct PqChunk { int type = -1, codec = 0; int64_t num_values = 0, total_compressed = 0, data_page_offset = 0, dict_page_offset = -1; std::vector<std::string> path; PqStats stats; };
struct PqRowGroup { std::vector<PqChunk> cols; int64_t num_rows = 0; };
struct PqFileMeta { std::vector<PqSchemaElem> schema; std::vector<PqRowGroup> groups; int64_t num_rows = 0; };

inline PqSchemaElem read_schema_elem(TReader& r) {
  PqSchemaElem s; int t, id, last = 0;
  while (r.field(t, id, last)) {
    switch (id) {
      case 1: s.type = (int)r.zigzag(); break; case 2: s.type_length = (int)r.zigzag(); break; case 3: s.repetition = (int)r.zigzag(); break;
      case 4: s.name = r.binary(); break; case 5: s.num_children = (int)r.zigzag(); break; case 6: s.converted = (int)r.zigzag(); break;
      case 7: s.scale = (int)r.zigzag(); break; case 8: s.precision = (int)r.zigzag(); break;
      case 10: {      // LogicalType union: field id = which
        int t2, id2, last2 = 0;
        while (r.field(t2, id2, last2)) {
          if (id2 == 1) s.logical_string = true; else if (id2 == 6) s.logical_date = true;
          if (id2 == 5) {      // DecimalType {1 scale, 2 precision}
            s.logical_decimal = true; int t3, id3, last3 = 0;
            while (r.field(t3, id3, last3)) { if (id3 == 1) s.scale = (int)r.zigzag(); else if (id3 == 2) s.precision = (int)r.zigzag(); else r.skip(t3); }
          } else if (id2 == 10) {      // IntType {1 bitWidth: i8, 2 isSigned: bool (in the field header)}
            int t3, id3, last3 = 0;
            while (r.field(t3, id3, last3)) { if (id3 == 1 && t3 == 3) { r.need(1); s.int_bits = (int)(int8_t)*r.p++; } else if (id3 == 2 && (t3 == 1 || t3 == 2)) s.int_signed = t3 == 1; else r.skip(t3); }
          } else if (id2 == 8) {      // TimestampType {1 isAdjustedToUTC, 2 unit: union {1 MILLIS, 2 MICROS, 3 NANOS}}
            int t3, id3, last3 = 0;
            while (r.field(t3, id3, last3)) {
              if (id3 == 2 && t3 == 12) { int t4, id4, last4 = 0; while (r.field(t4, id4, last4)) { if (id4 >= 1 && id4 <= 3) s.ts_unit = id4; r.skip(t4); } }
              else r.skip(t3);
            }
          } else r.skip(t2);
        }
        break;
      }
      default: r.skip(t);
    }
  }
  return s;
}
// parquet.thrift Type / ConvertedType / LogicalType of a leaf -> gpuq_type (+ precision / scale / bytes per value on the device); false = not read
// on the device.  INT96 is Impala's timestamp (nanoseconds of the day + Julian day) -> Timestamp(Nanosecond), as arrow's reader maps it.
inline bool pq_leaf_type(const PqSchemaElem& L, int& gt, int& gp, int& gs, int& width) {
  const bool dec = L.logical_decimal || L.converted == 5;
  gp = 0; gs = 0; width = 0;
  switch (L.type) {
    case 0: gt = GPUQ_BOOL; return true;
    case 1:
      if (dec) { gt = GPUQ_DECIMAL128; gp = L.precision; gs = L.scale; width = 16; return true; }
      if (L.logical_date || L.converted == 6) { gt = GPUQ_DATE32; width = 4; return true; }
      if (L.int_bits == 8 || L.converted == 15 || L.converted == 11) { const bool sg = L.int_bits ? L.int_signed : L.converted == 15; gt = sg ? GPUQ_INT8 : GPUQ_UINT8; width = 1; return true; }
      if (L.int_bits == 16 || L.converted == 16 || L.converted == 12) { const bool sg = L.int_bits ? L.int_signed : L.converted == 16; gt = sg ? GPUQ_INT16 : GPUQ_UINT16; width = 2; return true; }
      gt = ((L.int_bits == 32 && !L.int_signed) || L.converted == 13) ? GPUQ_UINT32 : GPUQ_INT32; width = 4; return true;
    case 2:
      if (dec) { gt = GPUQ_DECIMAL128; gp = L.precision; gs = L.scale; width = 16; return true; }
      if (L.ts_unit > 0 || L.converted == 9 || L.converted == 10) { gt = GPUQ_TIMESTAMP; gp = L.ts_unit > 0 ? L.ts_unit : (L.converted == 9 ? 1 : 2); width = 8; return true; }
      gt = ((L.int_bits == 64 && !L.int_signed) || L.converted == 14) ? GPUQ_UINT64 : GPUQ_INT64; width = 8; return true;
    case 3: gt = GPUQ_TIMESTAMP; gp = 3; width = 8; return true;
    case 4: gt = GPUQ_FLOAT32; width = 4; return true;
    case 5: gt = GPUQ_FLOAT64; width = 8; return true;
    case 6: if (dec) return false; gt = GPUQ_UTF8; return true;
    case 7: if (!dec || L.type_length < 1 || L.type_length > 16) return false; gt = GPUQ_DECIMAL128; gp = L.precision; gs = L.scale; width = 16; return true;
    default: return false;
  }
}
// Statistics {1 max, 2 min: binary (deprecated, signed order); 3 null_count, 4 distinct_count: i64; 5 max_value, 6 min_value: binary;
// 7 is_max_value_exact, 8 is_min_value_exact: bool}.  Unknown fields are skipped.  `e` bounds the read; a struct that cannot be walked
// to its STOP ends the footer parse as any other malformed Thrift does (it did before this struct was read, when it was skipped).
inline PqStats read_stats(TReader& r) {
  PqStats s; bool usable = true; int t, id, last = 0;
  while (r.field(t, id, last)) {
    const bool bin = t == 8, i64 = t == 6, boolean = t == 1 || t == 2;
    if (id == 1 && bin) { s.max_deprecated = r.binary(); s.has_max_deprecated = true; }
    else if (id == 2 && bin) { s.min_deprecated = r.binary(); s.has_min_deprecated = true; }
    else if (id == 3 && i64) { s.null_count = r.zigzag(); s.has_null_count = true; }
    else if (id == 5 && bin) { s.max_value = r.binary(); s.has_max_value = true; }
    else if (id == 6 && bin) { s.min_value = r.binary(); s.has_min_value = true; }
    else if (id == 7 && boolean) { s.is_max_exact = t == 1; s.has_is_max_exact = true; }
    else if (id == 8 && boolean) { s.is_min_exact = t == 1; s.has_is_min_exact = true; }
    else { if (id >= 1 && id <= 8 && id != 4) usable = false; r.skip(t); }      // a known member with another Thrift type: trust none of them
  }
  return usable ? s : PqStats();
}
inline PqChunk read_chunk(TReader& r) {
  PqChunk c; int t, id, last = 0;
  while (r.field(t, id, last)) {
    if (id == 3 && t == 12) {
      int t2, id2, last2 = 0;
      while (r.field(t2, id2, last2)) {
        switch (id2) {
          case 1: c.type = (int)r.zigzag(); break;
          case 3: { int et; const uint64_t n = r.list_header(et); for (uint64_t i = 0; i < n; ++i) c.path.push_back(r.binary()); break; }
          case 4: c.codec = (int)r.zigzag(); break; case 5: c.num_values = r.zigzag(); break; case 7: c.total_compressed = r.zigzag(); break;
          case 9: c.data_page_offset = r.zigzag(); break; case 11: c.dict_page_offset = r.zigzag(); break;
          case 12: if (t2 == 12) c.stats = read_stats(r); else r.skip(t2); break;
          default: r.skip(t2);
        }
      }
    } else r.skip(t);
  }
  return c;
}
inline PqFileMeta read_footer(const uint8_t* file, int64_t n) {
  if (n < 12 || std::memcmp(file, "PAR1", 4) != 0 || std::memcmp(file + n - 4, "PAR1", 4) != 0) throw std::runtime_error("parquet: missing PAR1 magic");
  uint32_t flen; std::memcpy(&flen, file + n - 8, 4);
  if ((int64_t)flen + 12 > n) throw std::runtime_error("parquet: footer length exceeds the file");
  TReader r{file + n - 8 - flen, file + n - 8};
  PqFileMeta m; int t, id, last = 0;
  while (r.field(t, id, last)) {
    if (id == 2) { int et; const uint64_t k = r.list_header(et); for (uint64_t i = 0; i < k; ++i) m.schema.push_back(read_schema_elem(r)); }
    else if (id == 3) m.num_rows = r.zigzag();
    else if (id == 4) {
      int et; const uint64_t k = r.list_header(et);
      for (uint64_t i = 0; i < k; ++i) {
        PqRowGroup g; int t2, id2, last2 = 0;
        while (r.field(t2, id2, last2)) {
          if (id2 == 1) { int et2; const uint64_t kc = r.list_header(et2); for (uint64_t j = 0; j < kc; ++j) g.cols.push_back(read_chunk(r)); }
          else if (id2 == 3) g.num_rows = r.zigzag();
          else r.skip(t2);
        }
        m.groups.push_back(std::move(g));
      }
    } else r.skip(t);
  }
  return m;
}
// The file offset at which a column chunk's pages begin: the dictionary page where there is one in front of the data pages
// (offset 0 is the file's magic: a writer that stores 0 there means "none").
inline int64_t pq_chunk_start(const PqChunk& K) { return K.dict_page_offset > 0 && K.dict_page_offset < K.data_page_offset ? K.dict_page_offset : K.data_page_offset; }

}  // namespace gpuq
