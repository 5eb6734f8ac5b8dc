// Aggregate descriptor -> scan program, accumulators, key layout and result projection (agg_compile.h).
//
// What the compile knows about an aggregate function is one row of AGG_FNS: the names it answers to, its traits, and four
// parts -- accumulators from the arguments (Single, Partial), accumulators from the state columns (Final, Merge), the state columns
// a Partial / Merge emits, the value a Single / Final emits.  A Partial's state columns (names, order, types) are the ones the Final of
// the same function reads by position: both are written next to each other in the function's definition below, and
// tests/test_cpu_agg_compile.py feeds every Partial's output to its Final.  A new function is a new row.
//
// The order in which accumulators are found or added and outputs are added to the programs decides register numbers and
// instruction order; tools/agg_compile_hashes.py prints a digest of every program of a grid of descriptors.
#include "agg_compile.h"
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <functional>

namespace gpuq {

gpuq_field_info make_field(const std::string& name, const DType& t, bool nullable) {
  gpuq_field_info f{};
  std::snprintf(f.name, sizeof(f.name), "%s", name.c_str());
  f.type = t.id; f.precision = t.p; f.scale = t.s; f.nullable = nullable;
  f.repr = (t.id == T_UTF8) ? GPUQ_REPR_PACKED15 : GPUQ_REPR_ARROW;
  f.width = (t.id == T_BOOL) ? 0 : type_width(t);
  return f;
}

KeySpec make_keyspec(const std::vector<int>& regs, const std::vector<DType>& types, bool null_word) {
  if (regs.size() > (size_t)MAX_KEYS) throw Unsupported("more than " + std::to_string(MAX_KEYS) + " key columns");
  KeySpec K{};
  K.n_keys = (int)regs.size(); K.null_word = null_word ? 1 : 0;
  int w = 0;
  for (size_t k = 0; k < regs.size(); ++k) {
    K.key_reg[k] = regs[k];
    const bool wide = types[k].id == T_DECIMAL128 || types[k].id == T_UTF8;
    K.key_wide[k] = wide;
    K.word_reg[w] = regs[k]; K.word_half[w] = 0; ++w;
    if (wide) { K.word_reg[w] = regs[k]; K.word_half[w] = 1; ++w; }
  }
  if (null_word) { K.word_reg[w] = 0; K.word_half[w] = 2; ++w; }
  K.key_words = w;
  return K;
}

namespace {

DType t_of(int id) { DType t; t.id = id; return t; }
DType dec_t(int p, int s) { DType t; t.id = T_DECIMAL128; t.p = std::min(p, 38); t.s = std::min(s, 38); return t; }
const DType BOOL = t_of(T_BOOL), I64 = t_of(T_INT64), U64 = t_of(T_UINT64), F64 = t_of(T_FLOAT64), WIDE = dec_t(38, 0);

// ---------------------------------------------------------------- group keys
// More than MAX_KEYS group columns (q10 groups by seven, q18 by five): the table still holds at most MAX_KEYS keys of up to 128 bits, so
// narrow keys are PACKED -- each biased to a non-negative number of `bits + 1` bits (+ 1 bit "is NULL"), shifted and OR-ed into 126-bit
// composites -- and the table groups by the composites.  The declared key columns are unpacked again over the GROUPS (the result
// projection divides by powers of two), so the table carries no extra state.  Utf8 / float keys take a slot of their own (the
// executor hands long or many Utf8 keys over as dictionary codes, which pack well).
// The rest of the compile sees key nodes go in (`nodes`: what the table groups by) and the declared key columns come out (`project`).
class GroupKeys {
 public:
  std::vector<NodeP> nodes; std::vector<std::string> names;
  std::string refuse;
  GroupKeys(ExprCompiler& ec, const std::vector<NodeP>& declared, const std::vector<std::string>& declared_names)
      : nodes(declared), names(declared_names), declared_(declared), declared_names_(declared_names), place_(declared.size()) {
    packed_ = declared.size() > (size_t)MAX_KEYS;
    if (!packed_) return;
    struct Slot { std::vector<size_t> ks; int bits = 0; bool solo = false; };
    std::vector<Slot> slots;
    for (size_t k = 0; k < declared.size(); ++k) {
      const int b = field_bits(declared[k]);
      if (b == 0 || b > 126) { Slot sl; sl.ks.push_back(k); sl.solo = true; slots.push_back(sl); continue; }
      bool placed = false;
      for (auto& sl : slots) if (!sl.solo && sl.bits + b <= 126) { sl.ks.push_back(k); sl.bits += b; placed = true; break; }
      if (!placed) { Slot sl; sl.ks.push_back(k); sl.bits = b; slots.push_back(sl); }
    }
    if (slots.size() > (size_t)MAX_KEYS) refuse = std::to_string(declared.size()) + " group-by columns need " + std::to_string(slots.size()) + " packed keys (" + std::to_string(MAX_KEYS) + " are held)";
    nodes.clear(); names.clear();
    for (size_t si = 0; si < slots.size() && si < (size_t)MAX_KEYS; ++si) {
      const Slot& sl = slots[si];
      if (sl.solo) { place_[sl.ks[0]].slot = (int)nodes.size(); place_[sl.ks[0]].own = true; nodes.push_back(declared[sl.ks[0]]); names.push_back(declared_names[sl.ks[0]]); continue; }
      NodeP acc; int shift = 0;
      for (size_t k : sl.ks) {
        NodeP v = to_field(ec, declared[k]);
        NodeP sh = shift ? ec.raw(OP_SHL, WIDE, false, 127, {v}, (uint32_t)shift) : v;
        acc = acc ? ec.raw(OP_BOR, WIDE, false, 127, {acc, sh}) : sh;
        place_[k].slot = (int)nodes.size(); place_[k].shift = shift; place_[k].width = field_bits(declared[k]);
        shift += place_[k].width;
      }
      nodes.push_back(acc); names.push_back("__packed" + std::to_string(si));
    }
  }
  size_t declared() const { return declared_.size(); }
  // the group columns in their declared order, over the result columns [0, nodes.size())
  void project(ExprCompiler& pc, std::vector<std::string>& out_names) const {
    for (size_t k = 0; k < declared_.size(); ++k) {
      const NodeP& n = declared_[k]; const Place& at = place_[k];
      out_names.push_back(declared_names_[k]);
      if (!packed_) { pc.add_output(pc.column((int)k)); continue; }
      if (at.slot < 0) { pc.add_output(pc.lit_null(n->type)); continue; }      // (refused operator: types only)
      if (at.own) { pc.add_output(pc.column(at.slot)); continue; }
      NodeP f = pc.column(at.slot);      // non-negative, < 2^126: truncating division is the shift
      if (at.shift) f = pc.raw(OP_DIV, WIDE, false, 127, {f, pc.lit_int(WIDE, (i128)1 << at.shift)});
      f = pc.raw(OP_MOD, WIDE, false, at.width, {f, pc.lit_int(WIDE, (i128)1 << at.width)});
      pc.add_output(from_field(pc, n, f));
    }
  }

 private:
  struct Place { int slot = -1, shift = 0, width = 0; bool own = false; };      // own: the key IS column `slot` of the result
  std::vector<NodeP> declared_; std::vector<std::string> declared_names_; std::vector<Place> place_; bool packed_ = false;
  // A key as a bit field of a composite and back: |value| < 2^bits -> value + 2^bits in [0, 2^(bits+1)), NULL -> bit bits+1 alone.
  static int field_bits(const NodeP& n) { return (n->type.id == T_UTF8 || n->type.is_float() || n->type.id == T_BOOL) ? 0 : n->bits + 1 + (n->nullable ? 1 : 0); }      // 0: does not pack
  static NodeP to_field(ExprCompiler& ec, const NodeP& n) {
    NodeP v = ec.raw(OP_ADD, WIDE, n->nullable, n->bits + 1, {n, ec.lit_int(WIDE, (i128)1 << n->bits)});
    if (!n->nullable) return v;
    NodeP flag = ec.raw(OP_SHL, WIDE, false, n->bits + 2, {ec.raw(OP_MOV, WIDE, false, 1, {ec.is_null(n, false)})}, (uint32_t)(n->bits + 1));
    return ec.raw(OP_BOR, WIDE, false, n->bits + 2, {ec.coalesce0(v), flag});
  }
  static NodeP from_field(ExprCompiler& pc, const NodeP& n, NodeP f) {
    NodeP v = pc.raw(OP_SUB, n->type, false, n->bits, {f, pc.lit_int(WIDE, (i128)1 << n->bits)});
    if (!n->nullable) return v;
    return pc.select(pc.raw(OP_GE, BOOL, false, 2, {f, pc.lit_int(WIDE, (i128)1 << (n->bits + 1))}), pc.lit_null(n->type), v);
  }
};

// ---------------------------------------------------------------- accumulators
struct AccDef { int kind; NodeP arg; DType type; };

// The scan side of one compile: the program over the input and the accumulators found so far.  Aggregates share accumulators
// (SUM(x) and AVG(x) keep one sum, every COUNT(*) one count), so all of them are asked for through acc().
struct Scan {
  ExprCompiler ec;
  std::vector<AccDef> accs;
  bool ungrouped = false;
  std::string fn;               // the function being compiled as the descriptor names it, upper-cased: error texts quote it
  const Json* desc = nullptr;   // ... and its aggr_expr entry
  // The moment aggregates sum over x - K.  K is run-time parameter k of the scan program and of the result projection
  // (ExprCompiler::param_f64); it is picked, on the device, from the values `origin_of[k]` takes on the rows that take part: a
  // second small program (`pick`, the same predicate) has them as its outputs.  One K per distinct argument.
  ExprCompiler pick;
  std::vector<NodeP> origin_of;
  explicit Scan(const Schema& in) : ec(in), pick(in) {}
  int origin(const NodeP& candidate) {
    for (size_t k = 0; k < origin_of.size(); ++k) if (origin_of[k]->key == candidate->key) return (int)k;
    if ((int)origin_of.size() >= MAX_ORIGINS) throw Unsupported("aggregate needs more than " + std::to_string(MAX_ORIGINS) + " moment arguments");
    origin_of.push_back(candidate); pick.add_output(candidate); return (int)origin_of.size() - 1;
  }

  int acc(int kind, NodeP arg, const DType& type) {
    for (size_t i = 0; i < accs.size(); ++i)
      if (accs[i].kind == kind && ((!arg && !accs[i].arg) || (arg && accs[i].arg && arg->key == accs[i].arg->key))) return (int)i;
    if ((int)accs.size() >= MAX_ACCS) throw Unsupported("aggregate needs more than " + std::to_string(MAX_ACCS) + " accumulators");
    accs.push_back({kind, arg, type}); return (int)accs.size() - 1;
  }
  [[noreturn]] void refuse_type(const DType& t) const { throw Unsupported(fn + " over " + t.to_string()); }
  // a value is NULL where no non-NULL argument was seen; ungrouped: zero input rows -> NULL
  bool may_be_null(const NodeP& x) const { return x->nullable || ungrouped; }
  // rows with a non-NULL x (no x: COUNT(*)); a non-nullable x shares the one row count
  int count(const NodeP& x) { return x && x->nullable ? acc(ACC_COUNT, x, I64) : acc(ACC_COUNT_STAR, nullptr, I64); }
  // the sum of an argument by its type.  sum_return_type [UPSTREAM-KNOWLEDGE]: decimal(p, s) -> decimal(p + 10, s); signed integers of
  // any width -> Int64, unsigned -> UInt64 (SUM) or through f64 (AVG); floats in f64
  int sum(const NodeP& x, bool exact_ints) {
    if (x->type.is_decimal()) return acc(ACC_SUM, x, dec_t(x->type.p + 10, x->type.s));
    if (x->type.is_int() && exact_ints) { const DType st = x->type.is_unsigned() ? U64 : I64; return acc(ACC_SUM, ec.cast(x, st), st); }
    if (x->type.is_float() || x->type.is_int()) return fsum(ec.cast(x, F64));
    refuse_type(x->type);
  }
  int fsum(const NodeP& x) { return acc(ACC_FSUM, x, F64); }
  // BIT_AND / BIT_OR / BIT_XOR keep the low 64 bits of the argument's two's-complement pattern; the declared type is the argument's
  int bitwise(int kind, const NodeP& x) { return acc(kind, x, x->type); }
  int minmax(const NodeP& x, bool minimum) { return x->type.is_float() ? acc(minimum ? ACC_FMIN : ACC_FMAX, x, x->type) : acc(minimum ? ACC_MIN : ACC_MAX, x, x->type); }
  // the variance family works in f64
  NodeP f64_arg(const NodeP& x) {
    if (!(x->type.is_float() || x->type.is_int() || x->type.is_decimal())) refuse_type(x->type);
    return ec.cast(x, F64);
  }
  NodeP second_f64_arg() {
    if (!desc->has("expr2")) throw std::runtime_error(fn + " needs two arguments (expr, expr2)");
    return ec.cast(ec.from_json(desc->at("expr2")), F64);
  }
  // merging Partial states: counts add up; a float state sums through COALESCE0 (an empty group's state is NULL) as FSUM, any other exactly
  int state_count(const NodeP& c) { return acc(ACC_SUM, ec.cast(c, I64), I64); }
  int state_sum(const NodeP& s) { return s->type.is_float() ? acc(ACC_FSUM, ec.coalesce0(s), s->type) : acc(ACC_SUM, s, s->type); }
};

// Final modes: the state columns arrive positionally after the group columns; every one is taken through here, in order
struct States {
  ExprCompiler& ec; size_t next, end;
  NodeP take() { if (next >= end) throw std::runtime_error("Final aggregate: input has too few state columns"); return ec.column((int)next++); }
  NodeP take_f64() { return ec.cast(take(), F64); }
};

struct AggFn;
// How one aggregate of the descriptor maps to accumulators (indices into Scan::accs)
struct AggPlan {
  const AggFn* fn = nullptr; std::string name;
  bool arg_nullable = false;    // the value goes through NULLIF0 on cnt (Scan::may_be_null of the argument)
  int arg_precision = 0;        // AVG over decimals: the argument's precision
  int cnt = -1, sum = -1, mm = -1;      // count / sum / min-max accumulators
  int sx = -1, sy = -1, sxx = -1, syy = -1, sxy = -1;      // variance family: f64 power sums about the origins
  int kx = -1, ky = -1;         // ... and which origins (Scan::origin)
};

// The result side: a post program over the SoA result [key_0.., acc_0..] and the names of its outputs
struct Post {
  ExprCompiler& pc; int nk; const std::vector<AccDef>& accs; std::vector<std::string>& names;
  NodeP acc(int i) { return pc.column(nk + i); }
  NodeP guard(const AggPlan& pl, NodeP v) { return pl.cnt >= 0 && pl.arg_nullable ? pc.nullif0(v, acc(pl.cnt)) : v; }
  void out(NodeP v, const std::string& name) { pc.add_output(v); names.push_back(name); }
  // a bitwise cell (lo = 64 pattern bits, hi = 0) as a value of its accumulator's integer type: sign- or zero-extended from that type's width
  NodeP bits_of(int i) { const DType& t = accs[i].type; return pc.raw(OP_WRAP, t, false, acc(i)->bits, {acc(i)}, (uint32_t)(type_width(t) * 8) | (t.is_unsigned() ? 0x100u : 0u)); }
};

// VARIANCE / STDDEV / COVARIANCE / CORRELATION (datafusion.proto:639-645).  The reference keeps Welford-style
// running (count, mean, m2[, algo_const]) states [UPSTREAM-KNOWLEDGE]; a data-parallel device cannot follow a
// row order, so the accumulators are order-free power sums in f64 -- of d = x - Kx and e = y - Ky, not of x and y:
// n, Sx = sum d, Sy = sum e, Sxx = sum d*d, Syy = sum e*e, Sxy = sum d*e, and the reference's state columns are derived
// from them (mean = Kx + Sx/n, m2 = Sxx - Sx^2/n, algo = Sxy - Sx*Sy/n).  The origin K is one value per argument and
// run, picked on the device from the rows that take part (Scan::origin; a Final picks it from the state means), so it
// lies inside the data's range R = max - min and |d| <= R: the subtraction in m2 then cancels like (R/sigma)^2
// whatever the data's offset from zero, where sums of x itself cancel like (mean/sigma)^2 -- STDDEV over a second of
// microsecond timestamps was noise.  |error(m2)| <= (3n + 8) * 2^-53 * (M2 + n R^2); tests/float_agg_exact.py states
// the bound, DESIGN.md ("Accuracy of the moment aggregates") what it leaves open: R spans every group of the operator.
// Both directions of the conversion, over a group's count n:
struct Moments {
  ExprCompiler& c; NodeP n, nf, zero;
  Moments(ExprCompiler& c_, NodeP count) : c(c_), n(count), nf(c_.cast(count, F64)), zero(c_.lit_f64(0.0)) {}
  // states -> power sums about (Ka, Kb), to be added up (a Final's scan program): Sa = n * (mean_a - Ka),
  // Sab = central_ab + n * (mean_a - Ka) * (mean_b - Kb)
  NodeP sum(NodeP off_a) { return c.binary("*", nf, off_a); }
  NodeP product_sum(NodeP central, NodeP off_a, NodeP off_b) { return c.binary("+", central, c.binary("*", nf, c.binary("*", off_a, off_b))); }
  // power sums -> states and statistics (the result projection)
  NodeP F(int op, NodeP l, NodeP r) { return c.raw(op, F64, false, 127, {l, r}); }
  NodeP sqrt(NodeP v) { return c.raw(OP_FSQRT, F64, false, 127, {v}); }
  NodeP n_is0() { return c.binary("=", n, c.lit_int(I64, 0)); }
  NodeP when0(NodeP v) { return c.select(n_is0(), zero, v); }                    // state columns of an empty group are 0
  NodeP nonneg(NodeP v) { return c.select(c.raw(OP_FLT, BOOL, false, 1, {v, zero}), zero, v); }   // rounding can leave -eps
  // the mean state of an empty group is 0, like every state column: NULL where n is 0, then NULL as 0 -- both in place, no register
  // for the test or the zero (tests/test_cpu_agg_compile.py, nine_aggregates: that Partial's states fit one post program only so)
  NodeP mean(NodeP sa, NodeP k) { return c.coalesce0(c.nullif0(F(OP_FADD, k, F(OP_FDIV, sa, nf)), n)); }
  NodeP central(NodeP sab, NodeP sa, NodeP sb) { return when0(F(OP_FSUB, sab, F(OP_FDIV, F(OP_FMUL, sa, sb), nf))); }
  NodeP m2(NodeP saa, NodeP sa) { return nonneg(central(saa, sa, sa)); }
  // sample statistics divide by n - 1 and need n >= 2, population by n and n >= 1; NULL otherwise
  NodeP per_n(NodeP v, bool population) { return F(OP_FDIV, v, population ? nf : F(OP_FSUB, nf, c.lit_f64(1.0))); }
  NodeP where_defined(NodeP v, bool population) { return c.select(population ? n_is0() : c.binary("<=", n, c.lit_int(I64, 1)), c.lit_null(F64), v); }
};

// ---------------------------------------------------------------- the aggregate functions
struct AggParts {
  void (*from_args)(Scan&, AggPlan&, NodeP x);      // Single, Partial: accumulators over the argument(s)
  void (*from_states)(Scan&, AggPlan&, States&);    // Final, FinalPartitioned, Merge: accumulators over the Partial's state columns
  void (*states)(Post&, const AggPlan&);            // Partial, Merge: the state columns, in the order from_states takes them
  void (*value)(Post&, const AggPlan&);             // Single, Final: the value
};
struct AggFn {
  std::vector<const char*> names;      // upper case; the first is the one the documents use
  AggParts parts;
  int args;                            // 1, 2, or 0: the argument may be left out (COUNT(*))
  bool minimum, population, stddev;    // MIN not MAX; divide by n not n - 1; the square root of the variance
  int kind = 0; const char* state = "";      // the bitwise family: its accumulator kind and its state column's suffix (format_state_name [UPSTREAM-KNOWLEDGE])
};
template <class D> AggParts parts() { return {D::from_args, D::from_states, D::states, D::value}; }

struct Count {
  static void from_args(Scan& s, AggPlan& pl, NodeP x) { pl.cnt = s.count(x); }
  static void from_states(Scan& s, AggPlan& pl, States& st) { pl.cnt = s.state_count(st.take()); }
  static void states(Post& p, const AggPlan& pl) { p.out(p.acc(pl.cnt), pl.name + "[count]"); }
  static void value(Post& p, const AggPlan& pl) { p.out(p.acc(pl.cnt), pl.name); }
};
struct Sum {
  static void from_args(Scan& s, AggPlan& pl, NodeP x) {
    pl.arg_nullable = s.may_be_null(x);
    pl.sum = s.sum(x, true);
    if (pl.arg_nullable) pl.cnt = s.count(x);
  }
  static void from_states(Scan& s, AggPlan& pl, States& st) {
    NodeP v = st.take();
    pl.arg_nullable = s.may_be_null(v);
    pl.sum = s.state_sum(v);
    if (pl.arg_nullable) pl.cnt = s.count(v);
  }
  static void states(Post& p, const AggPlan& pl) { p.out(p.guard(pl, p.acc(pl.sum)), pl.name + "[sum]"); }
  static void value(Post& p, const AggPlan& pl) { p.out(p.guard(pl, p.acc(pl.sum)), pl.name); }
};
struct Avg {
  static void from_args(Scan& s, AggPlan& pl, NodeP x) {
    pl.arg_nullable = s.may_be_null(x); pl.arg_precision = x->type.p;
    pl.sum = s.sum(x, false);
    pl.cnt = s.count(x);
  }
  static void from_states(Scan& s, AggPlan& pl, States& st) {
    NodeP c = st.take(), v = st.take();
    pl.arg_nullable = s.may_be_null(v);      // (read by `states` alone: a Merge hands the sum on NULL where the merged count is 0, as the Partial did)
    pl.cnt = s.state_count(c);
    pl.sum = s.state_sum(v);
    pl.arg_precision = std::max(1, v->type.p - 10);      // the sum state is Decimal(min(38,p+10), s); the argument was Decimal(p, s)
  }
  static void states(Post& p, const AggPlan& pl) {
    p.out(p.pc.cast(p.acc(pl.cnt), U64), pl.name + "[count]");
    p.out(p.guard(pl, p.acc(pl.sum)), pl.name + "[sum]");
  }
  static void value(Post& p, const AggPlan& pl) {
    const DType st = p.accs[pl.sum].type;
    if (st.is_float()) {
      NodeP cnt = p.pc.cast(p.acc(pl.cnt), F64);
      p.out(p.pc.nullif0(p.pc.raw(OP_FDIV, F64, true, 127, {p.acc(pl.sum), cnt}), p.acc(pl.cnt)), pl.name);
    } else {
      // Decimal AVG: sum * 10^(s_avg - s_sum) / count, truncating; count == 0 -> NULL (OP_DIV by zero)
      const DType rt = dec_t(pl.arg_precision + 4, st.s + 4);
      NodeP scaled = p.pc.raw(OP_MUL, rt, false, 127, {p.acc(pl.sum), p.pc.lit_int(WIDE, pow10_i128(rt.s - st.s))});
      p.out(p.pc.raw(OP_DIV, rt, true, 127, {scaled, p.acc(pl.cnt)}), pl.name);
    }
  }
};
struct MinMax {
  static void from_args(Scan& s, AggPlan& pl, NodeP x) {
    if (!(x->type.is_float() || x->type.is_int() || x->type.is_decimal() || x->type.is_temporal())) s.refuse_type(x->type);
    pl.arg_nullable = s.may_be_null(x);
    pl.mm = s.minmax(x, pl.fn->minimum);
    if (pl.arg_nullable) pl.cnt = s.count(x);
  }
  static void from_states(Scan& s, AggPlan& pl, States& st) {
    NodeP v = st.take();
    pl.arg_nullable = s.may_be_null(v);
    pl.mm = s.minmax(v, pl.fn->minimum);
    if (pl.arg_nullable) pl.cnt = s.count(v);
  }
  static void states(Post& p, const AggPlan& pl) { p.out(p.guard(pl, p.acc(pl.mm)), pl.name + (pl.fn->minimum ? "[min]" : "[max]")); }
  static void value(Post& p, const AggPlan& pl) { p.out(p.guard(pl, p.acc(pl.mm)), pl.name); }
};
// BIT_AND / BIT_OR / BIT_XOR (datafusion.proto:650-652) over the eight integer types: result and state have the argument's type
struct Bitwise {
  static void from_args(Scan& s, AggPlan& pl, NodeP x) {
    if (!x->type.is_int()) s.refuse_type(x->type);
    pl.arg_nullable = s.may_be_null(x);
    pl.mm = s.bitwise(pl.fn->kind, x);
    if (pl.arg_nullable) pl.cnt = s.count(x);
  }
  static void from_states(Scan& s, AggPlan& pl, States& st) { from_args(s, pl, st.take()); }      // the state merges as the argument folds
  static void states(Post& p, const AggPlan& pl) { p.out(p.guard(pl, p.bits_of(pl.mm)), pl.name + pl.fn->state); }
  static void value(Post& p, const AggPlan& pl) { p.out(p.guard(pl, p.bits_of(pl.mm)), pl.name); }
};
// BOOL_AND / BOOL_OR (datafusion.proto:653-654): the AND / OR of the 0/1 register value in an Int64-typed cell; the value is cell != 0
struct BoolAgg {
  static void from_args(Scan& s, AggPlan& pl, NodeP x) {
    if (x->type.id != T_BOOL) s.refuse_type(x->type);
    pl.arg_nullable = s.may_be_null(x);
    pl.mm = s.bitwise(pl.fn->kind, s.ec.cast(x, I64));
    if (pl.arg_nullable) pl.cnt = s.count(x);
  }
  static void from_states(Scan& s, AggPlan& pl, States& st) { from_args(s, pl, st.take()); }
  static NodeP truth(Post& p, const AggPlan& pl) { return p.guard(pl, p.pc.raw(OP_NE, BOOL, false, 2, {p.acc(pl.mm), p.pc.lit_int(I64, 0)})); }
  static void states(Post& p, const AggPlan& pl) { p.out(truth(p, pl), pl.name + pl.fn->state); }
  static void value(Post& p, const AggPlan& pl) { p.out(truth(p, pl), pl.name); }
};
// an argument (or a state mean) about its origin: x - K, NULL where x is
NodeP about(ExprCompiler& ec, const NodeP& x, int k) { return ec.binary("-", x, ec.param_f64(k)); }
// what a Final picks an origin from: the mean of a state row that stands for at least one input row (an empty group's mean is 0, not data)
NodeP mean_of_rows(ExprCompiler& ec, const NodeP& count, const NodeP& mean) {
  return ec.select(ec.binary(">", ec.cast(count, I64), ec.lit_int(I64, 0)), mean, ec.lit_null(F64));
}
// the two-argument functions skip a row where either argument is NULL, for every sum
void pair_up(ExprCompiler& ec, NodeP& x, NodeP& y) {
  NodeP both = ec.binary("AND", ec.is_null(x, true), ec.is_null(y, true));
  if (x->nullable || y->nullable) { NodeP x2 = ec.select(both, x, ec.lit_null(F64)); NodeP y2 = ec.select(both, y, ec.lit_null(F64)); x = x2; y = y2; }
}
struct Variance {      // and its square root
  static void from_args(Scan& s, AggPlan& pl, NodeP arg) {
    NodeP x = s.f64_arg(arg);
    pl.kx = s.origin(x);
    NodeP d = about(s.ec, x, pl.kx);
    pl.cnt = s.count(x); pl.sx = s.fsum(d); pl.sxx = s.fsum(s.ec.binary("*", d, d));
  }
  static void from_states(Scan& s, AggPlan& pl, States& st) {
    NodeP c = st.take(); Moments M(s.ec, c);
    pl.cnt = s.state_count(c);
    NodeP mean = st.take_f64(), m2 = st.take_f64();
    pl.kx = s.origin(mean_of_rows(s.ec, c, mean));
    NodeP d = about(s.ec, mean, pl.kx);
    pl.sx = s.state_sum(M.sum(d)); pl.sxx = s.state_sum(M.product_sum(m2, d, d));
  }
  static void states(Post& p, const AggPlan& pl) {
    Moments M(p.pc, p.acc(pl.cnt));
    p.out(p.pc.cast(M.n, U64), pl.name + "[count]");
    p.out(M.mean(p.acc(pl.sx), p.pc.param_f64(pl.kx)), pl.name + "[mean]");
    p.out(M.m2(p.acc(pl.sxx), p.acc(pl.sx)), pl.name + "[m2]");
  }
  static void value(Post& p, const AggPlan& pl) {
    Moments M(p.pc, p.acc(pl.cnt));
    NodeP v = M.per_n(M.m2(p.acc(pl.sxx), p.acc(pl.sx)), pl.fn->population);
    if (pl.fn->stddev) v = M.sqrt(v);
    p.out(M.where_defined(v, pl.fn->population), pl.name);
  }
};
struct Covariance {
  static void from_args(Scan& s, AggPlan& pl, NodeP arg) {
    NodeP x = s.f64_arg(arg), y = s.second_f64_arg();
    pair_up(s.ec, x, y);
    pl.kx = s.origin(x); pl.ky = s.origin(y);
    NodeP d = about(s.ec, x, pl.kx), e = about(s.ec, y, pl.ky);
    pl.cnt = s.count(x); pl.sx = s.fsum(d); pl.sy = s.fsum(e); pl.sxy = s.fsum(s.ec.binary("*", d, e));
  }
  static void from_states(Scan& s, AggPlan& pl, States& st) {
    NodeP c = st.take(); Moments M(s.ec, c);
    pl.cnt = s.state_count(c);
    NodeP mean1 = st.take_f64(), mean2 = st.take_f64(), algo = st.take_f64();
    pl.kx = s.origin(mean_of_rows(s.ec, c, mean1)); pl.ky = s.origin(mean_of_rows(s.ec, c, mean2));
    NodeP d = about(s.ec, mean1, pl.kx), e = about(s.ec, mean2, pl.ky);
    pl.sx = s.state_sum(M.sum(d)); pl.sy = s.state_sum(M.sum(e)); pl.sxy = s.state_sum(M.product_sum(algo, d, e));
  }
  static void states(Post& p, const AggPlan& pl) {
    Moments M(p.pc, p.acc(pl.cnt));
    p.out(p.pc.cast(M.n, U64), pl.name + "[count]");
    p.out(M.mean(p.acc(pl.sx), p.pc.param_f64(pl.kx)), pl.name + "[mean1]");
    p.out(M.mean(p.acc(pl.sy), p.pc.param_f64(pl.ky)), pl.name + "[mean2]");
    p.out(M.central(p.acc(pl.sxy), p.acc(pl.sx), p.acc(pl.sy)), pl.name + "[algoConst]");
  }
  static void value(Post& p, const AggPlan& pl) {
    Moments M(p.pc, p.acc(pl.cnt));
    p.out(M.where_defined(M.per_n(M.central(p.acc(pl.sxy), p.acc(pl.sx), p.acc(pl.sy)), pl.fn->population), pl.fn->population), pl.name);
  }
};
struct Correlation {
  static void from_args(Scan& s, AggPlan& pl, NodeP arg) {
    NodeP x = s.f64_arg(arg), y = s.second_f64_arg();
    pair_up(s.ec, x, y);
    pl.kx = s.origin(x); pl.ky = s.origin(y);
    NodeP d = about(s.ec, x, pl.kx), e = about(s.ec, y, pl.ky);
    pl.cnt = s.count(x); pl.sx = s.fsum(d); pl.sxx = s.fsum(s.ec.binary("*", d, d));
    pl.sy = s.fsum(e); pl.sxy = s.fsum(s.ec.binary("*", d, e)); pl.syy = s.fsum(s.ec.binary("*", e, e));
  }
  static void from_states(Scan& s, AggPlan& pl, States& st) {
    NodeP c = st.take(); Moments M(s.ec, c);
    pl.cnt = s.state_count(c);
    NodeP mean1 = st.take_f64(), m2_1 = st.take_f64(), mean2 = st.take_f64(), m2_2 = st.take_f64(), algo = st.take_f64();
    pl.kx = s.origin(mean_of_rows(s.ec, c, mean1)); pl.ky = s.origin(mean_of_rows(s.ec, c, mean2));
    NodeP d = about(s.ec, mean1, pl.kx), e = about(s.ec, mean2, pl.ky);
    pl.sx = s.state_sum(M.sum(d)); pl.sxx = s.state_sum(M.product_sum(m2_1, d, d));
    pl.sy = s.state_sum(M.sum(e)); pl.syy = s.state_sum(M.product_sum(m2_2, e, e));
    pl.sxy = s.state_sum(M.product_sum(algo, d, e));
  }
  static void states(Post& p, const AggPlan& pl) {
    Moments M(p.pc, p.acc(pl.cnt));
    p.out(p.pc.cast(M.n, U64), pl.name + "[count]");
    p.out(M.mean(p.acc(pl.sx), p.pc.param_f64(pl.kx)), pl.name + "[mean1]");
    p.out(M.m2(p.acc(pl.sxx), p.acc(pl.sx)), pl.name + "[m2_1]");
    p.out(M.mean(p.acc(pl.sy), p.pc.param_f64(pl.ky)), pl.name + "[mean2]");
    p.out(M.m2(p.acc(pl.syy), p.acc(pl.sy)), pl.name + "[m2_2]");
    p.out(M.central(p.acc(pl.sxy), p.acc(pl.sx), p.acc(pl.sy)), pl.name + "[algoConst]");
  }
  static void value(Post& p, const AggPlan& pl) {
    // corr = cov_pop / (sd_pop_x * sd_pop_y); 0 when either deviation is 0; NULL over no rows
    Moments M(p.pc, p.acc(pl.cnt));
    NodeP sx = M.sqrt(M.F(OP_FDIV, M.m2(p.acc(pl.sxx), p.acc(pl.sx)), M.nf)), sy = M.sqrt(M.F(OP_FDIV, M.m2(p.acc(pl.syy), p.acc(pl.sy)), M.nf));
    NodeP flat = p.pc.binary("OR", p.pc.raw(OP_FEQ, BOOL, false, 1, {sx, M.zero}), p.pc.raw(OP_FEQ, BOOL, false, 1, {sy, M.zero}));
    NodeP v = M.F(OP_FDIV, M.F(OP_FDIV, M.F(OP_FDIV, M.central(p.acc(pl.sxy), p.acc(pl.sx), p.acc(pl.sy)), M.nf), sx), sy);
    p.out(p.pc.select(M.n_is0(), p.pc.lit_null(F64), p.pc.select(flat, M.zero, v)), pl.name);
  }
};

// Function names: datafusion.proto:631-669 and the aliases SQL front ends send.  include/gpuq.h lists them for callers.
const AggFn AGG_FNS[] = {
  // names                                      parts                 args  minimum population stddev
  {{"COUNT"},                                   parts<Count>(),       0,    false,  false,     false},
  {{"SUM"},                                     parts<Sum>(),         1,    false,  false,     false},
  {{"AVG"},                                     parts<Avg>(),         1,    false,  false,     false},
  {{"MIN"},                                     parts<MinMax>(),      1,    true,   false,     false},
  {{"MAX"},                                     parts<MinMax>(),      1,    false,  false,     false},
  {{"VARIANCE", "VAR", "VAR_SAMP"},             parts<Variance>(),    1,    false,  false,     false},
  {{"VARIANCE_POP", "VAR_POP"},                 parts<Variance>(),    1,    false,  true,      false},
  {{"STDDEV", "STDDEV_SAMP"},                   parts<Variance>(),    1,    false,  false,     true},
  {{"STDDEV_POP"},                              parts<Variance>(),    1,    false,  true,      true},
  {{"COVARIANCE", "COVAR", "COVAR_SAMP"},       parts<Covariance>(),  2,    false,  false,     false},
  {{"COVARIANCE_POP", "COVAR_POP"},             parts<Covariance>(),  2,    false,  true,      false},
  {{"CORRELATION", "CORR"},                     parts<Correlation>(), 2,    false,  false,     false},
  {{"BIT_AND"},                                 parts<Bitwise>(),     1,    false,  false,     false,  ACC_BAND, "[bit_and]"},
  {{"BIT_OR"},                                  parts<Bitwise>(),     1,    false,  false,     false,  ACC_BOR,  "[bit_or]"},
  {{"BIT_XOR"},                                 parts<Bitwise>(),     1,    false,  false,     false,  ACC_BXOR, "[bit_xor]"},
  {{"BOOL_AND"},                                parts<BoolAgg>(),     1,    false,  false,     false,  ACC_BAND, "[bool_and]"},
  {{"BOOL_OR"},                                 parts<BoolAgg>(),     1,    false,  false,     false,  ACC_BOR,  "[bool_or]"},
};
const AggFn* find_agg_fn(const std::string& upper_name) {
  for (const AggFn& f : AGG_FNS) for (const char* n : f.names) if (upper_name == n) return &f;
  return nullptr;
}

}  // namespace

// ---------------------------------------------------------------- the compile
AggCompiled compile_aggregate(const Schema& in, const Json& d) {
  AggCompiled R;
  R.mode = d.get_str("mode", "Single");
  // Merge: states in, states out -- from_states on the scan side, as a Final, `states` on the result side, as a Partial.  DataFusion has no
  // such mode; the plan executor's lowering of grouping sets re-keys a Partial's output with it (plan_exec.cpp, GroupingExpand).
  const bool is_final = (R.mode == "Final" || R.mode == "FinalPartitioned" || R.mode == "Merge");
  const bool emit_state = (R.mode == "Partial" || R.mode == "Merge");
  if (!is_final && !emit_state && R.mode != "Single") throw std::runtime_error("unknown aggregate mode '" + R.mode + "'");
  R.strategy = d.get_str("strategy", "auto");
  R.expected_groups = d.get_i64("expected_groups", 0);
  Scan s(in);
  ExprCompiler& ec = s.ec;
  if (d.has("predicate")) ec.add_predicate(ec.from_json(d.at("predicate")));
  std::vector<NodeP> declared; std::vector<std::string> declared_names;
  if (d.has("group_expr")) for (const Json& g : d.at("group_expr").a) {
    declared.push_back(ec.from_json(g.at("expr"))); declared_names.push_back(g.get_str("name", "group" + std::to_string(declared.size() - 1)));
  }
  const GroupKeys keys(ec, declared, declared_names);
  R.refuse = keys.refuse;
  s.ungrouped = keys.nodes.empty();
  States states{ec, keys.declared(), in.fields.size()};
  std::vector<AggPlan> plans;
  for (const Json& a : d.at("aggr_expr").a) {
    s.fn = a.at("fn").str(); s.desc = &a;
    AggPlan pl; pl.name = a.get_str("name", s.fn);
    for (auto& ch : s.fn) ch = (char)std::toupper(ch);
    if (a.get_bool("distinct", false)) throw Unsupported("DISTINCT aggregates are not supported on device");
    pl.fn = find_agg_fn(s.fn);
    if (!is_final) {
      NodeP arg = a.has("expr") ? ec.from_json(a.at("expr")) : nullptr;
      // per-aggregate FILTER (AggregateExecNode.filter_expr, datafusion.proto:1437-1450): agg(x) FILTER (WHERE p) is agg over the rows
      // where p is true, i.e. agg(CASE WHEN p THEN x END) -- every accumulator here skips NULL arguments; COUNT(*) counts the 1s
      if (a.has("filter") && !a.at("filter").is_null()) {
        NodeP p = ec.from_json(a.at("filter"));
        if (p->type.id != T_BOOL) throw std::runtime_error("aggregate FILTER must be boolean");
        if (!arg) arg = ec.lit_int(I64, 1);
        arg = ec.select(p, arg, ec.lit_null(arg->type));
        if (a.has("expr2")) throw Unsupported("FILTER on a two-argument aggregate");
      }
      if (!arg && !(pl.fn && pl.fn->args == 0)) throw std::runtime_error(s.fn + " needs an argument");
      if (!pl.fn) throw Unsupported("aggregate function " + s.fn);
      pl.fn->parts.from_args(s, pl, arg);
    } else {
      if (!pl.fn) throw Unsupported("aggregate function " + s.fn);
      pl.fn->parts.from_states(s, pl, states);
    }
    plans.push_back(pl);
  }
  std::vector<AccDef>& accs = s.accs;
  if (accs.empty()) s.count(nullptr);   // GROUP BY without aggregates still needs a cell
  // scan program outputs: keys then accumulator arguments
  std::vector<int> key_slots, acc_slots(accs.size(), -1);
  for (auto& k : keys.nodes) key_slots.push_back(ec.add_output(k));
  for (size_t i = 0; i < accs.size(); ++i) if (accs[i].arg) acc_slots[i] = ec.add_output(accs[i].arg);
  R.prog = ec.finish();
  // the key-and-predicate program: what the runs count pass needs of `prog` (a head is decided by the key and by whether the row is
  // active; FILTER clauses and accumulator operands are outputs behind the keys and are no part of either)
  R.heads = ec.prune(R.prog, (int)keys.nodes.size());
  if (!s.origin_of.empty()) {      // (the predicate is a node of `ec`: a program is assembled from the DAG alone, whichever compiler built it)
    if (d.has("predicate")) s.pick.add_predicate(ec.from_json(d.at("predicate")));
    R.pick = s.pick.finish();
    R.n_origins = (int)s.origin_of.size();
  }
  const int nk = (int)keys.nodes.size();
  R.agg.n_keys = nk; R.agg.n_accs = (int)accs.size();
  std::vector<int> kregs; bool any_null_key = false;
  for (int k = 0; k < nk; ++k) {
    const NodeP& n = keys.nodes[k];
    R.agg.key_reg[k] = R.prog.out_reg[key_slots[k]]; kregs.push_back(R.agg.key_reg[k]);
    R.key_types.push_back(n->type); any_null_key = any_null_key || n->nullable;
    if (n->type.id == T_BOOL || n->type.id == T_NULL) throw Unsupported("group-by key of type " + n->type.to_string());
  }
  for (size_t i = 0; i < accs.size(); ++i) {
    R.agg.acc_kind[i] = accs[i].kind; R.agg.acc_reg[i] = accs[i].arg ? R.prog.out_reg[acc_slots[i]] : 0;
    R.acc_types.push_back(accs[i].type);
    R.acc_bits.push_back(accs[i].arg ? R.prog.out_bits[acc_slots[i]] : 1);
  }
  R.keys = make_keyspec(kregs, R.key_types, any_null_key);
  // The whole key in at most 62 bits (narrow integer / date columns, one NULL flag per nullable one): the global hash table keeps it in
  // the slot's state word (gpuq_kernels.h KeySpec::state_key).  Int64 and wider keys, strings and packed composites keep their key words.
  {
    int total = 0; bool narrow = nk > 0;
    for (int k = 0; k < nk && narrow; ++k) {
      int bits = 0; bool sgn = false;
      switch (keys.nodes[k]->type.id) {
        case T_INT8: bits = 8; sgn = true; break;   case T_UINT8: bits = 8; break;
        case T_INT16: bits = 16; sgn = true; break; case T_UINT16: bits = 16; break;
        case T_INT32: case T_DATE32: bits = 32; sgn = true; break; case T_UINT32: bits = 32; break;
        default: narrow = false;
      }
      R.keys.sk_bits[k] = bits; R.keys.sk_signed[k] = sgn; R.keys.sk_null[k] = keys.nodes[k]->nullable ? 1 : 0;
      total += bits + R.keys.sk_null[k];
    }
    R.keys.state_key = narrow && total <= 62;
  }

  // post programs over the SoA result: [key_0.., acc_0..] as raw (lo,hi) columns
  for (int k = 0; k < nk; ++k) { Field f; f.name = keys.names[k]; f.type = keys.nodes[k]->type; f.nullable = keys.nodes[k]->nullable; f.raw128 = 1; R.post_schema.fields.push_back(f); }
  for (size_t i = 0; i < accs.size(); ++i) { Field f; f.name = "acc" + std::to_string(i); f.type = accs[i].type; f.nullable = false; f.raw128 = 1; R.post_schema.fields.push_back(f); }
  // When all outputs do not fit one program, the plan list is split and each chunk becomes its own program over the same SoA
  // columns (a few extra launches over <= n_groups rows).
  std::function<void(size_t, size_t, bool)> emit = [&](size_t lo, size_t hi, bool with_keys) {
    ExprCompiler pc(R.post_schema);
    std::vector<std::string> names; CompiledProgram cp;
    try {
      if (with_keys) keys.project(pc, names);
      Post p{pc, nk, accs, names};
      for (size_t pi = lo; pi < hi; ++pi) (emit_state ? plans[pi].fn->parts.states : plans[pi].fn->parts.value)(p, plans[pi]);
      cp = pc.finish();
    }
    catch (const Unsupported&) { throw; }
    catch (const std::runtime_error&) {
      if (hi - lo + (with_keys ? 1 : 0) <= 1) throw;
      if (with_keys && hi > lo) { emit(lo, lo, true); emit(lo, hi, false); }
      else { const size_t mid = lo + (hi - lo) / 2; emit(lo, mid, with_keys); emit(mid, hi, false); }
      return;
    }
    if (cp.out_reg.empty()) return;
    const int first_out = (int)R.out_fields.size();
    for (size_t i = 0; i < cp.out_type.size(); ++i) R.out_fields.push_back(make_field(names[i], cp.out_type[i], cp.out_nullable[i]));
    R.posts.push_back({std::move(cp), first_out});
  };
  emit(0, plans.size(), true);
  return R;
}

}  // namespace gpuq
