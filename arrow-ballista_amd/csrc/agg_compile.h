// The aggregate compile (agg_compile.cpp): an "aggregate" operator descriptor -> everything the device runs for it.
// Pure host computation over a schema and a descriptor: no device, no operator handle; capi.cpp moves the result into
// its gpuq_op and uploads the programs.
#pragma once
#include "../../include/gpuq.h"
#include "expr_compile.h"
#include "gpuq_kernels.h"      // AggSpec, KeySpec, MAX_KEYS / MAX_ACCS; the error types
#include <string>
#include <vector>

namespace gpuq {

gpuq_field_info make_field(const std::string& name, const DType& t, bool nullable);
// key layout of a hash table (group-by, join, partition) over the registers a program leaves its keys in
KeySpec make_keyspec(const std::vector<int>& regs, const std::vector<DType>& types, bool null_word);

struct AggCompiled {
  std::string mode = "Single", strategy = "auto";
  i64 expected_groups = 0;
  CompiledProgram prog;             // the scan program: outputs are the keys, then the accumulator arguments
  // `prog` cut down to the keys and the predicate (ExprCompiler::prune): same registers, so `keys` addresses both; for every row the key
  // registers and the predicate are bit for bit those of `prog`.  Empty (!heads.pruned()) when that removes nothing: `prog` serves then.
  CompiledProgram heads;
  // The moment aggregates (VARIANCE .. CORRELATION) sum about origins picked at run time: run-time parameter k (param_imm of `prog`
  // and of every post program that reads it) is output k of `pick`, a program over the same input with the same predicate, taken
  // from the first row that passes and is not NULL there.  n_origins == 0: no moment aggregate, `pick` is empty.
  CompiledProgram pick; int n_origins = 0;
  AggSpec agg{}; KeySpec keys{};
  std::vector<DType> key_types, acc_types;
  std::vector<int> acc_bits;        // |argument| < 2^bits per accumulator (type-derived)
  Schema post_schema;               // the SoA result [key_0.., acc_0..] as raw (lo,hi) columns: what the post programs read
  // The result projection.  The post programs run in the same 16-register machine as every other program: when all outputs do
  // not fit one, the projection is split into chunks, each its own program over the same columns.
  struct Post { CompiledProgram prog; int first_out = 0; };      // first_out: index in out_fields of the chunk's first output
  std::vector<Post> posts;
  std::vector<gpuq_field_info> out_fields;
  std::string refuse;               // the operator compiles (its output types are known) but cannot run: why
};
AggCompiled compile_aggregate(const Schema& in, const Json& descriptor);

}  // namespace gpuq
