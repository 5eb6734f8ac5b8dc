// The exception types that map to the C ABI's status codes, and the one mapping between the two.  Plain C++ (no HIP): included by
// devbuf.h for every translation unit behind the C ABI, and by host-only programs on its own.
#pragma once
#include "../../include/gpuq.h"
#include <new>
#include <stdexcept>
#include <string>

namespace gpuq {

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };
struct Unsupported : std::runtime_error { using std::runtime_error::runtime_error; };
// The refusals the plan executor answers by running the operator again in another form (gpuq_last_refusal): what says so is the type,
// never the wording.  Every other Unsupported is final.
struct LongString : Unsupported { using Unsupported::Unsupported; };       // a Utf8 value beyond 15 bytes reached a packed key / comparison
struct WideSortKey : Unsupported { using Unsupported::Unsupported; };      // a composite sort key beyond 128 bits
struct NotNative : Unsupported { using Unsupported::Unsupported; };        // a plan node the native executor does not run
struct Capacity : std::runtime_error { using std::runtime_error::runtime_error; };
struct Retry : std::runtime_error { using std::runtime_error::runtime_error; };      // deferred execution: an assumption did not hold (GPUQ_ERR_RETRY)

// What the calling thread's last failing call refused (a gpuq_refusal).  Written by every catch clause that turns an exception into a
// status -- status_of_exception, and the units' own clauses in front of it, which record GPUQ_REFUSAL_NONE -- and by nothing else.
inline int& tls_refusal() { thread_local int r = GPUQ_REFUSAL_NONE; return r; }

// The one mapping from what the library throws to the C ABI's status codes.  Call it inside a catch block: it rethrows the exception
// in flight, returns its status and leaves its message in `err` (each boundary names its own thread-local string: the one behind its
// gpuq_*_last_error).  A unit with exception types of its own catches those first and hands everything else over.
inline int status_of_exception(std::string& err) {
  int& refusal = tls_refusal();
  refusal = GPUQ_REFUSAL_NONE;
  try { throw; }
  catch (const HipError& e) { err = e.what(); return GPUQ_ERR_HIP; }
  catch (const LongString& e) { err = e.what(); refusal = GPUQ_REFUSAL_LONG_STRING; return GPUQ_ERR_UNSUPPORTED; }
  catch (const WideSortKey& e) { err = e.what(); refusal = GPUQ_REFUSAL_WIDE_SORT_KEY; return GPUQ_ERR_UNSUPPORTED; }
  catch (const NotNative& e) { err = e.what(); refusal = GPUQ_REFUSAL_NODE_NOT_NATIVE; return GPUQ_ERR_UNSUPPORTED; }
  catch (const Unsupported& e) { err = e.what(); return GPUQ_ERR_UNSUPPORTED; }
  catch (const Capacity& e) { err = e.what(); return GPUQ_ERR_CAPACITY; }
  catch (const Retry& e) { err = e.what(); return GPUQ_ERR_RETRY; }
  catch (const std::bad_alloc&) { err = "out of host memory"; return GPUQ_ERR_INTERNAL; }
  catch (const std::exception& e) { err = e.what(); return GPUQ_ERR_INVALID; }
}
template <class F> int guarded_into(std::string& err, F&& f) {
  try { f(); return GPUQ_OK; }
  catch (...) { return status_of_exception(err); }
}
// ... and back, for a unit that calls the C ABI and goes on in C++: the Unsupported that a GPUQ_ERR_UNSUPPORTED with this refusal was
[[noreturn]] inline void throw_unsupported(int refusal, const std::string& msg) {
  switch (refusal) {
    case GPUQ_REFUSAL_LONG_STRING: throw LongString(msg);
    case GPUQ_REFUSAL_WIDE_SORT_KEY: throw WideSortKey(msg);
    case GPUQ_REFUSAL_NODE_NOT_NATIVE: throw NotNative(msg);
    default: throw Unsupported(msg);
  }
}

}  // namespace gpuq
