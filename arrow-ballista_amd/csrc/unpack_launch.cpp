// gpuq -- host side of the page / shuffle-block decompressors.
//   * ZSTD: the code object (kernels_zstd_dev.hip, embedded by build.py) is loaded as a module of its own on the first launch, per
//     device, and stays loaded.
//   * the parallel Snappy / LZ4 decoder (kernels_lz4.hip): the plan of one call -- block maps, round counts, scratch, launch order.
//     This is the only place that knows the kernels' scratch contract; callers hand over jobs with their placement fields.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <map>
#include <mutex>
#include <stdexcept>
#include <vector>
#include "devbuf.h"
#include "gpuq_kernels.h"

extern "C" const unsigned char gpuq_zstd_hsaco[];      // build/embedded_zstd.cpp (.incbin of the code object)

namespace gpuq {

static hipFunction_t zstd_kernel() {
  static std::mutex mu; static std::map<int, hipFunction_t> fns;
  int dev = 0; HIPCHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> g(mu);
  auto it = fns.find(dev);
  if (it != fns.end()) return it->second;
  hipModule_t mod = nullptr; hipFunction_t fn = nullptr;
  HIPCHECK(hipModuleLoadData(&mod, gpuq_zstd_hsaco));
  HIPCHECK(hipModuleGetFunction(&fn, mod, "gpuq_k_zstd_pages"));
  fns[dev] = fn;
  return fn;
}

size_t zstd_scratch_bytes(int n_pages) { return (size_t)n_pages * (size_t)(131072 + 64); }      // zs::BLOCK_MAX + 64 per page in flight

void launch_zstd_pages(hipStream_t s, const uint8_t* src, uint8_t* dst, const UnpackJob* jobs, const int32_t* which, int n, uint8_t* scratch, uint32_t* status) {
  if (n <= 0) return;
  void* args[] = {(void*)&src, (void*)&dst, (void*)&jobs, (void*)&which, (void*)&n, (void*)&scratch, (void*)&status};
  HIPCHECK(hipModuleLaunchKernel(zstd_kernel(), (unsigned)n, 1, 1, 64, 1, 1, 0, s, args, nullptr));
}

// ceil(log2(n)) + 1 doubling rounds close a chain of n links; one more is the round that finds nothing left
static int doubling_rounds(int64_t n) { int r = 1; while (((int64_t)1 << r) < n) ++r; return r + 1; }

void unpack_pages_parallel(hipStream_t s, const uint8_t* src, uint8_t* dst, const UnpackJob* jobs, int n, UnpackScratch& X, uint32_t* status) {
  if (n <= 0) return;
  // ---- what the jobs need.  A job whose prefix does not fit gets no block at all: k_sn_head refuses it.
  int64_t words = 0, slots = 0, max_frame = 0, max_in = 0;
  std::vector<uint2> blk, cblk;      // (job, first byte) per PJ_BLOCK_BYTES of output / of compressed positions, the end position included
  for (int k = 0; k < n; ++k) {
    const UnpackJob& j = jobs[k];
    if (j.mode == UNPACK_STORED || j.mode == UNPACK_ZSTD || j.raw_prefix > j.src_len || j.raw_prefix > j.dst_len) continue;
    const int64_t len = j.dst_len - j.raw_prefix, cl = j.src_len - j.raw_prefix;
    for (int64_t b = 0; b < len; b += PJ_BLOCK_BYTES) blk.push_back(make_uint2((uint32_t)k, (uint32_t)b));
    words = std::max(words, (j.s_off + len + 3) & ~(int64_t)3); max_frame = std::max(max_frame, j.p_base + len);
    if (!unpack_job_is_compressed(j)) continue;
    if (j.c_off != slots) throw std::logic_error("unpack_pages_parallel: the compressed jobs' c_off are not back to back");
    for (int64_t b = 0; b <= cl; b += PJ_BLOCK_BYTES) cblk.push_back(make_uint2((uint32_t)k, (uint32_t)b));
    slots += cl + 1; max_in = std::max(max_in, cl);
  }
  const int rounds = doubling_rounds(max_frame), mark_rounds = doubling_rounds(max_in + 1);
  // ---- scratch.  counts: a word per job for every mark round (+ the one before the first), then the same for the resolve rounds
  const size_t count_words = (size_t)(rounds + mark_rounds + 3) * (size_t)n, scan_bytes = exclusive_scan_ws_bytes(slots + 1);
  X.jobs.ensure((size_t)n * sizeof(UnpackJob) + 64); X.resolve.ensure((size_t)words * 4 + 64);
  X.blkmap.ensure(blk.size() * sizeof(uint2) + 64); X.cmap.ensure(cblk.size() * sizeof(uint2) + 64); X.counts.ensure(count_words * 4 + 64);
  X.jump_a.ensure((size_t)(slots + 1) * 4 + 64); X.jump_b.ensure((size_t)(slots + 1) * 4 + 64); X.olen.ensure((size_t)(slots + 1) * 4 + 64);
  X.mark.ensure((size_t)slots + 64); X.scan.ensure(scan_bytes);
  HIPCHECK(hipMemcpyAsync(X.jobs.p, jobs, (size_t)n * sizeof(UnpackJob), hipMemcpyHostToDevice, s));
  if (!blk.empty()) HIPCHECK(hipMemcpyAsync(X.blkmap.p, blk.data(), blk.size() * sizeof(uint2), hipMemcpyHostToDevice, s));
  if (!cblk.empty()) HIPCHECK(hipMemcpyAsync(X.cmap.p, cblk.data(), cblk.size() * sizeof(uint2), hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemsetAsync(X.counts.p, 0, count_words * 4, s));
  HIPCHECK(hipMemsetAsync(X.mark.p, 0, (size_t)slots + 64, s));
  const UnpackJob* dj = X.jobs.as<UnpackJob>();
  const uint2* bm = X.blkmap.as<uint2>(); const uint2* cm = X.cmap.as<uint2>();
  uint32_t* resolve = X.resolve.as<uint32_t>(); uint8_t* mark = X.mark.as<uint8_t>(); uint32_t* counts = X.counts.as<uint32_t>();
  const int nb = (int)blk.size(), nc = (int)cblk.size();
  // ---- front: which positions of the compressed streams are elements, and where their output goes
  launch_sn_head(s, src, dst, dj, n, mark, resolve, status);
  if (nb > 0) {
    if (nc > 0) {      // (none: linked LZ4 frames of stored blocks only -- k_sn_head has written every word, k_snappy_emit still has to write the bytes)
      uint32_t* ja = X.jump_a.as<uint32_t>(); uint32_t* jb = X.jump_b.as<uint32_t>();
      launch_sn_next(s, src, cm, nc, dj, ja, X.olen.as<uint32_t>());
      for (int r = 0; r < mark_rounds; ++r) { launch_sn_mark(s, cm, nc, dj, ja, jb, mark, counts + (size_t)r * n, counts + (size_t)(r + 1) * n, r == 0); std::swap(ja, jb); }
      int32_t* pos = X.jump_b.as<int32_t>();      // (both jump arrays are free now)
      launch_sn_lens(s, cm, nc, dj, mark, X.olen.as<uint32_t>(), pos, status);
      launch_exclusive_scan_i32(s, pos, slots, X.scan.p, scan_bytes);
      launch_sn_fill(s, src, cm, nc, dj, mark, pos, resolve, status);
    }
    // ---- back: copies resolved by pointer jumping, then the bytes
    uint32_t* c2 = counts + (size_t)(mark_rounds + 1) * n;
    for (int r = 0; r < rounds; ++r) launch_snappy_round(s, resolve, bm, nb, dj, c2 + (size_t)r * n, c2 + (size_t)(r + 1) * n, r == 0);
    launch_snappy_emit(s, resolve, bm, nb, dj, dst, status);
  }
  HIPCHECK(hipStreamSynchronize(s));      // the jobs and the maps are pageable host memory; the scratch is free for the next call
}

}  // namespace gpuq
