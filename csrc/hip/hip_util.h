// Host-side helpers shared by the HIP translation units of gpudpf._hip:
// error checking, typed views of the launchers' integer arguments, the
// domain check, the GEMMs' argument checks and K-split, the large-LDS
// opt-in, runtime -> compile-time PRF dispatch and the grow-only device
// scratch.  Internal: not part of dpf_hip_api.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>

#include "dpf_core.h"

#define HIP_CHECK(expr)                                                   \
  do {                                                                    \
    hipError_t _e = (expr);                                               \
    if (_e != hipSuccess)                                                 \
      throw std::runtime_error(std::string("HIP error: ") +              \
                               hipGetErrorString(_e) + " at " __FILE__   \
                               ":" + std::to_string(__LINE__));          \
  } while (0)

namespace gpudpf_hip {

// The PRF ids and the key wire layout (dpf_core.h).
using gpudpf::kCwPerSel;
using gpudpf::kKeyCwInt;
using gpudpf::kKeyInts;
using gpudpf::kKeyRootInt;
using gpudpf::PRF_AES128;
using gpudpf::PRF_CHACHA20;
using gpudpf::PRF_DUMMY;
using gpudpf::PRF_SALSA20;

using u32 = std::uint32_t;
using u64 = std::uint64_t;

// Device pointers and streams cross dpf_hip_api.h as integers: typed views.
template <class T>
T* as_ptr(std::uintptr_t p) {
  return reinterpret_cast<T*>(p);
}
inline hipStream_t as_stream(std::uintptr_t s) {
  return reinterpret_cast<hipStream_t>(s);
}

// The domain is n = 2^depth leaves, depth >= 1 (a key stages 64 levels of
// correction words; a depth that does not match n would index past them).
inline void check_domain(int depth, long long n) {
  if (depth < 1 || ((long long)1 << depth) != n)
    throw std::invalid_argument("bad depth/n");
}

// Launch-argument checks of the GEMM launchers, made before any HIP call.
inline void check_ptrs(const char* what,
                       std::initializer_list<std::uintptr_t> ptrs) {
  for (std::uintptr_t p : ptrs)
    if (!p) throw std::invalid_argument(std::string(what) + ": null pointer");
}
inline void check_dims(const char* what, std::initializer_list<long long> dims) {
  for (long long d : dims)
    if (d < 1)
      throw std::invalid_argument(std::string(what) +
                                  ": dimensions must be >= 1");
}

// A GEMM's K-split: slice i of `segs` covers rows [i*kchunk, (i+1)*kchunk)
// of K, clipped to K; kchunk is a multiple of the kernels' 64-row K step.
struct KSplit {
  long long segs, kchunk;
};

// `want` slices clamped to [1, ceil(K/64)], floored to a power of two if
// `pow2`, each ceil(K/segs) rows rounded up to 64 (ceil on both divisions:
// with floor(K/segs) the slices can stop short of K).  segs*kchunk >= K;
// trailing slices may start at or past K and add zero.
inline KSplit split_k(long long K, long long want, bool pow2) {
  const long long max_segs = (K + 63) / 64;
  long long segs = want < 1 ? 1 : want > max_segs ? max_segs : want;
  if (pow2)
    while (segs & (segs - 1)) segs &= segs - 1;  // keep the top bit
  return {segs, ((K + segs - 1) / segs + 63) / 64 * 64};
}

// Launches that ask for 64 KiB or more of dynamic LDS (every kernel that
// holds the replicated AES table) must raise the kernel's limit first;
// smaller launches need nothing.  Done once per (kernel, device), so a
// launch replayed or captured later makes no runtime call beyond the
// launch itself.
inline void allow_large_lds(const void* kern, std::size_t lds_bytes) {
  if (lds_bytes < 65536) return;
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  if (done.count({kern, dev})) return;
  HIP_CHECK(hipFuncSetAttribute(
      kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  done.insert({kern, dev});
}

// Runtime PRF id -> compile-time constant: calls f(std::integral_constant<
// int, PRF>{}) for the matching PRF, so a launcher picks its kernel
// instantiation with one generic lambda:
//   with_prf(prf, [&](auto P) { launch(kernel<decltype(P)::value>); });
template <class F>
void with_prf(int prf, F&& f) {
  switch (prf) {
    case PRF_DUMMY: f(std::integral_constant<int, PRF_DUMMY>{}); break;
    case PRF_SALSA20: f(std::integral_constant<int, PRF_SALSA20>{}); break;
    case PRF_CHACHA20: f(std::integral_constant<int, PRF_CHACHA20>{}); break;
    case PRF_AES128: f(std::integral_constant<int, PRF_AES128>{}); break;
    default: throw std::invalid_argument("unknown PRF");
  }
}

// Grow-only device scratch, one buffer per device, reused across launches
// and sized for the largest request seen.  Growth is geometric (2x).
//
// An outgrown buffer is deliberately LEAKED, never freed: a hipGraph
// captured while a launch used the old buffer holds its raw pointer and
// replays against it, so freeing would turn later replays into
// use-after-free.  With 2x growth the leaked memory stays below the live
// buffer's size.
//
// The buffer is shared by every launch on a device that uses the same
// instance: launches in flight on DIFFERENT streams would overwrite each
// other.  The python API serializes launches per call; callers that
// overlap launches across streams bring their own buffers.
class GrowScratch {
 public:
  // At least `bytes` bytes on the current device (nullptr for 0 bytes).
  void* get(std::size_t bytes) {
    if (bytes == 0) return nullptr;
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDevices)
      throw std::out_of_range("GrowScratch: no slot for device " +
                              std::to_string(dev));
    std::lock_guard<std::mutex> lock(mu_);
    if (bytes_[dev] < bytes) {
      std::size_t want = bytes_[dev] ? bytes_[dev] : bytes;
      while (want < bytes) want *= 2;
      void* p = nullptr;
      HIP_CHECK(hipMalloc(&p, want));
      ptr_[dev] = p;  // the old pointer is leaked on purpose, see above
      bytes_[dev] = want;
    }
    return ptr_[dev];
  }

 private:
  static constexpr int kMaxDevices = 64;
  std::mutex mu_;
  void* ptr_[kMaxDevices] = {};
  std::size_t bytes_[kMaxDevices] = {};
};

// The one buffer behind the eval kernel's global sibling stack and the BFS
// and cooperative frontiers (defined in dpf_eval.hip).  They share it
// because BFS alone may ask for tens of GiB.
extern GrowScratch g_eval_scratch;

}  // namespace gpudpf_hip
