// Measurement and unit-test probes of the device PRFs (prf_device.h): the
// PRF speed-of-light microbenchmark, the ALU / PRF probe kernels and the
// probe of the staged AES table.

#include <hip/hip_runtime.h>

#include "dpf_hip_api.h"
#include "hip_util.h"
#include "prf_device.h"

namespace gpudpf_hip {

// ---------------------------------------------------------------------------
// PRF speed-of-light microbenchmark: dependent chain of pair expansions on
// register data only (no DFS, no table, no LDS traffic beyond the AES
// table).  Upper-bounds what any expansion kernel could reach; the fused
// kernel's pair rate divided by this is its efficiency.
// ---------------------------------------------------------------------------
template <int PRF>
__global__ __launch_bounds__(PRF == PRF_AES128 ? 1024 : 256) void prf_sol_kernel(
    const u32* __restrict__ aes_tabs, u32* __restrict__ out, int iters) {
  extern __shared__ u32 smem[];
  const AesLds T = aes_lds_init<PRF>(smem, aes_tabs);
  uint4 seed = make_uint4(threadIdx.x + 1, blockIdx.x + 2, 3, 4);
  for (int i = 0; i < iters; ++i) {
    uint4 r0, r1;
    prf_pair<PRF>(seed, T, r0, r1);
    seed = make_uint4(r0.x ^ r1.x, r0.y ^ r1.y, r0.z ^ r1.z, r0.w ^ r1.w);
  }
  out[(u64)blockIdx.x * blockDim.x + threadIdx.x] = seed.x;
}

void launch_prf_sol(std::uintptr_t aes_tabs, std::uintptr_t out, int blocks,
                    int iters, int prf, std::uintptr_t stream) {
  const size_t shmem = aes_lds_u32(prf) * sizeof(u32);
  with_prf(prf, [&](auto P) {
    constexpr int PRF = decltype(P)::value;
    allow_large_lds((const void*)prf_sol_kernel<PRF>, shmem);
    // AES: same thread count in workgroups of 1024 where it divides: like
    // the eval kernel's K = 4, four times the waves share one 64 KiB table.
    const bool wide = PRF == PRF_AES128 && blocks % 4 == 0;
    hipLaunchKernelGGL(prf_sol_kernel<PRF>, dim3(wide ? blocks / 4 : blocks),
                       dim3(wide ? 1024 : 256), shmem, as_stream(stream),
                       as_ptr<const u32>(aes_tabs), as_ptr<u32>(out), iters);
  });
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// ALU / PRF probe kernels — the unit-test analog of the reference's
// dpf_gpu/tests/test_128_bit.cu:192-200 (device add/mul/pack asserted
// against host __int128): one element per thread, results compared
// elementwise against the CPU core in tests/test_gpu_alu.py.  These probe
// the EXACT device functions the production kernels inline (add128,
// prf_pair, prf_pair_low, prf_full with the replicated-LDS AES table), so
// a PRF-core bug fails a unit test, not only end-to-end reconstruction.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void probe_alu_kernel(
    const uint4* __restrict__ a, const uint4* __restrict__ b,
    uint4* __restrict__ add_out, uint4* __restrict__ mul_out, int count) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= count) return;
  add_out[i] = add128(a[i], b[i]);
  const unsigned __int128 x =
      ((unsigned __int128)(((u64)a[i].w << 32) | a[i].z) << 64) |
      (((u64)a[i].y << 32) | a[i].x);
  const unsigned __int128 y =
      ((unsigned __int128)(((u64)b[i].w << 32) | b[i].z) << 64) |
      (((u64)b[i].y << 32) | b[i].x);
  const unsigned __int128 r = x * y;
  const u64 lo = (u64)r, hi = (u64)(r >> 64);
  mul_out[i] = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
}

template <int PRF>
__global__ __launch_bounds__(256) void probe_prf_kernel(
    const uint4* __restrict__ seeds, const u32* __restrict__ aes_tabs,
    uint4* __restrict__ pair0, uint4* __restrict__ pair1,
    uint4* __restrict__ single0, uint4* __restrict__ single1,
    u32* __restrict__ low0, u32* __restrict__ low1, int count) {
  extern __shared__ u32 smem[];
  const AesLds T = aes_lds_init<PRF>(smem, aes_tabs);
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= count) return;
  const uint4 s = seeds[i];
  uint4 r0, r1;
  prf_pair<PRF>(s, T, r0, r1);
  pair0[i] = r0;
  pair1[i] = r1;
  single0[i] = prf_full<PRF>(s, 0, T);
  single1[i] = prf_full<PRF>(s, 1, T);
  u32 l0, l1;
  prf_pair_low<PRF>(s, T, l0, l1);
  low0[i] = l0;
  low1[i] = l1;
}

// The AES table as aes_lds_init stages it: one workgroup of `threads`
// threads stages and copies the AES_LDS_WORDS words out unchanged.  The
// staging loop strides by the workgroup size, so tests/
// test_gpu_aes_lds_layout.py runs it at every size the eval kernel uses.
__global__ __launch_bounds__(1024) void probe_aes_lds_kernel(
    const u32* __restrict__ aes_tabs, u32* __restrict__ out) {
  extern __shared__ u32 smem[];
  aes_lds_init<PRF_AES128>(smem, aes_tabs);
  for (int idx = (int)threadIdx.x; idx < AES_LDS_WORDS; idx += (int)blockDim.x)
    out[idx] = smem[idx];
}

void launch_probe_aes_lds(std::uintptr_t aes_tabs, std::uintptr_t out,
                          int threads, std::uintptr_t stream) {
  if (threads < 64 || threads > 1024 || threads % 64 != 0)
    throw std::invalid_argument(
        "probe_aes_lds: threads must be a multiple of 64 in [64, 1024]");
  check_ptrs("probe_aes_lds", {aes_tabs, out});
  const size_t shmem = aes_lds_u32(PRF_AES128) * sizeof(u32);
  allow_large_lds((const void*)probe_aes_lds_kernel, shmem);
  hipLaunchKernelGGL(probe_aes_lds_kernel, dim3(1), dim3(threads), shmem,
                     as_stream(stream), as_ptr<const u32>(aes_tabs),
                     as_ptr<u32>(out));
  HIP_CHECK(hipGetLastError());
}

void launch_probe_alu(std::uintptr_t a, std::uintptr_t b,
                      std::uintptr_t add_out, std::uintptr_t mul_out,
                      int count, std::uintptr_t stream) {
  const int blocks = (count + 255) / 256;
  hipLaunchKernelGGL(probe_alu_kernel, dim3(blocks), dim3(256), 0,
                     as_stream(stream), as_ptr<const uint4>(a),
                     as_ptr<const uint4>(b), as_ptr<uint4>(add_out),
                     as_ptr<uint4>(mul_out), count);
  HIP_CHECK(hipGetLastError());
}

void launch_probe_prf(std::uintptr_t seeds, std::uintptr_t aes_tabs,
                      std::uintptr_t pair0, std::uintptr_t pair1,
                      std::uintptr_t single0, std::uintptr_t single1,
                      std::uintptr_t low0, std::uintptr_t low1, int count,
                      int prf, std::uintptr_t stream) {
  const int blocks = (count + 255) / 256;
  const size_t shmem = aes_lds_u32(prf) * sizeof(u32);
  with_prf(prf, [&](auto P) {
    constexpr int PRF = decltype(P)::value;
    allow_large_lds((const void*)probe_prf_kernel<PRF>, shmem);
    hipLaunchKernelGGL(probe_prf_kernel<PRF>, dim3(blocks), dim3(256), shmem,
                       as_stream(stream), as_ptr<const uint4>(seeds),
                       as_ptr<const u32>(aes_tabs), as_ptr<uint4>(pair0),
                       as_ptr<uint4>(pair1), as_ptr<uint4>(single0),
                       as_ptr<uint4>(single1), as_ptr<u32>(low0),
                       as_ptr<u32>(low1), count);
  });
  HIP_CHECK(hipGetLastError());
}

}  // namespace gpudpf_hip
