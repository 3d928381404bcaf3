// The other expansion strategies, kept next to the production DFS kernel
// (dpf_eval.hip) as the test oracle and as measured research points: the
// naive per-leaf oracle, level-synchronized breadth-first expansion and
// the grid-wide cooperative single-key walk.

#include <hip/hip_runtime.h>
#include <hip/hip_cooperative_groups.h>

#include <stdexcept>

#include "dpf_hip_api.h"
#include "hip_util.h"
#include "prf_device.h"

namespace gpudpf_hip {

// ---------------------------------------------------------------------------
// Naive oracle kernel: EvaluateFlat per (key, leaf), natural order.
// (Test-only; uses the flat 4-table AES layout at aes_tabs[0..1279]:
// te0|te1|te2|te3|sbox.)
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint4 aes_flat(const u32* tabs, uint4 seed,
                                          u32 pos) {
  const u32* te0 = tabs;
  const u32* te1 = tabs + 256;
  const u32* te2 = tabs + 512;
  const u32* te3 = tabs + 768;
  const u32* sb = tabs + 1024;
  u32 rk[44];
  rk[0] = __builtin_bswap32(seed.x);
  rk[1] = __builtin_bswap32(seed.y);
  rk[2] = __builtin_bswap32(seed.z);
  rk[3] = __builtin_bswap32(seed.w);
  u32 rcon = 0x01u;
#pragma unroll
  for (int r = 1; r <= 10; ++r) {
    u32 w = rk[4 * r - 1];
    w = (w << 8) | (w >> 24);
    w = (sb[(w >> 24) & 0xff] << 24) | (sb[(w >> 16) & 0xff] << 16) |
        (sb[(w >> 8) & 0xff] << 8) | sb[w & 0xff];
    w ^= (rcon << 24);
    rcon = (rcon << 1) ^ ((rcon & 0x80u) ? 0x11bu : 0u);
    rcon &= 0xffu;
    rk[4 * r] = rk[4 * r - 4] ^ w;
    rk[4 * r + 1] = rk[4 * r - 3] ^ rk[4 * r];
    rk[4 * r + 2] = rk[4 * r - 2] ^ rk[4 * r + 1];
    rk[4 * r + 3] = rk[4 * r - 1] ^ rk[4 * r + 2];
  }
  u32 s0 = (pos << 24) ^ rk[0], s1 = rk[1], s2 = rk[2], s3 = rk[3];
#pragma unroll
  for (int r = 1; r < 10; ++r) {
    u32 n0 = te0[s0 >> 24] ^ te1[(s1 >> 16) & 0xff] ^ te2[(s2 >> 8) & 0xff] ^
             te3[s3 & 0xff] ^ rk[4 * r];
    u32 n1 = te0[s1 >> 24] ^ te1[(s2 >> 16) & 0xff] ^ te2[(s3 >> 8) & 0xff] ^
             te3[s0 & 0xff] ^ rk[4 * r + 1];
    u32 n2 = te0[s2 >> 24] ^ te1[(s3 >> 16) & 0xff] ^ te2[(s0 >> 8) & 0xff] ^
             te3[s1 & 0xff] ^ rk[4 * r + 2];
    u32 n3 = te0[s3 >> 24] ^ te1[(s0 >> 16) & 0xff] ^ te2[(s1 >> 8) & 0xff] ^
             te3[s2 & 0xff] ^ rk[4 * r + 3];
    s0 = n0; s1 = n1; s2 = n2; s3 = n3;
  }
  u32 o0 = ((sb[s0 >> 24] << 24) | (sb[(s1 >> 16) & 0xff] << 16) |
            (sb[(s2 >> 8) & 0xff] << 8) | sb[s3 & 0xff]) ^ rk[40];
  u32 o1 = ((sb[s1 >> 24] << 24) | (sb[(s2 >> 16) & 0xff] << 16) |
            (sb[(s3 >> 8) & 0xff] << 8) | sb[s0 & 0xff]) ^ rk[41];
  u32 o2 = ((sb[s2 >> 24] << 24) | (sb[(s3 >> 16) & 0xff] << 16) |
            (sb[(s0 >> 8) & 0xff] << 8) | sb[s1 & 0xff]) ^ rk[42];
  u32 o3 = ((sb[s3 >> 24] << 24) | (sb[(s0 >> 16) & 0xff] << 16) |
            (sb[(s1 >> 8) & 0xff] << 8) | sb[s2 & 0xff]) ^ rk[43];
  return make_uint4(__builtin_bswap32(o0), __builtin_bswap32(o1),
                    __builtin_bswap32(o2), __builtin_bswap32(o3));
}

template <int PRF>
__device__ __forceinline__ uint4 prf_naive(const u32* aes_lds, uint4 seed,
                                           u32 pos) {
  if constexpr (PRF == PRF_DUMMY) return prf_dummy_full(seed, pos);
  if constexpr (PRF == PRF_SALSA20) return salsa12_core(seed, pos);
  if constexpr (PRF == PRF_CHACHA20) return chacha12_core(seed, pos);
  if constexpr (PRF == PRF_AES128) return aes_flat(aes_lds, seed, pos);
}

template <int PRF>
__global__ __launch_bounds__(256) void dpf_naive_kernel(
    const int* __restrict__ keys, u32* __restrict__ out,
    const u32* __restrict__ aes_tabs, int depth, long long n) {
  extern __shared__ u32 smem[];
  uint4* cw_lds = reinterpret_cast<uint4*>(smem);
  u32* aes_lds = reinterpret_cast<u32*>(cw_lds + 2 * kCwPerSel);
  const int t = (int)threadIdx.x;
  const long long key_base = (long long)blockIdx.x * kKeyInts;
  for (int idx = t; idx < 2 * kCwPerSel; idx += blockDim.x)
    cw_lds[idx] =
        reinterpret_cast<const uint4*>(keys + key_base + kKeyCwInt)[idx];
  if constexpr (PRF == PRF_AES128) {
    for (int idx = t; idx < 1280; idx += blockDim.x)
      aes_lds[idx] = aes_tabs[idx];
  }
  __syncthreads();

  const long long leaf = (long long)blockIdx.y * blockDim.x + t;
  if (leaf >= n) return;
  uint4 key = key_root(keys + key_base);
  long long rem = leaf;
  for (int i = depth - 1; i >= 0; --i) {
    const u32 bit = (u32)(rem & 1);
    uint4 v = prf_naive<PRF>(aes_lds, key, bit);
    const int sel = (int)(key.x & 1u);
    key = add128(v, cw_lds[sel * kCwPerSel + i * 2 + (int)bit]);
    rem >>= 1;
  }
  out[(u64)blockIdx.x * (u64)n + (u64)leaf] = key.x;
}

// ---------------------------------------------------------------------------
// Level-synchronized breadth-first expansion (the reference's
// dpf_breadth_first.cu:35-103 strategy, completing the strategy matrix
// next to naive / fused / two-stage).  One kernel launch per tree level;
// ping-pong u128 seed frontiers in global scratch; the last level writes
// low-32 one-hot shares in NATURAL index order with two coalesced
// streams (leaf idx = parent_pos | bit << (depth-1), because the eval
// recurrence consumes index bits LSB-first).
//
// This strategy pays n*16 B of frontier traffic per level pair and
// depth kernel launches — the fused DFS kernel exists precisely to avoid
// that; BFS is kept as a measured research point, not the production
// path.
// ---------------------------------------------------------------------------
template <int PRF>
__global__ __launch_bounds__(256) void dpf_bfs_level_kernel(
    const int* __restrict__ keys, const uint4* __restrict__ parents,
    uint4* __restrict__ children, u32* __restrict__ out,
    const u32* __restrict__ aes_tabs, int level, int depth, long long n) {
  extern __shared__ u32 smem[];
  uint4* cw_lvl =
      reinterpret_cast<uint4*>(smem + aes_lds_u32(PRF));  // table first
  const int t = (int)threadIdx.x;
  const int key_id = (int)blockIdx.y;
  const long long key_base = (long long)key_id * kKeyInts;
  aes_stage_table<PRF>(smem, aes_tabs);
  // stage this level's 4 correction words (cw[sel][2i+b], i = eval level)
  const int i_eval = depth - 1 - level;
  if (t < 4) {
    const int sel = t >> 1, b = t & 1;
    cw_lvl[t] = reinterpret_cast<const uint4*>(keys + key_base + kKeyCwInt)
        [sel * kCwPerSel + i_eval * 2 + b];
  }
  __syncthreads();
  const AesLds T = AesLds::lane();

  const long long n_parents = (long long)1 << level;
  const long long p = (long long)blockIdx.x * blockDim.x + t;
  if (p >= n_parents) return;

  uint4 seed;
  if (level == 0) {
    seed = key_root(keys + key_base);
  } else {
    seed = parents[(u64)key_id * (n_parents) + (u64)p];
    // parents buffer is sized per level: indexed [key][p] with stride
    // n_parents (the launcher passes the matching base pointer)
  }
  const int sel = (int)(seed.x & 1u);
  uint4 c0, c1;
  prf_pair<PRF>(seed, T, c0, c1);
  c0 = add128(c0, cw_lvl[sel * 2 + 0]);
  c1 = add128(c1, cw_lvl[sel * 2 + 1]);
  if (level == depth - 1) {
    u32* orow = out + (u64)key_id * (u64)n;
    orow[p] = c0.x;
    orow[p + ((u64)1 << (depth - 1))] = c1.x;
  } else {
    uint4* crow = children + (u64)key_id * (n_parents * 2);
    crow[p] = c0;
    crow[p + n_parents] = c1;
  }
}

// ---------------------------------------------------------------------------
// Grid-wide cooperative single-key strategy (the reference's dpf_coop.cu:
// cudaLaunchCooperativeKernel + this_grid().sync() between tree levels,
// batch=1 only).  The whole grid walks one GGM tree breadth-first with a
// grid sync per level; with FUSED the leaves are MAC'd against the
// (leaf_perm-ordered) table into per-thread accumulators and combined
// with wrapping atomics — no second kernel.
//
// This exists for strategy-matrix completeness and as a measured
// comparison point: the production fused kernel's j-split serves the
// same single-key-latency role with NO grid-wide synchronization (its
// segments are independent), which is why it wins (see
// benchmarks/strategy_compare.py --coop).
// ---------------------------------------------------------------------------
template <int PRF, bool FUSED>
__global__ __launch_bounds__(256) void dpf_coop_kernel(
    const int* __restrict__ keys, const u32* __restrict__ table,
    u32* __restrict__ out, const u32* __restrict__ aes_tabs,
    uint4* __restrict__ ping, uint4* __restrict__ pong, int depth, int zlog,
    long long n) {
  extern __shared__ u32 smem[];
  const int t = (int)threadIdx.x;
  const AesLds T = aes_lds_init<PRF>(smem, aes_tabs);
  auto grid = cooperative_groups::this_grid();
  const long long gsize = (long long)gridDim.x * blockDim.x;
  const long long gtid = (long long)blockIdx.x * blockDim.x + t;
  const uint4* cw = reinterpret_cast<const uint4*>(keys + kKeyCwInt);

  u32 acc[16];
#pragma unroll
  for (int w = 0; w < 16; ++w) acc[w] = 0;

  for (int level = 0; level < depth; ++level) {
    const long long n_parents = (long long)1 << level;
    const int i_eval = depth - 1 - level;
    for (long long p = gtid; p < n_parents; p += gsize) {
      uint4 seed;
      if (level == 0) {
        seed = key_root(keys);
      } else {
        seed = ping[p];
      }
      const int sel = (int)(seed.x & 1u);
      uint4 c0, c1;
      prf_pair<PRF>(seed, T, c0, c1);
      c0 = add128(c0, cw[sel * kCwPerSel + i_eval * 2 + 0]);
      c1 = add128(c1, cw[sel * kCwPerSel + i_eval * 2 + 1]);
      if (level < depth - 1) {
        pong[p] = c0;
        pong[p + n_parents] = c1;
      } else {
        // natural leaf indices: p and p | n/2 (bits consumed LSB-first)
        const long long i0 = p, i1 = p | (n >> 1);
        if constexpr (FUSED) {
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const long long idx = q ? i1 : i0;
            const u32 v = q ? c1.x : c0.x;
            // leaf_perm(idx) in-kernel (see dpf_core.cc layout contract)
            const int ds = depth - zlog;
            const u32 tl = (u32)(idx & ((1u << zlog) - 1));
            const u32 tpos = __brev(tl) >> (32 - zlog);
            const u32 jm = (u32)((idx >> zlog) & (((long long)1 << (ds - 1)) - 1));
            const u32 j = ds > 1 ? (__brev(jm) >> (33 - ds)) : 0;
            const u32 b = (u32)(idx >> (depth - 1));
            const long long row = ((long long)j << (zlog + 1)) |
                                  ((long long)tpos << 1) | b;
            const u32* trow = table + (u64)row * 16;
#pragma unroll
            for (int w = 0; w < 16; ++w) acc[w] += v * trow[w];
          }
        } else {
          out[i0] = c0.x;
          out[i1] = c1.x;
        }
      }
    }
    if (level < depth - 1) {
      grid.sync();
      uint4* tmp = ping;
      ping = pong;
      pong = tmp;
    }
  }
  if constexpr (FUSED) {
#pragma unroll
    for (int w = 0; w < 16; ++w)
      if (acc[w]) atomicAdd(out + w, acc[w]);
  }
}

namespace {
template <int PRF, bool FUSED>
void launch_coop_t(const int* keys, const u32* table, u32* out,
                   const u32* aes_tabs, uint4* ping, uint4* pong, int depth,
                   int zlog, long long n, hipStream_t st) {
  auto kern = dpf_coop_kernel<PRF, FUSED>;
  const size_t shmem = aes_lds_u32(PRF) * sizeof(u32);
  allow_large_lds((const void*)kern, shmem);
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  int coop = 0;
  HIP_CHECK(hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch,
                                  dev));
  if (!coop)
    throw std::runtime_error("device does not support cooperative launch");
  int num_cu = 0;
  HIP_CHECK(hipDeviceGetAttribute(&num_cu,
                                  hipDeviceAttributeMultiprocessorCount, dev));
  int max_blocks = 0;
  HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &max_blocks, (const void*)kern, 256, shmem));
  long long grid = (long long)num_cu * max_blocks;
  const long long need = ((n / 2) + 255) / 256;  // widest level
  if (grid > need) grid = need;
  if (grid < 1) grid = 1;
  void* args[] = {(void*)&keys, (void*)&table, (void*)&out,
                  (void*)&aes_tabs, (void*)&ping, (void*)&pong,
                  (void*)&depth, (void*)&zlog, (void*)&n};
  HIP_CHECK(hipLaunchCooperativeKernel((const void*)kern,
                                       dim3((unsigned)grid), dim3(256), args,
                                       shmem, st));
}
}  // namespace

void launch_coop(std::uintptr_t keys, std::uintptr_t table, std::uintptr_t out,
                 std::uintptr_t aes_tabs, long long n, int depth, int zlog,
                 int prf, bool fused, std::uintptr_t stream) {
  check_domain(depth, n);
  // the in-kernel leaf_perm shifts by 32 - zlog and 33 - (depth - zlog)
  if (zlog < 6 || zlog >= depth)
    throw std::invalid_argument("zlog must be in [6, depth)");
  const size_t half = (size_t)(n / 2) * sizeof(uint4);
  uint4* ping =
      static_cast<uint4*>(g_eval_scratch.get(2 * half > 0 ? 2 * half : 32));
  uint4* pong = ping + (size_t)(n / 2);
  with_prf(prf, [&](auto P) {
    constexpr int PRF = decltype(P)::value;
    auto launch = fused ? launch_coop_t<PRF, true> : launch_coop_t<PRF, false>;
    launch(as_ptr<const int>(keys), as_ptr<const u32>(table), as_ptr<u32>(out),
           as_ptr<const u32>(aes_tabs), ping, pong, depth, zlog, n,
           as_stream(stream));
  });
}

namespace {
template <int PRF>
void launch_bfs_t(const int* keys, u32* out, const u32* aes_tabs,
                  uint4* ping, uint4* pong, int batch, long long n, int depth,
                  hipStream_t st) {
  const size_t shmem = aes_lds_u32(PRF) * sizeof(u32) + 4 * sizeof(uint4);
  allow_large_lds((const void*)dpf_bfs_level_kernel<PRF>, shmem);
  for (int level = 0; level < depth; ++level) {
    const long long n_parents = (long long)1 << level;
    const long long blocks = (n_parents + 255) / 256;
    const uint4* parents = (level & 1) ? pong : ping;
    uint4* children = (level & 1) ? ping : pong;
    hipLaunchKernelGGL(dpf_bfs_level_kernel<PRF>,
                       dim3((unsigned)blocks, (unsigned)batch), dim3(256),
                       shmem, st, keys, parents, children, out, aes_tabs,
                       level, depth, n);
    HIP_CHECK(hipGetLastError());
  }
}
}  // namespace

void launch_bfs(std::uintptr_t keys, std::uintptr_t out,
                std::uintptr_t aes_tabs, int batch, long long n, int depth,
                int prf, std::uintptr_t stream) {
  if (batch <= 0) return;
  check_domain(depth, n);
  // two ping-pong frontier buffers, each batch * n/2 seeds
  const size_t half = (size_t)batch * (size_t)(n / 2) * sizeof(uint4);
  if (2 * half > (size_t)48 << 30)
    throw std::invalid_argument("BFS frontier would exceed 48 GiB scratch");
  uint4* ping =
      static_cast<uint4*>(g_eval_scratch.get(2 * half > 0 ? 2 * half : 16));
  uint4* pong = ping + (size_t)batch * (size_t)(n / 2);
  with_prf(prf, [&](auto P) {
    launch_bfs_t<decltype(P)::value>(
        as_ptr<const int>(keys), as_ptr<u32>(out), as_ptr<const u32>(aes_tabs),
        ping, pong, batch, n, depth, as_stream(stream));
  });
}

void launch_naive(std::uintptr_t keys, std::uintptr_t out,
                  std::uintptr_t aes_tabs, int batch, long long n, int depth,
                  int prf, std::uintptr_t stream) {
  if (batch <= 0) return;
  check_domain(depth, n);
  const int threads = 256;
  dim3 grid((unsigned)batch, (unsigned)((n + threads - 1) / threads));
  const size_t shmem =
      2 * kCwPerSel * 16 + (prf == PRF_AES128 ? 1280 * 4 : 0);
  with_prf(prf, [&](auto P) {
    hipLaunchKernelGGL(dpf_naive_kernel<decltype(P)::value>, grid,
                       dim3(threads), shmem, as_stream(stream),
                       as_ptr<const int>(keys), as_ptr<u32>(out),
                       as_ptr<const u32>(aes_tabs), depth, n);
    HIP_CHECK(hipGetLastError());
  });
}

}  // namespace gpudpf_hip
