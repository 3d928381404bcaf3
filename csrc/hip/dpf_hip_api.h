// Host-side API of the gpudpf HIP kernel library, bound to python in
// hip_bindings.cc.  Implemented in dpf_eval.hip (fused / expand and their
// geometry queries), dpf_strategies.hip (bfs / coop / naive), dpf_probes.hip
// (prf_sol and the unit-test probes) and the three gemm files.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gpudpf_hip {

// Fused DPF expansion + table inner product (the production PIR path).
//   keys:  device ptr, int32 [batch][524]   (wire-format keys)
//   table: device ptr, u32 [n][entry_words] (leaf_perm-reordered rows)
//   out:   device ptr, u32 [batch][entry_words]
//   entry_words: u32 per table row, 16, 32, 48 or 64 (anything else:
//             std::invalid_argument before any HIP call).  A leaf's share is
//             computed once whatever the width
//   aes_tabs: device ptr to 5*256 u32 AES tables (only read for AES128)
//   scratch:  0 = the shared per-device sibling-stack scratch (launches on
//             one stream at a time); launches that may overlap on different
//             streams each pass their own device buffer of at least
//             eval_scratch_bytes(batch, depth, zlog) bytes (launch_expand too)
void launch_fused(std::uintptr_t keys, std::uintptr_t table, std::uintptr_t out,
                  std::uintptr_t aes_tabs, int batch, long long n, int depth,
                  int zlog, int prf, std::uintptr_t stream,
                  std::uintptr_t scratch = 0, std::size_t scratch_bytes = 0,
                  int entry_words = 16);
// (does not depend on entry_words)
std::size_t eval_scratch_bytes(int batch, int depth, int zlog);

// Binned variant of launch_fused (batch PIR): key i is evaluated against its
// own bin in one launch.
//   table: device ptr, u32 [num_bins][n][entry_words]; every block of
//          n = 1 << depth rows is in leaf_perm(n, zlog) order
//   bins:  device ptr, int32 [batch]; key i reads block bins[i].  The ids
//          live on the device, so the launcher cannot check them: the caller
//          guarantees 0 <= bins[i] < num_bins
// Geometry, scratch and output are those of launch_fused for one bin.
void launch_fused_binned(std::uintptr_t keys, std::uintptr_t table,
                         std::uintptr_t bins, std::uintptr_t out,
                         std::uintptr_t aes_tabs, int batch, long long n,
                         int depth, int zlog, long long num_bins, int prf,
                         std::uintptr_t stream, std::uintptr_t scratch = 0,
                         std::size_t scratch_bytes = 0, int entry_words = 16);

// Launch geometry of launch_fused / launch_expand, for tests that assert
// the regime they hit.  eval_slog: log2 of the per-key segment split
// (j-split); pure host arithmetic, no HIP call.  eval_units_per_wg: the
// (key, segment) units packed into one workgroup (1 unless prf is AES128);
// honours GPUDPF_AES_UNITS and otherwise queries the current device.  Rows
// wider than 16 words (entry_words as for launch_fused) take at most 2;
// lanes = 4 asks for a 16-word packed launch (launch_fused_packed,
// launch_expand_packed) and refuses every other width: the packed binned
// launch, which has them, is eval_units_per_wg_packed's (below).
int eval_slog(int batch, int depth, int zlog);
int eval_units_per_wg(int prf, int n_units, int entry_words = 16,
                      int lanes = 1);

// Packed keys (four u32 leaves per seed; dpf_core.h): launch_fused and
// launch_expand for a table of n = 4 << depth rows of 16 words in
// packed_perm(n, zlog) order, where depth is the keys' TREE depth D.
// Checked before any HIP call: depth >= 7, n == 4 << depth, zlog in
// [6, depth).  `out` must be 16-byte aligned.  eval_slog and
// eval_scratch_bytes serve them as they are, called with D;
// eval_units_per_wg with lanes = 4.
void launch_fused_packed(std::uintptr_t keys, std::uintptr_t table,
                         std::uintptr_t out, std::uintptr_t aes_tabs, int batch,
                         long long n, int depth, int zlog, int prf,
                         std::uintptr_t stream, std::uintptr_t scratch = 0,
                         std::size_t scratch_bytes = 0);
void launch_expand_packed(std::uintptr_t keys, std::uintptr_t out,
                          std::uintptr_t aes_tabs, int batch, long long n,
                          int depth, int zlog, int prf, std::uintptr_t stream,
                          std::uintptr_t scratch = 0,
                          std::size_t scratch_bytes = 0);

// Packed keys against bins (batch PIR), with rows of 16, 32, 48 or 64 words:
// launch_fused_binned for packed keys.
//   table: device ptr, u32 [num_bins][n][entry_words]; every block of
//          n = 4 << depth rows is in packed_perm(n, zlog) order (depth is the
//          keys' tree depth D)
//   bins:  as for launch_fused_binned, unchecked ids in [0, num_bins)
// Checked before any HIP call (std::invalid_argument): entry_words, depth in
// [7, 32], n == 4 << depth, zlog in [6, depth), num_bins >= 1 and
// num_bins * n * row bytes addressable, bins non-null when batch > 0, `out`
// 16-byte aligned, a caller's scratch of at least eval_scratch_bytes(batch,
// depth, zlog).  The only packed launch that serves rows wider than 16
// words: one bin is a plain packed table.  eval_units_per_wg_packed reports
// its units per workgroup (1 unless AES128: then at most 3 at 16 words, 2
// above; GPUDPF_AES_UNITS is clamped to that); pure host arithmetic.
void launch_fused_packed_binned(std::uintptr_t keys, std::uintptr_t table,
                                std::uintptr_t bins, std::uintptr_t out,
                                std::uintptr_t aes_tabs, int batch,
                                long long n, int depth, int zlog,
                                long long num_bins, int prf,
                                std::uintptr_t stream,
                                std::uintptr_t scratch = 0,
                                std::size_t scratch_bytes = 0,
                                int entry_words = 16);
int eval_units_per_wg_packed(int prf, int n_units, int entry_words);

// Full expansion to low-32 one-hot shares, permuted row order
//   out: device ptr, u32 [batch][n]  (row r = leaf_perm(idx))
void launch_expand(std::uintptr_t keys, std::uintptr_t out,
                   std::uintptr_t aes_tabs, int batch, long long n, int depth,
                   int zlog, int prf, std::uintptr_t stream,
                   std::uintptr_t scratch = 0, std::size_t scratch_bytes = 0);

// Level-synchronized breadth-first expansion (the reference's
// dpf_breadth_first.cu strategy): depth kernel launches, ping-pong u128
// frontiers in scratch, NATURAL-order low-32 one-hot output
//   out: device ptr, u32 [batch][n]
void launch_bfs(std::uintptr_t keys, std::uintptr_t out,
                std::uintptr_t aes_tabs, int batch, long long n, int depth,
                int prf, std::uintptr_t stream);

// Grid-wide cooperative single-key strategy (the reference's dpf_coop.cu):
// one cooperative launch walks one key's whole tree with a grid sync per
// level.  fused=true MACs the leaves against the permuted table into
// out[16] (zeroed by caller); fused=false writes natural-order one-hot
// low-32 shares to out[n].
void launch_coop(std::uintptr_t keys, std::uintptr_t table, std::uintptr_t out,
                 std::uintptr_t aes_tabs, long long n, int depth, int zlog,
                 int prf, bool fused, std::uintptr_t stream);

// Naive per-leaf oracle (O(n log n) PRFs), natural order output.  Test-only.
void launch_naive(std::uintptr_t keys, std::uintptr_t out,
                  std::uintptr_t aes_tabs, int batch, long long n, int depth,
                  int prf, std::uintptr_t stream);

// PRF speed-of-light microbenchmark: blocks x 256 threads each run a
// dependent chain of `iters` pair expansions; out: u32[blocks*256].
void launch_prf_sol(std::uintptr_t aes_tabs, std::uintptr_t out, int blocks,
                    int iters, int prf, std::uintptr_t stream);

// Unit-test probes (tests/test_gpu_alu.py; analog of the reference's
// dpf_gpu/tests/test_128_bit.cu).  All pointers are device int32/uint32
// buffers; u128 values are 4xu32 limbs little-endian.
void launch_probe_alu(std::uintptr_t a, std::uintptr_t b,
                      std::uintptr_t add_out, std::uintptr_t mul_out,
                      int count, std::uintptr_t stream);
void launch_probe_prf(std::uintptr_t seeds, std::uintptr_t aes_tabs,
                      std::uintptr_t pair0, std::uintptr_t pair1,
                      std::uintptr_t single0, std::uintptr_t single1,
                      std::uintptr_t low0, std::uintptr_t low1, int count,
                      int prf, std::uintptr_t stream);
// The AES table as the kernels stage it in LDS (prf_device.h), copied out by
// one workgroup of `threads` threads (a multiple of 64 up to 1024).
//   out: device ptr, u32 [16384]: word e*64 + h*32 + c is te0[e] (h = 0) or
//        te2[e] (h = 1) for every copy c
void launch_probe_aes_lds(std::uintptr_t aes_tabs, std::uintptr_t out,
                          int threads, std::uintptr_t stream);

// The three GEMMs.  Each splits K into `segs` slices of `kchunk` rows
// (KSplit and the shared arithmetic: hip_util.h), and each *_split query is
// the only place its launcher takes the split from: pure host arithmetic,
// no HIP call, std::invalid_argument for a shape the launcher rejects.  The
// launchers check shapes and pointers (non-null) before any HIP call.
struct KSplit;

// Exact u128 GEMM (research harness; gemm128.hip).  a: [M,K] u128 (as
// 4xint32 limbs), bt: [N,K] u128, c: [M,N] u128, partials: the caller's
// device scratch of partials_bytes >= gemm128_split(M,N,K).segs*M*N*16.
KSplit gemm128_split(long long M, long long N, long long K);
void launch_gemm128(std::uintptr_t a, std::uintptr_t bt, std::uintptr_t c,
                    std::uintptr_t partials, std::size_t partials_bytes,
                    long long M, long long N, long long K,
                    std::uintptr_t stream);

// MFMA mod-2^32 GEMM (gemm_u32.hip): digit decomposition + i8 matrix
// cores.  da/dbt: [4][M][K] / [4][N][K] int8 digit planes; c: [M][N] u32
// (zeroed by caller; K-split partials combine with wrapping atomicAdd).
// M%64, N%16 and K%64 must all be 0.  launch_digits writes the four planes
// of `count` u32 words, count words apart (count == 0 launches nothing).
KSplit gemm_u32_split(long long M, long long N, long long K);
void launch_digits(std::uintptr_t in, std::uintptr_t out, long long count,
                   std::uintptr_t stream);
void launch_gemm_u32_mfma(std::uintptr_t da, std::uintptr_t dbt,
                          std::uintptr_t c, long long M, long long N,
                          long long K, std::uintptr_t stream);

// Streaming mod-2^32 GEMM (gemm_stream.hip): reads the u32 table in place
// (no transposed copy, no digit planes) — the huge-table wide-entry path.
// a: [batch, K] u32 shares; b: [K, N] u32 table; c: [batch, N] u32
// (zeroed by caller).  batch <= 16 (python wrapper chunks larger) and
// N <= 65535*256.  Only this split drops the slices that would start at or
// past K; its partials (segs*batch*N u32, in a per-device scratch) stay
// within 1 GiB wherever one slice's do.
KSplit gemm_u32_stream_split(int batch, long long K, long long N);
void launch_gemm_u32_stream(std::uintptr_t a, std::uintptr_t b,
                            std::uintptr_t c, int batch, long long K,
                            long long N, std::uintptr_t stream);

}  // namespace gpudpf_hip
