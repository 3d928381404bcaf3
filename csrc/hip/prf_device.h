// Device PRFs and 128-bit helpers shared by every DPF kernel (dpf_eval.hip,
// dpf_strategies.hip, dpf_probes.hip).  They mirror csrc/core/prf.cc
// bit-exactly (tested by tests/test_gpu.py and tests/test_gpu_alu.py
// against the CPU core).
//
// CONTRACT for kernels that build an AesLds (see the AES section below):
// no static LDS, and the replicated te0 table (aes_stage_table) first in
// the dynamic LDS map, so that the table starts at LDS byte 0.
#pragma once
#include "hip_util.h"

namespace gpudpf_hip {

using u32 = std::uint32_t;
using u64 = std::uint64_t;

// ---------------------------------------------------------------------------
// 128-bit helpers (uint4 limbs, x = bits 31..0 ... w = bits 127..96)
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint4 add128(uint4 a, uint4 b) {
  u64 alo = ((u64)a.y << 32) | a.x, ahi = ((u64)a.w << 32) | a.z;
  u64 blo = ((u64)b.y << 32) | b.x, bhi = ((u64)b.w << 32) | b.z;
  u64 lo = alo + blo;
  u64 hi = ahi + bhi + (lo < alo ? 1u : 0u);
  return make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
}

__device__ __forceinline__ u32 rotl(u32 v, int s) {
  return (v << s) | (v >> (32 - s));  // lowers to v_alignbit_b32
}
__device__ __forceinline__ u32 rotr8(u32 v) { return (v >> 8) | (v << 24); }
__device__ __forceinline__ u32 rotr16(u32 v) { return (v >> 16) | (v << 16); }
__device__ __forceinline__ u32 rotr24(u32 v) { return (v >> 24) | (v << 8); }

// AES replicated-table geometry
#define AES_REP 64
#define AES_LDS_WORDS (256 * AES_REP)  // 64 KiB

// ---------------------------------------------------------------------------
// DUMMY: seed*(pos+4242) + (pos+4242) over Z_2^128
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint4 prf_dummy_full(uint4 seed, u32 pos) {
  unsigned __int128 s =
      ((unsigned __int128)(((u64)seed.w << 32) | seed.z) << 64) |
      (((u64)seed.y << 32) | seed.x);
  unsigned __int128 m = (unsigned __int128)(pos + 4242u);
  unsigned __int128 r = s * m + m;
  u64 lo = (u64)r, hi = (u64)(r >> 64);
  return make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
}

// ---------------------------------------------------------------------------
// Salsa20/12 (conventions: seed words 1..4 high->low, pos word 9, output
// words 1..4 — see csrc/core/prf.cc)
// ---------------------------------------------------------------------------
#define SALSA_QR(a, b, c, d)  \
  b ^= rotl(a + d, 7);        \
  c ^= rotl(b + a, 9);        \
  d ^= rotl(c + b, 13);       \
  a ^= rotl(d + c, 18)

__device__ __forceinline__ uint4 salsa12_core(uint4 seed, u32 pos) {
  const u32 c0 = 0x65787061u, c5 = 0x6e642033u, c10 = 0x322d6279u,
            c15 = 0x7465206bu;
  u32 x0 = c0, x1 = seed.w, x2 = seed.z, x3 = seed.y, x4 = seed.x, x5 = c5,
      x6 = 0, x7 = 0, x8 = 0, x9 = pos, x10 = c10, x11 = 0, x12 = 0, x13 = 0,
      x14 = 0, x15 = c15;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    SALSA_QR(x0, x4, x8, x12);
    SALSA_QR(x5, x9, x13, x1);
    SALSA_QR(x10, x14, x2, x6);
    SALSA_QR(x15, x3, x7, x11);
    SALSA_QR(x0, x1, x2, x3);
    SALSA_QR(x5, x6, x7, x4);
    SALSA_QR(x10, x11, x8, x9);
    SALSA_QR(x15, x12, x13, x14);
  }
  return make_uint4(x4 + seed.x, x3 + seed.y, x2 + seed.z, x1 + seed.w);
}

// Both children interleaved in one pass: the two blocks (pos=0 / pos=1)
// are independent dependency chains, so interleaving doubles the ILP the
// SIMD can draw on — the DFS runs at ~2 waves/SIMD where a single chain's
// QR latency is not fully hidden.
#define SALSA_QR2(a, b, c, d, a2, b2, c2, d2) \
  b ^= rotl(a + d, 7);   b2 ^= rotl(a2 + d2, 7);   \
  c ^= rotl(b + a, 9);   c2 ^= rotl(b2 + a2, 9);   \
  d ^= rotl(c + b, 13);  d2 ^= rotl(c2 + b2, 13);  \
  a ^= rotl(d + c, 18);  a2 ^= rotl(d2 + c2, 18)

__device__ __forceinline__ void salsa12_pair_core(uint4 seed, uint4& r0,
                                                  uint4& r1) {
  const u32 c0 = 0x65787061u, c5 = 0x6e642033u, c10 = 0x322d6279u,
            c15 = 0x7465206bu;
  u32 x0 = c0, x1 = seed.w, x2 = seed.z, x3 = seed.y, x4 = seed.x, x5 = c5,
      x6 = 0, x7 = 0, x8 = 0, x9 = 0, x10 = c10, x11 = 0, x12 = 0, x13 = 0,
      x14 = 0, x15 = c15;
  u32 y0 = c0, y1 = x1, y2 = x2, y3 = x3, y4 = x4, y5 = c5, y6 = 0, y7 = 0,
      y8 = 0, y9 = 1, y10 = c10, y11 = 0, y12 = 0, y13 = 0, y14 = 0, y15 = c15;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    SALSA_QR2(x0, x4, x8, x12, y0, y4, y8, y12);
    SALSA_QR2(x5, x9, x13, x1, y5, y9, y13, y1);
    SALSA_QR2(x10, x14, x2, x6, y10, y14, y2, y6);
    SALSA_QR2(x15, x3, x7, x11, y15, y3, y7, y11);
    SALSA_QR2(x0, x1, x2, x3, y0, y1, y2, y3);
    SALSA_QR2(x5, x6, x7, x4, y5, y6, y7, y4);
    SALSA_QR2(x10, x11, x8, x9, y10, y11, y8, y9);
    SALSA_QR2(x15, x12, x13, x14, y15, y12, y13, y14);
  }
  r0 = make_uint4(x4 + seed.x, x3 + seed.y, x2 + seed.z, x1 + seed.w);
  r1 = make_uint4(y4 + seed.x, y3 + seed.y, y2 + seed.z, y1 + seed.w);
}

// Leaf-level variant: only the LOW output word (out[4] = x4 + seed.x) is
// needed, so the final double-round computes just the dataflow cone of
// x4: row-QR(x5,x6,x7,x4) needs post-column x5 (full QR), x6 (b,c,d of
// its QR), x7 (b,c), x4 (b) — 39 ops instead of 96.
#define SALSA_QR2_HEAD1(a, b, c, d, a2, b2, c2, d2) /* b only */ \
  b ^= rotl(a + d, 7);   b2 ^= rotl(a2 + d2, 7)
#define SALSA_QR2_HEAD2(a, b, c, d, a2, b2, c2, d2) /* b, c */ \
  b ^= rotl(a + d, 7);   b2 ^= rotl(a2 + d2, 7);   \
  c ^= rotl(b + a, 9);   c2 ^= rotl(b2 + a2, 9)
#define SALSA_QR2_HEAD3(a, b, c, d, a2, b2, c2, d2) /* b, c, d */ \
  b ^= rotl(a + d, 7);   b2 ^= rotl(a2 + d2, 7);   \
  c ^= rotl(b + a, 9);   c2 ^= rotl(b2 + a2, 9);   \
  d ^= rotl(c + b, 13);  d2 ^= rotl(c2 + b2, 13)

__device__ __forceinline__ void salsa12_pair_low_core(uint4 seed, u32& lo0,
                                                      u32& lo1) {
  const u32 c0 = 0x65787061u, c5 = 0x6e642033u, c10 = 0x322d6279u,
            c15 = 0x7465206bu;
  u32 x0 = c0, x1 = seed.w, x2 = seed.z, x3 = seed.y, x4 = seed.x, x5 = c5,
      x6 = 0, x7 = 0, x8 = 0, x9 = 0, x10 = c10, x11 = 0, x12 = 0, x13 = 0,
      x14 = 0, x15 = c15;
  u32 y0 = c0, y1 = x1, y2 = x2, y3 = x3, y4 = x4, y5 = c5, y6 = 0, y7 = 0,
      y8 = 0, y9 = 1, y10 = c10, y11 = 0, y12 = 0, y13 = 0, y14 = 0, y15 = c15;
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    SALSA_QR2(x0, x4, x8, x12, y0, y4, y8, y12);
    SALSA_QR2(x5, x9, x13, x1, y5, y9, y13, y1);
    SALSA_QR2(x10, x14, x2, x6, y10, y14, y2, y6);
    SALSA_QR2(x15, x3, x7, x11, y15, y3, y7, y11);
    SALSA_QR2(x0, x1, x2, x3, y0, y1, y2, y3);
    SALSA_QR2(x5, x6, x7, x4, y5, y6, y7, y4);
    SALSA_QR2(x10, x11, x8, x9, y10, y11, y8, y9);
    SALSA_QR2(x15, x12, x13, x14, y15, y12, y13, y14);
  }
  // 6th double-round, pruned to the cone of x4/y4:
  SALSA_QR2_HEAD1(x0, x4, x8, x12, y0, y4, y8, y12);   // new x4 (b)
  SALSA_QR2(x5, x9, x13, x1, y5, y9, y13, y1);         // new x5 (a: full)
  SALSA_QR2_HEAD3(x10, x14, x2, x6, y10, y14, y2, y6); // new x6 (d)
  SALSA_QR2_HEAD2(x15, x3, x7, x11, y15, y3, y7, y11); // new x7 (c)
  SALSA_QR2_HEAD3(x5, x6, x7, x4, y5, y6, y7, y4);     // row: new x4 (d)
  lo0 = x4 + seed.x;
  lo1 = y4 + seed.x;
}

// ---------------------------------------------------------------------------
// ChaCha20/12 (seed words 4..7 high->low, pos word 13, output words 4..7)
// ---------------------------------------------------------------------------
#define CHACHA_QR(a, b, c, d) \
  a += b;  d ^= a;  d = rotl(d, 16); \
  c += d;  b ^= c;  b = rotl(b, 12); \
  a += b;  d ^= a;  d = rotl(d, 8);  \
  c += d;  b ^= c;  b = rotl(b, 7)

__device__ __forceinline__ uint4 chacha12_core(uint4 seed, u32 pos) {
  u32 x0 = 0x65787061u, x1 = 0x6e642033u, x2 = 0x322d6279u, x3 = 0x7465206bu;
  u32 x4 = seed.w, x5 = seed.z, x6 = seed.y, x7 = seed.x;
  u32 x8 = 0, x9 = 0, x10 = 0, x11 = 0, x12 = 0, x13 = pos, x14 = 0, x15 = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    CHACHA_QR(x0, x4, x8, x12);
    CHACHA_QR(x1, x5, x9, x13);
    CHACHA_QR(x2, x6, x10, x14);
    CHACHA_QR(x3, x7, x11, x15);
    CHACHA_QR(x0, x5, x10, x15);
    CHACHA_QR(x1, x6, x11, x12);
    CHACHA_QR(x2, x7, x8, x13);
    CHACHA_QR(x3, x4, x9, x14);
  }
  return make_uint4(x7 + seed.x, x6 + seed.y, x5 + seed.z, x4 + seed.w);
}

#define CHACHA_QR2(a, b, c, d, a2, b2, c2, d2)                      \
  a += b;  a2 += b2;  d ^= a;  d2 ^= a2;                            \
  d = rotl(d, 16);  d2 = rotl(d2, 16);                              \
  c += d;  c2 += d2;  b ^= c;  b2 ^= c2;                            \
  b = rotl(b, 12);  b2 = rotl(b2, 12);                              \
  a += b;  a2 += b2;  d ^= a;  d2 ^= a2;                            \
  d = rotl(d, 8);  d2 = rotl(d2, 8);                                \
  c += d;  c2 += d2;  b ^= c;  b2 ^= c2;                            \
  b = rotl(b, 7);  b2 = rotl(b2, 7)

__device__ __forceinline__ void chacha12_pair_core(uint4 seed, uint4& r0,
                                                   uint4& r1) {
  const u32 k0 = 0x65787061u, k1 = 0x6e642033u, k2 = 0x322d6279u,
            k3 = 0x7465206bu;
  u32 x0 = k0, x1 = k1, x2 = k2, x3 = k3;
  u32 x4 = seed.w, x5 = seed.z, x6 = seed.y, x7 = seed.x;
  u32 x8 = 0, x9 = 0, x10 = 0, x11 = 0, x12 = 0, x13 = 0, x14 = 0, x15 = 0;
  u32 y0 = k0, y1 = k1, y2 = k2, y3 = k3;
  u32 y4 = x4, y5 = x5, y6 = x6, y7 = x7;
  u32 y8 = 0, y9 = 0, y10 = 0, y11 = 0, y12 = 0, y13 = 1, y14 = 0, y15 = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    CHACHA_QR2(x0, x4, x8, x12, y0, y4, y8, y12);
    CHACHA_QR2(x1, x5, x9, x13, y1, y5, y9, y13);
    CHACHA_QR2(x2, x6, x10, x14, y2, y6, y10, y14);
    CHACHA_QR2(x3, x7, x11, x15, y3, y7, y11, y15);
    CHACHA_QR2(x0, x5, x10, x15, y0, y5, y10, y15);
    CHACHA_QR2(x1, x6, x11, x12, y1, y6, y11, y12);
    CHACHA_QR2(x2, x7, x8, x13, y2, y7, y8, y13);
    CHACHA_QR2(x3, x4, x9, x14, y3, y4, y9, y14);
  }
  r0 = make_uint4(x7 + seed.x, x6 + seed.y, x5 + seed.z, x4 + seed.w);
  r1 = make_uint4(y7 + seed.x, y6 + seed.y, y5 + seed.z, y4 + seed.w);
}

// Leaf-level variant: only out[7] = x7 + seed.x is needed.  Final
// double-round cone: diagonal QR(x2,x7,x8,x13) needs its full chain;
// its inputs need x2 (full col QR), x7 (full: b needs a,c,d), x8 (col
// QR c through the second c+=d), x13 (col QR d through the second
// d-rotate) — 56 ops instead of 96.
#define CHACHA_QR2_C10(a, b, c, d, a2, b2, c2, d2) /* c final (skip last b) */ \
  a += b;  a2 += b2;  d ^= a;  d2 ^= a2;                            \
  d = rotl(d, 16);  d2 = rotl(d2, 16);                              \
  c += d;  c2 += d2;  b ^= c;  b2 ^= c2;                            \
  b = rotl(b, 12);  b2 = rotl(b2, 12);                              \
  a += b;  a2 += b2;  d ^= a;  d2 ^= a2;                            \
  d = rotl(d, 8);  d2 = rotl(d2, 8);                                \
  c += d;  c2 += d2
#define CHACHA_QR2_D10(a, b, c, d, a2, b2, c2, d2) /* d final (skip last c,b) */ \
  a += b;  a2 += b2;  d ^= a;  d2 ^= a2;                            \
  d = rotl(d, 16);  d2 = rotl(d2, 16);                              \
  c += d;  c2 += d2;  b ^= c;  b2 ^= c2;                            \
  b = rotl(b, 12);  b2 = rotl(b2, 12);                              \
  a += b;  a2 += b2;  d ^= a;  d2 ^= a2;                            \
  d = rotl(d, 8);  d2 = rotl(d2, 8)

__device__ __forceinline__ void chacha12_pair_low_core(uint4 seed, u32& lo0,
                                                       u32& lo1) {
  const u32 k0 = 0x65787061u, k1 = 0x6e642033u, k2 = 0x322d6279u,
            k3 = 0x7465206bu;
  u32 x0 = k0, x1 = k1, x2 = k2, x3 = k3;
  u32 x4 = seed.w, x5 = seed.z, x6 = seed.y, x7 = seed.x;
  u32 x8 = 0, x9 = 0, x10 = 0, x11 = 0, x12 = 0, x13 = 0, x14 = 0, x15 = 0;
  u32 y0 = k0, y1 = k1, y2 = k2, y3 = k3;
  u32 y4 = x4, y5 = x5, y6 = x6, y7 = x7;
  u32 y8 = 0, y9 = 0, y10 = 0, y11 = 0, y12 = 0, y13 = 1, y14 = 0, y15 = 0;
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    CHACHA_QR2(x0, x4, x8, x12, y0, y4, y8, y12);
    CHACHA_QR2(x1, x5, x9, x13, y1, y5, y9, y13);
    CHACHA_QR2(x2, x6, x10, x14, y2, y6, y10, y14);
    CHACHA_QR2(x3, x7, x11, x15, y3, y7, y11, y15);
    CHACHA_QR2(x0, x5, x10, x15, y0, y5, y10, y15);
    CHACHA_QR2(x1, x6, x11, x12, y1, y6, y11, y12);
    CHACHA_QR2(x2, x7, x8, x13, y2, y7, y8, y13);
    CHACHA_QR2(x3, x4, x9, x14, y3, y4, y9, y14);
  }
  // 6th double-round, pruned to the cone of x7/y7:
  CHACHA_QR2_C10(x0, x4, x8, x12, y0, y4, y8, y12);   // x8 (c)
  CHACHA_QR2_D10(x1, x5, x9, x13, y1, y5, y9, y13);   // x13 (d)
  CHACHA_QR2(x2, x6, x10, x14, y2, y6, y10, y14);     // x2 (a: full)
  CHACHA_QR2(x3, x7, x11, x15, y3, y7, y11, y15);     // x7 (b: full)
  CHACHA_QR2(x2, x7, x8, x13, y2, y7, y8, y13);       // diagonal: x7 (b)
  lo0 = x7 + seed.x;
  lo1 = y7 + seed.x;
}

// ---------------------------------------------------------------------------
// AES-128, replicated-LDS variant (fused kernel).  The LDS holds te0
// replicated AES_REP = 64-way with a 256-byte entry stride: word (entry e,
// copy c) sits at LDS byte e*256 + c*4, and lane l always uses copy l%64.
//   * Bank = (addr/4)%32 = l%32 inside each 32-lane ds_read_b32 group:
//     conflict-free.
//   * The byte address of te0[byte K of w] is ONE v_perm_b32: byte 1 of
//     the address is byte K of w, byte 0 is lane*4 (<= 252), bytes 2..3
//     are zero.  (The 32-way layout needed bfe + shift-add + add.)
//   * The table starts at LDS byte 0, so that integer IS the address: the
//     access is formed as an address_space(3) load from it, with no add
//     of a table base.  This relies on every kernel that builds an AesLds
//     having no static LDS (dynamic LDS then starts at 0) and placing the
//     table first in its dynamic LDS map.
//   te0[x] bytes (MSB..LSB) = [2s, s, s, 3s];  te1 = ror8(te0),
//   te2 = ror16, te3 = ror24;  sbox[x] = byte2 of te0[x].
// ---------------------------------------------------------------------------
struct AesLds {
  u32 lane4;  // (threadIdx.x % 64) * 4
  typedef __attribute__((address_space(3))) const u32 lds_u32;
  static __device__ __forceinline__ u32 ld(u32 byte_addr) {
    return *reinterpret_cast<lds_u32*>(byte_addr);
  }
  // byte address of te0[byte K of w] (K = 0 is the LSB)
  template <int K>
  __device__ __forceinline__ u32 addr_b(u32 w) const {
    return __builtin_amdgcn_perm(w, lane4, 0x0c0c0000u | ((4u + K) << 8));
  }
  template <int K>
  __device__ __forceinline__ u32 te0_b(u32 w) const { return ld(addr_b<K>(w)); }
  template <int K>
  __device__ __forceinline__ u32 sbox_b(u32 w) const {
    return (te0_b<K>(w) >> 16) & 0xff;
  }
  __device__ __forceinline__ u32 te0(u32 x) const { return ld((x << 8) | lane4); }
};

// Stage the replicated te0 table at LDS byte 0 (all threads of the
// workgroup; the caller synchronizes).  `lds0` must be the start of the
// kernel's dynamic LDS.  Word index e*64 + c => consecutive threads write
// consecutive banks.
__device__ __forceinline__ void aes_stage_table(u32* lds0,
                                                const u32* __restrict__ aes_tabs) {
  for (int idx = (int)threadIdx.x; idx < AES_LDS_WORDS; idx += (int)blockDim.x)
    lds0[idx] = aes_tabs[idx >> 6];  // global layout: te0 at offset 0
}

__device__ __forceinline__ u32 xor3(u32 a, u32 b, u32 c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);  // a ^ b ^ c
}

// [S(a) S(b) S(c) S(d)] (MSB..LSB) from the four te0 words of a..d: sbox
// is byte 2 of te0, gathered by two v_perm_b32 with disjoint bytes (the
// caller xors the halves into its sum).
#define AES_SB_HI(ta, tb) __builtin_amdgcn_perm(ta, tb, 0x06020c0cu)
#define AES_SB_LO(tc, td) __builtin_amdgcn_perm(tc, td, 0x0c0c0602u)

// One MixColumns output word: te0[a.b3] ^ te1[b.b2] ^ te2[c.b1] ^
// te3[d.b0] ^ k as two 3-input xors.
#define AES_COL(T, a, b, c, d, k)                                         \
  xor3(xor3((T).template te0_b<3>(a), rotr8((T).template te0_b<2>(b)),    \
            rotr16((T).template te0_b<1>(c))),                            \
       rotr24((T).template te0_b<0>(d)), k)

// Both children (pos 0 and pos 1) with an ON-THE-FLY key schedule fused
// into the interleaved cipher rounds: the key-expansion sbox chain (4
// dependent LDS lookups per round) overlaps the 32 independent cipher
// lookups of the same round instead of standing alone as a 40-deep serial
// latency chain (PMC: SQ_WAIT_ANY was 31.5% of wave cycles with the
// standalone schedule).  Also drops the rk[44] register array.
template <bool LOW>
__device__ __forceinline__ void aes_cipher_pair(uint4 seed, const AesLds& T,
                                                uint4& ra, uint4& rb) {
  u32 k0 = __builtin_bswap32(seed.x), k1 = __builtin_bswap32(seed.y),
      k2 = __builtin_bswap32(seed.z), k3 = __builtin_bswap32(seed.w);
  u32 s0 = k0, s1 = k1, s2 = k2, s3 = k3;
  u32 u0 = (1u << 24) ^ k0, u1 = k1, u2 = k2, u3 = k3;
  u32 rcon = 0x01u;
  int r_begin = 1;
#ifndef GPUDPF_AES_NOSHARE
  // Shared-prefix rounds: the two children's plaintexts (pos 0 / pos 1)
  // differ in a single byte, so their states agree except for byte
  // (s0 >> 24) until MixColumns diffuses it — round 1 of child b costs
  // ONE extra T-lookup (all four output words share), and round 2 shares
  // 12 of its 16 lookups (each output word reads exactly one byte of the
  // diverged word 0).  Saves ~27 of ~320 lookups per pair; rounds 3+ are
  // fully diverged and run the common loop below.  A/B toggle:
  // compile with -DGPUDPF_AES_NOSHARE for the straight dual-cipher
  // variant (measured comparison in profiles/PROFILING.md).
  {
    // round 1.  s3 == k3 here (the position byte only enters s0), so the
    // four te0 words of s3 the cipher round reads anyway also carry the
    // sbox bytes of the round-1 key schedule: no separate sbox lookups.
    const u32 t33 = T.te0_b<3>(s3), t32 = T.te0_b<2>(s3),
              t31 = T.te0_b<1>(s3), t30 = T.te0_b<0>(s3);
    k0 = xor3(AES_SB_HI(t32, t31), AES_SB_LO(t30, t33), k0) ^ (rcon << 24);
    rcon = 0x02u;
    k1 ^= k0; k2 ^= k1; k3 ^= k2;
    const u32 a0 = T.addr_b<3>(s0);
    const u32 A = AesLds::ld(a0);
    u32 n0 = xor3(xor3(A, rotr8(T.te0_b<2>(s1)), rotr16(T.te0_b<1>(s2))),
                  rotr24(t30), k0);
    u32 n1 = xor3(xor3(T.te0_b<3>(s1), rotr8(T.te0_b<2>(s2)), rotr16(t31)),
                  rotr24(T.te0_b<0>(s0)), k1);
    u32 n2 = xor3(xor3(T.te0_b<3>(s2), rotr8(t32), rotr16(T.te0_b<1>(s0))),
                  rotr24(T.te0_b<0>(s1)), k2);
    u32 n3 = xor3(xor3(t33, rotr8(T.te0_b<2>(s0)), rotr16(T.te0_b<1>(s1))),
                  rotr24(T.te0_b<0>(s2)), k3);
    // child b differs in bit 0 of byte (s0 >> 24): entry index ^ 1 is
    // address ^ 256
    const u32 m0 = xor3(n0, A, AesLds::ld(a0 ^ 256u));
    // round 2
    k0 = xor3(AES_SB_HI(T.te0_b<2>(k3), T.te0_b<1>(k3)),
              AES_SB_LO(T.te0_b<0>(k3), T.te0_b<3>(k3)), k0) ^ (rcon << 24);
    rcon = 0x04u;
    k1 ^= k0; k2 ^= k1; k3 ^= k2;
    const u32 c0 = xor3(rotr8(T.te0_b<2>(n1)), rotr16(T.te0_b<1>(n2)),
                        rotr24(T.te0_b<0>(n3))) ^ k0;
    const u32 c1 = xor3(T.te0_b<3>(n1), rotr8(T.te0_b<2>(n2)),
                        rotr16(T.te0_b<1>(n3))) ^ k1;
    const u32 c2 = xor3(T.te0_b<3>(n2), rotr8(T.te0_b<2>(n3)),
                        rotr24(T.te0_b<0>(n1))) ^ k2;
    const u32 c3 = xor3(T.te0_b<3>(n3), rotr16(T.te0_b<1>(n1)),
                        rotr24(T.te0_b<0>(n2))) ^ k3;
    s0 = T.te0_b<3>(n0) ^ c0;
    u0 = T.te0_b<3>(m0) ^ c0;
    s1 = rotr24(T.te0_b<0>(n0)) ^ c1;
    u1 = rotr24(T.te0_b<0>(m0)) ^ c1;
    s2 = rotr16(T.te0_b<1>(n0)) ^ c2;
    u2 = rotr16(T.te0_b<1>(m0)) ^ c2;
    s3 = rotr8(T.te0_b<2>(n0)) ^ c3;
    u3 = rotr8(T.te0_b<2>(m0)) ^ c3;
    r_begin = 3;
  }
#endif
#pragma unroll
  for (int r = r_begin; r < 10; ++r) {
    // next round key (k0..k3 become rk[4r..4r+3])
    k0 = xor3(AES_SB_HI(T.te0_b<2>(k3), T.te0_b<1>(k3)),
              AES_SB_LO(T.te0_b<0>(k3), T.te0_b<3>(k3)), k0) ^ (rcon << 24);
    rcon = (rcon << 1) ^ ((rcon & 0x80u) ? 0x11bu : 0u);
    rcon &= 0xffu;
    k1 ^= k0; k2 ^= k1; k3 ^= k2;
    // cipher round r for both children
    u32 n0 = AES_COL(T, s0, s1, s2, s3, k0);
    u32 m0 = AES_COL(T, u0, u1, u2, u3, k0);
    u32 n1 = AES_COL(T, s1, s2, s3, s0, k1);
    u32 m1 = AES_COL(T, u1, u2, u3, u0, k1);
    u32 n2 = AES_COL(T, s2, s3, s0, s1, k2);
    u32 m2 = AES_COL(T, u2, u3, u0, u1, k2);
    u32 n3 = AES_COL(T, s3, s0, s1, s2, k3);
    u32 m3 = AES_COL(T, u3, u0, u1, u2, k3);
    s0 = n0; s1 = n1; s2 = n2; s3 = n3;
    u0 = m0; u1 = m1; u2 = m2; u3 = m3;
  }
  // round-10 key
  k0 = xor3(AES_SB_HI(T.te0_b<2>(k3), T.te0_b<1>(k3)),
            AES_SB_LO(T.te0_b<0>(k3), T.te0_b<3>(k3)), k0) ^ (rcon << 24);
  k1 ^= k0; k2 ^= k1; k3 ^= k2;
  // last round: [S(a.b3) S(b.b2) S(c.b1) S(d.b0)] ^ k
#define AES_LAST(a, b, c, d, k)                               \
  xor3(AES_SB_HI(T.te0_b<3>(a), T.te0_b<2>(b)),               \
       AES_SB_LO(T.te0_b<1>(c), T.te0_b<0>(d)), k)
  u32 o0 = AES_LAST(s0, s1, s2, s3, k0);
  u32 p0 = AES_LAST(u0, u1, u2, u3, k0);
  if constexpr (LOW) {
    ra = make_uint4(__builtin_bswap32(o0), 0, 0, 0);
    rb = make_uint4(__builtin_bswap32(p0), 0, 0, 0);
    return;
  }
  u32 o1 = AES_LAST(s1, s2, s3, s0, k1);
  u32 p1 = AES_LAST(u1, u2, u3, u0, k1);
  u32 o2 = AES_LAST(s2, s3, s0, s1, k2);
  u32 p2 = AES_LAST(u2, u3, u0, u1, k2);
  u32 o3 = AES_LAST(s3, s0, s1, s2, k3);
  u32 p3 = AES_LAST(u3, u0, u1, u2, k3);
#undef AES_LAST
  ra = make_uint4(__builtin_bswap32(o0), __builtin_bswap32(o1),
                  __builtin_bswap32(o2), __builtin_bswap32(o3));
  rb = make_uint4(__builtin_bswap32(p0), __builtin_bswap32(p1),
                  __builtin_bswap32(p2), __builtin_bswap32(p3));
}

// ---------------------------------------------------------------------------
// PRF dispatch (fused kernel: AES uses the replicated LDS table)
// ---------------------------------------------------------------------------
template <int PRF>
__device__ __forceinline__ uint4 prf_full(uint4 seed, u32 pos,
                                          const AesLds& T) {
  if constexpr (PRF == PRF_DUMMY) return prf_dummy_full(seed, pos);
  if constexpr (PRF == PRF_SALSA20) return salsa12_core(seed, pos);
  if constexpr (PRF == PRF_CHACHA20) return chacha12_core(seed, pos);
  if constexpr (PRF == PRF_AES128) {
    uint4 a, b;
    aes_cipher_pair<false>(seed, T, a, b);
    return pos ? b : a;
  }
}

template <int PRF>
__device__ __forceinline__ void prf_pair(uint4 seed, const AesLds& T,
                                         uint4& r0, uint4& r1) {
  if constexpr (PRF == PRF_AES128) {
    aes_cipher_pair<false>(seed, T, r0, r1);
  } else if constexpr (PRF == PRF_SALSA20) {
    salsa12_pair_core(seed, r0, r1);
  } else if constexpr (PRF == PRF_CHACHA20) {
    chacha12_pair_core(seed, r0, r1);
  } else {
    r0 = prf_full<PRF>(seed, 0, T);
    r1 = prf_full<PRF>(seed, 1, T);
  }
}

template <int PRF>
__device__ __forceinline__ void prf_pair_low(uint4 seed, const AesLds& T,
                                             u32& r0, u32& r1) {
  if constexpr (PRF == PRF_DUMMY) {
    r0 = seed.x * 4242u + 4242u;
    r1 = seed.x * 4243u + 4243u;
  } else if constexpr (PRF == PRF_SALSA20) {
    salsa12_pair_low_core(seed, r0, r1);
  } else if constexpr (PRF == PRF_CHACHA20) {
    chacha12_pair_low_core(seed, r0, r1);
  } else {
    uint4 a, b;
    aes_cipher_pair<true>(seed, T, a, b);
    r0 = a.x;
    r1 = b.x;
  }
}

}  // namespace gpudpf_hip
