// Device PRFs and 128-bit helpers shared by every DPF kernel (dpf_eval.hip,
// dpf_strategies.hip, dpf_probes.hip).  They mirror csrc/core/prf.cc
// bit-exactly (tested by tests/test_gpu.py and tests/test_gpu_alu.py
// against the CPU core).
//
// CONTRACT for kernels that build an AesLds (see the AES section below):
// no static LDS, and the replicated te0/te2 table (aes_stage_table) first in
// the dynamic LDS map, so that the table starts at LDS byte 0.
//
// How the file is organised, and how a change to it is checked for equal
// generated code: docs/KERNEL_NOTES.md.
#pragma once
#include "hip_util.h"

namespace gpudpf_hip {

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

// The unpacked root seed of the key that starts at `key` (wire layout in
// dpf_core.h)
__device__ __forceinline__ uint4 key_root(const int* key) {
  const int* rp = key + kKeyRootInt;
  return make_uint4((u32)rp[0], (u32)rp[1], (u32)rp[2], (u32)rp[3]);
}

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
// Salsa20/12 and ChaCha20/12 over N interleaved chains.  The state is
// x[word][chain]; chain i is the block at pos + i, so N = 2 from pos 0 is
// both children in one pass: the two blocks are independent dependency
// chains, so interleaving doubles the ILP the SIMD can draw on — the DFS
// runs at ~2 waves/SIMD where a single chain's QR latency is not fully
// hidden.  Every step of a quarter-round therefore runs over all chains
// before the next step starts.  The word indices are constants after
// inlining, so the state lives in registers.
//
// PART: a quarter-round runs only its first PART steps.  The LOW drivers
// (leaf level: only the low output word is needed) use it to prune the last
// double-round to the dataflow cone of that word.
// ---------------------------------------------------------------------------
// Every chain starts from the same 16 words; chain i adds i to word `pos_w`.
template <int N>
__device__ __forceinline__ void stream_init(u32 (&x)[16][N], int pos_w,
                                            const u32 (&init)[16]) {
#pragma unroll
  for (int w = 0; w < 16; ++w)
#pragma unroll
    for (int i = 0; i < N; ++i) x[w][i] = init[w] + (w == pos_w ? i : 0);
}

// Chain i's output: the feed-forward of the four words that held the seed,
// x[lo] (seed.x) down to x[lo - 3] (seed.w).
template <int N>
__device__ __forceinline__ uint4 stream_out(const u32 (&x)[16][N], int i,
                                            int lo, uint4 seed) {
  return make_uint4(x[lo][i] + seed.x, x[lo - 1][i] + seed.y,
                    x[lo - 2][i] + seed.z, x[lo - 3][i] + seed.w);
}

// ---------------------------------------------------------------------------
// Salsa20/12 (conventions: seed words 1..4 high->low, pos word 9, output
// words 1..4 — see csrc/core/prf.cc).  QR steps: 1 b, 2 c, 3 d, 4 a.
// ---------------------------------------------------------------------------
template <int PART = 4, int N>
__device__ __forceinline__ void salsa_qr(u32 (&x)[16][N], int a, int b, int c,
                                         int d) {
  auto step = [&](int t, int p, int q, int s) {
#pragma unroll
    for (int i = 0; i < N; ++i) x[t][i] ^= rotl(x[p][i] + x[q][i], s);
  };
  step(b, a, d, 7);
  if constexpr (PART > 1) step(c, b, a, 9);
  if constexpr (PART > 2) step(d, c, b, 13);
  if constexpr (PART > 3) step(a, d, c, 18);
}

// 12 rounds = 6 double-rounds (column, then row) on chains pos .. pos+N-1.
// LOW: only the low output word (out[4] = x4 + seed.x) is needed, so the
// final double-round computes just the dataflow cone of x4:
// row-QR(x5,x6,x7,x4) needs post-column x5 (full QR), x6 (b,c,d of its QR),
// x7 (b,c), x4 (b) — 39 ops instead of 96.  Only x[4] is then valid.
template <bool LOW, int N>
__device__ __forceinline__ void salsa12(uint4 seed, u32 pos, u32 (&x)[16][N]) {
  stream_init(x, 9, {0x65787061u, seed.w, seed.z, seed.y, seed.x, 0x6e642033u,
                     0, 0, 0, pos, 0x322d6279u, 0, 0, 0, 0, 0x7465206bu});
#pragma unroll
  for (int r = 0; r < (LOW ? 5 : 6); ++r) {
    salsa_qr(x, 0, 4, 8, 12);
    salsa_qr(x, 5, 9, 13, 1);
    salsa_qr(x, 10, 14, 2, 6);
    salsa_qr(x, 15, 3, 7, 11);
    salsa_qr(x, 0, 1, 2, 3);
    salsa_qr(x, 5, 6, 7, 4);
    salsa_qr(x, 10, 11, 8, 9);
    salsa_qr(x, 15, 12, 13, 14);
  }
  if constexpr (LOW) {
    salsa_qr<1>(x, 0, 4, 8, 12);   // new x4 (b)
    salsa_qr(x, 5, 9, 13, 1);      // new x5 (a: full)
    salsa_qr<3>(x, 10, 14, 2, 6);  // new x6 (d)
    salsa_qr<2>(x, 15, 3, 7, 11);  // new x7 (c)
    salsa_qr<3>(x, 5, 6, 7, 4);    // row: new x4 (d)
  }
}

__device__ __forceinline__ uint4 salsa12_core(uint4 seed, u32 pos) {
  u32 x[16][1];
  salsa12<false>(seed, pos, x);
  return stream_out(x, 0, 4, seed);
}

__device__ __forceinline__ void salsa12_pair_core(uint4 seed, uint4& r0,
                                                  uint4& r1) {
  u32 x[16][2];
  salsa12<false>(seed, 0, x);
  r0 = stream_out(x, 0, 4, seed);
  r1 = stream_out(x, 1, 4, seed);
}

__device__ __forceinline__ void salsa12_pair_low_core(uint4 seed, u32& lo0,
                                                      u32& lo1) {
  u32 x[16][2];
  salsa12<true>(seed, 0, x);
  lo0 = x[4][0] + seed.x;
  lo1 = x[4][1] + seed.x;
}

// ---------------------------------------------------------------------------
// ChaCha20/12 (seed words 4..7 high->low, pos word 13, output words 4..7).
// QR steps: 1 a+=b, 2 d^=a <<<16, 3 c+=d, 4 b^=c <<<12, 5 a+=b, 6 d^=a <<<8,
// 7 c+=d, 8 b^=c <<<7.  PART is 6 (d final), 7 (c final) or 8.
// ---------------------------------------------------------------------------
template <int PART = 8, int N>
__device__ __forceinline__ void chacha_qr(u32 (&x)[16][N], int a, int b, int c,
                                          int d) {
  static_assert(PART >= 6 && PART <= 8, "only the tail is ever pruned");
  auto add = [&](int t, int s) {
#pragma unroll
    for (int i = 0; i < N; ++i) x[t][i] += x[s][i];
  };
  auto xor_rotl = [&](int t, int s, int r) {
#pragma unroll
    for (int i = 0; i < N; ++i) x[t][i] ^= x[s][i];
#pragma unroll
    for (int i = 0; i < N; ++i) x[t][i] = rotl(x[t][i], r);
  };
  add(a, b);  xor_rotl(d, a, 16);
  add(c, d);  xor_rotl(b, c, 12);
  add(a, b);  xor_rotl(d, a, 8);
  if constexpr (PART > 6) add(c, d);
  if constexpr (PART > 7) xor_rotl(b, c, 7);
}

// 12 rounds = 6 double-rounds (column, then diagonal) on chains
// pos .. pos+N-1.  LOW: only out[7] = x7 + seed.x is needed.  Final
// double-round cone: diagonal QR(x2,x7,x8,x13) needs its full chain; its
// inputs need x2 (full col QR), x7 (full: b needs a,c,d), x8 (col QR c
// through the second c+=d), x13 (col QR d through the second d-rotate) —
// 56 ops instead of 96.  Only x[7] is then valid.
template <bool LOW, int N>
__device__ __forceinline__ void chacha12(uint4 seed, u32 pos,
                                         u32 (&x)[16][N]) {
  stream_init(x, 13, {0x65787061u, 0x6e642033u, 0x322d6279u, 0x7465206bu,
                      seed.w, seed.z, seed.y, seed.x, 0, 0, 0, 0, 0, pos, 0, 0});
#pragma unroll
  for (int r = 0; r < (LOW ? 5 : 6); ++r) {
    chacha_qr(x, 0, 4, 8, 12);
    chacha_qr(x, 1, 5, 9, 13);
    chacha_qr(x, 2, 6, 10, 14);
    chacha_qr(x, 3, 7, 11, 15);
    chacha_qr(x, 0, 5, 10, 15);
    chacha_qr(x, 1, 6, 11, 12);
    chacha_qr(x, 2, 7, 8, 13);
    chacha_qr(x, 3, 4, 9, 14);
  }
  if constexpr (LOW) {
    chacha_qr<7>(x, 0, 4, 8, 12);  // x8 (c)
    chacha_qr<6>(x, 1, 5, 9, 13);  // x13 (d)
    chacha_qr(x, 2, 6, 10, 14);    // x2 (a: full)
    chacha_qr(x, 3, 7, 11, 15);    // x7 (b: full)
    chacha_qr(x, 2, 7, 8, 13);     // diagonal: x7 (b)
  }
}

__device__ __forceinline__ uint4 chacha12_core(uint4 seed, u32 pos) {
  u32 x[16][1];
  chacha12<false>(seed, pos, x);
  return stream_out(x, 0, 7, seed);
}

__device__ __forceinline__ void chacha12_pair_core(uint4 seed, uint4& r0,
                                                   uint4& r1) {
  u32 x[16][2];
  chacha12<false>(seed, 0, x);
  r0 = stream_out(x, 0, 7, seed);
  r1 = stream_out(x, 1, 7, seed);
}

__device__ __forceinline__ void chacha12_pair_low_core(uint4 seed, u32& lo0,
                                                       u32& lo1) {
  u32 x[16][2];
  chacha12<true>(seed, 0, x);
  lo0 = x[7][0] + seed.x;
  lo1 = x[7][1] + seed.x;
}

// ---------------------------------------------------------------------------
// AES-128, replicated-LDS variant (fused kernel).  The LDS holds te0 and
// te2 = ror16(te0), each replicated AES_COPIES = 32-way, with a 256-byte
// entry stride: the word (entry e, copy c, half h) sits at LDS byte
// e*256 + h*128 + c*4, half 0 = te0[e], half 1 = te2[e], and lane l always
// uses copy l%32.
//   * Bank = (addr/4)%32 = (e*64 + h*32 + c)%32 = c.  A ds_read_b32 is
//     served in two groups of 32 lanes, {0-31} and {32-63}; inside a group
//     every lane has its own copy, hence its own bank: conflict-free.
//     Lanes l and l+32 share a copy but are never in the same group.
//   * The byte address of te0[byte K of w] is ONE v_perm_b32: byte 1 of
//     the address is byte K of w, byte 0 is (lane%32)*4 (<= 124), bytes
//     2..3 are zero.  te2[byte K of w] is the SAME address read at +128,
//     which is the ds_read_b32 immediate `offset:128`: no VALU
//     instruction, no second address register.
//   * The table starts at LDS byte 0, so that integer IS the address: the
//     access is formed as an address_space(3) load from it, with no add
//     of a table base.  This relies on every kernel that builds an AesLds
//     having no static LDS (dynamic LDS then starts at 0) and placing the
//     table first in its dynamic LDS map.
//   te0[x] bytes (MSB..LSB) = [2s, s, s, 3s];  te1 = ror8(te0),
//   te2 = ror16, te3 = ror24;  sbox[x] = byte 2 of te0[x] = byte 0 of
//   te2[x].
//
// Rotations.  Rotation commutes with xor, so a MixColumns word
//   te0[a] ^ ror8(te0[b]) ^ ror16(te0[c]) ^ ror24(te0[d]) ^ k
// is  xor3(te0[a], te2[c], ror8(xor3(te0[b], te2[d], rol8(k)))):  one
// rotate per word (AesLds::mix).  The key schedule is equivariant under
// byte rotation (RotWord and SubWord act bytewise; only the round constant
// moves, from byte 3 to byte 0), so aes_cipher_pair runs it on
// q = rol8(k) from the start and never forms k: the last round's sbox
// gather places its bytes one position up as well, and the rotation that
// is left folds into the byte swap at the cipher's exit (bswap_rol8).
//
// Everything the contract fixes is stated here: the table's size
// (aes_lds_u32: what a launcher adds to its dynamic LDS and a kernel skips
// to reach its own LDS), its staging (aes_stage_table) and the lane's
// binding (AesLds::lane); aes_lds_init is the three together.
// ---------------------------------------------------------------------------
constexpr int AES_COPIES = 32;            // one per lane of a ds_read_b32 group
constexpr int AES_REP = AES_COPIES * 2;   // words per entry: 32 te0, 32 te2
constexpr int AES_LDS_WORDS = 256 * AES_REP;  // 64 KiB
constexpr u32 AES_TE2_BYTES = AES_COPIES * 4;  // te2 half: +128 in the row

// u32s of dynamic LDS the table takes in front of a kernel's own LDS map
__host__ __device__ constexpr int aes_lds_u32(int prf) {
  return prf == PRF_AES128 ? AES_LDS_WORDS : 0;
}

__device__ __forceinline__ u32 xor3(u32 a, u32 b, u32 c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);  // a ^ b ^ c
}

// Two sbox bytes gathered into one word by a v_perm_b32: byte BA of `ta`
// goes to result byte PA, byte BB of `tb` to result byte PB, the other two
// bytes are zero.  sbox is byte 2 of a te0 word and byte 0 of a te2 word.
// Two gathers with disjoint bytes make a SubWord; the caller's three-input
// xor folds them into its sum.
template <int PA, int PB, int BA = 2, int BB = 2>
__device__ __forceinline__ u32 aes_sb_pair(u32 ta, u32 tb) {
  static_assert(PA != PB, "the two bytes land in different places");
  constexpr u32 sel = (0x0c0c0c0cu & ~(0xffu << (8 * PA)) &
                       ~(0xffu << (8 * PB))) |
                      ((4u + BA) << (8 * PA)) | ((u32)BB << (8 * PB));
  return __builtin_amdgcn_perm(ta, tb, sel);
}

// rol8(bswap32(x)) = bswap32(ror8(x)): between the little-endian seed /
// output words and the cipher's byte-rotated big-endian words, one v_perm_b32
__device__ __forceinline__ u32 bswap_rol8(u32 x) {
  return __builtin_amdgcn_perm(0u, x, 0x01020300u);
}

struct AesLds {
  u32 lane4;  // (threadIdx.x % 32) * 4
  // The calling lane's copy of the table
  static __device__ __forceinline__ AesLds lane() {
    return AesLds{((u32)threadIdx.x & (u32)(AES_COPIES - 1)) << 2};
  }
  typedef __attribute__((address_space(3))) const u32 lds_u32;
  static __device__ __forceinline__ u32 ld(u32 byte_addr) {
    return *reinterpret_cast<lds_u32*>(byte_addr);
  }
  // the te2 word of the row whose te0 word is at byte_addr: the constant
  // becomes the read's immediate offset
  static __device__ __forceinline__ u32 ld_te2(u32 byte_addr) {
    return reinterpret_cast<lds_u32*>(byte_addr)[AES_TE2_BYTES / 4];
  }
  // byte address of te0[byte K of w] (K = 0 is the LSB)
  template <int K>
  __device__ __forceinline__ u32 addr_b(u32 w) const {
    return __builtin_amdgcn_perm(w, lane4, 0x0c0c0000u | ((4u + K) << 8));
  }
  template <int K>
  __device__ __forceinline__ u32 te0_b(u32 w) const { return ld(addr_b<K>(w)); }
  template <int K>
  __device__ __forceinline__ u32 te2_b(u32 w) const {
    return ld_te2(addr_b<K>(w));
  }
  // The same three for byte K of the word k given as q = rol8(k): byte
  // (K+1)%4 of q
  template <int K>
  __device__ __forceinline__ u32 addr_kb(u32 q) const {
    return addr_b<(K + 1) & 3>(q);
  }
  template <int K>
  __device__ __forceinline__ u32 te0_kb(u32 q) const { return ld(addr_kb<K>(q)); }
  template <int K>
  __device__ __forceinline__ u32 te2_kb(u32 q) const {
    return ld_te2(addr_kb<K>(q));
  }
  // te0a ^ ror8(te0b) ^ te2c ^ ror8(te2d) ^ ror8(q) from four looked-up
  // words and q = rol8(round key word)
  static __device__ __forceinline__ u32 mix(u32 te0a, u32 te0b, u32 te2c,
                                            u32 te2d, u32 q) {
    return xor3(te0a, te2c, rotr8(xor3(te0b, te2d, q)));
  }
  // One output word in two halves: *_issue starts its four reads, and the
  // combine (mix, last, key of the Words) may come any time later.
  struct Words { u32 a, b, c, d; };
  // One MixColumns output word: te0[a.b3] ^ te1[b.b2] ^ te2[c.b1] ^
  // te3[d.b0] ^ k, given q = rol8(k)
  __device__ __forceinline__ Words col_issue(u32 a, u32 b, u32 c, u32 d) const {
    return {te0_b<3>(a), te0_b<2>(b), te2_b<1>(c), te2_b<0>(d)};
  }
  static __device__ __forceinline__ u32 mix(const Words& l, u32 q) {
    return mix(l.a, l.b, l.c, l.d, q);
  }
  // One last-round output word, rotated like its key word:
  // rol8([S(a.b3) S(b.b2) S(c.b1) S(d.b0)] ^ k), given q = rol8(k)
  __device__ __forceinline__ Words last_issue(u32 a, u32 b, u32 c,
                                              u32 d) const {
    return {te0_b<3>(a), te0_b<2>(b), te0_b<1>(c), te0_b<0>(d)};
  }
  static __device__ __forceinline__ u32 last(const Words& l, u32 q) {
    return xor3(aes_sb_pair<0, 3>(l.a, l.b), aes_sb_pair<2, 1>(l.c, l.d), q);
  }
  // SubWord(RotWord(.)) of the key schedule reads q3 = rol8(k3) as it would
  // read k3; key() is the new q0 before the round constant (in byte 0)
  __device__ __forceinline__ Words key_issue(u32 q3) const {
    return {te0_b<2>(q3), te0_b<1>(q3), te0_b<0>(q3), te0_b<3>(q3)};
  }
  static __device__ __forceinline__ u32 key(const Words& l, u32 q0) {
    return xor3(aes_sb_pair<3, 2>(l.a, l.b), aes_sb_pair<1, 0>(l.c, l.d), q0);
  }
};

// Stage the table at LDS byte 0 (all threads of the workgroup; the caller
// synchronizes); nothing for the other PRFs.  `lds0` must be the start of
// the kernel's dynamic LDS.  Word index e*64 + h*32 + c => consecutive
// threads write consecutive banks, and a wave writes one whole row: lanes
// 0-31 its te0 half, lanes 32-63 its te2 half.
template <int PRF>
__device__ __forceinline__ void aes_stage_table(
    u32* lds0, const u32* __restrict__ aes_tabs) {
  if constexpr (PRF == PRF_AES128) {
    // global layout: te0 at word 0, te2 at word 512
    for (int idx = (int)threadIdx.x; idx < AES_LDS_WORDS;
         idx += (int)blockDim.x)
      lds0[idx] = aes_tabs[(((idx >> 5) & 1) << 9) + (idx >> 6)];
  }
}

// The whole prologue of a kernel that stages nothing else: table, barrier
// (AES only), lane binding.
template <int PRF>
__device__ __forceinline__ AesLds aes_lds_init(
    u32* lds0, const u32* __restrict__ aes_tabs) {
  aes_stage_table<PRF>(lds0, aes_tabs);
  if constexpr (PRF == PRF_AES128) __syncthreads();
  return AesLds::lane();
}

// Both children (pos 0 and pos 1) with an ON-THE-FLY key schedule fused
// into the interleaved cipher rounds: the key-expansion sbox chain (4
// dependent LDS lookups per round) overlaps the 32 independent cipher
// lookups of the same round instead of standing alone as a 40-deep serial
// latency chain (PMC: SQ_WAIT_ANY was 31.5% of wave cycles with the
// standalone schedule).  Also drops the rk[44] register array.
//
// __builtin_amdgcn_sched_barrier(0) pins the order of lookups and combines:
// child a's round r is combined and its round r+1 issued (16 lookups) while
// child b's round r is in flight, then the other way round.  The s_waitcnt
// are the compiler's, counted because LDS reads return in order; one counts
// at most 15 LDS operations on gfx950, so a round's first wait drains to 14
// and issuing further ahead would leave no more in flight (KERNEL_NOTES.md).
template <bool LOW>
__device__ __forceinline__ void aes_cipher_pair(uint4 seed, const AesLds& T,
                                                uint4& ra, uint4& rb) {
  // The key schedule runs on q = rol8(round key) (header: Rotations).  Before
  // round 1 q0..q3 are also the state, read through the *_kb accessors.
  u32 q0 = bswap_rol8(seed.x), q1 = bswap_rol8(seed.y),
      q2 = bswap_rol8(seed.z), q3 = bswap_rol8(seed.w);
  u32 rcon = 0x02u;
  // Round 1.  The two children's plaintexts (pos 0 / pos 1) differ in a
  // single byte, so their states agree except for byte 3 of word 0: the 16
  // lookups x<word><byte> below are both children's, and child b costs ONE
  // more (x03b).  Bytes 3 and 2 of a word are read from te0, bytes 1 and 0
  // from te2, as col_issue does.
  const u32 a0 = T.addr_kb<3>(q0);
  const u32 x03 = AesLds::ld(a0), x02 = T.te0_kb<2>(q0),
            x01 = T.te2_kb<1>(q0), x00 = T.te2_kb<0>(q0);
  const u32 x13 = T.te0_kb<3>(q1), x12 = T.te0_kb<2>(q1),
            x11 = T.te2_kb<1>(q1), x10 = T.te2_kb<0>(q1);
  const u32 x23 = T.te0_kb<3>(q2), x22 = T.te0_kb<2>(q2),
            x21 = T.te2_kb<1>(q2), x20 = T.te2_kb<0>(q2);
  const u32 x33 = T.te0_kb<3>(q3), x32 = T.te0_kb<2>(q3),
            x31 = T.te2_kb<1>(q3), x30 = T.te2_kb<0>(q3);
  // bit 0 of that byte flips: entry index ^ 1 is address ^ 256
  const u32 x03b = AesLds::ld(a0 ^ 256u);
  __builtin_amdgcn_sched_barrier(0);  // 17 in flight
  // Round 1's key.  Word 3 of the state is the key word k3 (the position
  // byte only enters word 0), so x33..x30 also carry the sbox bytes of the
  // round-1 key schedule (byte 2 of a te0 word, byte 0 of a te2 word).
  // rol8([S(b2) S(b1) S(b0) S(b3)]) = [S(b1) S(b0) S(b3) S(b2)] of k3
  q0 = xor3(aes_sb_pair<3, 2, 0, 0>(x31, x30), aes_sb_pair<1, 0>(x33, x32),
            q0) ^ 0x01u;
  q1 ^= q0; q2 ^= q1; q3 ^= q2;
  u32 s0 = AesLds::mix(x03, x12, x21, x30, q0);
  u32 s1 = AesLds::mix(x13, x22, x31, x00, q1);
  u32 s2 = AesLds::mix(x23, x32, x01, x10, q2);
  u32 s3 = AesLds::mix(x33, x02, x11, x20, q3);
  // the un-rotated te0 term is the one that differs
  u32 u0 = xor3(s0, x03, x03b), u1 = s1, u2 = s2, u3 = s3;
  // Rounds 2..10.  q is rol8 of the key of the round being combined; `kw`,
  // the four sbox lookups of the next key, is issued a round ahead of the
  // combine that needs it, so it has always returned.
  using Words = AesLds::Words;
  u32 q[4] = {q0, q1, q2, q3};
  Words kw = T.key_issue(q[3]);
  auto key_step = [&](bool issue_next) {
    q[0] = AesLds::key(kw, q[0]) ^ rcon;
    rcon = (rcon << 1) ^ ((rcon & 0x80u) ? 0x11bu : 0u);
    rcon &= 0xffu;
    q[1] ^= q[0]; q[2] ^= q[1]; q[3] ^= q[2];
    if (issue_next) kw = T.key_issue(q[3]);
  };
  // Shared round 2: the states still agree in words 1..3 and each output
  // word reads one byte of word 0, so 12 of the 16 lookups are both children's
  // (~27 of ~320 per pair with round 1's): e<j> = te0, te0, te2, te2 of word j
  const Words e1 = T.col_issue(s1, s1, s1, s1),
              e2 = T.col_issue(s2, s2, s2, s2),
              e3 = T.col_issue(s3, s3, s3, s3);
  // is output word i of round r needed at all
  auto need = [](int i, int r) { return !(LOW && r == 10 && i > 0); };
  // start the lookups of output word i of round r from the state x
  auto issue = [&](const u32 (&x)[4], int i, int r) -> Words {
    if (r == 2) {  // only the byte of word 0 is the child's own
      switch (i) {
        case 0: return {T.te0_b<3>(x[0]), e1.b, e2.c, e3.d};
        case 1: return {e1.a, e2.b, e3.c, T.te2_b<0>(x[0])};
        case 2: return {e2.a, e3.b, T.te2_b<1>(x[0]), e1.d};
        default: return {e3.a, T.te0_b<2>(x[0]), e1.c, e2.d};
      }
    }
    const u32 a = x[i], b = x[(i + 1) & 3], c = x[(i + 2) & 3],
              d = x[(i + 3) & 3];
    return r == 10 ? T.last_issue(a, b, c, d) : T.col_issue(a, b, c, d);
  };
  // The lookups form a stream of 72 jobs, one output word each: round 2
  // child a words 0..3, child b words 0..3, round 3 child a ... round 10.
  // A step combines one child's round of four words, issued eight jobs
  // earlier, from l[c] into the state st[c], issues its next round and ends
  // at a scheduling barrier.  The barriers pin the phases, not the order
  // inside one: writing st[c][i] without n[], or looping over (round, child)
  // and i, is the same algebra but reorders a word's ds_read_b32 (tried).
  Words l[2][4];
  u32 st[2][4] = {{s0, s1, s2, s3}, {u0, u1, u2, u3}}, n[2][4];
  u32 out[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
  for (int k = 0; k < 72 + 8; k += 4) {
#pragma unroll
    for (int j = k - 8; j < k - 4; ++j) {
      if (j < 0) continue;
      const int c = (j >> 2) & 1, i = j & 3, r = 2 + (j >> 3);
      if ((j & 7) == 0) key_step(r < 10);  // round r's key
      if (!need(i, r)) continue;
      if (r == 10) {  // comes out as rol8(.)
        out[c][i] = bswap_rol8(AesLds::last(l[c][i], q[i]));
      } else {
        n[c][i] = AesLds::mix(l[c][i], q[i]);
        if (i == 3) {
#pragma unroll
          for (int w = 0; w < 4; ++w) st[c][w] = n[c][w];
        }
      }
    }
#pragma unroll
    for (int j = k; j < k + 4 && j < 72; ++j) {
      const int c = (j >> 2) & 1, i = j & 3, r = 2 + (j >> 3);
      if (need(i, r)) l[c][i] = issue(st[c], i, r);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  ra = make_uint4(out[0][0], out[0][1], out[0][2], out[0][3]);
  rb = make_uint4(out[1][0], out[1][1], out[1][2], out[1][3]);
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
