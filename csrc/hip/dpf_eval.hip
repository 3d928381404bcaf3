// MI355X (gfx950, CDNA4) HIP kernels for DPF expansion + fused PIR lookup.
//
// Design (MI355X-first, not a port — see SURVEY.md §7):
//   * One UNIT of Z = 1<<zlog threads (Z = 256 = 4 wave64 for n >= 512)
//     per (key, DFS segment); a 512-key batch is 2048 units.  A workgroup
//     is one unit, except for AES, where up to four units form one
//     workgroup and share the T-table (eval_units_per_wg).
//   * Phase 1: breadth-first expansion of the GGM root to Z frontier seeds
//     through an LDS ping-pong (zlog levels, ~2Z PRFs — negligible).
//   * Phase 2: each thread owns ONE subtree and walks it with a sibling-
//     stack DFS.  All threads execute the same DFS schedule => zero
//     divergence, and the stack index is wave-uniform per step so LDS
//     accesses are conflict-free b128 ops.  The two HOT stack levels
//     (popped on 3/4 of all steps) live in registers; the cold remainder
//     shares the phase-1 ping-pong LDS region (they are never live at the
//     same time), keeping LDS small enough for 3-4 units per CU.
//   * Each visited interior node expands BOTH children from one parent;
//     for AES this shares one key schedule across the two encryptions
//     (the reference re-expands per call: dpf_gpu/prf/prf.cu:159-184,
//     flagged in its own TODO dpf.py:32-33).
//   * Leaves: only the low 32 bits of a leaf share contribute to the
//     (mod 2^32-truncated) output, because truncation is a ring hom of
//     Z_2^128 -> Z_2^32.  The fused MAC is therefore 16 v_mad_u32 per leaf
//     against u32 table rows — 16x less arithmetic and 4x less table
//     traffic than the reference's mod-2^128 MAC (dpf_hybrid.cu:166-172),
//     with bit-identical output.  Table loads are issued BEFORE the leaf
//     PRFs of the same step, so ~1000 cycles of cipher work hides them.
//   * AES T-table: 256 rows of 256 bytes at LDS byte 0, each holding 32
//     copies of te0[entry] and 32 of te2[entry] = ror16(te0[entry]) (byte
//     entry*256 + half*128 + (lane%32)*4).  A ds_read_b32 is served in two
//     groups of 32 lanes, so inside a group every lane reads its own LDS
//     bank — measured 4.3x bank-conflict amplification with flat tables
//     (SQ_LDS_BANK_CONFLICT 3.5e10 vs SQ_INSTS_LDS 8.1e9, profiles/) — a
//     lookup address is one v_perm_b32 of a state word, and the te2 word
//     is the same address read with the immediate offset:128.  Rotation
//     commutes with xor, so a MixColumns word is
//     xor3(te0, te2, ror8(xor3(te0, te2, rol8(k)))): two v_bitop3_b32 and
//     ONE v_alignbit_b32, and the key schedule runs on rol8(k) throughout.
//     sbox[x] = byte 2 of te0[x], so the table serves the whole cipher.
//   * Table layout: row(idx) = j<<(zlog+1) | t<<1 | b (leaf_perm in
//     csrc/core/dpf_core.cc): at DFS step j the workgroup reads one
//     contiguous 32 KB slab; every lane reads its two rows as 8 contiguous
//     dwordx4 loads.  All workgroups stream the table in the same order
//     => cross-key reuse in L2/LLC.
//   * Wide rows: the fused kernel has a compile-time row width of W 16-word
//     blocks (rows of 16*W <= MAX_FUSED_WORDS u32).  A leaf pair's shares
//     are computed once and MACed into all 16*W columns; the rows are
//     loaded one column block at a time, the first before the leaf cipher
//     and each further one ahead of the previous block's MACs.
//
// This file holds the production DFS kernel and its launchers.  The device
// PRFs are in prf_device.h; the naive / BFS / cooperative strategies in
// dpf_strategies.hip; the speed-of-light and unit-test probes in
// dpf_probes.hip.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <stdexcept>

#include "dpf_hip_api.h"
#include "hip_util.h"
#include "prf_device.h"

namespace gpudpf_hip {

GrowScratch g_eval_scratch;

// DFS sibling-stack levels kept in LDS (deeper levels: registers;
// shallower: global scratch)
constexpr int MAX_LDS_LEVELS = 4;
// Most (key, segment) units one AES workgroup walks (they share the table)
constexpr int AES_MAX_UNITS = 4;
// The same for rows wider than 16 words.  The K = 4 kernel lives in 128
// VGPRs and uses 124 of them at 16 words, so it has no room for the 16*W
// accumulators of a wide row; at K <= 2 a workgroup is at most 8 waves and
// a wave may take 256.
constexpr int AES_MAX_UNITS_WIDE = 2;
// The same for packed keys (LANES = 4 below).  Their fused kernel keeps two
// lane blocks of row data (64 VGPRs) and eight shares beside the cipher: in
// the 128 VGPRs of K = 4 it spills (44 bytes of scratch per lane), at K = 3
// a wave may take 168 and it uses 139.  Packed rows wider than 16 words are
// wide first: K <= AES_MAX_UNITS_WIDE.
constexpr int AES_MAX_UNITS_PACKED = 3;
// Widest table row (u32) the fused kernel serves: W <= 4 column blocks
constexpr int MAX_FUSED_WORDS = gpudpf::kMaxFusedWords;

// Runtime row width -> compile-time column-block count W: calls
// f(std::integral_constant<int, W>{}) for rows of 16*W words, as with_prf
// does for the PRF.  The only statement of the widths the kernel serves.
template <class F>
void with_row_blocks(int entry_words, F&& f) {
  static_assert(MAX_FUSED_WORDS == 64, "one case per 16-word block");
  switch (entry_words) {
    case 16: f(std::integral_constant<int, 1>{}); break;
    case 32: f(std::integral_constant<int, 2>{}); break;
    case 48: f(std::integral_constant<int, 3>{}); break;
    case 64: f(std::integral_constant<int, 4>{}); break;
    default:
      throw std::invalid_argument("entry_words must be 16, 32, 48 or 64");
  }
}
inline void check_entry_words(int entry_words) {
  with_row_blocks(entry_words, [](auto) {});
}

// Geometry of one eval launch, the single statement of where every
// sibling-stack level lives and how large the LDS and scratch slices are.
// The kernel (indexing), the launcher (dynamic LDS size, scratch size) and
// eval_scratch_bytes all read it.
//
// Sibling-stack placement by pop frequency (level d pops once per
// 2^(DS-1-d) pairs): deepest two levels in registers, the next
// MAX_LDS_LEVELS in LDS, the shallow remainder in global scratch
// (touched <= 1/64 of steps) — keeping the per-unit LDS slice small
// enough that four units fit beside the 64 KB AES table.
struct EvalGeom {
  int Z;            // threads per unit
  int DS;           // subtree splits per thread (>= 1)
  int lds_levels;   // stack levels [lds_base, DS-3] live in LDS
  int lds_base;
  int glob_levels;  // stack levels [1, lds_base-1] live in global scratch
  int shared_u4;    // uint4s of the ping-pong / LDS-stack region of a unit
  int unit_u32;     // u32s of one unit's LDS slice: cw | shared | red

  // W: 16-word column blocks of a table row (1 for the expand kernel).
  // Only the reduction slice depends on it; the scratch does not.
  __host__ __device__ EvalGeom(int depth, int zlog, int W)
      : Z(1 << zlog),
        DS(depth - zlog),
        lds_levels(DS > 3 ? (DS - 3 < MAX_LDS_LEVELS ? DS - 3 : MAX_LDS_LEVELS)
                          : 0),
        lds_base(DS - 2 - lds_levels),
        // max(difference, 0), spelt so: from this form the compiler knows
        // the 64-bit scratch row offset has a non-negative factor
        glob_levels((DS - 3) - lds_levels > 0 ? (DS - 3) - lds_levels : 0),
        shared_u4(Z * (lds_levels > 2 ? lds_levels : 2)),
        unit_u32((2 * kCwPerSel + shared_u4) * 4 + (Z >> 6) * 16 * W) {}

  // Dynamic LDS bytes of a workgroup of K units: the replicated AES table
  // in front of the unit slices.  Largest: AES, K = 4, W = 1 at 137 KiB
  // (wide AES, K = 2, W = 4, packed or not: 102 KiB; packed K = 3: 119 KiB),
  // within the CU's 160 KiB.
  std::size_t lds_bytes(int prf, int K) const {
    return ((std::size_t)aes_lds_u32(prf) + (std::size_t)K * unit_u32) * 4;
  }
  // uint4s of global sibling-stack scratch in front of unit `unit`'s rows:
  // one Z-wide row per unit and global level (units index it, so it does
  // not depend on how units are grouped into workgroups)
  __host__ __device__ std::size_t scratch_u4(int unit) const {
    return (std::size_t)unit * glob_levels * Z;
  }
  // Scratch bytes a launch of n_units touches
  std::size_t scratch_bytes(int n_units) const {
    return scratch_u4(n_units) * sizeof(uint4);
  }
};

template <int PRF>
__device__ __forceinline__ void expand_pair(uint4 seed, int i,
                                            const uint4* cw_lds,
                                            const AesLds& T, uint4& c0,
                                            uint4& c1) {
  // Issue the correction-word reads BEFORE the PRF core: their address
  // depends only on the seed parity, and the ~600-instruction cipher
  // hides the LDS latency (left to itself the scheduler sinks them to
  // +5 instructions before their wait — measured in the .s).
  const int sel = (int)(seed.x & 1u);
  uint4 cw0 = cw_lds[sel * kCwPerSel + i * 2 + 0];
  uint4 cw1 = cw_lds[sel * kCwPerSel + i * 2 + 1];
  uint4 p0, p1;
  prf_pair<PRF>(seed, T, p0, p1);
  c0 = add128(p0, cw0);
  c1 = add128(p1, cw1);
}

// ---------------------------------------------------------------------------
// Main kernel.  A UNIT is Z threads walking one (key, segment) pair; a
// workgroup holds K units (K = 1 except for AES, where the K units share
// one 64 KiB te0/te2 table so the table does not cost occupancy).  Dynamic LDS
// map (the kernel has no static LDS, so it starts at LDS byte 0):
//   [aes: 0/16384 u32] then K unit slices of
//   [cw: 128 uint4][shared: Z*max(2, min(DS-3, 4)) uint4][red: Z/64*16*W u32]
// The `shared` region is the phase-1 ping-pong (2*Z uint4) first, then the
// cold DFS stack (LDS levels) — never live simultaneously.
// Hot stack levels DS-1 / DS-2 are the registers rtop1 / rtop2.
//
// Multi-unit indexing: unit = blockIdx.x*K + threadIdx.x/Z, t = threadIdx.x
// % Z.  Z is a multiple of 64, so a wave never straddles units and every
// per-unit branch is wave-uniform.  Units never communicate: key, segment,
// scratch row, cw/stack/red slices all index by unit, and partial sums
// meet only in the wrapping atomics.  The workgroup barriers (staging,
// the zlog phase-1 levels, the reduction) have trip counts that depend on
// kernel arguments only; surplus units of the last workgroup (unit >=
// n_units) join them but load no key or table data, write no scratch and
// issue no atomics.
// ---------------------------------------------------------------------------
// slog: log2 of the DFS range split — each key's 2^(DS-1) leaf pairs are
// divided over 2^slog units (j-split).  The split changes neither the
// table layout nor the per-thread subtree assignment: unit (key, seg)
// walks pairs [seg*P, (seg+1)*P) of every thread's subtree, paying one
// extra targeted descent (DS-1 pair expansions) to enter at seg*P.  Fused
// partials combine with wrapping u32 atomicAdd (exact mod 2^32).  This is
// what fills 256 CUs at small batch (batch 512 alone = only 2 units/CU) and
// doubles as the single-key low-latency mode (the reference needs a
// separate cooperative-groups kernel for that: dpf_coop.cu).
//
// BINNED (batch PIR): `table` is num_bins consecutive blocks of n rows, each
// in leaf_perm(n, zlog) order, and key i walks block bins[i].  Only the row
// base differs; the id is loaded once per unit and made scalar, so the base
// stays in SGPRs and the per-step row address stays scalar base + vector
// offset.  n is then the rows of ONE block.  The ids (int32 [batch], each in
// [0, num_bins)) arrive as an argument pack that is empty for the unbinned
// instantiations: an argument of any type, even an empty struct, would move
// their hidden kernel arguments and change their code.
//
// W (FUSED only): table rows and `out` rows are 16*W u32.  Row stride,
// bin-block stride, accumulators, reduction slice and atomics scale with
// it; phase 1, the descent, the stacks and the scratch do not.  Per step
// the leaf pair's (v0, v1) is computed once and MACed into all 16*W
// columns.  The two rows are loaded in 16-word column blocks (4 dwordx4 per
// row): block 0 before the leaf cipher, which hides it, and block c+1 just
// ahead of block c's 32 MACs, so at most two blocks (64 VGPRs) of row data
// are in flight beside the 16*W accumulators, not all 8*W loads.
//
// LANES = 4 (packed keys, dpf_core.h): `depth` is the tree depth D over the
// n / 4 nodes, and only the leaf step differs.  The leaf pair's full 128-bit
// PRF outputs give 8 shares, v0[c] / v1[c] = word c of the leaf + word c of
// its level-0 correction word (four u32 adds, no carries).  The table is in
// packed_perm order, row = j << (zlog+3) | t << 3 | b << 2 | c: a thread's 8
// rows are consecutive, and LANE BLOCK c (row c of both leaves, 8 dwordx4) is
// column block c of a leaf's 64-word "row" in the wide-row picture above.
// So the blocks are loaded exactly as there, block 0 before the cipher and
// block c+1 ahead of block c's MACs; what differs is that every block MACs
// into the SAME 16 accumulators with its own pair of shares.  The expand
// kernel stores the 8 shares in that row order as two 16-byte stores (`out`
// must be 16-byte aligned); it is W = 1 and unbinned.  `n` stays the row
// count of the table, 4 << depth.
//
// LANES = 4 with bins (FUSED only; the packed binned launcher) also takes
// W = 1..4.  A bin block is n = 4 << depth rows of ROW = 16*W words in
// packed_perm order, based at table + bin * n * ROW as above.  A thread's 8
// rows are still consecutive, now 8*ROW words; within them leaf b, lane c,
// column block cb, quad q is uint4 4*(b*RB + c*W + cb) + q with RB = 4*W, so
// block k = c*W + cb is loaded by the same load_block(k), in the same double
// buffer (block 0 before the cipher, block k+1 ahead of block k's MACs, its
// address tied to the eight shares for k = 0 and to four sums of block k-1's
// accumulator group after that).  Block k MACs the shares of lane k / W into
// the 16 sums of column block k % W.  Unbinned packed kernels stay W = 1:
// nothing reaches a wide one.
__device__ __forceinline__ const int* bin_ids(const int* ids) { return ids; }

template <int PRF, bool FUSED, int K, int W, int LANES, class... Bins>
__global__ __launch_bounds__(256 * K) void dpf_eval_kernel(
    const int* __restrict__ keys, const u32* __restrict__ table,
    u32* __restrict__ out, const u32* __restrict__ aes_tabs,
    uint4* __restrict__ scratch, int depth, int zlog, int slog, int n_units,
    long long n, Bins... bins) {
  constexpr bool BINNED = sizeof...(Bins) == 1;
  static_assert(BINNED ? FUSED : sizeof...(Bins) == 0, "bins: one const int*");
  static_assert(W >= 1 && 16 * W <= MAX_FUSED_WORDS && (FUSED || W == 1),
                "rows of 16*W words, wide only when fused");
  static_assert(W == 1 || K <= AES_MAX_UNITS_WIDE, "wide rows: K <= 2");
  static_assert(LANES == 1 || (LANES == 4 && (BINNED || W == 1)),
                "packed: four lanes; bins and wide rows only together");
  constexpr int ROW = 16 * W;  // u32 per table row and per out row
  // 16-word blocks loaded per leaf and step, and the u32 between the two
  // leaves' first blocks: the row's column blocks, or those of a node's four
  // lane rows (block k = lane * W + column block)
  constexpr int RB = LANES == 4 ? LANES * W : W;
  constexpr int LEAF = 16 * RB;
  extern __shared__ u32 smem[];
  const EvalGeom g(depth, zlog, W);
  const int Z = g.Z, DS = g.DS, lds_base = g.lds_base;
  const int t = (int)threadIdx.x & (Z - 1);
  const int u_local = K == 1 ? 0 : (int)threadIdx.x >> zlog;
  const int unit = (int)blockIdx.x * K + u_local;
  const bool active = unit < n_units;  // wave-uniform (Z % 64 == 0)
  const int key_id = unit >> slog;
  const int seg = unit & ((1 << slog) - 1);
  const long long key_base = (long long)key_id * kKeyInts;

  u32* unit_lds = smem + aes_lds_u32(PRF) + u_local * g.unit_u32;
  uint4* cw_lds = reinterpret_cast<uint4*>(unit_lds);  // 2 * kCwPerSel entries
  uint4* shared_region = cw_lds + 2 * kCwPerSel;
  u32* red = reinterpret_cast<u32*>(shared_region + g.shared_u4);
  uint4* gstack = scratch + g.scratch_u4(unit);

  // Stage codewords per unit; the AES te0/te2 table once per workgroup.
  if (active) {
    for (int idx = t; idx < 2 * kCwPerSel; idx += Z)
      cw_lds[idx] =
          reinterpret_cast<const uint4*>(keys + key_base + kKeyCwInt)[idx];
  }
  aes_stage_table<PRF>(smem, aes_tabs);
  const AesLds T = AesLds::lane();
  uint4* pp = shared_region;
  if (active && t == 0) pp[0] = key_root(keys + key_base);
  __syncthreads();

  // Phase 1: root -> Z frontier seeds (frontier position t has the
  // first-consumed index bit as its MSB: t = bitrev(idx & (Z-1))).
  uint4* a = pp;
  uint4* b = pp + Z;
  for (int l = 1; l <= zlog; ++l) {
    const int i = depth - l;
    if (active && t < (1 << l)) {
      uint4 parent = a[t >> 1];
      uint4 v = prf_full<PRF>(parent, (u32)(t & 1), T);
      const int sel = (int)(parent.x & 1u);
      b[t] = add128(v, cw_lds[sel * kCwPerSel + i * 2 + (t & 1)]);
    }
    __syncthreads();
    uint4* tmp = a;
    a = b;
    b = tmp;
  }
  uint4 cur = a[t];
  __syncthreads();  // everyone holds their frontier seed; pp is now free
  uint4* stack = shared_region;  // LDS stack levels [lds_base, DS-3]

  u32 acc[ROW];
#pragma unroll
  for (int w = 0; w < ROW; ++w) acc[w] = 0;

  if (active) {
    // Targeted descent to leaf-pair j_lo: at split d take bit (DS-1-d) of
    // j_lo, always recording the bit-1 child in the level's sibling slot
    // (when the bit is 1 the slot is stale, but it is provably rewritten by
    // a later descent before its next pop).
    const long long pairs = 1LL << (DS - 1);
    const long long j_lo = (long long)seg * (pairs >> slog);
    const long long j_hi = j_lo + (pairs >> slog);
    uint4 rtop1 = cur, rtop2 = cur;  // hot levels DS-1 / DS-2
    for (int d = 1; d <= DS - 1; ++d) {
      uint4 c0, c1;
      expand_pair<PRF>(cur, DS - d, cw_lds, T, c0, c1);
      if (d == DS - 1) rtop1 = c1;
      else if (d == DS - 2) rtop2 = c1;
      else if (d >= lds_base) stack[(d - lds_base) * Z + t] = c1;
      else gstack[(size_t)(d - 1) * Z + t] = c1;
      cur = ((j_lo >> (DS - 1 - d)) & 1) ? c1 : c0;
    }

    // leaf-level correction words (eval level 0) are read every iteration:
    // hoist their low words into registers.  For AES, whose K = 4 kernel
    // has 128 VGPRs to live in, into scalar ones: the values are the same
    // for the whole unit, hence for the wave.
    auto uni = [](u32 v) -> u32 {
      if constexpr (PRF == PRF_AES128) return __builtin_amdgcn_readfirstlane(v);
      else return v;
    };
    const u32 cwl[2][2] = {{uni(cw_lds[0].x), uni(cw_lds[1].x)},
                           {uni(cw_lds[kCwPerSel].x),
                            uni(cw_lds[kCwPerSel + 1].x)}};
    // packed: all four words of each, 16 u32
    uint4 cw4[2][2] = {};
    if constexpr (LANES == 4) {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const uint4 v = cw_lds[s * kCwPerSel + b];
          cw4[s][b] = make_uint4(uni(v.x), uni(v.y), uni(v.z), uni(v.w));
        }
    }

    // The unit's bin block.  key_id is the same for the whole unit, hence
    // for the wave (Z % 64 == 0), which the compiler cannot see for K > 1.
    // Surplus units never get here, so they never read bins.
    if constexpr (BINNED) {
      const u32 bin = __builtin_amdgcn_readfirstlane(
          (u32)bin_ids(bins...)[key_id]);
      table += (unsigned long long)bin * (unsigned long long)n *
               (unsigned long long)ROW;
    }

    for (long long j = j_lo; j < j_hi; ++j) {
      // Issue the first column block of the two table rows first: the
      // leaf ciphers below hide its latency.  rq[cb & 1][b] holds column
      // block cb of row b.
      uint4 rq[2][2][4];
      const uint4* rows = nullptr;
      auto load_block = [&](int cb) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          rq[cb & 1][0][q] = rows[4 * cb + q];
          rq[cb & 1][1][q] = rows[4 * (RB + cb) + q];
        }
      };
      if constexpr (FUSED) {
        rows = reinterpret_cast<const uint4*>(
            table + ((j << (zlog + 1)) + ((long long)t << 1)) * LEAF);
        load_block(0);
      }

      // The leaf pair's shares: v0 / v1, or at LANES = 4 word c of them in
      // v0l[c] / v1l[c]
      u32 v0, v1, v0l[LANES], v1l[LANES];
      if constexpr (LANES == 1) {
        u32 p0, p1;
        prf_pair_low<PRF>(cur, T, p0, p1);
        const int sel = (int)(cur.x & 1u);
        v0 = p0 + cwl[sel][0];
        v1 = p1 + cwl[sel][1];
      } else {
        uint4 p0, p1;
        const bool sel = (cur.x & 1u) != 0;
        prf_pair<PRF>(cur, T, p0, p1);
        const uint4 c0 = sel ? cw4[1][0] : cw4[0][0];
        const uint4 c1 = sel ? cw4[1][1] : cw4[0][1];
        v0l[0] = p0.x + c0.x; v0l[1] = p0.y + c0.y;
        v0l[2] = p0.z + c0.z; v0l[3] = p0.w + c0.w;
        v1l[0] = p1.x + c1.x; v1l[1] = p1.y + c1.y;
        v1l[2] = p1.z + c1.z; v1l[3] = p1.w + c1.w;
      }

      if constexpr (FUSED) {
#pragma unroll
        for (int cb = 0; cb < RB; ++cb) {
          // a column block has its own sums; the lane blocks share theirs
          u32* acc_c = acc + 16 * (LANES == 1 ? cb : cb % W);
          if constexpr (LANES == 4) {
            v0 = v0l[cb / W];
            v1 = v1l[cb / W];
            if (cb + 1 < RB) {
              // As for wide rows below: lane block cb+1 is in flight during
              // block cb's MACs and no sooner (all 32 loads ahead of the
              // cipher are 128 VGPRs of row data).
              int tt = t;
              if (cb == 0)
                asm volatile("" : "+v"(tt)
                             : "v"(v0l[0]), "v"(v0l[1]), "v"(v0l[2]),
                               "v"(v0l[3]), "v"(v1l[0]), "v"(v1l[1]),
                               "v"(v1l[2]), "v"(v1l[3]));
              else  // the sums block cb-1 has just added to
                asm volatile("" : "+v"(tt)
                             : "v"(acc[16 * ((cb - 1) % W) + 3]),
                               "v"(acc[16 * ((cb - 1) % W) + 7]),
                               "v"(acc[16 * ((cb - 1) % W) + 11]),
                               "v"(acc[16 * ((cb - 1) % W) + 15]));
              rows = reinterpret_cast<const uint4*>(
                  table + ((j << (zlog + 1)) + ((long long)tt << 1)) * LEAF);
              load_block(cb + 1);
            }
          }
          if constexpr (LANES == 1 && W > 1) if (cb + 1 < W) {
            // Block cb+1 is in flight during block cb's MACs and no sooner.
            // Left alone the compiler issues all 8*W loads ahead of the
            // cipher (128 VGPRs of row data at W = 4, which spills the AES
            // K = 2 kernel), so the address of a further block is made to
            // depend on what frees its registers: the leaf shares for
            // block 1, the sums of block cb-1 after that.  The statement
            // emits no instruction.
            int tt = t;
            if (cb == 0)
              asm volatile("" : "+v"(tt) : "v"(v0), "v"(v1));
            else
              asm volatile("" : "+v"(tt)
                           : "v"(acc_c[-13]), "v"(acc_c[-9]), "v"(acc_c[-5]),
                             "v"(acc_c[-1]));
            rows = reinterpret_cast<const uint4*>(
                table + ((j << (zlog + 1)) + ((long long)tt << 1)) * ROW);
            load_block(cb + 1);
          }
          const uint4* r0q = rq[cb & 1][0];
          const uint4* r1q = rq[cb & 1][1];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            acc_c[4 * q + 0] += v0 * r0q[q].x + v1 * r1q[q].x;
            acc_c[4 * q + 1] += v0 * r0q[q].y + v1 * r1q[q].y;
            acc_c[4 * q + 2] += v0 * r0q[q].z + v1 * r1q[q].z;
            acc_c[4 * q + 3] += v0 * r0q[q].w + v1 * r1q[q].w;
          }
          // Left alone the compiler sinks these MACs below the pop-and-
          // descend loop, so a block of row data (32 VGPRs) stays live
          // through the pair expansions.  The AES cipher needs those
          // registers for its lookups in flight (with them K = 4 spills),
          // so the sums are made to exist here.  The statement emits no
          // instruction.  Wide packed rows need it for every PRF: without it
          // each block's row data follows the sunk MACs and the stream
          // ciphers spill (docs/KERNEL_NOTES.md, "Packed bins").
          if constexpr (PRF == PRF_AES128 || (LANES == 4 && W > 1)) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
              asm volatile("" : "+v"(acc_c[4 * q]), "+v"(acc_c[4 * q + 1]),
                                "+v"(acc_c[4 * q + 2]), "+v"(acc_c[4 * q + 3]));
          }
        }
      } else {
        u32* orow = out + (u64)key_id * (u64)n +
                    (u64)((j << (zlog + 1)) + ((long long)t << 1)) * LANES;
        if constexpr (LANES == 1) {
          orow[0] = v0;
          orow[1] = v1;
        } else {
          uint4* o4 = reinterpret_cast<uint4*>(orow);
          o4[0] = make_uint4(v0l[0], v0l[1], v0l[2], v0l[3]);
          o4[1] = make_uint4(v1l[0], v1l[1], v1l[2], v1l[3]);
        }
      }

      if (j + 1 == j_hi) break;
      // Pop the deepest pending sibling (register-resident on 3/4 of steps)
      // and descend its bit-0 spine.
      const int c = (int)(__ffsll((unsigned long long)(j + 1)) - 1);
      if (c == 0) {
        cur = rtop1;
        continue;  // next leaf-parent is the sibling itself
      }
      const int dpop = DS - 1 - c;
      cur = (c == 1) ? rtop2
            : (dpop >= lds_base) ? stack[(dpop - lds_base) * Z + t]
                                 : gstack[(size_t)(dpop - 1) * Z + t];
      for (int d = dpop + 1; d <= DS - 1; ++d) {
        uint4 c0, c1;
        expand_pair<PRF>(cur, DS - d, cw_lds, T, c0, c1);
        if (d == DS - 1) rtop1 = c1;
        else if (d == DS - 2) rtop2 = c1;
        else if (d >= lds_base) stack[(d - lds_base) * Z + t] = c1;
        else gstack[(size_t)(d - 1) * Z + t] = c1;
        cur = c0;
      }
    }
  }

  if constexpr (FUSED) {
    // Wave shfl reduction, then cross-wave sum through LDS.
#pragma unroll
    for (int w = 0; w < ROW; ++w) {
      u32 v = acc[w];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      acc[w] = v;
    }
    // (per unit: wave = the unit's own wave index, red = its own slice)
    const int lane = t & 63, wave = t >> 6, nwaves = Z >> 6;
    if (lane == 0) {
#pragma unroll
      for (int w = 0; w < ROW; ++w) red[wave * ROW + w] = acc[w];
    }
    __syncthreads();
    if (active && t < ROW) {  // ROW <= 64 <= Z: one thread per column
      u32 s = 0;
      for (int wv = 0; wv < nwaves; ++wv) s += red[wv * ROW + t];
      // Wrapping u32 atomic add combines the 2^slog segment partials
      // exactly (mod 2^32); `out` is zeroed by the caller.
      atomicAdd(&out[(u64)key_id * ROW + t], s);
    }
  }
}

// ---------------------------------------------------------------------------
// Host launchers
// ---------------------------------------------------------------------------
namespace {

// j-split: grow the launch to >= 1024 units (4 per CU) so small
// batches still fill the chip; each extra split costs one targeted
// descent (DS-1 pair expansions) per unit — negligible against
// pairs/2^slog leaf pairs.
int slog_for(int batch, int DS) {
  int slog = 0;
  while ((batch << (slog + 1)) <= 2048 && slog + 2 <= DS - 1 && slog < 8)
    ++slog;
  return slog;
}

}  // namespace

// Units per workgroup (the kernel's K).  Only AES holds a table the units
// of a workgroup can share, so every other PRF runs K = 1.  With the
// 64 KiB table one AES workgroup is resident per CU whatever K is, so a
// launch takes ceil(workgroups / CUs) rounds of K units each.  A round gets
// cheaper per unit as K adds waves per SIMD, but not in proportion:
// measured at n = 2^20, batch 512 on MI355X (profiles/PROFILING.md) a
// round of 1/2/3/4 units took 3.6/4.6/5.2/7.5 ms (2.9/3.7/4.5/6.4 ms since
// the te0/te2 table rows: nearly the same ratios, so round_cost keeps the
// first set and no choice changes; 2.4/3.5/4.3/6.1 ms with the batched
// cipher, which would move only 6913..7168 units from K = 3 to K = 4, for
// 1.6% of that launch).  Take the K with the
// cheapest rounds x cost, the smallest on ties: 2048 units -> K = 4 (2
// rounds on 256 CUs); 1200 units -> K = 3; a single key's 256 segments ->
// K = 1 (one unit on every CU).  GPUDPF_AES_UNITS=1..4 forces K, for A/B
// runs and so that the tests reach every K; it is read at each launch (one
// getenv) so a single process can compare them.  Public (dpf_hip_api.h) so
// the tests can assert which K a launch took.
//
// The round costs are measured for 16-word rows only.  Rows wider than that
// allow K <= AES_MAX_UNITS_WIDE; nobody has measured their rounds, so they
// take the largest K allowed, and a forced K is clamped to it.
//
// Packed launches (lanes = 4) allow K <= AES_MAX_UNITS_PACKED, the largest K
// whose gfx950 code has no scratch.  Their round costs are not measured
// either: they take that K, and a forced K is clamped to it.
//
// Wide packed launches (the packed binned kernel at 32..64 words) are wide
// first: K <= AES_MAX_UNITS_WIDE, unmeasured, so that K.
namespace {

// The one statement of K, for any (entry_words, lanes) a kernel exists for;
// the public queries below and launch_eval_t read it.
int units_per_wg(int prf, int n_units, int entry_words, int lanes) {
  if (prf != PRF_AES128) return 1;
  const int kmax = entry_words > 16 ? AES_MAX_UNITS_WIDE
                   : lanes == 4     ? AES_MAX_UNITS_PACKED : AES_MAX_UNITS;
  if (const char* e = std::getenv("GPUDPF_AES_UNITS")) {
    const int v = std::atoi(e);
    if (v >= 1 && v <= AES_MAX_UNITS) return v < kmax ? v : kmax;
  }
  if (entry_words > 16 || lanes == 4) return kmax;
  int dev = 0, cus = 0;
  HIP_CHECK(hipGetDevice(&dev));
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                                  dev));
  if (cus < 1) cus = 1;
  static const int round_cost[AES_MAX_UNITS + 1] = {0, 36, 46, 52, 75};
  int best = 1;
  long best_cost = 0;
  for (int k = 1; k <= AES_MAX_UNITS; ++k) {
    const long wgs = (n_units + k - 1) / k;
    const long cost = ((wgs + cus - 1) / cus) * round_cost[k];
    if (k == 1 || cost < best_cost) {
      best = k;
      best_cost = cost;
    }
  }
  return best;
}

}  // namespace

// Speaks for plain launches and, with lanes = 4, for 16-word packed ones
// (launch_fused_packed, launch_expand_packed) only; the packed binned
// launcher's widths are eval_units_per_wg_packed's.
int eval_units_per_wg(int prf, int n_units, int entry_words, int lanes) {
  check_entry_words(entry_words);
  if (lanes != 1 && (lanes != 4 || entry_words != 16))
    throw std::invalid_argument("lanes must be 1, or 4 with 16-word rows");
  return units_per_wg(prf, n_units, entry_words, lanes);
}

int eval_units_per_wg_packed(int prf, int n_units, int entry_words) {
  check_entry_words(entry_words);
  return units_per_wg(prf, n_units, entry_words, /*lanes=*/4);
}

namespace {

// bins: nothing, or the binned kernel's device id array
template <int PRF, bool FUSED, int W, int LANES, class... Bins>
void launch_eval_t(const int* keys, const u32* table, u32* out,
                   const u32* aes_tabs, int batch, long long n, int depth,
                   int zlog, hipStream_t stream, uint4* own_scratch,
                   size_t own_scratch_bytes, Bins... bins) {
  const EvalGeom g(depth, zlog, W);
  const int slog = slog_for(batch, g.DS);
  const int n_units = batch << slog;
  const int K = units_per_wg(PRF, n_units, 16 * W, LANES);
  const size_t shmem = g.lds_bytes(PRF, K);
  if (shmem > 160 * 1024)
    throw std::invalid_argument("eval launch needs more LDS than a CU has");
  auto kern = dpf_eval_kernel<PRF, FUSED, 1, W, LANES, Bins...>;
  if constexpr (PRF == PRF_AES128) {
    constexpr int KMAX = W > 1        ? AES_MAX_UNITS_WIDE
                         : LANES == 4 ? AES_MAX_UNITS_PACKED : AES_MAX_UNITS;
    if (K == 2) kern = dpf_eval_kernel<PRF, FUSED, 2, W, LANES, Bins...>;
    if constexpr (KMAX >= 3)
      if (K == 3) kern = dpf_eval_kernel<PRF, FUSED, 3, W, LANES, Bins...>;
    if constexpr (KMAX >= 4)
      if (K == 4) kern = dpf_eval_kernel<PRF, FUSED, 4, W, LANES, Bins...>;
  }
  allow_large_lds((const void*)kern, shmem);
  // Caller-owned scratch (launches that may overlap on different streams
  // each bring their own: units with equal index in two kernels in flight
  // would overwrite each other's sibling stacks) or the shared per-device
  // buffer.
  const size_t need = g.scratch_bytes(n_units);
  uint4* scratch;
  if (own_scratch) {
    if (own_scratch_bytes < need)
      throw std::invalid_argument("scratch buffer smaller than "
                                  "eval_scratch_bytes(batch, depth, zlog)");
    scratch = own_scratch;
  } else {
    scratch = static_cast<uint4*>(g_eval_scratch.get(need));
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)((n_units + K - 1) / K)),
                     dim3((unsigned)(K * g.Z)), shmem, stream, keys, table,
                     out, aes_tabs, scratch, depth, zlog, slog, n_units, n,
                     bins...);
  HIP_CHECK(hipGetLastError());
}

template <bool FUSED, class... Bins>
void launch_eval_dispatch(std::uintptr_t keys, std::uintptr_t table,
                          std::uintptr_t out, std::uintptr_t aes_tabs,
                          int batch, long long n, int depth, int zlog, int prf,
                          std::uintptr_t stream, std::uintptr_t scratch,
                          std::size_t scratch_bytes, int entry_words,
                          Bins... bins) {
  check_entry_words(entry_words);
  if (batch <= 0) return;
  check_domain(depth, n);
  if (zlog < 6 || zlog >= depth)
    throw std::invalid_argument("zlog must be in [6, depth)");
  with_prf(prf, [&](auto P) {
    auto launch = [&](auto Wc) {
      launch_eval_t<decltype(P)::value, FUSED, decltype(Wc)::value, 1>(
          as_ptr<const int>(keys), as_ptr<const u32>(table), as_ptr<u32>(out),
          as_ptr<const u32>(aes_tabs), batch, n, depth, zlog,
          as_stream(stream), as_ptr<uint4>(scratch), scratch_bytes, bins...);
    };
    // only the fused kernel has wide instantiations
    if constexpr (FUSED) with_row_blocks(entry_words, launch);
    else launch(std::integral_constant<int, 1>{});
  });
}

// Packed launches: 16-word rows, no bins; depth is the tree depth D
template <bool FUSED>
void launch_packed_dispatch(std::uintptr_t keys, std::uintptr_t table,
                            std::uintptr_t out, std::uintptr_t aes_tabs,
                            int batch, long long n, int depth, int zlog,
                            int prf, std::uintptr_t stream,
                            std::uintptr_t scratch, std::size_t scratch_bytes) {
  // a unit is 64..256 threads with at least one leaf pair each
  if (depth < 7 || depth > gpudpf::kMaxDepth)
    throw std::invalid_argument("packed: tree depth must be in [7, 32]");
  if (n != (long long)4 << depth)
    throw std::invalid_argument("packed: n must be 4 << depth");
  if (zlog < 6 || zlog >= depth)
    throw std::invalid_argument("zlog must be in [6, depth)");
  if (batch <= 0) return;
  if (out % 16 != 0)
    throw std::invalid_argument("packed: out must be 16-byte aligned");
  with_prf(prf, [&](auto P) {
    launch_eval_t<decltype(P)::value, FUSED, 1, 4>(
        as_ptr<const int>(keys), as_ptr<const u32>(table), as_ptr<u32>(out),
        as_ptr<const u32>(aes_tabs), batch, n, depth, zlog, as_stream(stream),
        as_ptr<uint4>(scratch), scratch_bytes);
  });
}

}  // namespace

void launch_fused_packed(std::uintptr_t keys, std::uintptr_t table,
                         std::uintptr_t out, std::uintptr_t aes_tabs, int batch,
                         long long n, int depth, int zlog, int prf,
                         std::uintptr_t stream, std::uintptr_t scratch,
                         std::size_t scratch_bytes) {
  launch_packed_dispatch<true>(keys, table, out, aes_tabs, batch, n, depth,
                               zlog, prf, stream, scratch, scratch_bytes);
}

void launch_fused_packed_binned(std::uintptr_t keys, std::uintptr_t table,
                                std::uintptr_t bins, std::uintptr_t out,
                                std::uintptr_t aes_tabs, int batch,
                                long long n, int depth, int zlog,
                                long long num_bins, int prf,
                                std::uintptr_t stream, std::uintptr_t scratch,
                                std::size_t scratch_bytes, int entry_words) {
  check_entry_words(entry_words);
  if (depth < 7 || depth > gpudpf::kMaxDepth)
    throw std::invalid_argument("packed: tree depth must be in [7, 32]");
  if (n != (long long)4 << depth)
    throw std::invalid_argument("packed: n must be 4 << depth");
  if (zlog < 6 || zlog >= depth)
    throw std::invalid_argument("zlog must be in [6, depth)");
  if (num_bins < 1) throw std::invalid_argument("num_bins must be >= 1");
  const std::size_t row_bytes = 4 * (std::size_t)entry_words;
  if (num_bins > (long long)(SIZE_MAX / row_bytes) / n)
    throw std::invalid_argument("num_bins * n * row bytes overflows");
  if (batch > 0 && bins == 0)
    throw std::invalid_argument("bins must be a device pointer");
  if (out % 16 != 0)
    throw std::invalid_argument("packed: out must be 16-byte aligned");
  if (batch <= 0) return;
  // here, not only in launch_eval_t: AES raises its LDS limit (a HIP call)
  // before it gets there
  if (scratch && scratch_bytes < eval_scratch_bytes(batch, depth, zlog))
    throw std::invalid_argument("scratch buffer smaller than "
                                "eval_scratch_bytes(batch, depth, zlog)");
  with_prf(prf, [&](auto P) {
    with_row_blocks(entry_words, [&](auto Wc) {
      launch_eval_t<decltype(P)::value, true, decltype(Wc)::value, 4>(
          as_ptr<const int>(keys), as_ptr<const u32>(table), as_ptr<u32>(out),
          as_ptr<const u32>(aes_tabs), batch, n, depth, zlog,
          as_stream(stream), as_ptr<uint4>(scratch), scratch_bytes,
          as_ptr<const int>(bins));
    });
  });
}

void launch_expand_packed(std::uintptr_t keys, std::uintptr_t out,
                          std::uintptr_t aes_tabs, int batch, long long n,
                          int depth, int zlog, int prf, std::uintptr_t stream,
                          std::uintptr_t scratch, std::size_t scratch_bytes) {
  launch_packed_dispatch<false>(keys, /*table=*/0, out, aes_tabs, batch, n,
                                depth, zlog, prf, stream, scratch,
                                scratch_bytes);
}

void launch_fused(std::uintptr_t keys, std::uintptr_t table, std::uintptr_t out,
                  std::uintptr_t aes_tabs, int batch, long long n, int depth,
                  int zlog, int prf, std::uintptr_t stream,
                  std::uintptr_t scratch, std::size_t scratch_bytes,
                  int entry_words) {
  launch_eval_dispatch<true>(keys, table, out, aes_tabs, batch, n, depth, zlog,
                             prf, stream, scratch, scratch_bytes, entry_words);
}

void launch_fused_binned(std::uintptr_t keys, std::uintptr_t table,
                         std::uintptr_t bins, std::uintptr_t out,
                         std::uintptr_t aes_tabs, int batch, long long n,
                         int depth, int zlog, long long num_bins, int prf,
                         std::uintptr_t stream, std::uintptr_t scratch,
                         std::size_t scratch_bytes, int entry_words) {
  check_entry_words(entry_words);
  if (num_bins < 1) throw std::invalid_argument("num_bins must be >= 1");
  // the whole table (num_bins * n rows of 4 * entry_words bytes) must be
  // addressable
  const std::size_t row_bytes = 4 * (std::size_t)entry_words;
  if (n > 0 && num_bins > (long long)(SIZE_MAX / row_bytes) / n)
    throw std::invalid_argument("num_bins * n * row bytes overflows");
  if (batch > 0 && bins == 0)
    throw std::invalid_argument("bins must be a device pointer");
  launch_eval_dispatch<true>(keys, table, out, aes_tabs, batch, n, depth, zlog,
                             prf, stream, scratch, scratch_bytes, entry_words,
                             as_ptr<const int>(bins));
}

int eval_slog(int batch, int depth, int zlog) {
  if (batch <= 0 || zlog < 6 || zlog >= depth)
    throw std::invalid_argument("bad batch/depth/zlog");
  return slog_for(batch, depth - zlog);
}

std::size_t eval_scratch_bytes(int batch, int depth, int zlog) {
  const int slog = eval_slog(batch, depth, zlog);  // validates the arguments
  // the scratch does not depend on the row width
  return EvalGeom(depth, zlog, /*W=*/1).scratch_bytes(batch << slog);
}

void launch_expand(std::uintptr_t keys, std::uintptr_t out,
                   std::uintptr_t aes_tabs, int batch, long long n, int depth,
                   int zlog, int prf, std::uintptr_t stream,
                   std::uintptr_t scratch, std::size_t scratch_bytes) {
  launch_eval_dispatch<false>(keys, /*table=*/0, out, aes_tabs, batch, n, depth,
                              zlog, prf, stream, scratch, scratch_bytes,
                              /*entry_words=*/16);
}

}  // namespace gpudpf_hip
