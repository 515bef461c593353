// The skeleton of the wave-autonomous fused-convolution kernels, each piece defined once:
//   conv_os5_kernel (conv_wave5.hip, fp32), conv_os5h_kernel (conv_wave5h.hip, bf16 / fp16), conv_os5x_kernel (conv_wave5x.hip,
//   fp32 as three bf16 planes), conv_os6h_kernel (conv_wave6h.hip, weight-stationary half), conv_os4_kernel (conv_wave4.hip).
// Launch shape (config, tile size, 4- or 8-wave workgroups; the plan and the launch itself: conv_plan.h), workgroup id -> tile, the LDS layout of a tile
// with its offset-list prologue, group -> offset entry (`conv_locate`), the ticket-ordered commit, the two write-back functors,
// the fragment order of the prepared weights and the decoding of pcs_conv_epilogue. The .hip files keep what is theirs: operand
// loads, the MFMA schedule, pipelining and their debug / trace / ablation switches. Everything here is inlined into its caller
// and so compiled under that file's own flags (openpcseg_amd/build.py EXTRA_FLAGS).
// The kernels sit on the register limit and their allocation follows how the source is factored: a piece is shared with a kernel
// only where every instance keeps its spills, occupancy, LDS and MFMA count (tools/conv_static_ab.py; the table and what was
// tried are in profiles/conv_skeleton_refactor.md). The exceptions are named at each definition below; a kernel that keeps a
// piece inline carries the same text and a comment that points here.
#pragma once
#include "conv_common.h"

namespace pcs {

// ---- launch shape ----------------------------------------------------------------------------------------------------------
// the sink row below the accumulator tile (the padding rows of a row block commit into it)
constexpr int kConvSinkRows = 1;
// bytes of the fp32 accumulator tile: tile_rows + sink rows of 16 nctt columns + 4 of padding
constexpr size_t conv_tile_bytes(int tile_rows, int nctt) { return (size_t)((tile_rows + kConvSinkRows) * (16 * nctt + 4)) * 4; }
// the five offset tables behind the tile (kl_k / kl_s / kl_m [32], kl_g / kl_h [33]) and the ticket word
constexpr size_t kConvTableBytes = 5 * 33 * 4 + 16;
// what every launch-shape decision counts for a workgroup: tile + tables + slack
inline size_t conv5_lds_est(int tile_rows, int nctt) { return conv_tile_bytes(tile_rows, nctt) + 1024; }
// 4-wave workgroups while two of them fit a CU's LDS, else one 8-wave workgroup
inline bool conv_nw8(int tile_rows, int nctt) { return 2 * conv5_lds_est(tile_rows, nctt) > 160 * 1024; }

template <int NCTT, int NW_, int R_ = 1>
struct ConvWaveCfg {
  static constexpr int NW = NW_;
  static constexpr int R = R_;               // row blocks per group
  static constexpr int NT = 64 * NW;
  static constexpr int CT = 16 * NCTT;
  static constexpr int ACS = CT + 4;
  static constexpr int N4 = NCTT / 4;        // 64-column quads of interleaved 16-column tiles
  static constexpr int N2 = (NCTT % 4) / 2;  // one 32-column pair
  static constexpr int N1 = NCTT % 2;        // one single tile
  static constexpr int NWL = N4 + N2 + N1;   // fp32 W loads per contraction step
  static constexpr int SINK = kConvSinkRows;
};

// local column (inside a column tile of nctt 16-column tiles) that lane n of tile tl feeds -- the interleave the commit and the
// epilogue assume (quads of 4 tiles: 64 q + 4 n + f; a pair: + 2 n + f; a single: + n)
__host__ __device__ inline int conv_local_col(int nctt, int tl, int n) {
  const int n4 = nctt / 4, n2 = (nctt % 4) / 2;
  if (tl < 4 * n4) return 64 * (tl / 4) + 4 * n + (tl % 4);
  if (tl < 4 * n4 + 2 * n2) return 64 * n4 + 2 * n + (tl - 4 * n4);
  return 64 * n4 + 32 * n2 + n;
}

// Prepared weights (half and bf16x3 alike): 16-byte element i of a plane is lane (i & 63) of the 1 KB block (offset k, global
// 16-column tile gt, 32-channel step s), i >> 6 = (k * nt16 + gt) * ns + s. v[j] = Wmath[k][32 s + 8 g + j][column(gt, n)] with
// lane = 16 g + n and Wmath[k][c][col] = transpose ? W[k][col][c] : W[k][c][col] (W is (K, A, B) fp32: forward contracts over
// A = cin, dgrad over B = cout). Columns and channels beyond the matrix are zero.
__device__ __forceinline__ void conv_wfrag_values(const float *__restrict__ W, int64_t i, int A, int B, int transpose, int nctt,
                                                  int nt16, int ns, float (&v)[8]) {
  const int ccon = transpose ? B : A, ccols = transpose ? A : B;
  const int lane = (int)(i & 63);
  int64_t b = i >> 6;
  const int s = (int)(b % ns); b /= ns;
  const int gt = (int)(b % nt16);
  const int k = (int)(b / nt16);
  const int n = lane & 15, g = lane >> 4;
  const int col = (gt / nctt) * 16 * nctt + conv_local_col(nctt, gt % nctt, n);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = 32 * s + 8 * g + j;
    v[j] = 0.f;
    if (col < ccols && c < ccon)
      v[j] = transpose ? W[((int64_t)k * A + col) * B + c] : W[((int64_t)k * A + c) * B + col];
  }
}

// pcs_conv_epilogue of the _ex entry points -> addend / act_slope of the kernels (ReLU = their LeakyReLU branch with slope 0;
// act_slope 0 reads as 1: a zeroed struct is the plain call). post_scale / post_shift: the struct's trailing fields, touched only
// under PCS_EP_POST_AFFINE (a caller built against the shorter struct never sets the bit); has_stats: the call asks for BatchNorm
// partials, which the post-affine mode does not produce. `who` heads the error texts.
inline int conv_decode_epilogue(const pcs_conv_epilogue *ep, const char *who, uintptr_t addend_align, bool has_stats,
                                const void *&addend, float &act_slope, const float *&post_scale, const float *&post_shift) {
  addend = ep ? ep->addend : nullptr;
  post_scale = post_shift = nullptr;
  if (addend && ((uintptr_t)addend & (addend_align - 1))) { set_error("%s: misaligned addend", who); return PCS_EINVAL; }
  if (ep && ep->act_slope != 0.f && ep->act_slope != 1.f) act_slope = ep->act_slope;
  if (ep && (ep->flags & ~(PCS_EP_RELU | PCS_EP_POST_AFFINE))) { set_error("%s: unknown pcs_conv_epilogue.flags bits", who); return PCS_EINVAL; }
  if (ep && (ep->flags & PCS_EP_RELU)) act_slope = 0.f;
  if (ep && (ep->flags & PCS_EP_POST_AFFINE)) {
    if (!ep->post_scale || !ep->post_shift || (((uintptr_t)ep->post_scale | (uintptr_t)ep->post_shift) & 15)) {
      set_error("%s: PCS_EP_POST_AFFINE needs 16-byte-aligned post_scale and post_shift", who);
      return PCS_EINVAL;
    }
    if (has_stats) { set_error("%s: PCS_EP_POST_AFFINE does not go with bn_partial", who); return PCS_EINVAL; }
    post_scale = ep->post_scale; post_shift = ep->post_shift;
  }
  return PCS_OK;
}

// ---- workgroup id -> (slot of the launch order, column tile) ---------------------------------------------------------------
// Workgroup b runs on XCD b % 8 (observed dispatch order, speed only). Row order (no `order`): slot = row tile, and with REMAP
// every XCD takes one CONTIGUOUS range of tiles, so that neighbouring tiles -- which gather overlapping src rows -- share that
// XCD's L2 (bijective for any grid size). Heaviest-first order: row tile = a.order[slot], the slots dealt round-robin over the
// XCDs with the column tiles of one row tile back to back on ONE XCD (they gather the same A rows); that grid is padded to
// 8 * ncoltiles, so the caller returns where slot >= a.ntiles before it reads a.order[slot] (the return stays in the kernel:
// returned through a flag it costs a second copy of the exit path). conv_os5x_kernel runs without REMAP (kept as measured);
// conv_os4_kernel is not ORDERED (it ignores a.order: unpadded grid).
template <bool REMAP, bool ORDERED = true, typename Args>
__device__ __forceinline__ void conv_block_slot(const Args &a, int64_t &slot, int &ctile) {
  unsigned bid = blockIdx.x;
  if (REMAP && !(ORDERED && a.order)) {
    const unsigned nb = gridDim.x, q = nb >> 3, r = nb & 7, xcd = bid & 7, idx = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  slot = bid / a.ncoltiles;
  ctile = bid % a.ncoltiles;
  if (ORDERED && a.order) {
    const unsigned xcd = bid & 7, idx = bid >> 3;
    slot = (int64_t)(idx / a.ncoltiles) * 8 + xcd;
    ctile = idx % a.ncoltiles;
  }
}

// ---- the tile in LDS -------------------------------------------------------------------------------------------------------
// [T + SINK][ACS] fp32 accumulator (rows >= T = sink for padding rows), then (TABLES) the offset lists of the tile's non-empty
// offsets, then the ticket word. acc_lds / commit_lds: LDS byte addresses for the commit.
struct ConvTileLds {
  float *acc;
  int *kl_k;  // [32] offset id
  int *kl_s;  // [32] first pair
  int *kl_m;  // [32] #pairs
  int *kl_g;  // [33] first FULL group (prefix over the offsets)
  int *kl_h;  // [33] first partial group (prefix)
  int *commit;
  unsigned acc_lds, commit_lds;
};
template <typename C, bool TABLES>
__device__ __forceinline__ ConvTileLds conv_tile_lds(char *smem, int T) {
  ConvTileLds t;
  t.acc = reinterpret_cast<float *>(smem);
  int *end = reinterpret_cast<int *>(t.acc + (T + C::SINK) * C::ACS);
  t.kl_k = end; t.kl_s = t.kl_k + 32; t.kl_m = t.kl_s + 32; t.kl_g = t.kl_m + 32; t.kl_h = t.kl_g + 33;
  t.commit = TABLES ? t.kl_h + 33 : end;
  t.commit_lds = (unsigned)(size_t)(__attribute__((address_space(3))) int *)t.commit;
  t.acc_lds = (unsigned)(size_t)(__attribute__((address_space(3))) float *)t.acc;
  return t;
}

// Offset-list prologue: wave 0 lists the non-empty offsets of the tile with the prefix of their row-block groups (groups of R
// row blocks + at most one shorter group per offset; both prefixes in one packed scan) and resets the ticket, every thread
// zeroes the tile (nk_s: a __shared__ word of the kernel's own). Behind its barrier: nk offsets, total_full full groups, total_grp groups in all -- wave-uniform scalars, so
// the group loops and their branches stay uniform.
// Group order = commit order: all full groups (R row blocks, equal duration) in ascending offset order, then the partial
// groups. Waves take groups round-robin and commit in order, so neighbours of equal length never wait for each other (with
// offset-major numbering a short group queued behind a long one idled its wave: 9-12 % of the wave time in the ticket wait,
// tools/conv_trace.py). The order depends on the map only: deterministic.
template <typename C, typename Args>
__device__ __forceinline__ void conv_offset_prologue(const ConvTileLds &t, const Args &a, int64_t tile, int T, int tid, int lane,
                                                     int wid, int *nk_s, int &nk, int &total_full, int &total_grp) {
  constexpr int R = C::R;
  const int64_t nt1 = a.ntiles + 1;
  if (wid == 0) {
    const int k = lane;
    int s0 = 0, m = 0;
    if (k < a.K) {
      s0 = a.seg[(int64_t)k * nt1 + tile];
      m = a.seg[(int64_t)k * nt1 + tile + 1] - s0;
    }
    const unsigned long long mask = __ballot(m > 0);
    const int nrb = (m + 15) >> 4;
    const int nfull = nrb / R, npart = (nrb % R) ? 1 : 0;
    int incl = nfull | (npart << 16);
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    if (m > 0) {
      const int pos = __popcll(mask & ((1ULL << lane) - 1ULL));
      t.kl_k[pos] = k; t.kl_s[pos] = s0; t.kl_m[pos] = m;
      t.kl_g[pos] = (incl & 0xFFFF) - nfull; t.kl_h[pos] = (incl >> 16) - npart;
    }
    const int total = __shfl(incl, 63, 64);
    if (lane == 0) {
      const int nkk = __popcll(mask);
      *nk_s = nkk; t.kl_g[nkk] = total & 0xFFFF; t.kl_h[nkk] = total >> 16; *t.commit = 0;
    }
  }
  {  // zero the tile: (T + SINK) * ACS floats, a multiple of four
    float4 *z = reinterpret_cast<float4 *>(t.acc);
    const int n4 = (T + C::SINK) * (C::ACS / 4);
    for (int i = tid; i < n4; i += C::NT) z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  nk = __builtin_amdgcn_readfirstlane(*nk_s);
  total_full = total_grp = 0;
  if (nk > 0) {
    total_full = __builtin_amdgcn_readfirstlane(t.kl_g[nk]);
    total_grp = total_full + __builtin_amdgcn_readfirstlane(t.kl_h[nk]);
  }
}

// group grp -> its offset entry (the hint only moves forward inside a phase; bit 5 = partial-group phase), the row blocks really
// present (nr), and per row block this lane's pair index and whether its row is a real pair (vmask bit r).
// Used by conv_os5_kernel. Inline in conv_os5h_kernel and conv_os5x_kernel: through this function their R = 3 instances at 128 /
// 96 columns spill two more registers.
template <int R>
__device__ __forceinline__ void conv_locate(const ConvTileLds &t, int total_full, int l15, int grp, int &i_hint, int *pidx,
                                            unsigned &vmask, int &nr) {
  int rb0, e;
  if (grp < total_full) {
    e = i_hint;
    while (t.kl_g[e + 1] <= grp) ++e;
    i_hint = e;
    rb0 = (grp - t.kl_g[e]) * R;
    nr = R;
  } else {
    const int q = grp - total_full;
    e = (i_hint & 32) ? (i_hint & 31) : 0;
    while (t.kl_h[e + 1] <= q) ++e;
    i_hint = e | 32;
    const int nrb = (t.kl_m[e] + 15) >> 4;
    rb0 = (nrb / R) * R;
    nr = nrb - rb0;
  }
  const int m = t.kl_m[e];
  vmask = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int rk = (rb0 + r) * 16 + l15;
    const bool v = rk < m;
    vmask |= v ? (1u << r) : 0u;
    pidx[r] = t.kl_s[e] + (v ? rk : m - 1);  // padding rows re-read the slice's last pair
  }
}

// ---- the ticket-ordered commit of a group's row blocks ---------------------------------------------------------------------
// The commits of a workgroup form ONE serial chain (ticket order = group order: race-free, bit-reproducible sums); on the sparse
// full-resolution levels (384-row tiles, 8 waves, ~62 groups per tile) that chain, not the MFMA pipe, bounds the tile. So
//   conv_commit_addr   forms the LDS byte addresses of this lane's pieces BEFORE the ticket wait (dq: the 16-byte column pieces
//                      of the quads, dp: the 8-byte pair / 4-byte single); dloc = tile row of this lane's pair, T = sink;
//   conv_ticket_wait   spins on the ticket, acquire fence;
//   conv_commit_rows   raises the wave's priority while it holds the ticket (its VALU / LDS instructions otherwise queue behind
//                      the MFMA streams of the waves sharing its SIMD: +8 % and +3 % at stride 1), adds the accumulators into
//                      the tile, hands the ticket on, drops the priority.
// A kernel calls the three in a row; trace points, a no-commit ablation or a timer go between the calls.
// Used by conv_os5x_kernel. Inline (the same scheme, written out) in conv_os5_kernel, conv_os5h_kernel and conv_os6h_kernel:
// through these functions conv_os5's 128-column TAIL instances spill (0 -> 2 registers), conv_os5h's 128-column instances gain
// spills, conv_os6h's two-row-block <6, 4> instances go from 24 to 68 spilled registers.
template <int ACS, int NCTT, int RN>
__device__ __forceinline__ void conv_commit_addr(unsigned acc_lds, const int (&dloc)[RN], int g, int l15, unsigned (&dq)[RN][4],
                                                 unsigned (&dp)[RN][4]) {
  constexpr int N4 = NCTT / 4, N2 = (NCTT % 4) / 2;
  int doff[RN][4];
#pragma unroll
  for (int r = 0; r < RN; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int dl = __shfl(dloc[r], 4 * g + j, 64);  // dloc of compact row 4 g + j lives in lanes l15 == 4 g + j
      doff[r][j] = dl * ACS;
    }
#pragma unroll
  for (int r = 0; r < RN; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dq[r][j] = acc_lds + 4u * (unsigned)doff[r][j] + 16u * l15;
      dp[r][j] = acc_lds + 4u * (unsigned)doff[r][j] + 256u * N4 + (N2 ? 8u : 4u) * l15;
      asm volatile("" : "+v"(dq[r][j]), "+v"(dp[r][j]));  // formed here, not sunk into the critical section
    }
}

__device__ __forceinline__ void conv_ticket_wait(int *commit, int ticket, int lane) {
  if (lane == 0) {
    while (__hip_atomic_load(commit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != ticket) __builtin_amdgcn_s_sleep(1);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Rows 0 .. min(NRC, nr) - 1 of acc (NRC at compile time; nr may be a wave-uniform run-time count, pass NRC otherwise), RB row
// blocks per round. A round is three phases, each behind a compiler barrier: every LDS read (one latency for all of them),
// every add, every write -- interleaved, a group went through ~8 read-wait-add rounds, each a full LDS latency, inside the one
// serial chain of the workgroup. RB is the caller's register budget (all row blocks in one round where they fit).
// HARDWARE ASSUMPTION, stated here once for every wave kernel: the LDS executes ONE wave's DS instructions
// in program order. The ticket store stays behind the tile writes in program order, so it is a bare ds_write_b32 that does not
// wait for them to complete (the compiler puts the completion wait, s_waitcnt lgkmcnt(0), in front of a store of its own).
template <int NCTT, int RB, int NRC, int RN>
__device__ __forceinline__ void conv_commit_rows(const unsigned (&dq)[RN][4], const unsigned (&dp)[RN][4],
                                                 const f32x4 (&acc)[RN][NCTT], int nr, unsigned commit_lds, int next_ticket,
                                                 int lane) {
  constexpr int N4 = NCTT / 4, N2 = (NCTT % 4) / 2, N1 = NCTT % 2;
  typedef float v2f __attribute__((ext_vector_type(2)));  // native vectors: the HIP float4 / float2 structs do not assign across address spaces
  typedef __attribute__((address_space(3))) const f32x4 lds_cf4;
  typedef __attribute__((address_space(3))) const v2f lds_cf2;
  typedef __attribute__((address_space(3))) const float lds_cf1;
  typedef __attribute__((address_space(3))) f32x4 lds_f4;
  typedef __attribute__((address_space(3))) v2f lds_f2;
  typedef __attribute__((address_space(3))) float lds_f1;
  __builtin_amdgcn_s_setprio(3);
#pragma unroll
  for (int r0 = 0; r0 < NRC; r0 += RB) {
    f32x4 v4[RB][4][N4 > 0 ? N4 : 1];
    v2f v2[RB][4];
    float v1[RB][4];
#pragma unroll
    for (int rr = 0; rr < RB && r0 + rr < NRC; ++rr)
      if (r0 + rr < nr) {  // wave-uniform
        const int r = r0 + rr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int q = 0; q < N4; ++q) v4[rr][j][q] = *(lds_cf4 *)(size_t)(dq[r][j] + 256u * q);
          if (N2) v2[rr][j] = *(lds_cf2 *)(size_t)dp[r][j];
          if (N1) v1[rr][j] = *(lds_cf1 *)(size_t)(dp[r][j] + 128u * N2);
        }
      }
    asm volatile("" ::: "memory");
#pragma unroll
    for (int rr = 0; rr < RB && r0 + rr < NRC; ++rr)
      if (r0 + rr < nr) {
        const int r = r0 + rr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int q = 0; q < N4; ++q) {
            v4[rr][j][q].x += acc[r][4 * q + 0][j]; v4[rr][j][q].y += acc[r][4 * q + 1][j];
            v4[rr][j][q].z += acc[r][4 * q + 2][j]; v4[rr][j][q].w += acc[r][4 * q + 3][j];
          }
          if (N2) { v2[rr][j].x += acc[r][4 * N4 + 0][j]; v2[rr][j].y += acc[r][4 * N4 + 1][j]; }
          if (N1) v1[rr][j] += acc[r][NCTT - 1][j];
        }
      }
    asm volatile("" ::: "memory");
#pragma unroll
    for (int rr = 0; rr < RB && r0 + rr < NRC; ++rr)
      if (r0 + rr < nr) {
        const int r = r0 + rr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int q = 0; q < N4; ++q) *(lds_f4 *)(size_t)(dq[r][j] + 256u * q) = v4[rr][j][q];
          if (N2) *(lds_f2 *)(size_t)dp[r][j] = v2[rr][j];
          if (N1) *(lds_f1 *)(size_t)(dp[r][j] + 128u * N2) = v1[rr][j];
        }
      }
    asm volatile("" ::: "memory");
  }
  if (lane == 0) asm volatile("ds_write_b32 %0, %1" ::"v"(commit_lds), "v"(next_ticket) : "memory");
  __builtin_amdgcn_s_setprio(0);
}

// ---- write-back functors for conv_tile_epilogue: + addend, LeakyReLU / ReLU, store; they return the value AS STORED --------
// PCS_EP_POST_AFFINE (post_scale != nullptr, a kernel argument: wave-uniform): LeakyReLU / ReLU, * scale + shift, + addend, store.
// The quads of this thread's four columns are loaded once, in front of the row loop (conv_post_quad: a thread of
// conv_tile_epilogue keeps its column quad cq = 4 (tid % (CT / 4)) for all its rows); without the mode they are never read.
struct ConvPostQuad { float4 s, t; };
template <int CT>
__device__ __forceinline__ ConvPostQuad conv_post_quad(const float *post_scale, const float *post_shift, int n0, int cout, int tid) {
  ConvPostQuad p;
  p.s = make_float4(1.f, 1.f, 1.f, 1.f);
  p.t = make_float4(0.f, 0.f, 0.f, 0.f);
  const int c = n0 + 4 * (tid % (CT / 4));
  if (post_scale && c < cout) {  // cout % 4 == 0: a quad is inside or outside as a whole
    p.s = *reinterpret_cast<const float4 *>(post_scale + c);
    p.t = *reinterpret_cast<const float4 *>(post_shift + c);
  }
  return p;
}
__device__ __forceinline__ void conv_leaky(float4 &v, float act_slope) {
  v.x = v.x < 0.f ? v.x * act_slope : v.x; v.y = v.y < 0.f ? v.y * act_slope : v.y;
  v.z = v.z < 0.f ? v.z * act_slope : v.z; v.w = v.w < 0.f ? v.w * act_slope : v.w;
}
__device__ __forceinline__ void conv_affine(float4 &v, const ConvPostQuad &p) {
  v.x = v.x * p.s.x + p.t.x; v.y = v.y * p.s.y + p.t.y; v.z = v.z * p.s.z + p.t.z; v.w = v.w * p.s.w + p.t.w;
}
struct ConvStoreF32 {
  float *drow;          // dst row 0 of the tile, first column of the column tile
  const float *addend;  // (n_dst, ldd) or nullptr
  int64_t row0;
  int n0, ldd;
  float act_slope;
  const float *post_scale;  // nullptr: bias, addend, activation (the order of every call before PCS_EP_POST_AFFINE)
  ConvPostQuad post;
  __device__ __forceinline__ float4 operator()(int r, int cq, const float4 &v0) const {
    float4 v = v0;
    if (post_scale) {  // kernel argument: uniform
      if (act_slope != 1.f) conv_leaky(v, act_slope);
      conv_affine(v, post);
    }
    if (addend) {  // kernel argument: uniform
      const float4 ad = *reinterpret_cast<const float4 *>(addend + (row0 + r) * (int64_t)ldd + n0 + cq);
      v.x += ad.x; v.y += ad.y; v.z += ad.z; v.w += ad.w;
    }
    if (!post_scale && act_slope != 1.f) conv_leaky(v, act_slope);
    *reinterpret_cast<float4 *>(drow + (int64_t)r * ldd + cq) = v;
    return v;
  }
};
// fp32 tile -> halfs, 8-byte stores; the addend is added in fp32 before the rounding. Used by conv_os6h_kernel's fallback
// branch; conv_os5h_kernel keeps the same lambda inline (register allocation, as above).
template <typename HT>
struct ConvStoreHalf {
  uint16_t *drow;
  const uint16_t *addend;
  int64_t row0;
  int n0, ldd;
  float act_slope;
  const float *post_scale;  // as ConvStoreF32: the post-affine order, everything in fp32, one rounding below
  ConvPostQuad post;
  __device__ __forceinline__ float4 operator()(int r, int cq, const float4 &v0) const {
    float4 v = v0;
    if (post_scale) {  // kernel argument: uniform
      if (act_slope != 1.f) conv_leaky(v, act_slope);
      conv_affine(v, post);
    }
    if (addend) {  // kernel argument: uniform
      const uint2 ad = *reinterpret_cast<const uint2 *>(addend + (row0 + r) * (int64_t)ldd + n0 + cq);
      v.x += h2f(HT{}, (uint16_t)(ad.x & 0xFFFFu)); v.y += h2f(HT{}, (uint16_t)(ad.x >> 16));
      v.z += h2f(HT{}, (uint16_t)(ad.y & 0xFFFFu)); v.w += h2f(HT{}, (uint16_t)(ad.y >> 16));
    }
    if (!post_scale && act_slope != 1.f) conv_leaky(v, act_slope);
    const uint16_t hx = f2h(HT{}, v.x), hy = f2h(HT{}, v.y), hz = f2h(HT{}, v.z), hw = f2h(HT{}, v.w);
    uint2 o;
    o.x = hx | ((uint32_t)hy << 16);
    o.y = hz | ((uint32_t)hw << 16);
    *reinterpret_cast<uint2 *>(drow + (int64_t)r * ldd + cq) = o;
    return make_float4(h2f(HT{}, hx), h2f(HT{}, hy), h2f(HT{}, hz), h2f(HT{}, hw));
  }
};

}  // namespace pcs
