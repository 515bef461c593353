// Wave-autonomous fused convolution with row-block groups ("wave5"): the kernel behind every >= 64-channel layer.
#include "conv_plan.h"

using namespace pcs;

namespace {

#if PCS_TRACE
__device__ long long *g_conv_trace;   // [block][wave][8]: t_entry, t_start, t_end, loop, ticket, commit, groups, t_exit
constexpr int kTraceBlocks = 8192;
#endif

// ================================================================================================
// wave5 = the wave4 design (conv_wave4.hip: register-direct operands in MFMA layout, interleaved column tiles,
// sched_group_barrier software pipeline, cross-group prefetch, ticket-ordered LDS commit) + row-block GROUPS: one wave
// applies each W operand block to a group of up to R consecutive row blocks of the same offset (R accumulator sets),
// so the W stream per compact row drops R-fold where an offset has >= R row blocks in the tile -- with one row block
// per step every 16 rows stream their own copy of W[k] (Cin x CT fp32, 37-131 KB) out of L2. The tile height is a
// run-time parameter chosen per layer (pcs_conv_pick_tile_rows).
// TAIL = false: cin % 32 == 0 (an even number of whole 16-channel blocks: the straight-line two-stage pipeline).
// TAIL = true: any cin % 4 == 0 (56, 112, 168, 336 ... of RPVNet cr 1.75, 48 of cr 0.5): the last block may hold
// 4 / 8 / 12 channels -- its out-of-range lane groups read a clamped (in-row) address and contribute exact zeros --
// and an odd number of blocks ends the group one pipeline stage early (the next group's first block lands in the
// other register set and is moved over).
// ================================================================================================
template <int NCTT, int NW, int MINW, int R, bool TAIL>
__global__ void __launch_bounds__(64 * NW, MINW) conv_os5_kernel(ConvArgs a) {
  using C = ConvWaveCfg<NCTT, NW, R>;
  const int T = a.tile_rows;  // any multiple of 16: the host picks it per layer (pcs_conv_pick_tile_rows)
  PCS_T(const long long tr_entry = wall_clock64(); long long tr_loop = 0, tr_ticket = 0, tr_commit = 0; int tr_groups = 0;)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ConvTileLds tl = conv_tile_lds<C, true>(smem, T);
  float *acc_l = tl.acc;
  int *commit = tl.commit;
  const unsigned commit_lds = tl.commit_lds, acc_lds = tl.acc_lds;

  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // a scalar: wave-level loops and branches stay uniform
  const int g = lane >> 4, l15 = lane & 15;
  int64_t slot;
  int ctile;
  conv_block_slot<true>(a, slot, ctile);
  if (a.order && slot >= a.ntiles) return;  // the grid of an ordered launch is padded to 8 * ncoltiles
  const int64_t tile = a.order ? (int64_t)a.order[slot] : slot;
  const int n0 = ctile * C::CT;
  const int64_t row0 = tile * T;
  __shared__ int nk_s;
  int nk, total_full, total_grp;  // wave-uniform scalars
  conv_offset_prologue<C>(tl, a, tile, T, tid, lane, wid, &nk_s, nk, total_full, total_grp);

  const int cin4 = a.cin - 4;
  const int nb16 = TAIL ? (a.cin + 15) >> 4 : a.cin >> 4;  // 16-channel contraction blocks
  const int cinp = nb16 * 16;
  int col4[C::N4 > 0 ? C::N4 : 1];
#pragma unroll
  for (int q = 0; q < C::N4; ++q) {
    const int c = 64 * q + 4 * l15;
    col4[q] = (n0 + c + 4 <= a.cout) ? c : 0;
  }
  const int c2 = 64 * C::N4 + 2 * l15;
  const int col2 = (n0 + c2 + 2 <= a.cout) ? c2 : 0;
  const int c1 = 64 * C::N4 + 32 * C::N2 + l15;
  const int col1 = (n0 + c1 < a.cout) ? c1 : 0;

  struct Frag {  // one 16-channel block: A pieces of the R row blocks + the shared W rows
    float4 a[R];
    float4 b4[4][C::N4 > 0 ? C::N4 : 1];
    float2 b2[4];
    float b1[4];
  };
  struct Ctx {  // one group: R row blocks of one offset
    const float *srow0[R];
    const float *Wk;
    int dloc[R];
    int nr;  // row blocks really present (1..R)
    unsigned vmask;  // bit r: this lane's row of block r is a real pair
  };
  // PCS_ABLATE5 (debug builds): 3 = no operand loads inside the channel loop, 5 = no W loads, 6 = no A loads there
  auto load_frag = [&](Frag &f, const Ctx &cx, int c0, bool in_loop = false) {
    int ca = c0 + 4 * g;  // !TAIL: always inside the row
    if (TAIL) ca = ca < cin4 ? ca : cin4;  // a lane group beyond cin re-reads the row's last piece; masked in mfma_frag
    (void)in_loop;
#if PCS_ABLATE5 == 3
    if (in_loop) return;
#endif
#if PCS_ABLATE5 != 6
#pragma unroll
    for (int r = 0; r < R; ++r) f.a[r] = *reinterpret_cast<const float4 *>(cx.srow0[r] + ca);
#else
    if (!in_loop) for (int r = 0; r < R; ++r) f.a[r] = *reinterpret_cast<const float4 *>(cx.srow0[r] + ca);
#endif
#if PCS_ABLATE5 == 5
    if (in_loop) return;
#endif
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float *wp = cx.Wk + (int64_t)(ca + e) * a.cout;
#pragma unroll
      for (int q = 0; q < C::N4; ++q) f.b4[e][q] = *reinterpret_cast<const float4 *>(wp + col4[q]);
      if (C::N2) f.b2[e] = *reinterpret_cast<const float2 *>(wp + col2);
      if (C::N1) f.b1[e] = wp[col1];
    }
  };
  auto locate = [&](int grp, int &i_hint, int *pidx, unsigned &vmask, int &nr) {
    conv_locate<R>(tl, total_full, l15, grp, i_hint, pidx, vmask, nr);
  };
  auto make_ctx = [&](Ctx &cx, const int2 *pr, unsigned vmask, int nr, int i_k) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
#if PCS_ALIAS == 2   /* debug build: gather replaced by the dst row itself (sequential, L2-friendly A operand) */
      cx.srow0[r] = a.src + (int64_t)(a.src_col ? pr[r].x : pr[r].y) * a.cin;
#else
      cx.srow0[r] = a.src + (int64_t)(a.src_col ? pr[r].y : pr[r].x) * a.cin;
#endif
      cx.dloc[r] = ((vmask >> r) & 1u) ? (int)((a.src_col ? pr[r].x : pr[r].y) - row0) : T;
    }
    cx.vmask = vmask;
    cx.nr = nr;
#if PCS_ALIAS == 1   /* debug build: every offset reads W[0] (W operand always L1/L2-hot) */
    cx.Wk = a.W + n0;
#else
    cx.Wk = a.W + (int64_t)tl.kl_k[i_k & 31] * a.cin * a.cout + n0;
#endif
  };

  int i = 0;
  Ctx cur;
  Frag f0, f1;
  if (wid < total_grp) {
    int pidx[R]; unsigned vm; int nr;
    locate(wid, i, pidx, vm, nr);
    int2 pr[R];
#pragma unroll
    for (int r = 0; r < R; ++r) pr[r] = reinterpret_cast<const int2 *>(a.pairs)[pidx[r]];
    make_ctx(cur, pr, vm, nr, i);
    load_frag(f0, cur, 0);
  }
  PCS_T(const long long tr_start = wall_clock64();)
  // One group = NRC row blocks of one offset: R for the full groups, 1 for the partial ones (R = 2). A lambda per NRC so
  // that each of the two group loops below has ONE straight-line body: with both bodies behind a branch inside one loop the
  // register allocator resolved the loop-carried operand registers (the next group's prefetched first block) with ~30
  // copies at the join -- and the s_waitcnt vmcnt(0) those copies need sat in front of every ticket wait.
  static_assert(R == 2, "partial groups are handled as single row blocks");
  auto run_group = [&](const int grp, auto nrc_tag) {
    constexpr int NRC = decltype(nrc_tag)::value;
    PCS_T(const long long tr_a = wall_clock64();)
    const int grpn = grp + C::NW < total_grp ? grp + C::NW : grp;
    int in = i, pidx_n[R], nr_n; unsigned vm_n;
    locate(grpn, in, pidx_n, vm_n, nr_n);
    int2 pr_n[R];
#pragma unroll
    for (int r = 0; r < R; ++r) pr_n[r] = reinterpret_cast<const int2 *>(a.pairs)[pidx_n[r]];

    f32x4 acc[R][NCTT];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int t = 0; t < NCTT; ++t) acc[r][t] = (f32x4){0, 0, 0, 0};
    const unsigned vmask = cur.vmask;
    constexpr int nr = NRC;
    // MFMAs of one 16-channel block for the first NR row blocks of the group (NR is wave-uniform)
    // last_tag: the block is the layer's last one (only there can lane groups lie beyond cin)
    auto mfma_frag = [&](const Frag &f, auto nr_tag, auto last_tag) {
      constexpr int NR = decltype(nr_tag)::value;
      constexpr bool LAST = decltype(last_tag)::value;
      const bool cok = !(TAIL && LAST) || (cinp - 16 + 4 * g < a.cin);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const bool ok = ((vmask >> r) & 1u) && cok;
          const float av = ok ? (e == 0 ? f.a[r].x : (e == 1 ? f.a[r].y : (e == 2 ? f.a[r].z : f.a[r].w))) : 0.f;
#if PCS_ABLATE5 == 2   /* debug build: consume the operands with one VALU op each, no MFMA */
#pragma unroll
          for (int q = 0; q < C::N4; ++q)
            acc[r][4 * q][0] += av * (f.b4[e][q].x + f.b4[e][q].y + f.b4[e][q].z + f.b4[e][q].w);
          if (C::N2) acc[r][4 * C::N4][0] += av * (f.b2[e].x + f.b2[e].y);
          if (C::N1) acc[r][NCTT - 1][0] += av * f.b1[e];
          continue;
#endif
#pragma unroll
          for (int q = 0; q < C::N4; ++q) {
            acc[r][4 * q + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, f.b4[e][q].x, acc[r][4 * q + 0], 0, 0, 0);
            acc[r][4 * q + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, f.b4[e][q].y, acc[r][4 * q + 1], 0, 0, 0);
            acc[r][4 * q + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, f.b4[e][q].z, acc[r][4 * q + 2], 0, 0, 0);
            acc[r][4 * q + 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, f.b4[e][q].w, acc[r][4 * q + 3], 0, 0, 0);
          }
          if (C::N2) {
            acc[r][4 * C::N4 + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, f.b2[e].x, acc[r][4 * C::N4 + 0], 0, 0, 0);
            acc[r][4 * C::N4 + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, f.b2[e].y, acc[r][4 * C::N4 + 1], 0, 0, 0);
          }
          if (C::N1) acc[r][NCTT - 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, f.b1[e], acc[r][NCTT - 1], 0, 0, 0);
        }
      }
    };
    Ctx nxt;
    // one scheduling region per block: per contraction step e the W loads of the NEXT block (plus,
    // first, its R A pieces), then this block's NR*NCTT MFMAs of step e
#define PCS_PIPE5(LOAD, FR, NRV, LASTV)                                                            \
  LOAD; mfma_frag(FR, std::integral_constant<int, NRV>{}, std::integral_constant<bool, LASTV>{});  \
  __builtin_amdgcn_sched_group_barrier(0x020, R + C::NWL, 0);                                      \
  __builtin_amdgcn_sched_group_barrier(0x008, NRV * NCTT, 0);                                      \
  __builtin_amdgcn_sched_group_barrier(0x020, C::NWL, 0);                                          \
  __builtin_amdgcn_sched_group_barrier(0x008, NRV * NCTT, 0);                                      \
  __builtin_amdgcn_sched_group_barrier(0x020, C::NWL, 0);                                          \
  __builtin_amdgcn_sched_group_barrier(0x008, NRV * NCTT, 0);                                      \
  __builtin_amdgcn_sched_group_barrier(0x020, C::NWL, 0);                                          \
  __builtin_amdgcn_sched_group_barrier(0x008, NRV * NCTT, 0);                                      \
  __builtin_amdgcn_sched_barrier(0);
#define PCS_BODY5(NRV)                                                                             \
  if (!TAIL || !(nb16 & 1)) { /* an even number of blocks */                                       \
    for (int c0 = 0; c0 < cinp - 32; c0 += 32) {                                                   \
      PCS_PIPE5(load_frag(f1, cur, c0 + 16, true), f0, NRV, false)                                 \
      PCS_PIPE5(load_frag(f0, cur, c0 + 32, true), f1, NRV, false)                                 \
    }                                                                                              \
    PCS_PIPE5(load_frag(f1, cur, cinp - 16, true), f0, NRV, false)                                 \
    make_ctx(nxt, pr_n, vm_n, nr_n, in);                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                             \
    PCS_PIPE5(load_frag(f0, nxt, 0), f1, NRV, true)                                                \
  } else { /* odd: the loop leaves the last block in f0 */                                         \
    for (int c0 = 0; c0 < cinp - 16; c0 += 32) {                                                   \
      PCS_PIPE5(load_frag(f1, cur, c0 + 16, true), f0, NRV, false)                                 \
      PCS_PIPE5(load_frag(f0, cur, c0 + 32, true), f1, NRV, false)                                 \
    }                                                                                              \
    make_ctx(nxt, pr_n, vm_n, nr_n, in);                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                             \
    PCS_PIPE5(load_frag(f1, nxt, 0), f0, NRV, true)                                                \
    f0 = f1;                                                                                       \
  }
    { PCS_BODY5(NRC) }
#undef PCS_BODY5
#undef PCS_PIPE5
    // ---- in-order commit of the group's row blocks -------------------------------------------------------
    // The commits of a workgroup form ONE serial chain (ticket order = group order: bit-reproducible sums); on the
    // sparse full-resolution levels (384-row tiles, 8 waves, ~62 groups per tile) that chain, not the MFMA pipe,
    // bounds the tile. So the row addresses are formed BEFORE the ticket wait, and the wave raises its priority while
    // it holds the ticket (its VALU / LDS instructions otherwise queue behind the MFMA streams of the waves sharing
    // its SIMD): +8 % and +3 % at stride 1. A second ticket for half of the columns bought nothing on top.
    // (inline here, not conv_commit_* of conv_wave_common.h -- the reference definition, where the LDS ordering assumption is
    // stated: shared, this kernel's register allocation moved and instances gained spills; profiles/conv_skeleton_refactor.md)
    PCS_T(const long long tr_b = wall_clock64();)
    int doff[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int dl = __shfl(cur.dloc[r], 4 * g + j, 64);
        doff[r][j] = dl * C::ACS;
      }
    unsigned dq[R][4], dp[R][4];  // LDS byte addresses of this lane's pieces of the rows it commits
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        dq[r][j] = acc_lds + 4u * (unsigned)doff[r][j] + 16u * l15;
        dp[r][j] = acc_lds + 4u * (unsigned)doff[r][j] + 256u * C::N4 + (C::N2 ? 8u : 4u) * l15;
        asm volatile("" : "+v"(dq[r][j]), "+v"(dp[r][j]));  // formed BEFORE the ticket wait, not sunk into the critical section
      }
    if (lane == 0) {
      while (__hip_atomic_load(commit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != grp)
        __builtin_amdgcn_s_sleep(1);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    __builtin_amdgcn_s_setprio(3);
    PCS_T(const long long tr_c = wall_clock64();)
    {
      // Three phases, each behind a compiler barrier: every LDS read of the group (one latency for all of them), every
      // add, every write. Round 2's interleaving went through ~8 read-wait-add rounds per group, each a full LDS
      // latency, inside the one serial chain of the workgroup; the LDS byte addresses (dq: the 16-byte column pieces,
      // dp: the 8-byte pair) are formed before the ticket wait.
      typedef float v2f __attribute__((ext_vector_type(2)));  // native vectors: the HIP float4 / float2 structs do not assign across address spaces
      typedef __attribute__((address_space(3))) const f32x4 lds_cf4;
      typedef __attribute__((address_space(3))) const v2f lds_cf2;
      typedef __attribute__((address_space(3))) const float lds_cf1;
      typedef __attribute__((address_space(3))) f32x4 lds_f4;
      typedef __attribute__((address_space(3))) v2f lds_f2;
      typedef __attribute__((address_space(3))) float lds_f1;
      // all row blocks of the group in one round while the registers allow it (<= 96 columns), else one round per block
      constexpr int RB = (NCTT <= 6) ? NRC : 1;
#pragma unroll
      for (int r0 = 0; r0 < NRC; r0 += RB) {
        f32x4 v4[RB][4][C::N4 > 0 ? C::N4 : 1];
        v2f v2[RB][4];
        float v1[RB][4];
#pragma unroll
        for (int rr = 0; rr < RB; ++rr)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = r0 + rr;
#pragma unroll
            for (int q = 0; q < C::N4; ++q) v4[rr][j][q] = *(lds_cf4 *)(size_t)(dq[r][j] + 256u * q);
            if (C::N2) v2[rr][j] = *(lds_cf2 *)(size_t)dp[r][j];
            if (C::N1) v1[rr][j] = *(lds_cf1 *)(size_t)(dp[r][j] + 128u * C::N2);
          }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int rr = 0; rr < RB; ++rr)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = r0 + rr;
#pragma unroll
            for (int q = 0; q < C::N4; ++q) {
              v4[rr][j][q].x += acc[r][4 * q + 0][j]; v4[rr][j][q].y += acc[r][4 * q + 1][j];
              v4[rr][j][q].z += acc[r][4 * q + 2][j]; v4[rr][j][q].w += acc[r][4 * q + 3][j];
            }
            if (C::N2) { v2[rr][j].x += acc[r][4 * C::N4 + 0][j]; v2[rr][j].y += acc[r][4 * C::N4 + 1][j]; }
            if (C::N1) v1[rr][j] += acc[r][NCTT - 1][j];
          }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int rr = 0; rr < RB; ++rr)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = r0 + rr;
#pragma unroll
            for (int q = 0; q < C::N4; ++q) *(lds_f4 *)(size_t)(dq[r][j] + 256u * q) = v4[rr][j][q];
            if (C::N2) *(lds_f2 *)(size_t)dp[r][j] = v2[rr][j];
            if (C::N1) *(lds_f1 *)(size_t)(dp[r][j] + 128u * C::N2) = v1[rr][j];
          }
        asm volatile("" ::: "memory");
      }
    }
    // the ticket store stays behind the tile writes in program order and the LDS keeps a wave's instructions in order; a
    // bare ds_write_b32 because the compiler puts the completion wait (s_waitcnt lgkmcnt(0)) in front of its own store
    // (the hardware assumption is stated once, at conv_commit_rows in conv_wave_common.h)
    if (lane == 0) asm volatile("ds_write_b32 %0, %1" ::"v"(commit_lds), "v"(grp + 1) : "memory");
    __builtin_amdgcn_s_setprio(0);
    PCS_T(const long long tr_d = wall_clock64(); tr_loop += tr_b - tr_a; tr_ticket += tr_c - tr_b; tr_commit += tr_d - tr_c; ++tr_groups;)
    cur = nxt;
    i = in;
  };
  {  // wave-uniform loops, no barrier inside: the full groups, then the partial ones (= the commit order)
    int grp = wid;
    for (; grp < total_full; grp += C::NW) run_group(grp, std::integral_constant<int, R>{});
    for (; grp < total_grp; grp += C::NW) run_group(grp, std::integral_constant<int, 1>{});
  }
  PCS_T(const long long tr_end = wall_clock64();)
  __syncthreads();
  const int rows = (int)((a.n_dst - row0) < (int64_t)T ? (a.n_dst - row0) : (int64_t)T);
  float *drow = a.dst + row0 * a.cout + n0;
  const int ldd = a.cout;
  conv_tile_epilogue<C::CT, C::NT>(acc_l, C::ACS, rows, n0, a.cout, a.bias, a.stats ? a.stats + tile * 2 * a.cout : nullptr, tid,
                                   ConvStoreF32{drow, a.addend, row0, n0, ldd, a.act_slope, a.post_scale,
                                                conv_post_quad<C::CT>(a.post_scale, a.post_shift, n0, a.cout, tid)});
#if PCS_TRACE
  if (lane == 0 && blockIdx.x < kTraceBlocks && g_conv_trace) {
    long long *t = g_conv_trace + ((int64_t)blockIdx.x * 8 + wid) * 8;
    t[0] = tr_entry; t[1] = tr_start; t[2] = tr_end; t[3] = tr_loop; t[4] = tr_ticket; t[5] = tr_commit;
    t[6] = tr_groups; t[7] = wall_clock64();
  }
#endif
}

#if PCS_TRACE
long long *g_trace_host_ptr = nullptr;
void trace_prepare(hipStream_t st) {
  if (!g_trace_host_ptr) {
    (void)hipMalloc(&g_trace_host_ptr, (size_t)kTraceBlocks * 64 * sizeof(long long));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_conv_trace), &g_trace_host_ptr, sizeof(g_trace_host_ptr));
  }
  (void)hipMemsetAsync(g_trace_host_ptr, 0, (size_t)kTraceBlocks * 64 * sizeof(long long), st);
}
#endif

template <int NCTT, int NW, int MINW, int R, bool TAIL>
int launch_conv5(const ConvArgs &a, const ConvPlan &p, hipStream_t st) {
  constexpr auto kern = conv_os5_kernel<NCTT, NW, MINW, R, TAIL>;
  return conv_wave_launch<kern>(a, p, st, "pcs_conv", "pcs_conv_gather_gemm_f32(wave5)", [&](int64_t nblocks) {
    PCS_T(trace_prepare(st);)
    static const int dbg = getenv("PCS_CONV_DEBUG") ? atoi(getenv("PCS_CONV_DEBUG")) : 0;  // debug: launch shape + residency
    static long long dbg_last = -1;
    const long long dbg_key = ((long long)a.tile_rows << 32) ^ ((long long)a.cin << 16) ^ a.cout;
    if (dbg && dbg_key != dbg_last) {
      dbg_last = dbg_key;
      int nb = 0;
      (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void *>(kern), p.nt, p.lds);
      fprintf(stderr, "[pcs_conv] wave5<%d,%d,%d,%d%s> T=%d cin=%d cout=%d grid=%lld lds=%zu resident WG/CU=%d (waves/SIMD=%d)\n", NCTT, NW,
              MINW, R, TAIL ? ",tail" : "", a.tile_rows, a.cin, a.cout, (long long)nblocks, p.lds, nb, nb * NW / 4);
    }
  });
}

}  // namespace

#if PCS_TRACE
// debug builds only: phase timers of the last v5 launch, [block < 8192][wave < 8][8] int64 (synchronises the device)
extern "C" int pcs_debug_conv_trace(long long *host_out) {
  if (!g_trace_host_ptr || !host_out) return PCS_EINVAL;
  if (hipDeviceSynchronize() != hipSuccess) return PCS_ELAUNCH;
  return hipMemcpy(host_out, g_trace_host_ptr, (size_t)kTraceBlocks * 64 * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess ? PCS_OK : PCS_ELAUNCH;
}
#endif

int pcs::launch_conv_wave5(const ConvArgs &a, const ConvPlan &p, hipStream_t st) {
#define PCS_CONV5_CASE(N)                                                                           \
  case N:                                                                                           \
    if (p.nt == 512) return p.tail ? launch_conv5<N, 8, 2, 2, true>(a, p, st) : launch_conv5<N, 8, 2, 2, false>(a, p, st);  \
    return p.tail ? launch_conv5<N, 4, 2, 2, true>(a, p, st) : launch_conv5<N, 4, 2, 2, false>(a, p, st);
  switch (p.nctt) {
    PCS_CONV5_CASE(2)
    PCS_CONV5_CASE(4)
    PCS_CONV5_CASE(6)
    PCS_CONV5_CASE(8)
  }
#undef PCS_CONV5_CASE
  set_error("pcs_conv_gather_gemm_f32: unreachable");
  return PCS_EINVAL;
}
