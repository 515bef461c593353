// Sparse 3-D convolution on gfx950: output-stationary fused gather-GEMM-accumulate for forward, dgrad and transposed
// convolutions, fp32 storage + fp32 MFMA (v_mfma_f32_16x16x4_f32). This file: the route (conv_plan.h), the tile-height picker, the
// shape queries and the fp32 C entry point; the kernels live in conv_wave5.hip (>= 64 channels), conv_wave4.hip (other
// 16-byte-granular shapes) and conv_block.hip (everything else); the weight gradient in conv_wgrad.hip.
#include <math.h>

#include "conv_plan.h"

using namespace pcs;

namespace pcs {

ConvEnv &conv_env() {   // each value is read once
  auto num = [](const char *v, int dflt) { return v ? atoi(v) : dflt; };
  static ConvEnv env = {num(getenv("PCS_CONV_TILE"), 0),  num(getenv("PCS_CONV_NCTT"), 0), num(getenv("PCS_CONV_NW"), 0),
                        num(getenv("PCS_CONVH_NCTT"), 0), num(getenv("PCS_CONVH_R"), 0),   num(getenv("PCS_CONVX_R"), 0),
                        num(getenv("PCS_CONVH_WS"), 1)};
  return env;
}

ConvPlan conv_route(ConvKind kind, int dtype, int cin, int cout, int K, int T, int flags) {   // T: tile_rows
  const ConvEnv &env = conv_env();
  ConvPlan p;
  p.dtype = dtype;
  if (cin <= 0 || cout <= 0 || K <= 0) return p;
  p.tail = (cin % 32) != 0;
  bool nw8 = false, fit_height = T >= 16;   // fit_height: the heights at which the family can leave statistics at all
  size_t tables = kConvTableBytes;          // what the family keeps in LDS behind the accumulator tile
  if (kind == ConvKind::f32) {
    p.vec = cin % 4 == 0 && cout % 4 == 0 && !(flags & kConvUnaligned);
    if (p.vec && conv5_applies(cin, cout, K)) {
      p.family = ConvFamily::wave5;
      p.nctt = conv5_nctt(cout, T);   // wide outputs on tall tiles: 64-column tiles
      if (env.nctt && p.nctt > env.nctt) p.nctt = env.nctt;
      nw8 = env.nw ? env.nw == 8 : conv_nw8(T, p.nctt);
      // groups of 2 row blocks (groups of 3 / 4 were instantiated and measured through round 2: within +-1 % where they fit
      // the registers -- the W stream they save is not what bounds the kernel -- and spilling at 6 / 8 column tiles)
      p.R = 2;
    } else if (p.vec && K <= 32) {
      p.family = ConvFamily::wave4;   // 4 waves with <= 168 VGPRs: 3 workgroups per CU; four 32-entry offset tables + ticket
      p.nctt = conv_nctt(cout);
      tables = 4 * 32 * 4 + 32;
      fit_height = T == 64 || T == 128;
    } else {
      p.family = ConvFamily::block;   // column tile: 32 cg with cg in 1 .. 4; wider outputs are covered by several column tiles
      const int cg = cout > 96 ? 4 : (cout + 31) / 32;
      p.nctt = 2 * cg;
      p.nt = cg == 1 ? 256 : 128 * cg;
      // conv_block.hip: accumulator [T][32 cg + 4], W chunk [32][32 cg + 16], gathered rows [T][34], two row maps [T]
      p.lds = (size_t)(T * (32 * cg + 4) + T * 34 + 32 * (32 * cg + 16)) * 4 + (size_t)2 * T * 4;
      fit_height = false;
    }
    p.takes_extras = p.family != ConvFamily::block;
    p.reads_order = p.family == ConvFamily::wave5;
  } else {
    if (!(kind == ConvKind::half ? convh_applies(cin, cout, K) : convx_applies(cin, cout, K))) return p;
    const ConvPreparedGeom g = conv_prepared_geom(cin, cout, kind == ConvKind::x3);
    p.nctt = g.nctt; p.nt16 = g.nt16; p.ns = g.ns;
    const Conv6hInstance *ws = conv6h_instance(p.nctt, p.ns, env.ws_ab);
    if (kind == ConvKind::x3) {
      p.family = ConvFamily::wave5x;
      // Row blocks per group. The kernel is bound by the vector-memory address path (TA 78-87 % busy, MFMA pipe 29-37 %,
      // profiles/round3_convx.md): per row block and step a column tile costs 2 A loads + 3 N / R weight-fragment loads, so R is
      // the lever -- four row blocks per group at <= 64 columns (1.11x R = 2), three at 96 (1.08-1.10x; what the 256 registers of
      // two waves per SIMD hold), 32 columns lose with R > 2
      p.R = env.x_r >= 2 && env.x_r <= 4 ? (p.nctt == 6 && env.x_r > 3 ? 3 : env.x_r) : (p.nctt == 6 ? 3 : (p.nctt == 4 ? 4 : 2));
    } else if (env.ws_mode() && conv6h_applies(cin, cout, K) && (ws->kc == 1 || T <= 160)) {
      p.family = ConvFamily::wave6h;   // its chunked-contraction instances only on tiles of <= 160 rows
      p.rs = ws->rs; p.kc = ws->kc;
      tables = 64;   // no offset tables in LDS: the slice table lives in registers
    } else {
      p.family = ConvFamily::wave5h;
      if (env.h_nctt && p.nctt > env.h_nctt && cout % (16 * env.h_nctt) == 0 && !(flags & kConvStats)) p.nctt = env.h_nctt;
      // row blocks per group: the kernel is bound by the vector-memory address unit (TA ~65-80 % busy, MFMA pipe 10-20 %,
      // profiles/round3_convh_pmc.md): one 16-byte operand load per lane feeds R N / (R + N) MFMAs, so more row blocks per B
      // fragment = fewer loads per MFMA as far as the registers allow; 2 was picked (profiles/round3_convh_group_rows.txt)
      p.R = !p.tail && !(flags & kConvPostAffine) && env.h_r >= 2 && env.h_r <= 4 ? env.h_r : 2;
    }
    nw8 = conv_nw8(T, p.nctt);
    p.reads_order = true;
    p.takes_extras = kind == ConvKind::half;
  }
  if (p.family != ConvFamily::block) {
    p.nt = nw8 ? 512 : 256;
    p.lds = conv_tile_bytes(T, p.nctt) + tables;
  }
  p.ncoltiles = (int)ceil_div(cout, 16 * p.nctt);
  p.emits_stats = fit_height && conv_stats_fit(T, 16 * p.nctt, p.nt);
  return p;
}

}  // namespace pcs

namespace {

int device_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) cus = n;
    else cus = 256;
  }
  return cus;
}

// dst[k][b][a] = src[k][a][b]: per-offset transposed weights for dgrad (a few MB per layer, once per backward pass).
// 32x32 LDS tiles (+1 padding), 128-byte lines on both sides -- the generic strided copy ran at ~0.7 TB/s here.
__global__ void __launch_bounds__(256) transpose_kab_kernel(const float *__restrict__ src, int A, int B,
                                                            float *__restrict__ dst) {
  __shared__ float tile[32][33];
  const int k = blockIdx.z, a0 = blockIdx.y * 32, b0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const float *s = src + (int64_t)k * A * B;
  float *d = dst + (int64_t)k * A * B;
#pragma unroll
  for (int r = ty; r < 32; r += 8)
    if (a0 + r < A && b0 + tx < B) tile[r][tx] = s[(int64_t)(a0 + r) * B + b0 + tx];
  __syncthreads();
#pragma unroll
  for (int r = ty; r < 32; r += 8)
    if (b0 + r < B && a0 + tx < A) d[(int64_t)(b0 + r) * A + a0 + tx] = tile[tx][r];
}

}  // namespace

extern "C" int pcs_transpose_kab_f32(const float *src, int32_t K, int32_t A, int32_t B, float *dst, void *stream) {
  if (K <= 0 || A <= 0 || B <= 0 || K > 65535 || !src || !dst) { set_error("pcs_transpose_kab_f32: bad args"); return PCS_EINVAL; }
  hipLaunchKernelGGL(transpose_kab_kernel, dim3((unsigned)ceil_div(B, 32), (unsigned)ceil_div(A, 32), (unsigned)K), dim3(256),
                     0, as_stream(stream), src, A, B, dst);
  return check_launch("pcs_transpose_kab_f32");
}

// Bumped whenever a fused-conv kernel, its launch shape picker or its epilogue changes: measurements keyed to kernels
// (profiles/*_conv_traffic.json) carry the revision they were taken on and bench.py refuses a stale one.
extern "C" const char *pcs_conv_kernel_revision(void) { return "r6.1"; }

extern "C" int32_t pcs_conv_tile_rows(int32_t cin, int32_t cout) {
  (void)cin;
  (void)cout;
  return 128;
}

// Output tile height for one layer call (profiles/round2_tile_sweep_{f32,bf16}.md: every k3 shape of MinkUNet-34 on the
// 12-frame maps x 13 heights). Model of one launch: the workgroups of a CU share its MFMA pipe, so the launch takes
// (workgroups per CU) x (work of one workgroup), work = pairs per tile + the padding of half a 16-row block per offset;
// the last, partly filled round of workgroups counts half (heaviest-first tile order: the light tiles fill it).
// Tall tiles pad less but fit fewer workgroups per CU (LDS holds the fp32 accumulator tile).
namespace {
double launch_cost(int64_t n_dst, int T, int64_t ncol, double ppr, int K) {
  const double per_cu = (double)(ceil_div(n_dst, T) * ncol) / (double)device_cus();
  const double rounds = 0.5 * (ceil(per_cu) + per_cu);
  return rounds * (T * ppr + 8.0 * K);
}
}  // namespace

extern "C" int32_t pcs_conv_pick_tile_rows_dt(int64_t n_dst, int64_t n_pairs, int32_t K, int32_t cin, int32_t cout,
                                              int32_t dtype) {
  if (n_dst <= 0 || K <= 0 || cin <= 0 || cout <= 0) return 128;
  if (!(dtype == 0 ? conv5_applies(cin, cout, K) : convh_applies(cin, cout, K))) return 128;
  if (conv_env().tile > 0) return conv_env().tile;
  const double ppr = (double)n_pairs / (double)n_dst;
  const int nctt = conv_nctt(cout);
  if (dtype != 0) {
    // 16-bit MFMA kernels: bound by the operand stream and, on the sparse levels, by the serial commit chain of a
    // workgroup -- two (or more) 4-wave workgroups per CU beat one tall 8-wave workgroup except on the >= 256-channel
    // deep levels, where the tall tile's lower padding and W reuse win (224 / 288 rows)
    if (cin >= 256 && cout >= 256) {
      // the weight-stationary kernel's chunked instances (conv_wave6h.hip) want two 4-wave workgroups per CU: 1.06-1.18x on 384
      // channels and on the small stride-16 level; 256 -> 256 on a big level stays on conv_os5h's tall 8-wave tile (0.97x)
      const ConvPlan ws = conv_route(ConvKind::half, dtype, cin, cout, K, 144, 0);
      if (ws.family == ConvFamily::wave6h && ws.kc > 1 && (cin > 256 || cout > 256 || n_dst <= 65536)) return 144;
      const int64_t ncol = ceil_div(cout, 16 * nctt);
      return launch_cost(n_dst, 288, ncol, ppr, K) <= launch_cost(n_dst, 224, ncol, ppr, K) ? 288 : 224;
    }
    // up to the tallest tile that fits twice per CU (192 rows at 96 columns, 144 at 128); below a few rounds of
    // workgroups the height that fills the last round
    const int64_t ncol = ceil_div(cout, 16 * nctt);
    const int tmax = nctt == 6 ? 192 : 144;
    int best = tmax;
    double best_cost = launch_cost(n_dst, tmax, ncol, ppr, K);
    for (int T = tmax - 16; T >= tmax - 48; T -= 16) {
      const double c = launch_cost(n_dst, T, ncol, ppr, K);
      if (c < best_cost * 0.97) { best = T; best_cost = c; }
    }
    return best;
  }
  if (conv5_nctt(cout, 192) <= 4) {
    // <= 64-column tiles (32 / 64 outputs, or >= 128 outputs as 64-column tiles): 192..288 rows, 2-3 workgroups per CU
    const int64_t ncol = ceil_div(cout, 16 * conv5_nctt(cout, 192));
    int best = 224;
    double best_cost = 0;
    for (int T = 192; T <= 288; T += 32) {
      const double c = launch_cost(n_dst, T, ncol, ppr, K);
      if (best_cost == 0 || c < best_cost) { best = T; best_cost = c; }
    }
    return best;
  }
  // 96-column tiles (and other shapes of six / eight 16-column tiles that are not multiples of 64)
  const int64_t ncol = ceil_div(cout, 16 * nctt);
  const int64_t slots = (int64_t)device_cus() * 2;
  // many rounds of workgroups and few pairs per row (strides 1/2: 4-5.5 pairs per row, 1.28-1.36x MFMA padding at
  // 128 rows): one 8-wave workgroup per CU on the tallest tile the LDS holds pads 1.12-1.17x
  if (ceil_div(n_dst, 128) * ncol >= 8 * slots && ppr < 6.5) {
    int T = 384;
    while (T > 128 && conv5_lds_est(T, nctt) > kMaxDynLds) T -= 32;
    if (T >= 192) return T;
  }
  int best = 128;
  double best_cost = launch_cost(n_dst, 128, ncol, ppr, K) * 0.97;
  for (int T = 80; T <= 192; T += 16) {
    if (T == 128) continue;
    if (conv_nw8(T, nctt)) continue;  // keep two workgroups per CU
    const double c = launch_cost(n_dst, T, ncol, ppr, K);
    if (c < best_cost) { best = T; best_cost = c; }
  }
  return best;
}

extern "C" int32_t pcs_conv_pick_tile_rows(int64_t n_dst, int64_t n_pairs, int32_t K, int32_t cin, int32_t cout) {
  return pcs_conv_pick_tile_rows_dt(n_dst, n_pairs, K, cin, cout, 0);
}

// 1 when the fused convolution of this shape can leave per-tile BatchNorm partial sums in its write-back (the wave
// kernels; the tile must hold the reduction scratch). dtype 0: fp32 kernels, 1 / 2: half kernels.
extern "C" int32_t pcs_conv_emits_bn_partials(int32_t cin, int32_t cout, int32_t K, int32_t tile_rows, int32_t dtype) {
  return conv_route(conv_kind_of(dtype), dtype, cin, cout, K, tile_rows, kConvStats).emits_stats;
}

// 1 when the fused convolution of this shape reads `tile_order` (the wave-autonomous kernels), whatever the tile height
extern "C" int32_t pcs_conv_uses_tile_order(int32_t cin, int32_t cout, int32_t K, int32_t dtype) {
  return conv_route(conv_kind_of(dtype), dtype, cin, cout, K, 128, kConvOrder).reads_order;
}

extern "C" int32_t pcs_conv_supports_epilogue(int32_t cin, int32_t cout, int32_t K, int32_t dtype) {
  return conv_route(conv_kind_of(dtype), dtype, cin, cout, K, 128, kConvExtras).takes_extras;
}

extern "C" int32_t pcs_conv_x3_emits_bn_partials(int32_t cin, int32_t cout, int32_t K, int32_t tile_rows) {
  return conv_route(ConvKind::x3, 0, cin, cout, K, tile_rows, kConvStats).emits_stats;
}

// measurement / test entry, not part of the contract: the plan a call of this kind, shape, height and flags (kConv* bits) runs on
extern "C" void pcs_debug_conv_plan(int32_t kind, int32_t dtype, int32_t cin, int32_t cout, int32_t K, int32_t tile_rows,
                                    int32_t flags, int32_t out[12]) {
  const ConvPlan p = conv_route((ConvKind)kind, dtype, cin, cout, K, tile_rows, flags);
  const int32_t v[12] = {(int32_t)p.family, p.nctt, p.ncoltiles, p.nt, p.tail, p.R, p.rs, p.kc, p.nt16, p.ns, (int32_t)p.lds,
                         (p.emits_stats ? 1 : 0) | (p.reads_order ? 2 : 0) | (p.takes_extras ? 4 : 0)};
  for (int i = 0; i < 12; ++i) out[i] = v[i];
}

extern "C" int pcs_conv_gather_gemm_f32(const float *src, int64_t n_src, int32_t cin,
                                        const float *W, int32_t K, int32_t cout,
                                        const int32_t *pairs, int32_t src_col,
                                        const int32_t *seg, int32_t tile_rows, int64_t n_dst,
                                        const float *bias, float *dst, double *bn_partial,
                                        const int32_t *tile_order, void *stream) {
  return pcs_conv_gather_gemm_f32_ex(src, n_src, cin, W, K, cout, pairs, src_col, seg, tile_rows, n_dst, bias, nullptr, dst,
                                     bn_partial, tile_order, stream);
}

extern "C" int pcs_conv_gather_gemm_f32_ex(const float *src, int64_t n_src, int32_t cin,
                                           const float *W, int32_t K, int32_t cout,
                                           const int32_t *pairs, int32_t src_col,
                                           const int32_t *seg, int32_t tile_rows, int64_t n_dst,
                                           const float *bias, const pcs_conv_epilogue *ep, float *dst, double *bn_partial,
                                           const int32_t *tile_order, void *stream) {
  const char *who = "pcs_conv_gather_gemm_f32";
  // no alignment rule: tensors off 16 bytes run on the generic kernel
  const int rc = conv_check_call(who, nullptr, cin, cout, K, n_src, n_dst, src_col, true, src, W, seg, dst, false, tile_rows);
  if (rc != PCS_OK || n_dst == 0) return rc;
  const void *addend = nullptr;
  float act_slope = 1.f;
  const float *post_scale = nullptr, *post_shift = nullptr;
  if (conv_decode_epilogue(ep, "pcs_conv_gather_gemm_f32_ex", 16, bn_partial != nullptr, addend, act_slope, post_scale, post_shift) != PCS_OK)
    return PCS_EINVAL;
  const bool extras = addend || act_slope != 1.f || post_scale;
  const bool aligned = (((uintptr_t)src | (uintptr_t)W | (uintptr_t)dst | (uintptr_t)bias) & 15) == 0;
  const ConvPlan p = conv_route(ConvKind::f32, 0, cin, cout, K, tile_rows, (bn_partial ? kConvStats : 0) | (tile_order ? kConvOrder : 0) |
                                (extras ? kConvExtras : 0) | (post_scale ? kConvPostAffine : 0) | (aligned ? 0 : kConvUnaligned));
  if (bn_partial && !p.emits_stats) return conv_no_stats(who);
  if (extras && !p.takes_extras) {
    set_error("pcs_conv_gather_gemm_f32_ex: this shape runs on the generic kernel, which takes no write-back extras (pcs_conv_supports_epilogue)");
    return PCS_EUNSUPPORTED;
  }
  ConvArgs a = conv_args<ConvArgs>(src, bias, dst, pairs, seg, n_dst, tile_rows, cin, cout, K, src_col, bn_partial, tile_order, p);
  a.W = W; a.addend = reinterpret_cast<const float *>(addend); a.act_slope = act_slope; a.post_scale = post_scale; a.post_shift = post_shift;
  hipStream_t st = as_stream(stream);
  if (p.family == ConvFamily::wave5) return launch_conv_wave5(a, p, st);
  if (tile_rows != 64 && tile_rows != 128) { set_error("%s: this shape takes tile_rows 64 or 128", who); return PCS_EUNSUPPORTED; }
  return p.family == ConvFamily::wave4 ? launch_conv_wave4(a, p, st) : launch_conv_block(a, p, st);
}
