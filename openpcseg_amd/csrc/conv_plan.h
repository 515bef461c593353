// Host side of the forward / input-gradient convolution, each decision made once: conv_env() reads the
// debug / A-B environment, conv_route() turns entry kind + shape + tile height + what the call carries into a ConvPlan that the
// entries launch from, the shape queries answer from and pcs_debug_conv_plan writes out; conv_prepared_geom() is the geometry of
// prepared weights, conv_check_call() / conv_args() the prologue the entries share. The launchers only pick a template instance.
#pragma once
#include "conv_wave_common.h"

namespace pcs {

// ---- environment -----------------------------------------------------------------------------------------------------------
struct ConvEnv {
  int tile;     // PCS_CONV_TILE: the picker returns this height for every wave-kernel shape
  int nctt;     // PCS_CONV_NCTT: wave5 column tiles of at most this many 16-column tiles (2 / 4 / 6 / 8)
  int nw;       // PCS_CONV_NW: wave5 workgroups of 8 waves (8) or 4 (any other value)
  int h_nctt;   // PCS_CONVH_NCTT: wave5h column tiles narrowed to this width where it divides cout (not with statistics)
  int h_r;      // PCS_CONVH_R: wave5h row blocks per group, 2 .. 4 (A/B; the TAIL and post-affine instances exist for 2 only)
  int x_r;      // PCS_CONVX_R: wave5x row blocks per group, 2 .. 4 (A/B; at most 3 at 96 columns)
  int ws;       // PCS_CONVH_WS: 0 wave5h for everything, 1 (default) wave6h where it measured faster, >= 2 wherever it has an instance
  int ws_debug = -1, ws_ab = 0;   // pcs_debug_convh_ws: mode override (-1 = PCS_CONVH_WS) and the two-row-block A/B instances
  int ws_mode() const { return ws_debug >= 0 ? ws_debug : ws; }
};
ConvEnv &conv_env();   // conv.hip

// ---- predicates the route is written in (conv_nctt, conv5_nctt, conv5_applies, convh_applies: conv_common.h) -------------------
// bf16x3: 16-column MFMA tiles per column tile: 2, 4 or 6 (>= 112 output columns as 64-column tiles)
__host__ __device__ inline int convx_nctt(int cout) {
  const int n = (cout + 15) / 16;
  if (n <= 2) return 2;
  if (n <= 4) return 4;
  if (n <= 6) return 6;
  return 4;
}
inline bool convx_applies(int cin, int cout, int K) {
  return cin % 8 == 0 && cin >= 32 && cout % 4 == 0 && cout >= 32 && K <= 32 && convx_nctt(cout) * 16 >= 32;
}

// The weight-stationary kernel's instances: X(nctt, ns, rs, kc, ab) = 16-column tiles per column tile, 32-channel steps of the
// layer, row blocks per sub-group, contraction chunks (the kernel holds ns / kc steps of weight fragments: ns / kc x nctt
// fragments of 4 registers stay resident next to rs x nctt accumulators and two sets of ns / kc x rs gathered pieces), ab = 1: an
// A/B instance, reached only through pcs_debug_convh_ws(.., rs = 1) (two row blocks: spills a few registers).
// kc > 1: 192 / 256 / 384 input channels on 128-column tiles, 192 / 256 on 96-column tiles.
#define PCS_CONV6H_INSTANCES(X)                                                                                                  \
  X(6, 3, 2, 1, 0) X(6, 4, 2, 1, 1) X(8, 3, 2, 1, 1) X(8, 4, 1, 1, 0) X(4, 2, 2, 1, 0) X(8, 2, 2, 1, 0) X(4, 4, 2, 1, 0)         \
  X(6, 2, 2, 1, 0) X(2, 2, 2, 1, 0) X(2, 1, 2, 1, 0) X(4, 1, 2, 1, 0) X(6, 1, 2, 1, 0) X(8, 1, 2, 1, 0) X(6, 4, 1, 1, 0)         \
  X(8, 3, 1, 1, 0) X(8, 8, 1, 2, 0) X(8, 12, 1, 3, 0) X(8, 6, 1, 2, 0) X(6, 6, 2, 2, 0) X(6, 8, 1, 2, 0)
struct Conv6hInstance { int nctt, ns, rs, kc, ab; };
inline const Conv6hInstance *conv6h_instance(int nctt, int ns, bool ab) {
#define PCS_CONV6H_ROW(N, S, R, KC, AB) {N, S, R, KC, AB},
  static constexpr Conv6hInstance table[] = {PCS_CONV6H_INSTANCES(PCS_CONV6H_ROW)};
  for (const auto &e : table)
    if (e.nctt == nctt && e.ns == ns && e.ab == (int)ab) return &e;
  return ab ? conv6h_instance(nctt, ns, false) : nullptr;
}
inline bool conv6h_applies(int cin, int cout, int K) {
  if (!convh_applies(cin, cout, K) || cin % 32) return false;
  const Conv6hInstance *e = conv6h_instance(conv_nctt(cout), cin / 32, false);
  if (!e) return false;
  const int nctt = e->nctt, ns = e->ns;
  if (conv_env().ws_mode() >= 2 || e->kc > 1) return true;
  // measured on the 12-frame bench maps (profiles/round6_convh_ws.md): 1.2-1.3x on the 64 ... 128-channel layers; the thin
  // shapes (<= 2 weight fragments per step and tile, or one step) stay on conv_wave5h.hip
  // chunked contractions (192 ... 384 input channels): 1.06-1.26x on 4-wave workgroups (tiles <= 160 rows, two per CU), 0.6-0.8x on
  // the 8-wave ones -- the route sends only tiles of <= 160 rows there, the picker (conv.hip) asks for 144 rows where that pays
  // (everything but 256 -> 256 on the big stride-8 level: 0.97x)
  if (K <= 8) return ns * nctt >= 16 && ns >= 3;   // k = 2 strided / transposed maps: one pair per row and offset
  return ns * nctt >= 8 && ns >= 2 && !(nctt == 8 && ns == 2);
}

// ---- prepared weights ------------------------------------------------------------------------------------------------------
// nt16 16-column tiles (whole column tiles of nctt) x ns 32-channel steps of 1 KB blocks per offset and plane; x3: three planes
struct ConvPreparedGeom { int nctt, nt16, ns; size_t plane_bytes, bytes; };   // bytes: per offset, of one plane and of all
inline ConvPreparedGeom conv_prepared_geom(int ccon, int ccols, bool x3) {
  ConvPreparedGeom g;
  g.nctt = x3 ? convx_nctt(ccols) : conv_nctt(ccols);
  g.nt16 = (int)ceil_div(ccols, 16 * g.nctt) * g.nctt;
  g.ns = (int)ceil_div(ccon, 32);
  g.plane_bytes = (size_t)g.nt16 * g.ns * 1024;
  g.bytes = (x3 ? 3 : 1) * g.plane_bytes;
  return g;
}

// ---- the plan --------------------------------------------------------------------------------------------------------------
enum class ConvKind { f32 = 0, half = 1, x3 = 2 };   // the three entries
enum class ConvFamily { none = 0, block, wave4, wave5, wave5h, wave6h, wave5x };   // none: the entry does not serve the shape
// what the call carries (pcs_debug_conv_plan takes the same bits)
enum : int { kConvStats = 1, kConvOrder = 2, kConvExtras = 4, kConvPostAffine = 8, kConvUnaligned = 16 };

struct ConvPlan {
  ConvFamily family = ConvFamily::none;
  int dtype = 0;                // 0 fp32, 1 bf16, 2 fp16 storage
  int nctt = 0, ncoltiles = 0;  // 16-column units per column tile (block: 32 cg columns = 2 cg units), column tiles per row tile
  int nt = 0;                   // threads per workgroup
  int tail = 0, R = 1;          // cin % 32 != 0 (TAIL instances); row blocks per group
  int rs = 0, kc = 0;           // wave6h: row blocks per sub-group, contraction chunks
  int nt16 = 0, ns = 0;         // conv_prepared_geom (half, x3)
  size_t lds = 0;
  bool vec = false;             // fp32: 16-byte-granular rows on aligned tensors (block: its VEC instance)
  bool emits_stats = false, reads_order = false, takes_extras = false;   // at this height / for this shape
};
// tile_rows is taken as given (conv_check_call holds its rules; the wave launch refuses a tile that exceeds the LDS)
ConvPlan conv_route(ConvKind kind, int dtype, int cin, int cout, int K, int tile_rows, int flags);   // conv.hip
inline ConvKind conv_kind_of(int dtype) { return dtype == 0 ? ConvKind::f32 : ConvKind::half; }

// ---- the checked prologue of the entries -----------------------------------------------------------------------------------
// PCS_OK: go on, or n_dst == 0 and there is nothing to launch. `unserved`: the entry's text when the route found no family.
inline int conv_check_call(const char *who, const char *unserved, int cin, int cout, int K, int64_t n_src, int64_t n_dst, int src_col,
                           bool dtype_ok, const void *src, const void *W, const void *seg, const void *dst, bool misaligned,
                           int tile_rows) {
  if (cin <= 0 || cout <= 0 || K <= 0 || n_dst < 0 || n_src < 0 || (src_col != 0 && src_col != 1) || !dtype_ok) {
    set_error("%s: bad sizes", who);
    return PCS_EINVAL;
  }
  if (unserved) { set_error("%s: %s", who, unserved); return PCS_EUNSUPPORTED; }
  if (n_dst == 0) return PCS_OK;
  if (!W || !seg || !dst || (n_src > 0 && !src)) { set_error("%s: null pointer", who); return PCS_EINVAL; }
  if (misaligned) { set_error("%s: misaligned pointer", who); return PCS_EINVAL; }
  if (tile_rows < 16 || tile_rows > 512 || tile_rows % 16) { set_error("%s: tile_rows must be a multiple of 16 in [16, 512]", who); return PCS_EINVAL; }
  return PCS_OK;
}

inline int conv_no_stats(const char *who) {
  set_error("%s: this shape / tile height does not produce BatchNorm partials (ask the entry's emits_bn_partials query)", who);
  return PCS_EUNSUPPORTED;
}

// the fields ConvArgs, ConvArgsH and ConvArgsX share (their layouts stay their own: profiles/conv_skeleton_refactor.md)
template <typename Args>
Args conv_args(const void *src, const float *bias, void *dst, const int32_t *pairs, const int32_t *seg, int64_t n_dst, int tile_rows,
               int cin, int cout, int K, int src_col, double *stats, const int32_t *order, const ConvPlan &p) {
  Args a;
  a.src = static_cast<decltype(a.src)>(src); a.bias = bias; a.dst = static_cast<decltype(a.dst)>(dst); a.pairs = pairs; a.seg = seg;
  a.n_dst = n_dst; a.ntiles = ceil_div(n_dst, tile_rows); a.tile_rows = tile_rows;
  a.cin = cin; a.cout = cout; a.K = K; a.src_col = src_col; a.ncoltiles = p.ncoltiles; a.stats = stats; a.order = order;
  return a;
}

// One launch of a wave kernel from its plan: grid (padded to 8 * ncoltiles for the round-robin deal of an ordered launch), the
// checks, the once-only attribute of this kernel instance (the function is a template on the kernel pointer), `pre(nblocks)` right
// before the launch (trace preparation, debug prints). `who` heads the error texts, `label` names the launch to check_launch.
template <auto Kern, typename Args, typename Pre = void (*)(int64_t)>
int conv_wave_launch(const Args &a, const ConvPlan &p, hipStream_t st, const char *who, const char *label, Pre pre = [](int64_t) {}) {
  const bool pad8 = a.order != nullptr && p.family != ConvFamily::wave4;   // conv_os4_kernel ignores the order: unpadded grid
  const int64_t nblocks = pad8 ? ceil_div(a.ntiles, 8) * 8 * a.ncoltiles : a.ntiles * a.ncoltiles;
  if (nblocks <= 0) return PCS_OK;
  if (nblocks > 0x7FFFFFFF) { set_error("%s: grid too large", who); return PCS_EUNSUPPORTED; }
  if (p.lds > kMaxDynLds) { set_error("%s: tile_rows too large for this column tile", who); return PCS_EUNSUPPORTED; }
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxDynLds);
    attr_set = true;
  }
  pre(nblocks);
  hipLaunchKernelGGL(Kern, dim3((unsigned)nblocks), dim3(p.nt), p.lds, st, a);
  return check_launch(label);
}

// launchers: the switch from plan values to a template instance
int launch_conv_block(const ConvArgs &a, const ConvPlan &p, hipStream_t st);   // any shape; tile_rows 64 / 128
int launch_conv_wave4(const ConvArgs &a, const ConvPlan &p, hipStream_t st);   // cin % 4 == 0, cout % 4 == 0, K <= 32; tile_rows 64 / 128
int launch_conv_wave5(const ConvArgs &a, const ConvPlan &p, hipStream_t st);   // conv5_applies(); any tile_rows % 16 == 0

}  // namespace pcs
