// The skeleton of the kernels over a raw batch, each piece defined once:
//   scantransform.hip, cylscan.hip, scanmix.hip (rows of frames under parameter rows), rangescan.hip, rangeproj.hip (range views)
//   and predict.hip (the voted prediction tail, which shares the span search and the confusion matrix with the KNN vote).
// The clamped row range of a frame, the raw row load, the V parameter rows in LDS, the float64 affine map of one row (section 7h),
// the chip-sized grid along a frame with the dispatch over the compiled vote bound, the span search, the per-workgroup confusion
// matrix and float32(pi). The .hip files keep what is theirs: the azimuth chains (range_column, ring_proj_x, row_buckets,
// cyl_cell and the yaw of range_scan_point_kernel restate different reference functions, each pinned to its own fixture), their
// stores and their reductions. Everything here is inlined into its caller.
// These kernels are register-sensitive, so a piece is shared with a kernel only where every instance keeps its spills, scratch, LDS
// and occupancy (tools/conv_static_ab.py; the table is in profiles/scan_kernels_refactor.md). Every instance does today. A kernel
// that loses them to a later change keeps the piece inline, with a comment that points here.
#pragma once
#include <type_traits>

#include "pcs_common.h"

namespace pcs {

constexpr int kScanBlock = 256;
constexpr int kScanMaxExtra = PCS_SCAN_MAX_COLUMNS - 3;
constexpr float kPiF = 3.14159265358979323846f;      // float32(np.pi) = 3.1415927410125732
constexpr float kTwoPiF = 6.28318530717958647692f;   // float32(2 * np.pi)

// ---- rows of a frame --------------------------------------------------------------------------------------------------------
struct FrameRows { int64_t lo, hi; };

// rows [lo, hi) of frame f with 0 <= lo <= hi <= n: nothing outside the n rows is ever addressed, whatever the offsets say
__device__ __forceinline__ FrameRows frame_rows(const int64_t *__restrict__ offsets, int f, int64_t n) {
  FrameRows r = {offsets[f], offsets[f + 1]};
  r.lo = r.lo < 0 ? 0 : (r.lo > n ? n : r.lo);
  r.hi = r.hi > n ? n : r.hi;
  if (r.hi < r.lo) r.hi = r.lo;
  return r;
}

struct RawRow { float x, y, z, extra[kScanMaxExtra]; };   // the columns past the C of the batch are 0

// ROW16: C == 4 and `pts` 16-byte aligned -- one 16-byte load
template <bool ROW16>
__device__ __forceinline__ RawRow load_raw_row(const float *__restrict__ pts, int64_t i, int C) {
  RawRow r;
  if (ROW16) {
    const float4 q = *reinterpret_cast<const float4 *>(pts + i * 4);
    r.x = q.x; r.y = q.y; r.z = q.z; r.extra[0] = q.w;
#pragma unroll
    for (int k = 1; k < kScanMaxExtra; ++k) r.extra[k] = 0.f;
  } else {
    const float *p = pts + i * C;
    r.x = p[0]; r.y = p[1]; r.z = p[2];
#pragma unroll
    for (int k = 0; k < kScanMaxExtra; ++k) r.extra[k] = 3 + k < C ? p[3 + k] : 0.f;
  }
  return r;
}

// the V parameter rows (cos, sin, scale, sx, sy, jx, jy, jz) of frame f, vote-major in `params`, into sp[V * 8]; the caller owns
// the barrier
__device__ __forceinline__ void stage_params(double *sp, const double *__restrict__ params, int V, int F, int f) {
  for (int j = threadIdx.x; j < V * 8; j += kScanBlock) sp[j] = params[((int64_t)(j >> 3) * F + f) * 8 + (j & 7)];
}

// One row under one parameter row. Contraction is switched off for this body: a fused multiply-add skips the rounding of the
// product that NumPy's float64 arithmetic performs, and the float32 result can then differ in its last bit.
__device__ __forceinline__ void affine_row(float x, float y, float z, const double *__restrict__ p, float &fx, float &fy, float &fz) {
#pragma clang fp contract(off)
  const double c = p[0], s = p[1], scale = p[2];
  const double xd = (double)x, yd = (double)y;
  const double a = xd * c, b = yd * (-s);
  const double d = xd * s, e = yd * c;
  double X = a + b, Y = d + e, Z = (double)z;
  X = X * scale; Y = Y * scale; Z = Z * scale;
  X = X * p[3]; Y = Y * p[4];
  X = X + p[5]; Y = Y + p[6]; Z = Z + p[7];
  fx = (float)X; fy = (float)Y; fz = (float)Z;
}

// ---- launch shape -----------------------------------------------------------------------------------------------------------
// workgroups along a frame: `chip` workgroups shared among the other grid axes, never more than the rows can use
inline int frame_grid(int64_t n, int64_t per_row, int64_t others, int64_t chip) {
  int64_t g = chip / others;
  const int64_t most = ceil_div(n * per_row, kScanBlock);
  if (g > most) g = most;
  return (int)(g < 1 ? 1 : g);
}

// the voted kernels': 256 CUs x 4 workgroups of the light instances (<= 4 votes), x 2 of the heavy ones (2 waves per SIMD fit)
inline int vote_grid(int64_t n, int num_frames, int num_votes) { return frame_grid(n, 1, num_frames, num_votes <= 4 ? 1024 : 512); }

inline bool scan_sizes_ok(int64_t n, int32_t num_frames, int32_t num_votes) {
  return n >= 0 && num_votes >= 1 && num_votes <= PCS_SCAN_MAX_VOTES && num_frames >= 1 && num_frames <= 65535;
}

// The compiled bound VB of a kernel's vote loop (num_votes <= VB) and its row form: launch(vb, row16) is called once with two
// std::integral_constant, so the caller names its instance as kernel<decltype(vb)::value, decltype(row16)::value>.
template <typename Launch>
inline void dispatch_votes(int num_votes, bool row16, Launch &&launch) {
  auto rows = [&](auto vb) {
    if (row16) launch(vb, std::true_type{});
    else launch(vb, std::false_type{});
  };
  if (num_votes == 1) rows(std::integral_constant<int, 1>{});
  else if (num_votes <= 4) rows(std::integral_constant<int, 4>{});
  else if (num_votes <= 10) rows(std::integral_constant<int, 10>{});
  else rows(std::integral_constant<int, PCS_SCAN_MAX_VOTES>{});
}

// ---- points of scenes -------------------------------------------------------------------------------------------------------
// the span that holds i: the last b < count with off[b] <= i (off ascending). Whether i really lies inside is the caller's test.
__device__ __forceinline__ int span_of(const int64_t *__restrict__ off, int count, int64_t i) {
  int lo = 0, hi = count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// The confusion matrix of a launch, counted per workgroup (kScanBlock lanes) in dynamic LDS -- int32, nc * nc cells -- and flushed
// once with 64-bit global atomic adds of the non-zero cells: integer sums, exact and identical from run to run. The caller owns
// the barriers after the clear and before the flush.
__device__ __forceinline__ int32_t *lds_hist() {
  extern __shared__ int32_t lhist[];
  return lhist;
}

__device__ __forceinline__ void lds_hist_clear(int32_t *lhist, int cells) {
  for (int j = threadIdx.x; j < cells; j += kScanBlock) lhist[j] = 0;
}

// fast_hist's mask: a label outside [0, nc) is not counted
__device__ __forceinline__ void lds_hist_count(int32_t *lhist, int nc, int64_t label, int pred) {
  if (label >= 0 && label < nc) atomicAdd(&lhist[(int)label * nc + pred], 1);
}

__device__ __forceinline__ void lds_hist_flush(const int32_t *lhist, int cells, int64_t *hist) {
  for (int j = threadIdx.x; j < cells; j += kScanBlock) {
    const int32_t v = lhist[j];
    if (v) atomicAdd(reinterpret_cast<unsigned long long *>(hist) + j, (unsigned long long)v);
  }
}

}  // namespace pcs
