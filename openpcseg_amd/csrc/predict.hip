// Prediction tail of an evaluation pass on the device -- gfx950, one launch per batch, no host synchronisation.
// The reference maps voxel logits back to points scene by scene on the host
// (R:pcseg/model/segmentor/voxel/minkunet/minkunet.py:436-455: three boolean masks, two gathers that materialise
// (points, classes), argmax or softmax, .cpu() per scene) and scores them with np.bincount (R:infer.py:35-52 fast_hist).
// Here, per point i of scene b: row = row_offset[b] + inverse[i];
//   votes[i] += softmax(logits[row])      (optional: the reference's return_tta output, summed over passes)
//   pred[i]   = first arg-max of votes[i] (vote mode) or of logits[row]
//   hist[labels[i]][pred[i]] += 1         for labels in [0, c)  (fast_hist's mask)
// One thread per point, 16-byte row loads when c % 4 == 0. The confusion matrix is counted per workgroup in LDS (int32, c * c
// cells: 1.6 KB at c = 20) and flushed once per workgroup with 64-bit global atomic adds of the non-zero cells: integer sums,
// so the result is exact and identical from run to run (lds_hist_* of raw_scan.h, shared with the KNN vote of rangescan.hip, as is
// span_of: the scene whose span holds a point). A row outside its scene is refused BEFORE an address is formed.
#include <math.h>

#include "pcs_common.h"
#include "raw_scan.h"

using namespace pcs;

namespace {

constexpr int kBlock = 256;   // the kernel's launch bound AND its launch
static_assert(kBlock == kScanBlock, "lds_hist_clear / lds_hist_flush stride by kScanBlock: the workgroup must have as many lanes");

struct PredictArgs {
  const float *logits;
  int64_t m;
  int c;
  const int64_t *inverse;
  int64_t n;
  const int64_t *point_offset, *row_offset;
  int n_scenes;
  const int64_t *labels;
  float *votes;
  int64_t *pred;
  int64_t *hist;
  int32_t *bad;
};

// first arg-max of x[0..c) (+ v[0..c) when ADD), VEC: 16-byte pieces
template <bool VEC>
__device__ __forceinline__ int row_argmax(const float *__restrict__ x, int c) {
  float bv = x[0];
  int bj = 0;
  if (VEC) {
    for (int j = 0; j < c; j += 4) {
      const float4 q = *reinterpret_cast<const float4 *>(x + j);
      if (q.x > bv) { bv = q.x; bj = j; }
      if (q.y > bv) { bv = q.y; bj = j + 1; }
      if (q.z > bv) { bv = q.z; bj = j + 2; }
      if (q.w > bv) { bv = q.w; bj = j + 3; }
    }
  } else {
    for (int j = 1; j < c; ++j) {
      const float v = x[j];
      if (v > bv) { bv = v; bj = j; }
    }
  }
  return bj;
}

// v[0..c) += softmax(x[0..c)) in fp32 (maximum subtracted); returns the first arg-max of the updated v
template <bool VEC>
__device__ __forceinline__ int row_vote(const float *__restrict__ x, float *__restrict__ v, int c) {
  float mx = x[0], sum = 0.f;
  if (VEC) {
    for (int j = 0; j < c; j += 4) {
      const float4 q = *reinterpret_cast<const float4 *>(x + j);
      mx = fmaxf(fmaxf(mx, fmaxf(q.x, q.y)), fmaxf(q.z, q.w));
    }
    for (int j = 0; j < c; j += 4) {
      const float4 q = *reinterpret_cast<const float4 *>(x + j);
      sum += expf(q.x - mx); sum += expf(q.y - mx); sum += expf(q.z - mx); sum += expf(q.w - mx);
    }
  } else {
    for (int j = 1; j < c; ++j) mx = fmaxf(mx, x[j]);
    for (int j = 0; j < c; ++j) sum += expf(x[j] - mx);
  }
  float bv = -INFINITY;
  int bj = 0;
  if (VEC) {
    for (int j = 0; j < c; j += 4) {
      const float4 q = *reinterpret_cast<const float4 *>(x + j);
      float4 a = *reinterpret_cast<const float4 *>(v + j);
      a.x += expf(q.x - mx) / sum; a.y += expf(q.y - mx) / sum; a.z += expf(q.z - mx) / sum; a.w += expf(q.w - mx) / sum;
      *reinterpret_cast<float4 *>(v + j) = a;
      if (a.x > bv) { bv = a.x; bj = j; }
      if (a.y > bv) { bv = a.y; bj = j + 1; }
      if (a.z > bv) { bv = a.z; bj = j + 2; }
      if (a.w > bv) { bv = a.w; bj = j + 3; }
    }
  } else {
    for (int j = 0; j < c; ++j) {
      const float a = v[j] + expf(x[j] - mx) / sum;
      v[j] = a;
      if (a > bv) { bv = a; bj = j; }
    }
  }
  return bj;
}

template <bool VEC>
__global__ void __launch_bounds__(kBlock) predict_points_kernel(PredictArgs a) {
  int32_t *lhist = lds_hist();   // c * c cells when a.hist, else nothing
  const int c = a.c, cells = a.hist ? c * c : 0;
  lds_hist_clear(lhist, cells);
  if (cells) __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = a.inverse ? a.inverse[i] : i;
    int64_t base = 0, rows = a.m;
    bool ok = true;
    if (a.n_scenes > 0) {
      const int lo = span_of(a.point_offset, a.n_scenes, i);   // the scene whose point span holds i
      ok = i >= a.point_offset[lo] && i < a.point_offset[lo + 1];
      base = a.row_offset[lo];
      rows = a.row_offset[lo + 1] - base;
    }
    // range first, address second: nothing outside logits is ever read
    ok = ok && r >= 0 && r < rows && base >= 0 && base + r < a.m;
    int p = -1;
    if (ok) {
      const float *x = a.logits + (base + r) * c;
      p = a.votes ? row_vote<VEC>(x, a.votes + i * c, c) : row_argmax<VEC>(x, c);
    } else {
      atomicOr(a.bad, 1);
    }
    if (a.pred) a.pred[i] = p;
    if (cells && p >= 0) lds_hist_count(lhist, c, a.labels[i], p);
  }
  if (cells) {
    __syncthreads();
    lds_hist_flush(lhist, cells, a.hist);
  }
}

}  // namespace

extern "C" int pcs_predict_points_f32(const float *logits, int64_t m, int32_t c, const int64_t *inverse, int64_t n,
                                      const int64_t *point_offset, const int64_t *row_offset, int32_t n_scenes,
                                      const int64_t *labels, float *votes, int64_t *pred, int64_t *hist, int32_t *bad_flag,
                                      void *stream) {
  if (n < 0 || m < 0 || c <= 0 || c > 64 || n_scenes < 0) { set_error("pcs_predict_points_f32: bad sizes (1 <= c <= 64)"); return PCS_EINVAL; }
  if (n_scenes > 0 && (!point_offset || !row_offset)) { set_error("pcs_predict_points_f32: n_scenes > 0 needs point_offset and row_offset"); return PCS_EINVAL; }
  if (!inverse && n_scenes == 0 && n != m) { set_error("pcs_predict_points_f32: without an inverse map n must equal m"); return PCS_EINVAL; }
  if (!inverse && n_scenes > 0) { set_error("pcs_predict_points_f32: scene offsets need an inverse map"); return PCS_EINVAL; }
  if (!votes && !pred && !hist) { set_error("pcs_predict_points_f32: nothing to compute (votes, pred and hist are all NULL)"); return PCS_EINVAL; }
  if (hist && !labels) { set_error("pcs_predict_points_f32: hist needs labels"); return PCS_EINVAL; }
  if (n == 0) return PCS_OK;
  if (!bad_flag || (m > 0 && !logits)) { set_error("pcs_predict_points_f32: null pointer"); return PCS_EINVAL; }
  PredictArgs a;
  a.logits = logits; a.m = m; a.c = c; a.inverse = inverse; a.n = n;
  a.point_offset = n_scenes > 0 ? point_offset : nullptr; a.row_offset = n_scenes > 0 ? row_offset : nullptr; a.n_scenes = n_scenes;
  a.labels = labels; a.votes = votes; a.pred = pred; a.hist = hist; a.bad = bad_flag;
  const bool vec = c % 4 == 0 && (((uintptr_t)logits | (uintptr_t)votes) & 15) == 0;
  const size_t lds = hist ? (size_t)c * c * sizeof(int32_t) : 0;
  const dim3 grid(stream_grid(n, kBlock)), block(kBlock);
  if (vec)
    hipLaunchKernelGGL(predict_points_kernel<true>, grid, block, lds, as_stream(stream), a);
  else
    hipLaunchKernelGGL(predict_points_kernel<false>, grid, block, lds, as_stream(stream), a);
  return check_launch("pcs_predict_points_f32");
}
