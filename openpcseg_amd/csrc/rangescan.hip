// The range-view dataset's scan and its KNN label vote on the device -- gfx950, fp32, no host read.
// The reference runs the first per scan in the dataloader workers with NumPy (R:pcseg/data/dataset/semantickitti/laserscan.py:174-238
// do_range_projection, :389-400 do_label_projection; semantickitti_rv.py:284-334 the six input channels and the label remap) and the
// second per scan from about fifteen torch launches (R:pcseg/model/segmentor/range/utils.py:291-341 KNN.forward: two F.unfold tensors
// of search^2 x H W, a gather to search^2 x n, topk, two more gathers, scatter_add_ into a one-hot tensor, argmax).
//   range_scan_point_kernel   one lane per RAW point: depth, yaw, pitch and the pixel in the float32 chain of
//                             openpcseg_amd/rangescan.py (nothing contracted, arctan2 / arcsin in double rounded once), then ONE
//                             64-bit atomicMin of (float bits of depth << 32 | index within the frame) into winner[scene][y][x].
//                             Positive finite floats order as their bits, so the minimum is the contract's (depth, index) rule and
//                             does not depend on the order the atomics retire in. ~120 k points of a scan spread over 131 072
//                             pixels: no hot address.
//   range_scan_pixel_kernel   one lane per pixel: decodes the winner (its depth IS the high word) and writes the six input channels,
//                             the label through the optional table, the mask and proj_idx; consecutive lanes on consecutive
//                             addresses of every plane.
//   range_knn_vote_kernel<S>  one lane per point of the whole batch: S x S window reads of the (L2-resident) range and label images,
//                             the knn-of-S^2 selection and the vote in registers. Selection and counting are written as fully
//                             unrolled pairwise comparisons -- rank of a candidate = the candidates ahead of it in (distance,
//                             position) order; votes of a candidate's class = the selected candidates with its class -- so every
//                             array index is a compile-time constant and nothing goes to scratch. The optional confusion matrix is
//                             counted per workgroup in LDS and flushed with 64-bit atomic adds: lds_hist_* of raw_scan.h, shared
//                             with csrc/predict.hip, as is span_of (the frame or scene whose rows hold a point).
// Traffic per point at c = 4: the projection reads 16 B (+ 8 B of offsets, cached) and writes 12 B plus one atomic; the pixel pass
// reads 8 B and gathers 16 (+ 8) B per hit pixel and writes 40 B per pixel; the vote reads 12 B per point and S^2 x 12 B of the two
// images through the caches and writes 8 B.
#include <math.h>

#include "pcs_common.h"
#include "raw_scan.h"

using namespace pcs;

namespace {

constexpr int kBlock = 256;   // every kernel's launch bound AND its launch
static_assert(kBlock == kScanBlock, "lds_hist_clear / lds_hist_flush stride by kScanBlock: the workgroup must have as many lanes");
constexpr unsigned long long kEmptyPixel = ~0ULL;
constexpr int kMaxClass = 64;

bool image_sizes_ok(int32_t S, int32_t H, int32_t W) {
  return S >= 1 && H >= 1 && W >= 1 && (int64_t)S * H * W < ((int64_t)1 << 31);
}

struct ScanArgs {
  const float *points;
  int64_t n;
  int c;
  const int64_t *off;
  int F, H, W;
  float fov_down_abs, fov_total;
  const int64_t *labels, *lut;
  int lut_size, mask_hit;
  unsigned long long *winner;
  float *scan, *mask_rv, *unproj;
  int64_t *label_rv;
  int32_t *proj_idx, *px, *py, *bad;
};

__global__ void __launch_bounds__(kBlock) range_scan_point_kernel(ScanArgs a) {
#pragma clang fp contract(off)
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kBlock) {
    const float *row = a.points + i * a.c;
    const float x = row[0], y = row[1], z = row[2];
    float d = x * x;
    const float yy = y * y, zz = z * z;
    d = d + yy;
    d = d + zz;
    const float depth = sqrtf(d);
    const int f = span_of(a.off, a.F, i);
    const int64_t local = i - a.off[f];
    const float ratio = z / depth;
    // every comparison is false for a NaN: a row that is not finite anywhere fails here, before any address is formed. |z / depth|
    // exceeds 1 only where z * z went into the subnormals (x = y = 0, |z| ~ 1e-20): such a row has no pitch and is a bad row too.
    const bool ok = isfinite(x) && isfinite(y) && isfinite(z) && isfinite(depth) && depth > 0.f && fabsf(ratio) <= 1.0f && local >= 0 &&
                    local < ((int64_t)1 << 31) && i < a.off[f + 1];
    a.unproj[i] = depth;
    if (!ok) {
      a.px[i] = -1;
      a.py[i] = -1;
      *a.bad = 1;
      continue;
    }
    const float yaw = -(float)atan2((double)y, (double)x);
    const float pitch = (float)asin((double)ratio);
    float fx = yaw / kPiF;
    fx = fx + 1.0f;
    fx = 0.5f * fx;
    fx = fx * (float)a.W;
    float fy = pitch + a.fov_down_abs;
    fy = fy / a.fov_total;
    fy = 1.0f - fy;
    fy = fy * (float)a.H;
    fx = fmaxf(0.f, fminf((float)(a.W - 1), floorf(fx)));   // a NaN cannot arrive here; fmaxf would turn it into 0 all the same
    fy = fmaxf(0.f, fminf((float)(a.H - 1), floorf(fy)));
    const int ix = (int)fx, iy = (int)fy;
    a.px[i] = ix;
    a.py[i] = iy;
    const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)(uint32_t)local;
    atomicMin(a.winner + ((int64_t)f * a.H + iy) * a.W + ix, key);
  }
}

__global__ void __launch_bounds__(kBlock) range_scan_pixel_kernel(ScanArgs a) {
#pragma clang fp contract(off)
  const int64_t plane = (int64_t)a.H * a.W, pixels = plane * a.F;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * kBlock) {
    const int64_t s = p / plane, hw = p - s * plane;
    const unsigned long long key = a.winner[p];
    float x = -1.f, y = -1.f, z = -1.f, rem = -1.f, range = -1.f, mask = 0.f;
    int32_t idx = -1;
    int64_t label = 0;
    const int64_t r = a.off[s] + (int64_t)(key & 0xFFFFFFFFULL);
    if (key != kEmptyPixel && r >= 0 && r < a.n) {
      const float *row = a.points + r * a.c;
      x = row[0]; y = row[1]; z = row[2]; rem = row[3];
      range = __uint_as_float((uint32_t)(key >> 32));
      idx = (int32_t)(key & 0xFFFFFFFFULL);
      mask = (a.mask_hit || idx > 0) ? 1.f : 0.f;
      if (a.labels) {
        label = a.labels[r] & 0xFFFF;
        if (a.lut && label < a.lut_size) label = a.lut[label];
      }
    }
    float *dst = a.scan + s * 6 * plane + hw;
    dst[0] = x / 50.0f;
    dst[plane] = y / 50.0f;
    dst[2 * plane] = z / 3.0f;
    dst[3 * plane] = rem;
    dst[4 * plane] = range / 80.0f;
    dst[5 * plane] = mask;
    a.label_rv[p] = label;
    a.mask_rv[p] = mask;
    a.proj_idx[p] = idx;
  }
}

// ---- the vote ---------------------------------------------------------------------------------------------------------------------
struct VoteArgs {
  const float *range;        // (B, H, W)
  const int64_t *argmax;     // (B, H, W)
  int B, H, W;
  const float *unproj;
  const int32_t *px, *py;
  int64_t n;
  const int64_t *off;        // (B + 1) point boundaries
  int knn, num_class;
  float cutoff;
  const int64_t *labels;
  int64_t *hist, *pred;
  float w[49];               // 1 - gaussian, row-major; S * S entries used
};

template <int S>
__global__ void __launch_bounds__(kBlock) range_knn_vote_kernel(VoteArgs a) {
#pragma clang fp contract(off)
  constexpr int K = S * S, PAD = (S - 1) / 2, CENTRE = (K - 1) / 2;
  int32_t *lhist = lds_hist();   // num_class^2 cells when a.hist, else nothing
  const int nc = a.num_class, cells = a.hist ? nc * nc : 0;
  lds_hist_clear(lhist, cells);
  if (cells) __syncthreads();
  const int64_t plane = (int64_t)a.H * a.W;
  // ONE point per lane, no grid stride: in a loop the compiler keeps every kernel argument, the S * S weights among them, in scalar
  // registers across the iterations and spills them (102 for S = 7). The loop below runs once; it is a loop for its `continue`.
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  for (bool once = i < a.n; once; once = false) {
    const int b = span_of(a.off, a.B, i);
    const int px = a.px[i], py = a.py[i];
    // the pixel is checked before any address is formed; a bad point predicts 0 and is not counted
    if (!(i >= a.off[b] && i < a.off[b + 1] && px >= 0 && px < a.W && py >= 0 && py < a.H)) {
      a.pred[i] = 0;
      continue;
    }
    const float u = a.unproj[i];
    const float *img = a.range + b * plane;
    const int64_t *arg = a.argmax + b * plane;
    float d[K];
    int e[K];     // the candidate's bin: its pixel's label (-2 when the int64 value is no class), the extra bin num_class beyond the
                  // cutoff, -1 once not selected
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int yy = py + k / S - PAD, xx = px + k % S - PAD;
      float r = 0.f;
      int l = 0;
      if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) {   // zero padding, no azimuthal wrap
        r = img[(int64_t)yy * a.W + xx];
        const int64_t l64 = arg[(int64_t)yy * a.W + xx];
        l = (l64 >= 0 && l64 < nc) ? (int)l64 : -2;        // the range test on the whole 64 bits: 2^32 + 3 is not class 3
      }
      if (r < 0.f) r = INFINITY;
      if (k == CENTRE) r = u;
      float t = r - u;
      t = fabsf(t);
      d[k] = t * a.w[k];
      e[k] = l;
    }
    int rank[K];
#pragma unroll
    for (int k = 0; k < K; ++k) rank[k] = 0;
#pragma unroll
    for (int k = 1; k < K; ++k) {
#pragma unroll
      for (int j = 0; j < k; ++j) {
        const int ahead = d[j] <= d[k] ? 1 : 0;   // j < k: on equal distances the lower window position comes first
        rank[k] += ahead;
        rank[j] += 1 - ahead;
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      int bin = (a.cutoff > 0.f && d[k] > a.cutoff) ? nc : e[k];
      e[k] = rank[k] < a.knn ? bin : -1;
    }
    int cnt[K];
#pragma unroll
    for (int k = 0; k < K; ++k) cnt[k] = 1;
#pragma unroll
    for (int k = 1; k < K; ++k) {
#pragma unroll
      for (int j = 0; j < k; ++j) {
        const int same = e[j] == e[k] ? 1 : 0;
        cnt[k] += same;
        cnt[j] += same;
      }
    }
    // argmax over classes 1 .. nc - 1, the lowest class on equal counts: maximise count * 128 + (127 - class); no vote at all is
    // "count 0, class 1", what the reference's argmax over zeros gives
    int best = 126;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int score = (e[k] >= 1 && e[k] < nc) ? cnt[k] * 128 + (127 - e[k]) : 0;
      best = score > best ? score : best;
    }
    const int p = 127 - (best & 127);
    a.pred[i] = p;
    if (cells) lds_hist_count(lhist, nc, a.labels[i], p);
  }
  if (cells) {
    __syncthreads();
    lds_hist_flush(lhist, cells, a.hist);
  }
}

}  // namespace

extern "C" int64_t pcs_range_scan_ws_bytes(int32_t num_frames, int32_t H, int32_t W) {
  if (!image_sizes_ok(num_frames, H, W)) {
    set_error("pcs_range_scan_ws_bytes: bad sizes (frames >= 1, H >= 1, W >= 1, frames * H * W < 2^31)");
    return -1;
  }
  return (int64_t)num_frames * H * W * (int64_t)sizeof(unsigned long long);
}

extern "C" int pcs_range_scan_f32(const float *points, int64_t n, int32_t c, const int64_t *frame_offsets, int32_t num_frames,
                                  const int64_t *labels, const int64_t *lut, int32_t lut_size, int32_t H, int32_t W,
                                  float fov_down_abs, float fov_total, int32_t mask_hit, void *winner, float *scan,
                                  int64_t *label_rv, float *mask_rv, int32_t *proj_idx, int32_t *proj_x, int32_t *proj_y,
                                  float *unproj_range, int32_t *bad, void *stream) {
  if (!image_sizes_ok(num_frames, H, W) || c < 4 || n < 0 || n >= ((int64_t)1 << 31) || lut_size < 0 || !(fov_total > 0.f) ||
      !isfinite(fov_total) || !isfinite(fov_down_abs)) {
    set_error("pcs_range_scan_f32: bad args (0 <= n < 2^31, c >= 4, frames >= 1, H >= 1, W >= 1, frames * H * W < 2^31, "
              "lut_size >= 0, finite fov with a positive total)");
    return PCS_EINVAL;
  }
  if (!winner || !scan || !label_rv || !mask_rv || !proj_idx || !bad || !frame_offsets || (lut_size > 0 && !lut) ||
      (n > 0 && (!points || !proj_x || !proj_y || !unproj_range))) {
    set_error("pcs_range_scan_f32: null pointer");
    return PCS_EINVAL;
  }
  hipStream_t st = as_stream(stream);
  const int64_t pixels = (int64_t)num_frames * H * W;
  if (const int rc = fill_async("pcs_range_scan_f32", st, winner, 0xFF, (size_t)pixels * sizeof(unsigned long long))) return rc;
  if (const int rc = fill_async("pcs_range_scan_f32", st, bad, 0, sizeof(int32_t))) return rc;
  ScanArgs a;
  a.points = points; a.n = n; a.c = c; a.off = frame_offsets; a.F = num_frames; a.H = H; a.W = W;
  a.fov_down_abs = fov_down_abs; a.fov_total = fov_total;
  a.labels = labels; a.lut = lut_size > 0 ? lut : nullptr; a.lut_size = lut_size; a.mask_hit = mask_hit != 0;
  a.winner = reinterpret_cast<unsigned long long *>(winner);
  a.scan = scan; a.mask_rv = mask_rv; a.unproj = unproj_range; a.label_rv = label_rv; a.proj_idx = proj_idx;
  a.px = proj_x; a.py = proj_y; a.bad = bad;
  if (n > 0) {
    hipLaunchKernelGGL(range_scan_point_kernel, dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, st, a);
    const int rc = check_launch("pcs_range_scan_f32 (points)");
    if (rc != PCS_OK) return rc;
  }
  hipLaunchKernelGGL(range_scan_pixel_kernel, dim3(stream_grid(pixels, kBlock)), dim3(kBlock), 0, st, a);
  return check_launch("pcs_range_scan_f32 (pixels)");
}

extern "C" int pcs_range_knn_vote(const float *proj_range, const int64_t *proj_argmax, int32_t num_scenes, int32_t H, int32_t W,
                                  const float *unproj_range, const int32_t *proj_x, const int32_t *proj_y, int64_t n,
                                  const int64_t *point_offset, int32_t search, int32_t knn, float cutoff,
                                  const float *weights_host, int32_t num_class, const int64_t *labels, int64_t *hist,
                                  int64_t *pred, void *stream) {
  if (search != 3 && search != 5 && search != 7) {
    set_error("pcs_range_knn_vote: search must be 3, 5 or 7 (got %d)", (int)search);
    return PCS_EINVAL;
  }
  if (knn < 1 || knn > search * search) {
    set_error("pcs_range_knn_vote: 1 <= knn <= search^2 (got knn %d for search %d)", (int)knn, (int)search);
    return PCS_EINVAL;
  }
  if (!(cutoff >= 0.f)) {
    set_error("pcs_range_knn_vote: cutoff >= 0 (0 = off)");
    return PCS_EINVAL;
  }
  if (num_class < 2 || num_class > kMaxClass) {
    set_error("pcs_range_knn_vote: 2 <= num_class <= %d (got %d)", kMaxClass, (int)num_class);
    return PCS_EINVAL;
  }
  if (!image_sizes_ok(num_scenes, H, W) || n < 0 || n >= ((int64_t)1 << 31)) {
    set_error("pcs_range_knn_vote: bad sizes (0 <= n < 2^31, scenes >= 1, H >= 1, W >= 1, scenes * H * W < 2^31)");
    return PCS_EINVAL;
  }
  if (hist && !labels) {
    set_error("pcs_range_knn_vote: hist needs labels");
    return PCS_EINVAL;
  }
  if (!weights_host) {
    set_error("pcs_range_knn_vote: null pointer (weights)");
    return PCS_EINVAL;
  }
  if (n == 0) return PCS_OK;
  if (!proj_range || !proj_argmax || !unproj_range || !proj_x || !proj_y || !point_offset || !pred) {
    set_error("pcs_range_knn_vote: null pointer");
    return PCS_EINVAL;
  }
  VoteArgs a;
  a.range = proj_range; a.argmax = proj_argmax; a.B = num_scenes; a.H = H; a.W = W;
  a.unproj = unproj_range; a.px = proj_x; a.py = proj_y; a.n = n; a.off = point_offset;
  a.knn = knn; a.num_class = num_class; a.cutoff = cutoff; a.labels = labels; a.hist = hist; a.pred = pred;
  for (int k = 0; k < 49; ++k) a.w[k] = k < search * search ? weights_host[k] : 0.f;
  const size_t lds = hist ? (size_t)num_class * num_class * sizeof(int32_t) : 0;
  const dim3 grid((unsigned)ceil_div(n, kBlock)), block(kBlock);   // one point per lane
  hipStream_t st = as_stream(stream);
  if (search == 3)
    hipLaunchKernelGGL(range_knn_vote_kernel<3>, grid, block, lds, st, a);
  else if (search == 5)
    hipLaunchKernelGGL(range_knn_vote_kernel<5>, grid, block, lds, st, a);
  else
    hipLaunchKernelGGL(range_knn_vote_kernel<7>, grid, block, lds, st, a);
  return check_launch("pcs_range_knn_vote");
}
