// The fusion dataset's range view of a collated batch on the device -- gfx950, fp32, two launches, no
// host read. The reference runs it per frame and per vote in the dataloader workers with NumPy
// (R:pcseg/data/dataset/semantickitti/semantickitti_fusion.py:64-114 get_range_image, :198-245 the collates' range_pxpy table):
// the frame's DEDUPLICATED voxel rows (lidar.F, not the raw points) are projected onto an H x W image, the azimuth shifted by a
// random cut, and `image[iy, ix] = value` in row order leaves the LAST row that hits a pixel in it.
//   range_project_kernel   one lane per voxel row: the float32 azimuth chain of openpcseg_amd/rangeview.py (arctan2 in double
//                          rounded once, as cyl_cell.h), the pxpy row, and atomicMax(winner[scene][iy][ix], row). The maximum does
//                          not depend on the order the atomics retire in, and rows of a scene ascend in the collate's order, so it
//                          IS the reference's last write: the image is bit-reproducible. ~92 k rows of a scene spread over 131 072
//                          pixels: no hot address.
//   range_fill_kernel      pixel-major: a lane reads the winners of four consecutive pixels (one 16-byte load), gathers the winning
//                          rows and writes the five planes with 16-byte stores, consecutive lanes on consecutive addresses. A scalar
//                          instance serves a W that is no multiple of four.
// Traffic per scene at 64 x 2048, c = 5: the projection reads 4 c + 4 B and writes 12 B per row plus one atomic; the fill reads
// 0.5 MB of winners and the gathered rows and writes 2.6 MB.
#include <math.h>

#include "pcs_common.h"
#include "raw_scan.h"   // kPiF, kTwoPiF

using namespace pcs;

namespace {

constexpr int kBlock = kScanBlock;

bool range_sizes_ok(int32_t S, int32_t H, int32_t W) {
  return S >= 1 && H >= 2 && W >= 2 && (int64_t)S * H * W < ((int64_t)1 << 31);
}

// (x, y) under the scene's cut -> the column as a float (already rounded to an integer value). Contraction is switched off for
// this body: NumPy rounds every product, quotient and sum of the chain on its own (DESIGN.md section 7h gives the reason).
__device__ __forceinline__ float range_column(float x, float y, float cut, int W) {
#pragma clang fp contract(off)
  float yaw = (float)atan2((double)y, (double)(-x));
  yaw = yaw + cut;
  float r = fmodf(yaw, kTwoPiF);     // exact; NumPy's remainder then moves a negative result up by the (positive) divisor
  if (r < 0.f) r = r + kTwoPiF;      // may give exactly float32(2 pi) for a tiny negative yaw: column W - 1
  yaw = r - kPiF;
  float p = yaw / kPiF;
  p = p + 1.0f;
  p = 0.5f * p;
  p = p * (float)(W - 1);
  return rintf(p);
}

__device__ __forceinline__ float norm_coord(float rounded, int extent) {
#pragma clang fp contract(off)
  double v = (double)rounded / (double)(extent - 1);   // the rounded integer / (extent - 1), float64 as the reference's
  v = v - 0.5;
  v = 2.0 * v;
  return (float)v;
}

__global__ void __launch_bounds__(kBlock) range_project_kernel(const float *__restrict__ feats, int64_t n, int c,
                                                               const int32_t *__restrict__ scenes, const float *__restrict__ cuts,
                                                               int S, int H, int W, int32_t *__restrict__ winner,
                                                               float *__restrict__ pxpy, int32_t *__restrict__ bad) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const float *row = feats + i * c;
    const float x = row[0], y = row[1], ring = row[4];
    const int s = scenes[i];
    const bool scene_ok = s >= 0 && s < S;
    const float cut = scene_ok ? cuts[s] : 0.f;
    const float fx = range_column(x, y, cut, W);
    const float fy = rintf(ring);
    float *o = pxpy + i * 3;
    o[0] = (float)s;
    o[1] = norm_coord(fx, W);
    o[2] = norm_coord(fy, H);
    // every comparison is false for a NaN: a row that is not finite anywhere in the chain fails here, before any address is formed
    const bool ok = scene_ok && isfinite(x) && isfinite(y) && fy >= 0.f && fy <= (float)(H - 1) && fx >= 0.f && fx <= (float)(W - 1);
    if (ok)
      atomicMax(winner + ((int64_t)s * H + (int)fy) * W + (int)fx, (int32_t)i);
    else
      *bad = 1;
  }
}

struct Pixel {
  float ch[5];
};

__device__ __forceinline__ Pixel range_pixel(const float *__restrict__ feats, int64_t n, int c, int32_t w) {
#pragma clang fp contract(off)
  Pixel p;
  if (w < 0 || (int64_t)w >= n) {   // the empty pixel: 25 (0 - 0.4), 20 (0 - 0.5), 0, 0, 0
    p.ch[0] = -10.f; p.ch[1] = -10.f; p.ch[2] = 0.f; p.ch[3] = 0.f; p.ch[4] = 0.f;
    return p;
  }
  const float *row = feats + (int64_t)w * c;
  const float x = row[0], y = row[1], z = row[2], refl = row[3];
  float d = x * x;
  const float yy = y * y, zz = z * z;
  d = d + yy;
  d = d + zz;
  const float inv = 1.0f / sqrtf(d);
  double a = (double)inv - 0.4;
  a = 25.0 * a;
  double b = (double)refl - 0.5;
  b = 20.0 * b;
  p.ch[0] = (float)a; p.ch[1] = (float)b; p.ch[2] = x; p.ch[3] = y; p.ch[4] = z;
  return p;
}

// VEC: four pixels per lane (H * W % 4 == 0, so a group of four never leaves its scene; winner and image 16-byte aligned)
template <bool VEC>
__global__ void __launch_bounds__(kBlock) range_fill_kernel(const int32_t *__restrict__ winner, const float *__restrict__ feats,
                                                            int64_t n, int c, int64_t pixels, int64_t plane,
                                                            float *__restrict__ image) {
  constexpr int kPer = VEC ? 4 : 1;
  const int64_t groups = pixels / kPer;
  for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kBlock) {
    const int64_t p0 = g * kPer;
    const int64_t s = p0 / plane, hw = p0 - s * plane;
    float *dst = image + s * 5 * plane + hw;
    if (VEC) {
      const int4 w = *reinterpret_cast<const int4 *>(winner + p0);
      const Pixel a = range_pixel(feats, n, c, w.x), b = range_pixel(feats, n, c, w.y), cpx = range_pixel(feats, n, c, w.z),
                  d = range_pixel(feats, n, c, w.w);
#pragma unroll
      for (int k = 0; k < 5; ++k)
        *reinterpret_cast<float4 *>(dst + k * plane) = make_float4(a.ch[k], b.ch[k], cpx.ch[k], d.ch[k]);
    } else {
      const Pixel a = range_pixel(feats, n, c, winner[p0]);
#pragma unroll
      for (int k = 0; k < 5; ++k) dst[k * plane] = a.ch[k];
    }
  }
}

}  // namespace

extern "C" int64_t pcs_range_project_ws_bytes(int32_t num_scenes, int32_t H, int32_t W) {
  if (!range_sizes_ok(num_scenes, H, W)) {
    set_error("pcs_range_project_ws_bytes: bad sizes (scenes >= 1, H >= 2, W >= 2, scenes * H * W < 2^31)");
    return -1;
  }
  return (int64_t)num_scenes * H * W * (int64_t)sizeof(int32_t);
}

extern "C" int pcs_range_project_f32(const float *feats, int64_t n, int32_t c, const int32_t *scenes, const float *cuts32,
                                     int32_t num_scenes, int32_t H, int32_t W, int32_t *winner, float *pxpy, int32_t *bad,
                                     void *stream) {
  if (!range_sizes_ok(num_scenes, H, W) || c < 5 || n < 0 || n >= ((int64_t)1 << 31)) {
    set_error("pcs_range_project_f32: bad args (0 <= n < 2^31, c >= 5, scenes >= 1, H >= 2, W >= 2, scenes * H * W < 2^31)");
    return PCS_EINVAL;
  }
  if (!winner || !bad || (n > 0 && (!feats || !scenes || !cuts32 || !pxpy))) {
    set_error("pcs_range_project_f32: null pointer");
    return PCS_EINVAL;
  }
  hipStream_t st = as_stream(stream);
  if (const int rc = fill_async("pcs_range_project_f32", st, winner, 0xFF, (size_t)num_scenes * H * W * sizeof(int32_t))) return rc;
  if (const int rc = fill_async("pcs_range_project_f32", st, bad, 0, sizeof(int32_t))) return rc;
  if (n == 0) return PCS_OK;
  hipLaunchKernelGGL(range_project_kernel, dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, st, feats, n, (int)c, scenes, cuts32,
                     (int)num_scenes, (int)H, (int)W, winner, pxpy, bad);
  return check_launch("pcs_range_project_f32");
}

extern "C" int pcs_range_image_fill_f32(const int32_t *winner, const float *feats, int64_t n, int32_t c, int32_t num_scenes,
                                        int32_t H, int32_t W, float *image, void *stream) {
  if (!range_sizes_ok(num_scenes, H, W) || c < 5 || n < 0 || n >= ((int64_t)1 << 31)) {
    set_error("pcs_range_image_fill_f32: bad args (0 <= n < 2^31, c >= 5, scenes >= 1, H >= 2, W >= 2, scenes * H * W < 2^31)");
    return PCS_EINVAL;
  }
  if (!winner || !image || (n > 0 && !feats)) {
    set_error("pcs_range_image_fill_f32: null pointer");
    return PCS_EINVAL;
  }
  const int64_t plane = (int64_t)H * W, pixels = plane * num_scenes;
  const bool vec = W % 4 == 0 && (((uintptr_t)winner | (uintptr_t)image) & 15) == 0;
  hipStream_t st = as_stream(stream);
  if (vec)
    hipLaunchKernelGGL((range_fill_kernel<true>), dim3(stream_grid(pixels / 4, kBlock)), dim3(kBlock), 0, st, winner, feats, n,
                       (int)c, pixels, plane, image);
  else
    hipLaunchKernelGGL((range_fill_kernel<false>), dim3(stream_grid(pixels, kBlock)), dim3(kBlock), 0, st, winner, feats, n, (int)c,
                       pixels, plane, image);
  return check_launch("pcs_range_image_fill_f32");
}
