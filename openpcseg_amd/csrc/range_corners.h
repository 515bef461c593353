// The bilinear sample of a (B, C, H, W) range feature map at a point (frame, x, y): frame check, corner offsets and
// weights, and the accumulation over the four corners. One definition for the kernels that sample a range image:
// range_sample_fwd_kernel / range_corners_kernel (rangesample.hip) and range_point_merge_kernel (rangemerge.hip)
// compile the same expressions, so they give the same bits.
#pragma once
#include "pcs_common.h"

namespace pcs {

struct Corners {
  int64_t off[4];   // offset of the corner inside one (H, W) plane, -1 = outside the image
  float w[4];
};

// the frame of a point: an integer in [0, B), else -1 (a point of no frame samples nothing)
__device__ __forceinline__ int frame_of(float fb, int B) {
  int b = (int)fb;
  if (!(fb >= 0.f) || b >= B || (float)b != fb) b = -1;
  return b;
}

// grid_sampler_compute_source_index + the four bilinear weights of torch's grid_sampler_2d (GridSampler.cuh), fp32 like there
__device__ __forceinline__ Corners corners_of(float x, float y, int H, int W) {
  const float ix = ((x + 1.f) * (float)W - 1.f) / 2.f;
  const float iy = ((y + 1.f) * (float)H - 1.f) / 2.f;
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
  Corners c;
  c.w[0] = ((float)x1 - ix) * ((float)y1 - iy);   // nw
  c.w[1] = (ix - (float)x0) * ((float)y1 - iy);   // ne
  c.w[2] = ((float)x1 - ix) * (iy - (float)y0);   // sw
  c.w[3] = (ix - (float)x0) * (iy - (float)y0);   // se
  const bool vx0 = x0 >= 0 && x0 < W, vx1 = x1 >= 0 && x1 < W, vy0 = y0 >= 0 && y0 < H, vy1 = y1 >= 0 && y1 < H;
  c.off[0] = (vx0 && vy0) ? (int64_t)y0 * W + x0 : -1;
  c.off[1] = (vx1 && vy0) ? (int64_t)y0 * W + x1 : -1;
  c.off[2] = (vx0 && vy1) ? (int64_t)y1 * W + x0 : -1;
  c.off[3] = (vx1 && vy1) ? (int64_t)y1 * W + x1 : -1;
  return c;
}

// the sample of one (H, W) plane: from zero in nw, ne, sw, se order (torch's order of accumulation)
__device__ __forceinline__ float sample_plane(const float *__restrict__ pl, const Corners &cn) {
  float v = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (cn.off[k] >= 0) v += pl[cn.off[k]] * cn.w[k];
  return v;
}

}  // namespace pcs
