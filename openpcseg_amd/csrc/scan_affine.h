// What the kernels over a raw batch share (scantransform.hip, cylscan.hip): the float64 affine map of one row under one
// parameter row, the size rule of their entries and the chip-sized grid along a frame.
#pragma once
#include "pcs_common.h"

namespace pcs {

constexpr int kScanBlock = 256;

// One row under one parameter row (cos, sin, scale, sx, sy, jx, jy, jz). Contraction is switched off for this body: a fused
// multiply-add skips the rounding of the product that NumPy's float64 arithmetic performs, and the float32 result can then
// differ in its last bit.
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

// workgroups along a frame: `chip` workgroups shared among the other grid axes, never more than the rows can use
inline int frame_grid(int64_t n, int64_t per_row, int64_t others, int64_t chip) {
  int64_t g = chip / others;
  const int64_t most = ceil_div(n * per_row, kScanBlock);
  if (g > most) g = most;
  return (int)(g < 1 ? 1 : g);
}

inline bool scan_sizes_ok(int64_t n, int32_t num_frames, int32_t num_votes) {
  return n >= 0 && num_votes >= 1 && num_votes <= PCS_SCAN_MAX_VOTES && num_frames >= 1 && num_frames <= 65535;
}

}  // namespace pcs
