// The cylindrical partition of one point (cylinder.hip, cylscan.hip): cart2polar and the cell of
// R:pcseg/data/dataset/semantickitti/semantickitti_cylinder.py:19-22 and :144-158 in the reference's arithmetic -- float32
// products / sums / quotients as the _rn intrinsics (no contraction), IEEE sqrtf, arctan2 in double rounded once, the clip, the
// cell index and the cell centre in float64.
#pragma once
#include <math.h>

#include "pcs_common.h"

namespace pcs {

struct CylCfg {
  double lo[3], hi[3], interval[3];
};

// HOST: min / max / grid -> cfg; false where the grid is < 2 or max <= min along some axis
inline bool cyl_cfg(const double *space_min3, const double *space_max3, const int32_t *grid3, CylCfg &cfg) {
  for (int d = 0; d < 3; ++d) {
    if (grid3[d] < 2 || !(space_max3[d] > space_min3[d])) return false;
    cfg.lo[d] = space_min3[d];
    cfg.hi[d] = space_max3[d];
    cfg.interval[d] = (space_max3[d] - space_min3[d]) / (double)(grid3[d] - 1);  // crop_range / (grid - 1) (:151)
  }
  return true;
}

// (x, y, z) -> pol = (rho, phi in degrees, z), the cell index and the cell centre
__device__ __forceinline__ void cyl_cell(float x, float y, float z, const CylCfg &cfg, float (&pol)[3], int (&idx)[3],
                                         float (&centre)[3]) {
  // cart2polar (:19-22), float32 like NumPy on a float32 scan
  const float rho = sqrtf(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)));
  const float phi = (float)atan2((double)y, (double)x);
  // xyz_pol[:, 1] / np.pi * 180. (:145): float32 array with Python scalars -> float32 arithmetic
  const float deg = __fmul_rn(__fdiv_rn(phi, 3.14159265358979323846f), 180.0f);
  pol[0] = rho; pol[1] = deg; pol[2] = z;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    // np.clip(float32, int64 bounds) -> float64; (c - min) / intervals; floor; astype(int) (:153)
    double c = (double)pol[d];
    c = c < cfg.lo[d] ? cfg.lo[d] : (c > cfg.hi[d] ? cfg.hi[d] : c);
    idx[d] = (int)floor((c - cfg.lo[d]) / cfg.interval[d]);
    // (point_coord.astype(float32) + 0.5) * intervals + min_bound (:157), float64, stored as float32 (:165)
    centre[d] = (float)(((double)((float)idx[d] + 0.5f)) * cfg.interval[d] + cfg.lo[d]);
  }
}

}  // namespace pcs
