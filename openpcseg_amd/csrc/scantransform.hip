// The dataset transform of a raw batch on the device -- gfx950, two launches and a fill, no host read.
// The reference runs it per scan in the dataloader workers with NumPy (R:tools/utils/common/seg_utils.py:43-100 aug_points:
// rotate, scale, flip, jitter in float64; R:pcseg/data/dataset/semantickitti/semantickitti_voxel.py:83-114: the result is stored
// back as float32 -- it is also the voxel's feature --, round(xyz / voxel_size) in float32, minus the scan's minimum), once per
// vote under test-time augmentation (:62-69, ten votes per scan). Here, for every raw row and every vote v of its frame f, with
// the parameter row (cos, sin, scale, sx, sy, jx, jy, jz) of (v, f):
//   X = double(x) * c + double(y) * (-s);  Y = double(x) * s + double(y) * c;  Z = double(z)      (np.dot with the rotation matrix)
//   X, Y, Z *= scale;  X *= sx;  Y *= sy;  X, Y, Z += jx, jy, jz                                   (no multiply-add is fused)
//   fx, fy, fz = float(X), float(Y), float(Z)       -> feats row v * n + i, the other columns copied through
//   q = int(rintf(fx / voxel_size))                 -> coords row v * n + i, and the minimum of (v, f)
// pcs_scan_shift then subtracts the minimum of (v, f) and writes the scene v * F + f of every row.
// Traffic: the scan is read once (4 C B per row) whatever the number of votes; per vote 4 C + 12 B are written, and the shift
// reads and writes 12 B and writes 8 B. A workgroup stays inside one frame (the frame is a grid axis) and keeps the 3 V running
// minima in registers over its grid-stride loop; the grid is sized to the chip, not to the rows. The minima do NOT end in
// atomicMin: all of them live in one or two cache lines, and device-scope atomics on one line retire one after the other
// (measured: ~8 ns each -- 24 576 of them, one per wave, vote and axis, took 190 of the kernel's 193 us on twelve full scans).
// Instead every workgroup reduces its waves through LDS, stores its 3 V partial minima, and takes a ticket of its frame (one
// atomic add per workgroup); the workgroup that draws the frame's last ticket reduces the partials into `mins`.
// The row range of a frame, the row load, the parameter rows in LDS, the grid and the vote dispatch are raw_scan.h's.
#include <math.h>

#include "pcs_common.h"
#include "raw_scan.h"

using namespace pcs;

namespace {

constexpr int kBlock = kScanBlock;
constexpr int kMaxExtra = kScanMaxExtra;

__global__ void __launch_bounds__(kBlock) scan_fill_kernel(int32_t *__restrict__ dst, int count, int32_t value) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) dst[i] = value;
}

// VB: compiled bound of the vote loop (V <= VB; the minima are VB x 3 registers). ROW16: C == 4 and both row arrays 16-byte
// aligned -- one 16-byte load and one 16-byte store per row. counters (F) int32, zero on entry; partials (F, gridDim.x, V, 3).
template <int VB, bool ROW16>
__global__ void __launch_bounds__(kBlock) scan_transform_kernel(const float *__restrict__ pts, int64_t n, int C,
                                                                const int64_t *__restrict__ frame_offsets, int F,
                                                                const double *__restrict__ params, int V, float voxel,
                                                                float *__restrict__ feats, int32_t *__restrict__ coords,
                                                                int32_t *__restrict__ mins, int32_t *__restrict__ counters,
                                                                int32_t *partials) {
  __shared__ double sp[VB * 8];
  __shared__ int red[kBlock / kWave][VB * 3];
  __shared__ int is_last;
  const int f = blockIdx.y;
  const FrameRows fr = frame_rows(frame_offsets, f, n);
  const int64_t lo = fr.lo, hi = fr.hi;
  // the workgroups of this frame that have rows: the others leave at once and take no ticket
  const int64_t want = hi > lo ? (hi - lo + kBlock - 1) / kBlock : 0;
  const int active = want < (int64_t)gridDim.x ? (int)want : (int)gridDim.x;
  if (active == 0) {   // an empty frame keeps INT32_MAX
    if (blockIdx.x == 0)
      for (int j = threadIdx.x; j < V * 3; j += kBlock) mins[((int64_t)(j / 3) * F + f) * 3 + j % 3] = INT32_MAX;
    return;
  }
  if ((int)blockIdx.x >= active) return;   // the same for the whole workgroup
  stage_params(sp, params, V, F, f);
  __syncthreads();
  int mn[VB][3];
#pragma unroll
  for (int v = 0; v < VB; ++v) mn[v][0] = mn[v][1] = mn[v][2] = INT32_MAX;
  for (int64_t i = lo + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < hi; i += (int64_t)gridDim.x * kBlock) {
    const RawRow r = load_raw_row<ROW16>(pts, i, C);
#pragma unroll
    for (int v = 0; v < VB; ++v) {
      if (v < V) {
        float fx, fy, fz;
        affine_row(r.x, r.y, r.z, sp + v * 8, fx, fy, fz);
        const int64_t row = (int64_t)v * n + i;
        if (ROW16) {
          *reinterpret_cast<float4 *>(feats + row * 4) = make_float4(fx, fy, fz, r.extra[0]);
        } else {
          float *o = feats + row * C;
          o[0] = fx; o[1] = fy; o[2] = fz;
#pragma unroll
          for (int k = 0; k < kMaxExtra; ++k)
            if (3 + k < C) o[3 + k] = r.extra[k];
        }
        const int q[3] = {(int)rintf(__fdiv_rn(fx, voxel)), (int)rintf(__fdiv_rn(fy, voxel)), (int)rintf(__fdiv_rn(fz, voxel))};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          coords[row * 3 + d] = q[d];
          mn[v][d] = q[d] < mn[v][d] ? q[d] : mn[v][d];
        }
      }
    }
  }
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int v = 0; v < VB; ++v) {
    if (v < V) {   // uniform: whole waves take the reduction
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const int a = wave_min(mn[v][d]);
        if (lane == 0) red[wave][v * 3 + d] = a;
      }
    }
  }
  __syncthreads();
  const int cells = V * 3;   // <= 48: one lane each
  int32_t *mine = partials + ((int64_t)f * gridDim.x + blockIdx.x) * cells;
  if ((int)threadIdx.x < cells) {
    int a = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kBlock / kWave; ++w) a = red[w][threadIdx.x] < a ? red[w][threadIdx.x] : a;
    mine[threadIdx.x] = a;
  }
  __threadfence();   // the partials are visible device-wide before the ticket is
  __syncthreads();
  if (threadIdx.x == 0) is_last = atomicAdd(&counters[f], 1) == active - 1;
  __syncthreads();
  if (!is_last) return;
  __threadfence();   // every other workgroup's ticket, and so its partials, came before
  // the frame's last workgroup: wave w folds the partials of workgroups w, w + 4, ... cell by cell, then the waves are folded
  const int32_t *all = partials + (int64_t)f * gridDim.x * cells;
  int a = INT32_MAX;
  if (lane < cells)
    for (int b = wave; b < active; b += kBlock / kWave) {
      const int t = __hip_atomic_load(all + (int64_t)b * cells + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      a = t < a ? t : a;
    }
  __syncthreads();   // red is reused
  if (lane < cells) red[wave][lane] = a;
  __syncthreads();
  if ((int)threadIdx.x < cells) {
    a = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kBlock / kWave; ++w) a = red[w][threadIdx.x] < a ? red[w][threadIdx.x] : a;
    mins[((int64_t)(threadIdx.x / 3) * F + f) * 3 + threadIdx.x % 3] = a;
  }
}

// one (frame, vote) per (blockIdx.y, blockIdx.z); the frame's 3 * rows coordinates as one flat range
__global__ void __launch_bounds__(kBlock) scan_shift_kernel(int32_t *__restrict__ coords, int64_t n,
                                                            const int64_t *__restrict__ frame_offsets, int F,
                                                            const int32_t *__restrict__ mins, int64_t *__restrict__ frames) {
  const int f = blockIdx.y, v = blockIdx.z;
  const FrameRows rows = frame_rows(frame_offsets, f, n);
  const int64_t lo = rows.lo, hi = rows.hi;
  const int64_t scene = (int64_t)v * F + f;
  const int32_t m0 = mins[scene * 3 + 0], m1 = mins[scene * 3 + 1], m2 = mins[scene * 3 + 2];
  int32_t *c = coords + (int64_t)v * n * 3;
  int64_t *fr = frames + (int64_t)v * n;
  for (int64_t e = lo * 3 + (int64_t)blockIdx.x * kBlock + threadIdx.x; e < hi * 3; e += (int64_t)gridDim.x * kBlock) {
    const int64_t row = e / 3;
    const int d = (int)(e - row * 3);
    c[e] -= d == 0 ? m0 : (d == 1 ? m1 : m2);
    if (d == 0) fr[row] = scene;
  }
}

}  // namespace

extern "C" int64_t pcs_scan_transform_ws_bytes(int64_t n, int32_t num_frames, int32_t num_votes) {
  if (!scan_sizes_ok(n, num_frames, num_votes)) { set_error("pcs_scan_transform_ws_bytes: bad sizes"); return PCS_EINVAL; }
  const int64_t g = vote_grid(n, num_frames, num_votes);
  return (int64_t)sizeof(int32_t) * num_frames * (1 + g * num_votes * 3);   // tickets, then the partial minima
}

extern "C" int pcs_scan_transform(const float *points, int64_t n, int32_t c, const int64_t *frame_offsets, int32_t num_frames,
                                  const double *params, int32_t num_votes, float voxel_size, float *feats, int32_t *coords,
                                  int32_t *mins, void *ws, int64_t ws_bytes, void *stream) {
  if (!scan_sizes_ok(n, num_frames, num_votes) || c < 3 || c > PCS_SCAN_MAX_COLUMNS || !(voxel_size > 0.f)) {
    set_error("pcs_scan_transform: bad args (n >= 0, 3 <= c <= %d, 1 <= votes <= %d, 1 <= frames <= 65535, voxel_size > 0)",
              PCS_SCAN_MAX_COLUMNS, PCS_SCAN_MAX_VOTES);
    return PCS_EINVAL;
  }
  if (!mins || !frame_offsets || !params || !ws || (n > 0 && (!points || !feats || !coords))) {
    set_error("pcs_scan_transform: null pointer");
    return PCS_EINVAL;
  }
  const int64_t need = pcs_scan_transform_ws_bytes(n, num_frames, num_votes);
  if (ws_bytes < need) return ws_too_small("pcs_scan_transform", ws_bytes, need);
  hipStream_t st = as_stream(stream);
  int32_t *counters = reinterpret_cast<int32_t *>(ws), *partials = counters + num_frames;
  hipLaunchKernelGGL(scan_fill_kernel, dim3(stream_grid(num_frames, kBlock)), dim3(kBlock), 0, st, counters, num_frames, 0);
  const bool row16 = c == 4 && (((uintptr_t)points | (uintptr_t)feats) & 15) == 0;
  const dim3 grid(vote_grid(n, num_frames, num_votes), num_frames);   // n == 0: one workgroup per frame writes INT32_MAX
  dispatch_votes(num_votes, row16, [&](auto vb, auto r16) {
    hipLaunchKernelGGL((scan_transform_kernel<decltype(vb)::value, decltype(r16)::value>), grid, dim3(kBlock), 0, st, points, n, c,
                       frame_offsets, num_frames, params, num_votes, voxel_size, feats, coords, mins, counters, partials);
  });
  return check_launch("pcs_scan_transform");
}

extern "C" int pcs_scan_shift(int32_t *coords, int64_t n, const int64_t *frame_offsets, int32_t num_frames, const int32_t *mins,
                              int32_t num_votes, int64_t *frames, void *stream) {
  if (!scan_sizes_ok(n, num_frames, num_votes)) {
    set_error("pcs_scan_shift: bad args (n >= 0, 1 <= votes <= %d, 1 <= frames <= 65535)", PCS_SCAN_MAX_VOTES);
    return PCS_EINVAL;
  }
  if (n == 0) return PCS_OK;
  if (!coords || !frame_offsets || !mins || !frames) { set_error("pcs_scan_shift: null pointer"); return PCS_EINVAL; }
  const dim3 grid(frame_grid(n, 3, (int64_t)num_frames * num_votes, 256 * 8), num_frames, num_votes);
  hipLaunchKernelGGL(scan_shift_kernel, grid, dim3(kBlock), 0, as_stream(stream), coords, n, frame_offsets, num_frames, mins, frames);
  return check_launch("pcs_scan_shift");
}
