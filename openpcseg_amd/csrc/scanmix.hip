// PolarMix / LaserMix of two raw batches on the device -- gfx950. The reference mixes two scans per frame
// in the dataloader workers with NumPy (R:pcseg/data/dataset/semantickitti/semantickitti.py:98-177, PolarMix_semantickitti.py,
// LaserMix_semantickitti.py): boolean masks, np.delete, np.concatenate, np.dot. The output length depends on the data, so this is
// a stable partition into buckets: count, turn the counts into bases, place.
//   bucket 0          rows of scan 1 that stay (outside the sector; all of them without a swap or a mix)
//   bucket 1          rows of scan 2 inside the sector
//   buckets 2 .. 9    rows of scan 2 of instance class 0 .. 7 of the class table (a row of scan 2 may also sit in bucket 1)
//   then the instance list (buckets 2 .. 9) again, rotated by Omega[0], and again, rotated by Omega[1]: the same ranks at a fixed
//   distance, no count of their own. A row of scan 2 is written up to four times.
// LaserMix with radian thresholds (mode 2) uses the same machinery: bucket b = band b, fed by scan 1 where b is even and by scan 2
// where it is odd; nothing is rotated.
// row_buckets() decides a row's buckets; the count pass and the place pass both call it on the same stretch of rows
// (stretch_of()), so they cannot disagree. A workgroup owns one contiguous stretch of both scans of its frame (the frame is grid
// axis y, the grid is sized to the chip), writes its ten counts, a small pass turns them into per-workgroup bases and per-frame
// totals, a one-workgroup pass into the frames' first output rows. No atomics: the order of the output is a pure function of the
// input. Inside a workgroup the ranks are stable: wave ballots, the four waves folded through LDS, a running base per bucket in
// LDS. In the place pass the two scans of a stretch are grid axis z: no bucket takes rows of both scans, so the halves share the
// workgroup's bases without sharing a running count (and each half holds one scan's pointers: with both, and the bases in
// registers, the kernel spilled scalar registers). The bucket loops stay rolled for the same reason.
// The clamped row range of a frame (frame_rows) and the wave scans are shared: raw_scan.h, pcs_common.h.
// The rotated copies go through affine_row() of raw_scan.h under (cos w, sin w, 1, 1, 1, 0, 0, 0): np.dot(float32 rows,
// float64 matrix) stored as float32. The sector test is float32: yaw = -float(atan2(double(y), double(x))), strictly between
// the float32 edges. The ring column (get_kitti_points_ringID) is a flag per mixed row, rocprim's inclusive scan over the batch
// and a pass that subtracts the frame's base: the first row of a frame never flags.
#include <math.h>

#include <rocprim/device/device_scan.hpp>

#include "pcs_common.h"
#include "raw_scan.h"

using namespace pcs;

namespace {

constexpr int kBlock = kScanBlock;
constexpr int kWaves = kBlock / kWave;
constexpr int kBuckets = PCS_MIX_BUCKETS;
constexpr int kStride = PCS_MIX_PLAN_STRIDE;
constexpr int kMaxThresholds = 5;
constexpr int kLut = 256;

struct FramePlan {
  int mode;   // 0 scan 1 unchanged, 1 PolarMix, 2 LaserMix bands
  float alpha, beta;
  bool swap, paste;
  int nt;
  const double *t;   // the frame's thresholds, read where they are used: five float64 would cost ten scalar registers
};

__device__ __forceinline__ FramePlan load_plan(const double *__restrict__ plan, int f) {
  const double *p = plan + (int64_t)f * kStride;
  FramePlan fp;
  fp.mode = (int)p[0];
  fp.alpha = (float)p[1];
  fp.beta = (float)p[2];
  fp.swap = p[3] != 0.0;
  fp.paste = p[4] != 0.0;
  int nt = (int)p[5];
  fp.nt = nt < 0 ? 0 : (nt > kMaxThresholds ? kMaxThresholds : nt);
  fp.t = p + 6;
  return fp;
}

// label -> its instance bucket (2 + position in the class table) or -1, in LDS: one read per row instead of eight compares
// against sixteen scalar registers. Classes outside 0 .. 255 are skipped (the host refuses them).
__device__ __forceinline__ void fill_lut(signed char *lut, const int64_t *__restrict__ classes, int ncls) {
  for (int j = threadIdx.x; j < kLut; j += kBlock) lut[j] = -1;
  __syncthreads();
  if ((int)threadIdx.x < ncls && threadIdx.x < PCS_MIX_MAX_CLASSES) {
    const int64_t c = classes[threadIdx.x];
    if (c >= 0 && c < kLut) lut[c] = (signed char)(2 + threadIdx.x);
  }
  __syncthreads();
}

struct Buckets {
  int primary, inst;   // -1: none
};

// The one decision both passes share. scan: 0 = the frame's own scan, 1 = its partner.
__device__ __forceinline__ Buckets row_buckets(const FramePlan &fp, const signed char *lut, int scan, float x, float y, float z,
                                               int64_t label) {
#pragma clang fp contract(off)
  Buckets b = {-1, -1};
  if (fp.mode == 0 || (fp.mode == 1 && !fp.swap)) {   // no angle is needed
    b.primary = scan == 0 ? 0 : -1;
  } else {
    // ONE arctan2 serves both angles (its polynomial's constants are held in scalar registers): the azimuth of PolarMix's
    // sector, the inclination of LaserMix's bands
    double num = (double)y, den = (double)x;
    if (fp.mode == 2) {
      const double xx = den * den, yy = num * num;
      num = (double)z;
      den = sqrt(xx + yy);
    }
    const double angle = atan2(num, den);
    if (fp.mode == 1) {
      const float yaw = -(float)angle;
      const bool in = yaw > fp.alpha && yaw < fp.beta;
      b.primary = scan == 0 ? (in ? -1 : 0) : (in ? 1 : -1);
    } else {
      int band = 0;
#pragma unroll
      for (int k = 0; k < kMaxThresholds; ++k) band += (k < fp.nt && angle <= fp.t[k]) ? 1 : 0;
      b.primary = (band & 1) == scan ? band : -1;
    }
  }
  if (fp.mode == 1 && scan == 1 && fp.paste && label >= 0 && label < kLut) b.inst = lut[label];
  return b;
}

// rows [lo, hi) of workgroup b of G along a frame's rows [flo, fhi): contiguous, ascending in b, whole tiles of kBlock rows
__device__ __forceinline__ FrameRows stretch_of(const int64_t *__restrict__ offsets, int f, int64_t n, int G, int b) {
  const FrameRows fr = frame_rows(offsets, f, n);
  const int64_t flo = fr.lo, fhi = fr.hi;
  int64_t per = (fhi - flo + G - 1) / G;
  per = (per + kBlock - 1) / kBlock * kBlock;
  FrameRows s;
  s.lo = flo + (int64_t)b * per;
  s.hi = s.lo + per;
  if (s.lo > fhi) s.lo = fhi;
  if (s.hi > fhi) s.hi = fhi;
  return s;
}

// Not raw_scan.h's load_raw_row: a mixed row is always four columns and travels whole, as the float4 it is stored back as, and
// ROW16 says only that the array is 16-byte aligned.
template <bool ROW16>
__device__ __forceinline__ float4 load_row(const float *__restrict__ pts, int64_t i) {
  if (ROW16) return *reinterpret_cast<const float4 *>(pts + i * 4);
  const float *p = pts + i * 4;
  return make_float4(p[0], p[1], p[2], p[3]);
}

template <bool ROW16>
__device__ __forceinline__ void store_row(float *__restrict__ out, int64_t row, int cout, float x, float y, float z, float w) {
  if (ROW16) {
    *reinterpret_cast<float4 *>(out + row * 4) = make_float4(x, y, z, w);
  } else {
    float *o = out + row * cout;
    o[0] = x; o[1] = y; o[2] = z; o[3] = w;
  }
}

// counts (F, G, kBuckets) int32: every cell is written
template <bool ROW16>
__global__ void __launch_bounds__(kBlock) mix_count_kernel(const float *__restrict__ pts1, int64_t n1, const int64_t *__restrict__ off1,
                                                           const float *__restrict__ pts2, const int64_t *__restrict__ lab2, int64_t n2,
                                                           const int64_t *__restrict__ off2, const double *__restrict__ plan,
                                                           const int64_t *__restrict__ classes, int ncls, int32_t *__restrict__ counts) {
  __shared__ int red[kWaves][kBuckets];
  __shared__ signed char lut[kLut];
  const int f = blockIdx.y, b = blockIdx.x, G = gridDim.x;
  const FramePlan fp = load_plan(plan, f);
  fill_lut(lut, classes, ncls);
  int c[kBuckets];
#pragma unroll
  for (int k = 0; k < kBuckets; ++k) c[k] = 0;
  for (int scan = 0; scan < 2; ++scan) {
    const float *pts = scan ? pts2 : pts1;
    const FrameRows s = stretch_of(scan ? off2 : off1, f, scan ? n2 : n1, G, b);
    for (int64_t i = s.lo + threadIdx.x; i < s.hi; i += kBlock) {
      const float4 r = load_row<ROW16>(pts, i);
      const int64_t label = (scan && fp.mode == 1) ? lab2[i] : -1;
      const Buckets bk = row_buckets(fp, lut, scan, r.x, r.y, r.z, label);
#pragma unroll
      for (int k = 0; k < kBuckets; ++k) c[k] += (bk.primary == k ? 1 : 0) + (bk.inst == k ? 1 : 0);
    }
  }
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int k = 0; k < kBuckets; ++k) {
    const int a = wave_sum(c[k]);
    if (lane == 0) red[wave][k] = a;
  }
  __syncthreads();
  if ((int)threadIdx.x < kBuckets) {
    int a = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) a += red[w][threadIdx.x];
    counts[((int64_t)f * G + b) * kBuckets + threadIdx.x] = a;
  }
}

// one workgroup per frame: counts (F, G, kBuckets) -> the same cells as exclusive sums along G, totals (F, kBuckets)
__global__ void __launch_bounds__(kBlock) mix_bases_kernel(int32_t *__restrict__ counts, int G, int32_t *__restrict__ totals) {
  const int f = blockIdx.x;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  int32_t *mine = counts + (int64_t)f * G * kBuckets;
  for (int k = wave; k < kBuckets; k += kWaves) {   // uniform per wave
    int carry = 0;
    for (int g0 = 0; g0 < G; g0 += kWave) {
      const int g = g0 + lane;
      const int v = g < G ? mine[(int64_t)g * kBuckets + k] : 0;
      const int incl = wave_inclusive(v, lane);
      if (g < G) mine[(int64_t)g * kBuckets + k] = carry + incl - v;
      carry += __shfl(incl, kWave - 1, 64);
    }
    if (lane == 0) totals[(int64_t)f * kBuckets + k] = carry;
  }
}

__device__ __forceinline__ int64_t mixed_rows(const int32_t *__restrict__ totals, const double *__restrict__ plan, int f) {
  int64_t all = 0, inst = 0;
#pragma unroll
  for (int k = 0; k < kBuckets; ++k) {
    const int t = totals[(int64_t)f * kBuckets + k];
    all += t;
    if (k >= 2) inst += t;
  }
  return (int)plan[(int64_t)f * kStride] == 1 ? all + 2 * inst : all;
}

// one workgroup: frame_base (F + 1) int64 = the first mixed row of every frame, frame_base[F] = all rows
__global__ void __launch_bounds__(kBlock) mix_frame_base_kernel(const int32_t *__restrict__ totals, const double *__restrict__ plan, int F,
                                                                int64_t *__restrict__ frame_base) {
  __shared__ int64_t wsum[kWaves];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  int64_t carry = 0;
  for (int f0 = 0; f0 < F; f0 += kBlock) {
    const int f = f0 + threadIdx.x;
    const int64_t v = f < F ? mixed_rows(totals, plan, f) : 0;
    const int64_t incl = wave_inclusive(v, lane);
    if (lane == kWave - 1) wsum[wave] = incl;
    __syncthreads();
    int64_t before = 0, block = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) before += wsum[w];
      block += wsum[w];
    }
    if (f < F) frame_base[f] = carry + before + incl - v;
    carry += block;
    __syncthreads();   // wsum is written again
  }
  if (threadIdx.x == 0) frame_base[F] = carry;
}

// wbase: mix_bases_kernel's cells. Every store is checked against the m rows the host sized the output to.
template <bool ROW16_IN, bool ROW16_OUT>
__global__ void __launch_bounds__(kBlock) mix_place_kernel(const float *__restrict__ pts1, const int64_t *__restrict__ lab1, int n1,
                                                           const int64_t *__restrict__ off1, const float *__restrict__ pts2,
                                                           const int64_t *__restrict__ lab2, int n2, const int64_t *__restrict__ off2,
                                                           const double *__restrict__ plan, const int64_t *__restrict__ classes, int ncls,
                                                           const double *__restrict__ omega, const int32_t *__restrict__ wbase,
                                                           const int32_t *__restrict__ totals, const int64_t *__restrict__ frame_base,
                                                           int64_t m, int cout, float *__restrict__ out, int64_t *__restrict__ out_labels) {
  __shared__ int wcnt[2][kWaves][kBuckets];
  __shared__ int sbase[2][kBuckets];   // the running bases, relative to the frame's first mixed row (a frame has fewer than 2^31)
  __shared__ double som[16];
  __shared__ signed char lut[kLut];
  const int f = blockIdx.y, b = blockIdx.x, G = gridDim.x;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  const FramePlan fp = load_plan(plan, f);
  if (threadIdx.x < 16) som[threadIdx.x] = omega[threadIdx.x];
  const int64_t first = frame_base[f];
  int inst_total = 0;
  {
    int at = 0;
#pragma unroll
    for (int k = 0; k < kBuckets; ++k) {
      const int t = totals[(int64_t)f * kBuckets + k];
      if ((int)threadIdx.x == k) sbase[0][k] = at + wbase[((int64_t)f * G + b) * kBuckets + k];
      at += t;
      if (k >= 2) inst_total += t;
    }
  }
  if (fp.mode != 1) inst_total = 0;
  fill_lut(lut, classes, ncls);
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (kWave - lane));
  int par = 0;
  __syncthreads();   // som, sbase
  {
    // grid axis z is the scan: no bucket takes rows of both scans, so the two halves of a workgroup's stretch share the bases
    // without sharing a running count
    const int scan = blockIdx.z;
    const float *pts = scan ? pts2 : pts1;
    const int64_t *lab = scan ? lab2 : lab1;
    const FrameRows s = stretch_of(scan ? off2 : off1, f, scan ? n2 : n1, G, b);
    for (int64_t i0 = s.lo; i0 < s.hi; i0 += kBlock) {   // the same trips for the whole workgroup
      const int64_t i = i0 + threadIdx.x;
      const bool valid = i < s.hi;
      float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
      int64_t label = -1;
      Buckets bk = {-1, -1};
      if (valid) {
        r = load_row<ROW16_IN>(pts, i);
        label = lab[i];
        bk = row_buckets(fp, lut, scan, r.x, r.y, r.z, label);
      }
      int rank_p = 0, rank_q = 0;
#pragma unroll 1
      for (int k = 0; k < kBuckets; ++k) {
        const unsigned long long bal = __ballot(bk.primary == k || bk.inst == k);
        if (lane == 0) wcnt[par][wave][k] = __popcll(bal);
        const int rk = __popcll(bal & below);
        if (bk.primary == k) rank_p = rk;
        if (bk.inst == k) rank_q = rk;
      }
      __syncthreads();
      int64_t dst_p = -1, dst_q = -1;
#pragma unroll 1
      for (int k = 0; k < kBuckets; ++k) {
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
          const int t = wcnt[par][w][k];
          if (w < wave) before += t;
          all += t;
        }
        const int at = sbase[par][k];
        if (bk.primary == k) dst_p = first + (at + before + rank_p);
        if (bk.inst == k) dst_q = first + (at + before + rank_q);
        if ((int)threadIdx.x == k) sbase[par ^ 1][k] = at + all;   // read after the next tile's barrier
      }
      par ^= 1;   // the next tile writes the other halves, which nobody reads before its barrier: one barrier per tile
      if (dst_p >= 0 && dst_p < m) {
        store_row<ROW16_OUT>(out, dst_p, cout, r.x, r.y, r.z, r.w);
        out_labels[dst_p] = label;
      }
      if (dst_q >= 0 && dst_q + 2 * (int64_t)inst_total < m) {
        store_row<ROW16_OUT>(out, dst_q, cout, r.x, r.y, r.z, r.w);
        out_labels[dst_q] = label;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          float fx, fy, fz;
          affine_row(r.x, r.y, r.z, som + j * 8, fx, fy, fz);
          const int64_t d = dst_q + (int64_t)(j + 1) * inst_total;
          store_row<ROW16_OUT>(out, d, cout, fx, fy, fz, r.w);
          out_labels[d] = label;
        }
      }
    }
  }
}

// ---- the ring column --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ring_proj_x(float x, float y) {
#pragma clang fp contract(off)
  const float yaw = -(float)atan2((double)y, (double)(-x));
  const float t = __fdiv_rn(yaw, kPiF) + 1.0f;
  return 0.5f * t;
}

__global__ void __launch_bounds__(kBlock) ring_flag_kernel(const float *__restrict__ pts, int64_t m, int c,
                                                           const int64_t *__restrict__ frame_base, int32_t *__restrict__ flags) {
  const int f = blockIdx.y;
  const int lane = threadIdx.x & (kWave - 1);
  const FrameRows s = frame_rows(frame_base, f, m);   // the mixed rows of frame f
  for (int64_t i0 = s.lo + (int64_t)blockIdx.x * kBlock; i0 < s.hi; i0 += (int64_t)gridDim.x * kBlock) {   // uniform per workgroup
    const int64_t i = i0 + threadIdx.x;
    const bool valid = i < s.hi;
    const float px = valid ? ring_proj_x(pts[i * c], pts[i * c + 1]) : 0.f;
    float prev = __shfl_up(px, 1, 64);
    if (lane == 0 && valid && i > s.lo) prev = ring_proj_x(pts[(i - 1) * c], pts[(i - 1) * c + 1]);
    if (valid) flags[i] = (i > s.lo && px < 0.2f && prev > 0.8f) ? 1 : 0;   // the first row of a frame never flags
  }
}

__global__ void __launch_bounds__(kBlock) ring_store_kernel(float *__restrict__ pts, int64_t m, int c, const int64_t *__restrict__ frame_base,
                                                            const int32_t *__restrict__ scanned) {
  const int f = blockIdx.y;
  const FrameRows s = frame_rows(frame_base, f, m);   // the mixed rows of frame f
  const int32_t before = s.lo > 0 && s.lo < s.hi ? scanned[s.lo - 1] : 0;
  for (int64_t i = s.lo + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < s.hi; i += (int64_t)gridDim.x * kBlock) {
    int r = scanned[i] - before;
    r = r < 0 ? 0 : (r > 63 ? 63 : r);
    pts[i * c + 4] = (float)r;
  }
}

int mix_grid(int64_t n1, int64_t n2, int num_frames) { return frame_grid(n1 > n2 ? n1 : n2, 1, num_frames, 1024); }

bool mix_sizes_ok(int64_t n1, int64_t n2, int32_t num_frames) {
  return n1 >= 0 && n2 >= 0 && n1 < ((int64_t)1 << 31) && n2 < ((int64_t)1 << 31) && n1 + 4 * n2 < ((int64_t)1 << 31) && num_frames >= 1 &&
         num_frames <= 65535;
}

bool ring_sizes_ok(int64_t m, int32_t c, int32_t num_frames) {
  return m >= 0 && m < ((int64_t)1 << 31) && c >= 5 && c <= PCS_SCAN_MAX_COLUMNS && num_frames >= 1 && num_frames <= 65535;
}

int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

bool ring_temp_bytes(int64_t m, size_t *bytes) {
  *bytes = 0;
  if (m == 0) return true;
  const hipError_t e = rocprim::inclusive_scan(nullptr, *bytes, (const int32_t *)nullptr, (int32_t *)nullptr, (size_t)m, rocprim::plus<int32_t>(),
                                               (hipStream_t)0);
  if (e != hipSuccess) { set_error("pcs_scan_ring: rocprim temporary-storage query failed: %s", hipGetErrorString(e)); return false; }
  return true;
}

}  // namespace

extern "C" int64_t pcs_scan_mix_ws_bytes(int64_t n1, int64_t n2, int32_t num_frames) {
  if (!mix_sizes_ok(n1, n2, num_frames)) { set_error("pcs_scan_mix_ws_bytes: bad sizes"); return PCS_EINVAL; }
  return (int64_t)sizeof(int32_t) * num_frames * mix_grid(n1, n2, num_frames) * kBuckets;
}

extern "C" int pcs_scan_mix_count(const float *points1, int64_t n1, const int64_t *frame_offsets1, const float *points2,
                                  const int64_t *labels2, int64_t n2, const int64_t *frame_offsets2, int32_t num_frames, const double *plan,
                                  const int64_t *classes, int32_t num_classes, void *ws, int64_t ws_bytes, int32_t *totals,
                                  int64_t *frame_base, void *stream) {
  if (!mix_sizes_ok(n1, n2, num_frames) || num_classes < 0 || num_classes > PCS_MIX_MAX_CLASSES) {
    set_error("pcs_scan_mix_count: bad args (n1, n2 >= 0, n1 + 4 n2 < 2^31, 1 <= frames <= 65535, 0 <= classes <= %d)", PCS_MIX_MAX_CLASSES);
    return PCS_EINVAL;
  }
  if (!frame_offsets1 || !frame_offsets2 || !plan || !ws || !totals || !frame_base || (num_classes > 0 && !classes) ||
      (n1 > 0 && !points1) || (n2 > 0 && (!points2 || !labels2))) {
    set_error("pcs_scan_mix_count: null pointer");
    return PCS_EINVAL;
  }
  const int64_t need = pcs_scan_mix_ws_bytes(n1, n2, num_frames);
  if (ws_bytes < need) return ws_too_small("pcs_scan_mix_count", ws_bytes, need);
  hipStream_t st = as_stream(stream);
  int32_t *counts = reinterpret_cast<int32_t *>(ws);
  const int G = mix_grid(n1, n2, num_frames);
  const dim3 grid(G, num_frames);
  const bool row16 = (((uintptr_t)points1 | (uintptr_t)points2) & 15) == 0;
  if (row16)
    hipLaunchKernelGGL((mix_count_kernel<true>), grid, dim3(kBlock), 0, st, points1, n1, frame_offsets1, points2, labels2, n2, frame_offsets2,
                       plan, classes, num_classes, counts);
  else
    hipLaunchKernelGGL((mix_count_kernel<false>), grid, dim3(kBlock), 0, st, points1, n1, frame_offsets1, points2, labels2, n2, frame_offsets2,
                       plan, classes, num_classes, counts);
  hipLaunchKernelGGL(mix_bases_kernel, dim3(num_frames), dim3(kBlock), 0, st, counts, G, totals);
  hipLaunchKernelGGL(mix_frame_base_kernel, dim3(1), dim3(kBlock), 0, st, totals, plan, num_frames, frame_base);
  return check_launch("pcs_scan_mix_count");
}

extern "C" int pcs_scan_mix_place(const float *points1, const int64_t *labels1, int64_t n1, const int64_t *frame_offsets1,
                                  const float *points2, const int64_t *labels2, int64_t n2, const int64_t *frame_offsets2,
                                  int32_t num_frames, const double *plan, const int64_t *classes, int32_t num_classes, const double *omega,
                                  const void *ws, int64_t ws_bytes, const int32_t *totals, const int64_t *frame_base, int64_t m, int32_t c_out,
                                  float *out_points, int64_t *out_labels, void *stream) {
  if (!mix_sizes_ok(n1, n2, num_frames) || num_classes < 0 || num_classes > PCS_MIX_MAX_CLASSES || m < 0 || m > n1 + 4 * n2 || c_out < 4 ||
      c_out > PCS_SCAN_MAX_COLUMNS) {
    set_error("pcs_scan_mix_place: bad args (n1, n2 >= 0, n1 + 4 n2 < 2^31, 1 <= frames <= 65535, 0 <= classes <= %d, 0 <= m <= n1 + 4 n2, "
              "4 <= c_out <= %d)", PCS_MIX_MAX_CLASSES, PCS_SCAN_MAX_COLUMNS);
    return PCS_EINVAL;
  }
  if (!frame_offsets1 || !frame_offsets2 || !plan || !omega || !ws || !totals || !frame_base || (num_classes > 0 && !classes) ||
      (n1 > 0 && (!points1 || !labels1)) || (n2 > 0 && (!points2 || !labels2)) || (m > 0 && (!out_points || !out_labels))) {
    set_error("pcs_scan_mix_place: null pointer");
    return PCS_EINVAL;
  }
  const int64_t need = pcs_scan_mix_ws_bytes(n1, n2, num_frames);
  if (ws_bytes < need) return ws_too_small("pcs_scan_mix_place", ws_bytes, need);
  if (m == 0) return PCS_OK;
  hipStream_t st = as_stream(stream);
  const int32_t *wbase = reinterpret_cast<const int32_t *>(ws);
  const dim3 grid(mix_grid(n1, n2, num_frames), num_frames, 2);
  const bool in16 = (((uintptr_t)points1 | (uintptr_t)points2) & 15) == 0;
  const bool out16 = c_out == 4 && ((uintptr_t)out_points & 15) == 0;
#define PCS_MIX_PLACE(IN, OUT)                                                                                                          \
  hipLaunchKernelGGL((mix_place_kernel<IN, OUT>), grid, dim3(kBlock), 0, st, points1, labels1, (int)n1, frame_offsets1, points2, labels2, (int)n2, \
                     frame_offsets2, plan, classes, num_classes, omega, wbase, totals, frame_base, m, c_out, out_points, out_labels)
  if (in16 && out16) PCS_MIX_PLACE(true, true);
  else if (in16) PCS_MIX_PLACE(true, false);
  else if (out16) PCS_MIX_PLACE(false, true);
  else PCS_MIX_PLACE(false, false);
#undef PCS_MIX_PLACE
  return check_launch("pcs_scan_mix_place");
}

extern "C" int64_t pcs_scan_ring_ws_bytes(int64_t m) {
  if (m < 0 || m >= ((int64_t)1 << 31)) { set_error("pcs_scan_ring_ws_bytes: bad sizes"); return PCS_EINVAL; }
  size_t temp = 0;
  if (!ring_temp_bytes(m, &temp)) return PCS_EINVAL;
  return 2 * align256(m * (int64_t)sizeof(int32_t)) + align256((int64_t)temp);   // flags, their inclusive sums, rocprim's temporaries
}

extern "C" int pcs_scan_ring_f32(float *points, int64_t m, int32_t c, const int64_t *frame_base, int32_t num_frames, void *ws,
                                 int64_t ws_bytes, void *stream) {
  if (!ring_sizes_ok(m, c, num_frames)) {
    set_error("pcs_scan_ring_f32: bad args (0 <= m < 2^31, 5 <= c <= %d, 1 <= frames <= 65535)", PCS_SCAN_MAX_COLUMNS);
    return PCS_EINVAL;
  }
  if (m == 0) return PCS_OK;
  if (!points || !frame_base || !ws) { set_error("pcs_scan_ring_f32: null pointer"); return PCS_EINVAL; }
  size_t temp = 0;
  if (!ring_temp_bytes(m, &temp)) return PCS_EINVAL;
  const int64_t cells = align256(m * (int64_t)sizeof(int32_t));
  const int64_t need = 2 * cells + align256((int64_t)temp);
  if (ws_bytes < need) return ws_too_small("pcs_scan_ring_f32", ws_bytes, need);
  hipStream_t st = as_stream(stream);
  char *base = reinterpret_cast<char *>(ws);
  int32_t *flags = reinterpret_cast<int32_t *>(base), *scanned = reinterpret_cast<int32_t *>(base + cells);
  const dim3 grid(frame_grid(m, 1, num_frames, 2048), num_frames);
  // rows outside every frame (frame_base not covering [0, m)) would keep garbage flags: clear them first
  if (const int rc = fill_async("pcs_scan_ring_f32", st, flags, 0, (size_t)m * sizeof(int32_t))) return rc;
  hipLaunchKernelGGL(ring_flag_kernel, grid, dim3(kBlock), 0, st, points, m, c, frame_base, flags);
  const hipError_t e = rocprim::inclusive_scan(base + 2 * cells, temp, (const int32_t *)flags, scanned, (size_t)m, rocprim::plus<int32_t>(), st);
  if (e != hipSuccess) { set_error("pcs_scan_ring_f32: rocprim::inclusive_scan: %s", hipGetErrorString(e)); return PCS_ELAUNCH; }
  hipLaunchKernelGGL(ring_store_kernel, grid, dim3(kBlock), 0, st, points, m, c, frame_base, scanned);
  return check_launch("pcs_scan_ring_f32");
}
