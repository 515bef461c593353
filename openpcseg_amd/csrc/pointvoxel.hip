// K7-K10 point<->voxel kernels + calc_ti_weights -- gfx950; feature rows in fp32, bf16 or fp16 (row_storage.h).
// Reference semantics: TS:torchsparse/backend/voxelize/voxelize_cuda.cu:12-80,
// TS:torchsparse/backend/devoxelize/devoxelize_cuda.cu:11-98,
// TS:torchsparse/nn/functional/devoxelize.py:10-48.
// All HBM-bound. The reference launches <<<N, c>>> (c-thread blocks: 4 threads for c = 4), dispatches over
// AT_DISPATCH_FLOATING_TYPES_AND_HALF and accumulates the 8 trilinear corners in scalar_t through global memory; here a
// 256-thread workgroup covers 256/TX rows with TX lanes x V elements per row (V = a 16-byte piece, 4 elements or 1),
// every sum lives in fp32 registers in a fixed order, and every output row is written once with ONE rounding (no memset,
// no atomics). 16-bit rows are half the bytes, and no cast pass stands before or behind the kernel. The reference's atomic
// forms of K7 and K10 are kept for fp32 only.
#include <type_traits>

#include "row_storage.h"

using namespace pcs;

namespace {

template <int V> struct Vec;
template <> struct Vec<4> { using T = float4; };
template <> struct Vec<1> { using T = float; };

__device__ __forceinline__ float4 vscale(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ float vscale(float a, float s) { return a * s; }
__device__ __forceinline__ float4 vdiv(float4 a, float s) { return make_float4(a.x / s, a.y / s, a.z / s, a.w / s); }
__device__ __forceinline__ float vdiv(float a, float s) { return a / s; }
__device__ __forceinline__ void vatomic_add(float *p, float4 v) {
  atomicAdd(p + 0, v.x); atomicAdd(p + 1, v.y); atomicAdd(p + 2, v.z); atomicAdd(p + 3, v.w);
}
__device__ __forceinline__ void vatomic_add(float *p, float v) { atomicAdd(p, v); }

// ---- K7: scatter-mean (the reference's atomic form, fp32) -------------------------------------------------------------
template <int V>
__global__ void __launch_bounds__(256) voxelize_fwd_kernel(const float *__restrict__ feats,
                                                           const int32_t *__restrict__ idx,
                                                           const int32_t *__restrict__ counts,
                                                           int64_t n, int64_t m, int c, int cv,
                                                           float *out) {
  using VT = typename Vec<V>::T;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; i < n;
       i += (int64_t)gridDim.x * blockDim.y) {
    const int32_t pos = idx[i];
    if (pos < 0 || pos >= m) continue;
    const int32_t cnt = counts[pos];
    if (cnt == 0) continue;
    const float fc = (float)cnt;
    const VT *src = reinterpret_cast<const VT *>(feats + i * c);
    float *dst = out + (int64_t)pos * c;
    for (int j = threadIdx.x; j < cv; j += blockDim.x) vatomic_add(dst + j * V, vdiv(src[j], fc));
  }
}

// ---- K10: trilinear scatter -------------------------------------------------------------------
template <int V>
__global__ void __launch_bounds__(256) devoxelize_bwd_kernel(const float *__restrict__ gout,
                                                             const int32_t *__restrict__ idx8,
                                                             const float *__restrict__ w8,
                                                             int64_t n, int c, int cv,
                                                             float *gfeat) {
  using VT = typename Vec<V>::T;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; i < n;
       i += (int64_t)gridDim.x * blockDim.y) {
    int32_t id[8];
    float w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { id[k] = idx8[i * 8 + k]; w[k] = w8[i * 8 + k]; }
    const VT *src = reinterpret_cast<const VT *>(gout + i * c);
    for (int j = threadIdx.x; j < cv; j += blockDim.x) {
      const VT g = src[j];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (id[k] >= 0) vatomic_add(gfeat + (int64_t)id[k] * c + j * V, vscale(g, w[k]));
      }
    }
  }
}

// ---- calc_ti_weights ----------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ti_weights_kernel(const float *__restrict__ coords, int ld,
                                                         const int64_t *__restrict__ idxq,
                                                         int64_t n, float scale, float inv_s3,
                                                         int scaled, float *__restrict__ w) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float x = coords[i * ld + 0], y = coords[i * ld + 1], z = coords[i * ld + 2];
    float xf, yf, zf;
    if (scaled) {
      xf = floorf(x / scale) * scale; yf = floorf(y / scale) * scale; zf = floorf(z / scale) * scale;
    } else {
      xf = floorf(x); yf = floorf(y); zf = floorf(z);
    }
    const float xc = xf + scale, yc = yf + scale, zc = zf + scale;
    const float ax[2] = {xc - x, x - xf}, ay[2] = {yc - y, y - yf}, az[2] = {zc - z, z - zf};
    float wk[8];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {  // corner order = get_kernel_offsets(2): z fastest
      float v = (ax[(k >> 2) & 1] * ay[(k >> 1) & 1]) * az[k & 1];
      if (scaled) v *= inv_s3;
      if (idxq[(int64_t)k * n + i] == -1) v = 0.f;
      wk[k] = v;
      sum += v;
    }
    const float den = sum + 1e-8f;
#pragma unroll
    for (int k = 0; k < 8; ++k) w[(int64_t)k * n + i] = wk[k] / den;
  }
}

// ---- voxel_to_point map in one pass -------------------------------------------------------
// What R:pcseg/model/segmentor/voxel/minkunet/utils.py:69-105 builds with floor / cat / K2 (8 hashes per point) /
// hashquery (table rebuilt) / calc_ti_weights (~25 kernels) / two transposes: for every point the rows of the 8
// corner voxels of its stride-s cell (-1 = absent) and the trilinear weights, already in the (N,8) layout K9 reads.
// Corner order = get_kernel_offsets(2, s): z fastest. Weights in the reference's fp32 op order (ti_weights_kernel).
__global__ void __launch_bounds__(256) corner_map_kernel(const float *__restrict__ coords, int ld, int64_t n, int stride,
                                                         TableView table, int32_t *__restrict__ idx8,
                                                         float *__restrict__ w8) {
  const float scale = (float)stride;
  const float inv_s3 = 1.0f / (scale * scale * scale);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float x = coords[i * ld + 0], y = coords[i * ld + 1], z = coords[i * ld + 2];
    const int b = (int)coords[i * ld + ld - 1];
    const int bx = (int)floorf(x / scale) * stride, by = (int)floorf(y / scale) * stride, bz = (int)floorf(z / scale) * stride;
    float xf, yf, zf;
    if (stride != 1) {
      xf = floorf(x / scale) * scale; yf = floorf(y / scale) * scale; zf = floorf(z / scale) * scale;
    } else {
      xf = floorf(x); yf = floorf(y); zf = floorf(z);
    }
    const float xc = xf + scale, yc = yf + scale, zc = zf + scale;
    const float ax[2] = {xc - x, x - xf}, ay[2] = {yc - y, y - yf}, az[2] = {zc - z, z - zf};
    float wk[8];
    int id[8];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int ix = (k >> 2) & 1, iy = (k >> 1) & 1, iz = k & 1;
      id[k] = table_lookup(table, fnv60(bx + ix * stride, by + iy * stride, bz + iz * stride, b));
      float v = (ax[ix] * ay[iy]) * az[iz];
      if (stride != 1) v *= inv_s3;
      if (id[k] < 0) v = 0.f;
      wk[k] = v;
      sum += v;
    }
    const float den = sum + 1e-8f;
    int4 *io = reinterpret_cast<int4 *>(idx8 + i * 8);
    float4 *wo = reinterpret_cast<float4 *>(w8 + i * 8);
    io[0] = make_int4(id[0], id[1], id[2], id[3]);
    io[1] = make_int4(id[4], id[5], id[6], id[7]);
    wo[0] = make_float4(wk[0] / den, wk[1] / den, wk[2] / den, wk[3] / den);
    wo[1] = make_float4(wk[4] / den, wk[5] / den, wk[6] / den, wk[7] / den);
  }
}

// R consecutive entries of a run: their R row loads issued together, then added in entry order (divide, then add:
// voxelize_cuda.cu:27-29)
template <typename ET, int V, int R>
__device__ __forceinline__ void vox_rows(Acc<V> &acc, const typename Elem<ET>::T *__restrict__ feats,
                                         const int64_t *__restrict__ ord, int c, int j, float fc) {
  int64_t p[R];
  typename Raw<ET, V>::T r[R];
#pragma unroll
  for (int u = 0; u < R; ++u) p[u] = ord[u];
#pragma unroll
  for (int u = 0; u < R; ++u) r[u] = ld_row<ET, V>(feats + p[u] * c, j);
#pragma unroll
  for (int u = 0; u < R; ++u) add_div(acc, widen(ET{}, r[u]), fc);
}

// the same for K10: entry p = flat position i * 8 + k of (point, corner); weight w8[p], row gout[p >> 3]
template <typename ET, int V, int R>
__device__ __forceinline__ void devox_rows(Acc<V> &acc, const typename Elem<ET>::T *__restrict__ gout,
                                           const int64_t *__restrict__ ord, const float *__restrict__ w8, int c, int j) {
  int64_t p[R];
  float w[R];
  typename Raw<ET, V>::T r[R];
#pragma unroll
  for (int u = 0; u < R; ++u) p[u] = ord[u];
#pragma unroll
  for (int u = 0; u < R; ++u) { w[u] = w8[p[u]]; r[u] = ld_row<ET, V>(gout + (p[u] >> 3) * c, j); }
#pragma unroll
  for (int u = 0; u < R; ++u) add_mul(acc, w[u], widen(ET{}, r[u]));
}

// ---- K7, contention-free form: out[v] = sum over the run of v of feats[order[e]] / counts[v], a per-voxel segmented mean
// over a CSR of the points (order = point rows sorted by voxel, rowptr (m+1)). The atomic form above runs at 0.55 TB/s on
// 1.4 M points (random voxel rows), this one at gather speed.
// U independent row loads in flight per lane: 2, or 4 for 16-bit rows (a half row's registers are half as many; what is
// left of a run after the groups of 4 goes as a pair and a single). The loaded rows are added in `order` order whatever U
// is, so both give the same bits.
template <typename ET, int V, int U>
__global__ void __launch_bounds__(256) voxelize_fwd_csr_kernel(const typename Elem<ET>::T *__restrict__ feats,
                                                               const int64_t *__restrict__ order,
                                                               const int64_t *__restrict__ rowptr,
                                                               const int32_t *__restrict__ counts, int64_t m, int c, int cv,
                                                               typename Elem<ET>::T *__restrict__ out) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; v < m; v += (int64_t)gridDim.x * blockDim.y) {
    const int64_t e0 = rowptr[v], e1 = rowptr[v + 1];
    const int32_t cnt = counts[v];
    const float fc = (float)(cnt > 0 ? cnt : 1);
    typename Elem<ET>::T *dst = out + v * c;
    for (int j = threadIdx.x; j < cv; j += blockDim.x) {
      Acc<V> acc;
      azero(acc);
      if (cnt != 0) {
        int64_t e = e0;
        for (; e + U <= e1; e += U) vox_rows<ET, V, U>(acc, feats, order + e, c, j, fc);
        if (U == 4 && e + 2 <= e1) { vox_rows<ET, V, 2>(acc, feats, order + e, c, j, fc); e += 2; }
        if (e < e1) vox_rows<ET, V, 1>(acc, feats, order + e, c, j, fc);
      }
      st_row<ET, V>(dst, j, acc);
    }
  }
}

// ---- K8: gin[i] = gout[idx[i]] / counts[idx[i]], exact zeros where the point has no voxel --------------------------------
// A -0 gradient keeps each storage format's bits as they were when the formats had a kernel each: the fp32 rows store the
// quotient itself (-0 stays -0), the 16-bit rows the quotient added to +0 (-0 becomes +0).
template <typename ET, int V>
__global__ void __launch_bounds__(256) voxelize_bwd_kernel(const typename Elem<ET>::T *__restrict__ gout,
                                                           const int32_t *__restrict__ idx,
                                                           const int32_t *__restrict__ counts, int64_t n, int c, int cv,
                                                           typename Elem<ET>::T *__restrict__ gin) {
  constexpr bool kQuotient = std::is_same<ET, Fp32>::value;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; i < n; i += (int64_t)gridDim.x * blockDim.y) {
    const int32_t pos = idx[i];
    typename Elem<ET>::T *dst = gin + i * c;
    const int32_t cnt = pos >= 0 ? counts[pos] : 0;
    Acc<V> zero;
    azero(zero);
    if (cnt == 0) {
      for (int j = threadIdx.x; j < cv; j += blockDim.x) st_row<ET, V>(dst, j, zero);
      continue;
    }
    const float fc = (float)cnt;
    const typename Elem<ET>::T *src = gout + (int64_t)pos * c;
    for (int j = threadIdx.x; j < cv; j += blockDim.x) {
      const Acc<V> g = widen(ET{}, ld_row<ET, V>(src, j));
      Acc<V> r;
#pragma unroll
      for (int q = 0; q < V; ++q) r.f[q] = kQuotient ? g.f[q] / fc : zero.f[q] + g.f[q] / fc;
      st_row<ET, V>(dst, j, r);
    }
  }
}

// ---- K9: trilinear gather, the 8 corners summed in registers in k = 0..7 order -------------------------------------------
template <typename ET, int V>
__global__ void __launch_bounds__(256) devoxelize_fwd_kernel(const typename Elem<ET>::T *__restrict__ feat,
                                                             const int32_t *__restrict__ idx8,
                                                             const float *__restrict__ w8, int64_t n, int c, int cv,
                                                             typename Elem<ET>::T *__restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; i < n; i += (int64_t)gridDim.x * blockDim.y) {
    int32_t id[8];
    float w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { id[k] = idx8[i * 8 + k]; w[k] = w8[i * 8 + k]; }
    typename Elem<ET>::T *dst = out + i * c;
    for (int j = threadIdx.x; j < cv; j += blockDim.x) {
      Acc<V> acc;
      azero(acc);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (id[k] >= 0) add_mul(acc, w[k], widen(ET{}, ld_row<ET, V>(feat + (int64_t)id[k] * c, j)));
      }
      st_row<ET, V>(dst, j, acc);
    }
  }
}

// ---- K10, contention-free form: gfeat[v] = sum over the run of v of w8[order[e]] * gout[order[e] >> 3], a per-voxel
// segmented reduction over a CSR of the (point, corner) entries. entries sorted by voxel: order[e] = flat index i*8+k into
// idx8/w8; rowptr (m+1). One row of TX lanes per voxel, U independent row loads in flight, added in `order` order; every
// gfeat row is written exactly once (no memset, no atomics, deterministic). The reference's atomicAdd form
// (devoxelize_cuda.cu:37-57) serialises badly when thousands of points share a coarse voxel (stride 16: ~250 entries per voxel).
template <typename ET, int V, int U>
__global__ void __launch_bounds__(256) devoxelize_bwd_csr_kernel(const typename Elem<ET>::T *__restrict__ gout,
                                                                 const int64_t *__restrict__ order,
                                                                 const int64_t *__restrict__ rowptr,
                                                                 const float *__restrict__ w8, int64_t m, int c, int cv,
                                                                 typename Elem<ET>::T *__restrict__ gfeat) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; v < m; v += (int64_t)gridDim.x * blockDim.y) {
    const int64_t e0 = rowptr[v], e1 = rowptr[v + 1];
    typename Elem<ET>::T *dst = gfeat + v * c;
    for (int j = threadIdx.x; j < cv; j += blockDim.x) {
      Acc<V> acc;
      azero(acc);
      int64_t e = e0;
      for (; e + U <= e1; e += U) devox_rows<ET, V, U>(acc, gout, order + e, w8, c, j);
      if (U == 4 && e + 2 <= e1) { devox_rows<ET, V, 2>(acc, gout, order + e, w8, c, j); e += 2; }
      if (e < e1) devox_rows<ET, V, 1>(acc, gout, order + e, w8, c, j);
      st_row<ET, V>(dst, j, acc);
    }
  }
}

// The same reduction for NARROW rows (at most 8 vectors, 16-byte granular in fp32: the class scores the workload devoxelises
// since round 4; c <= 64 at V = 8, c <= 32 at V = 4): one WAVE per voxel, 8 x-lanes over the row's vectors times 8 entry lanes
// striding over the voxel's segment, two independent row loads in flight per lane, the 8 partial rows combined by shuffles in
// a fixed order (deterministic). A coarse voxel's ~250 entries are 32 trips of 8 independent row loads instead of 125 trips
// of two in one thread row, and a stride-1 voxel's 8 entries are one trip.
template <typename ET, int V>
__global__ void __launch_bounds__(256) devoxelize_bwd_csr_narrow_kernel(const typename Elem<ET>::T *__restrict__ gout,
                                                                        const int64_t *__restrict__ order,
                                                                        const int64_t *__restrict__ rowptr,
                                                                        const float *__restrict__ w8, int64_t m, int c, int cv,
                                                                        typename Elem<ET>::T *__restrict__ gfeat) {
  const int x = threadIdx.x & 7, el = (threadIdx.x >> 3) & 7, wv = threadIdx.x >> 6;
  for (int64_t v = (int64_t)blockIdx.x * 4 + wv; v < m; v += (int64_t)gridDim.x * 4) {   // (uniform over the wave)
    const int64_t e0 = rowptr[v], e1 = rowptr[v + 1];
    Acc<V> acc;
    azero(acc);
    for (int64_t e = e0 + el; e < e1; e += 16) {
      const int64_t p0 = order[e];
      const bool two = e + 8 < e1;
      const int64_t p1 = two ? order[e + 8] : p0;
      const float w0 = w8[p0], w1 = w8[p1];
      if (x < cv) {
        const typename Raw<ET, V>::T r0 = ld_row<ET, V>(gout + (p0 >> 3) * c, x);
        const typename Raw<ET, V>::T r1 = ld_row<ET, V>(gout + (p1 >> 3) * c, x);
        add_mul(acc, w0, widen(ET{}, r0));
        if (two) add_mul(acc, w1, widen(ET{}, r1));   // (not a zero weight: 0 x Inf of a diverged gradient must not turn into NaN here)
      }
    }
#pragma unroll
    for (int o = 32; o >= 8; o >>= 1) {
#pragma unroll
      for (int q = 0; q < V; ++q) acc.f[q] += __shfl_down(acc.f[q], o, 64);
    }
    if (el == 0 && x < cv) st_row<ET, V>(gfeat + v * c, x, acc);
  }
}

// Row loads in flight per lane in the two segmented lane-row kernels, 16-bit rows only (fp32 rows: always 2). Measured on the
// 12-scan bench batch, bf16 (profiles/pointvoxel_half_bench.json): 4 loads win where the runs are long -- stride 16 / C 256:
// voxelize 354 -> 287 us, devoxelize backward 806 -> 581 us; stride 4 / C 128: 150 -> 146 and 200 -> 175 us -- and lose on a
// stride-1 level, where a voxel has a handful of entries (C 96 devoxelize backward 184 -> 217 us). m is the proxy for the run
// length, with the threshold the wave-per-voxel form already uses. 0 = this rule; pcs_debug_pointvoxel_h_inflight forces 2 or 4.
int g_inflight = 0;
template <typename ET> constexpr int kMostLoads = std::is_same<ET, Fp32>::value ? 2 : 4;   // (no U = 4 instance of an fp32 kernel)
bool four_loads(int dtype, int64_t m) { return dtype != 0 && (g_inflight == 4 || (g_inflight == 0 && m <= 400000)); }

// elements per access for rows of c elements behind these base pointers: a 16-byte piece, 4 halfs (8 B) or 1
int vec_width(int dtype, int c, const void *a, const void *b) {
  const int piece = dtype == 0 ? 4 : 8;
  if (c % piece == 0 && aligned(a, 16) && aligned(b, 16)) return piece;
  if (dtype != 0 && (c & 3) == 0 && aligned(a, 8) && aligned(b, 8)) return 4;
  return 1;
}

// The CSR entries and K8 / K9 behind the _f32 (h = false, dtype 0) and _h (h = true: dtype must be 1 or 2) C entries;
// `what` names the entry in the error texts
template <typename ET> const typename Elem<ET>::T *rows(const void *p) { return reinterpret_cast<const typename Elem<ET>::T *>(p); }
template <typename ET> typename Elem<ET>::T *rows(void *p) { return reinterpret_cast<typename Elem<ET>::T *>(p); }

int voxelize_fwd_csr_any(const char *what, bool h, int32_t dtype, const void *feats, const int64_t *order, const int64_t *rowptr,
                         const int32_t *counts, int64_t m, int32_t c, void *out, void *stream) {
  if (m < 0 || c <= 0) { set_error("%s: bad sizes", what); return PCS_EINVAL; }
  if (h && bad_half(what, dtype)) return PCS_EINVAL;
  if (m == 0) return PCS_OK;
  if (!order || !rowptr || !counts || !out) { set_error("%s: null pointer", what); return PCS_EINVAL; }
  hipStream_t st = as_stream(stream);
  const int vw = vec_width(dtype, c, feats, out);
  const bool four = four_loads(dtype, m);
  const RowLaunch rl = row_launch(m, c / vw, kRowsPow2);
  PCS_DTYPE_VEC(dtype, vw, {
    if (four) hipLaunchKernelGGL((voxelize_fwd_csr_kernel<ET, V, kMostLoads<ET>>), rl.grid, rl.block, 0, st, rows<ET>(feats), order, rowptr, counts, m, c, rl.cv, rows<ET>(out));
    else hipLaunchKernelGGL((voxelize_fwd_csr_kernel<ET, V, 2>), rl.grid, rl.block, 0, st, rows<ET>(feats), order, rowptr, counts, m, c, rl.cv, rows<ET>(out));
  });
  return check_launch(what);
}

int voxelize_bwd_any(const char *what, bool h, int32_t dtype, const void *gout, const int32_t *idx, const int32_t *counts, int64_t n,
                     int32_t c, void *gin, void *stream) {
  if (n < 0 || c <= 0) { set_error("%s: bad sizes", what); return PCS_EINVAL; }
  if (h && bad_half(what, dtype)) return PCS_EINVAL;
  if (n == 0) return PCS_OK;
  if (!gout || !idx || !counts || !gin) { set_error("%s: null pointer", what); return PCS_EINVAL; }
  const int vw = vec_width(dtype, c, gout, gin);
  const RowLaunch rl = row_launch(n, c / vw, kRowsPow2);
  PCS_DTYPE_VEC(dtype, vw, hipLaunchKernelGGL((voxelize_bwd_kernel<ET, V>), rl.grid, rl.block, 0, as_stream(stream), rows<ET>(gout),
                                              idx, counts, n, c, rl.cv, rows<ET>(gin)));
  return check_launch(what);
}

int devoxelize_fwd_any(const char *what, bool h, int32_t dtype, const void *feat, const int32_t *idx8, const float *w8, int64_t n,
                       int32_t c, void *out, void *stream) {
  if (n < 0 || c <= 0) { set_error("%s: bad sizes", what); return PCS_EINVAL; }
  if (h && bad_half(what, dtype)) return PCS_EINVAL;
  if (n == 0) return PCS_OK;
  if (!idx8 || !w8 || !out) { set_error("%s: null pointer", what); return PCS_EINVAL; }
  const int vw = vec_width(dtype, c, feat, out);
  const RowLaunch rl = row_launch(n, c / vw, kRowsPow2);
  PCS_DTYPE_VEC(dtype, vw, hipLaunchKernelGGL((devoxelize_fwd_kernel<ET, V>), rl.grid, rl.block, 0, as_stream(stream), rows<ET>(feat),
                                              idx8, w8, n, c, rl.cv, rows<ET>(out)));
  return check_launch(what);
}

int devoxelize_bwd_csr_any(const char *what, bool h, int32_t dtype, const void *gout, const int64_t *order, const int64_t *rowptr,
                           const float *w8, int64_t m, int32_t c, void *gfeat, void *stream) {
  if (m < 0 || c <= 0) { set_error("%s: bad sizes", what); return PCS_EINVAL; }
  if (h && bad_half(what, dtype)) return PCS_EINVAL;
  if (m == 0) return PCS_OK;
  if (!gout || !order || !rowptr || !w8 || !gfeat) { set_error("%s: null pointer", what); return PCS_EINVAL; }
  hipStream_t st = as_stream(stream);
  const int vw = vec_width(dtype, c, gout, gfeat);
  // wave-per-voxel form: long segments (coarse levels) of narrow rows, up to 8 vectors = 128 bytes (fp32 c <= 32, 16-bit
  // c <= 64 at V = 8). On a stride-1 level (~8 entries per voxel, m ~ 1 M) most of its entry lanes idle and the
  // row-per-thread-row form is 2x faster [r4: 257 vs 117 us]; m is the proxy for the segment length here (the entry count
  // is not an argument of this call)
  if (vw != 1 && c / vw <= 8 && m <= 400000) {
    int64_t g = ceil_div(m, 4);
    if (g > 256 * 64) g = 256 * 64;
    PCS_DTYPE(dtype, {
      if (vw == Piece<ET>::V) hipLaunchKernelGGL((devoxelize_bwd_csr_narrow_kernel<ET, Piece<ET>::V>), dim3((unsigned)g), dim3(256), 0, st, rows<ET>(gout), order, rowptr, w8, m, c, c / vw, rows<ET>(gfeat));
      else hipLaunchKernelGGL((devoxelize_bwd_csr_narrow_kernel<ET, 4>), dim3((unsigned)g), dim3(256), 0, st, rows<ET>(gout), order, rowptr, w8, m, c, c / vw, rows<ET>(gfeat));
    });
  } else {
    const bool four = four_loads(dtype, m);
    const RowLaunch rl = row_launch(m, c / vw, kRowsPow2);
    PCS_DTYPE_VEC(dtype, vw, {
      if (four) hipLaunchKernelGGL((devoxelize_bwd_csr_kernel<ET, V, kMostLoads<ET>>), rl.grid, rl.block, 0, st, rows<ET>(gout), order, rowptr, w8, m, c, rl.cv, rows<ET>(gfeat));
      else hipLaunchKernelGGL((devoxelize_bwd_csr_kernel<ET, V, 2>), rl.grid, rl.block, 0, st, rows<ET>(gout), order, rowptr, w8, m, c, rl.cv, rows<ET>(gfeat));
    });
  }
  return check_launch(what);
}

}  // namespace

extern "C" void pcs_debug_pointvoxel_h_inflight(int32_t loads) { g_inflight = (loads == 2 || loads == 4) ? loads : 0; }

extern "C" int pcs_voxelize_fwd_csr_f32(const float *feats, const int64_t *order, const int64_t *rowptr,
                                        const int32_t *counts, int64_t m, int32_t c, float *out, void *stream) {
  return voxelize_fwd_csr_any("pcs_voxelize_fwd_csr", false, 0, feats, order, rowptr, counts, m, c, out, stream);
}
extern "C" int pcs_voxelize_fwd_csr_h(const void *feats, const int64_t *order, const int64_t *rowptr, const int32_t *counts,
                                      int64_t m, int32_t c, int32_t dtype, void *out, void *stream) {
  return voxelize_fwd_csr_any("pcs_voxelize_fwd_csr_h", true, dtype, feats, order, rowptr, counts, m, c, out, stream);
}

extern "C" int pcs_voxelize_bwd_f32(const float *gout, const int32_t *idx, const int32_t *counts,
                                    int64_t n, int32_t c, float *gin, void *stream) {
  return voxelize_bwd_any("pcs_voxelize_bwd", false, 0, gout, idx, counts, n, c, gin, stream);
}
extern "C" int pcs_voxelize_bwd_h(const void *gout, const int32_t *idx, const int32_t *counts, int64_t n, int32_t c,
                                  int32_t dtype, void *gin, void *stream) {
  return voxelize_bwd_any("pcs_voxelize_bwd_h", true, dtype, gout, idx, counts, n, c, gin, stream);
}

extern "C" int pcs_devoxelize_fwd_f32(const float *feat, const int32_t *idx8, const float *w8,
                                      int64_t n, int32_t c, float *out, void *stream) {
  return devoxelize_fwd_any("pcs_devoxelize_fwd", false, 0, feat, idx8, w8, n, c, out, stream);
}
extern "C" int pcs_devoxelize_fwd_h(const void *feat, const int32_t *idx8, const float *w8, int64_t n, int32_t c,
                                    int32_t dtype, void *out, void *stream) {
  return devoxelize_fwd_any("pcs_devoxelize_fwd_h", true, dtype, feat, idx8, w8, n, c, out, stream);
}

extern "C" int pcs_devoxelize_bwd_csr_f32(const float *gout, const int64_t *order,
                                          const int64_t *rowptr, const float *w8, int64_t m,
                                          int32_t c, float *gfeat, void *stream) {
  return devoxelize_bwd_csr_any("pcs_devoxelize_bwd_csr", false, 0, gout, order, rowptr, w8, m, c, gfeat, stream);
}
extern "C" int pcs_devoxelize_bwd_csr_h(const void *gout, const int64_t *order, const int64_t *rowptr, const float *w8,
                                        int64_t m, int32_t c, int32_t dtype, void *gfeat, void *stream) {
  return devoxelize_bwd_csr_any("pcs_devoxelize_bwd_csr_h", true, dtype, gout, order, rowptr, w8, m, c, gfeat, stream);
}

extern "C" int pcs_voxelize_fwd_f32(const float *feats, const int32_t *idx,
                                    const int32_t *counts, int64_t n, int64_t m, int32_t c,
                                    float *out, void *stream) {
  if (n < 0 || m < 0 || c <= 0) { set_error("pcs_voxelize_fwd: bad sizes"); return PCS_EINVAL; }
  hipStream_t st = as_stream(stream);
  if (m > 0) {
    if (!out) { set_error("pcs_voxelize_fwd: null out"); return PCS_EINVAL; }
    if (hipMemsetAsync(out, 0, (size_t)m * c * 4, st) != hipSuccess) { set_error("pcs_voxelize_fwd: memset failed"); return PCS_ELAUNCH; }
  }
  if (n == 0 || m == 0) return PCS_OK;
  if (!feats || !idx || !counts) { set_error("pcs_voxelize_fwd: null input"); return PCS_EINVAL; }
  if ((c & 3) == 0 && aligned(feats, 16)) {
    RowLaunch rl = row_launch(n, c / 4, kRowsPow2);
    hipLaunchKernelGGL(voxelize_fwd_kernel<4>, rl.grid, rl.block, 0, st, feats, idx, counts, n, m, c, rl.cv, out);
  } else {
    RowLaunch rl = row_launch(n, c, kRowsPow2);
    hipLaunchKernelGGL(voxelize_fwd_kernel<1>, rl.grid, rl.block, 0, st, feats, idx, counts, n, m, c, rl.cv, out);
  }
  return check_launch("pcs_voxelize_fwd");
}

extern "C" int pcs_devoxelize_bwd_f32(const float *gout, const int32_t *idx8, const float *w8,
                                      int64_t n, int64_t m, int32_t c, float *gfeat,
                                      void *stream) {
  if (n < 0 || m < 0 || c <= 0) { set_error("pcs_devoxelize_bwd: bad sizes"); return PCS_EINVAL; }
  hipStream_t st = as_stream(stream);
  if (m > 0) {
    if (!gfeat) { set_error("pcs_devoxelize_bwd: null gfeat"); return PCS_EINVAL; }
    if (hipMemsetAsync(gfeat, 0, (size_t)m * c * 4, st) != hipSuccess) { set_error("pcs_devoxelize_bwd: memset failed"); return PCS_ELAUNCH; }
  }
  if (n == 0 || m == 0) return PCS_OK;
  if (!gout || !idx8 || !w8) { set_error("pcs_devoxelize_bwd: null pointer"); return PCS_EINVAL; }
  if ((c & 3) == 0 && aligned(gout, 16)) {
    RowLaunch rl = row_launch(n, c / 4, kRowsPow2);
    hipLaunchKernelGGL(devoxelize_bwd_kernel<4>, rl.grid, rl.block, 0, st, gout, idx8, w8, n, c, rl.cv, gfeat);
  } else {
    RowLaunch rl = row_launch(n, c, kRowsPow2);
    hipLaunchKernelGGL(devoxelize_bwd_kernel<1>, rl.grid, rl.block, 0, st, gout, idx8, w8, n, c, rl.cv, gfeat);
  }
  return check_launch("pcs_devoxelize_bwd");
}

extern "C" int pcs_ti_weights_f32(const float *coords, int32_t coord_ld, const int64_t *idx_query,
                                  int64_t n, float scale, float *w, void *stream) {
  if (n < 0 || coord_ld < 3) { set_error("pcs_ti_weights: bad sizes"); return PCS_EINVAL; }
  if (n == 0) return PCS_OK;
  if (!coords || !idx_query || !w) { set_error("pcs_ti_weights: null pointer"); return PCS_EINVAL; }
  const int scaled = (scale != 1.0f);
  const float inv_s3 = 1.0f / (scale * scale * scale);
  hipLaunchKernelGGL(ti_weights_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, as_stream(stream),
                     coords, coord_ld, idx_query, n, scale, inv_s3, scaled, w);
  return check_launch("pcs_ti_weights");
}

extern "C" int pcs_corner_map_f32(const float *coords, int32_t coord_ld, int64_t n, int32_t stride, const void *table,
                                  int64_t capacity, int32_t *idx8, float *w8, void *stream) {
  if (n < 0 || coord_ld < 4 || stride <= 0 || !table || capacity <= 0 || (capacity & (capacity - 1))) {
    set_error("pcs_corner_map_f32: bad args");
    return PCS_EINVAL;
  }
  if (n == 0) return PCS_OK;
  if (!coords || !idx8 || !w8 || !aligned(idx8, 16) || !aligned(w8, 16)) { set_error("pcs_corner_map_f32: bad pointers"); return PCS_EINVAL; }
  hipLaunchKernelGGL(corner_map_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, as_stream(stream), coords, coord_ld, n,
                     stride, make_view(table, capacity), idx8, w8);
  return check_launch("pcs_corner_map_f32");
}

