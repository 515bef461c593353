// K7-K10 point<->voxel kernels with 16-bit feature storage (bf16 / fp16) -- gfx950. The fp32 twins: pointvoxel.hip.
// Reference semantics: TS:torchsparse/backend/voxelize/voxelize_cuda.cu:12-80 and
// TS:torchsparse/backend/devoxelize/devoxelize_cuda.cu:11-98, which the reference dispatches over
// AT_DISPATCH_FLOATING_TYPES_AND_HALF and accumulates in scalar_t through global memory. Here the features arrive and
// leave in 16 bits, every sum lives in fp32 registers in a fixed order and is rounded ONCE on the store (nearest even).
// All HBM-bound: half rows are half the bytes of pointvoxel.hip's, and no cast pass stands before or behind the kernel.
// Same launch shape as the fp32 kernels: a 256-thread workgroup covers 256/TX rows, TX lanes x V halfs per row with
// V = 8 (16-byte accesses), 4 (8-byte) or 1; every output row is written exactly once (no memset, no atomics).
#include "pcs_common.h"

using namespace pcs;

namespace {

// storage formats (the dtype argument of the C entries: 1 bf16, 2 fp16); all arithmetic is fp32
struct B16 {};
struct H16 {};
__device__ __forceinline__ float h2f(B16, uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
__device__ __forceinline__ float h2f(H16, uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
__device__ __forceinline__ uint16_t f2h(B16, float f) {  // round to nearest even; NaN stays NaN
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
__device__ __forceinline__ uint16_t f2h(H16, float f) { const _Float16 h = (_Float16)f; return __builtin_bit_cast(uint16_t, h); }

// V halfs of a row as they sit in memory
template <int V> struct Raw;
template <> struct Raw<8> { using T = uint4; };
template <> struct Raw<4> { using T = uint2; };
template <> struct Raw<1> { using T = uint16_t; };

template <int V> struct Acc { float f[V]; };

template <int V> __device__ __forceinline__ typename Raw<V>::T ld_raw(const uint16_t *row, int j) {
  return reinterpret_cast<const typename Raw<V>::T *>(row)[j];
}
template <typename HT> __device__ __forceinline__ void unpack2(uint32_t r, float &lo, float &hi) {
  lo = h2f(HT{}, (uint16_t)(r & 0xFFFFu));
  hi = h2f(HT{}, (uint16_t)(r >> 16));
}
template <typename HT> __device__ __forceinline__ Acc<8> widen(const uint4 &r) {
  Acc<8> a;
  unpack2<HT>(r.x, a.f[0], a.f[1]); unpack2<HT>(r.y, a.f[2], a.f[3]);
  unpack2<HT>(r.z, a.f[4], a.f[5]); unpack2<HT>(r.w, a.f[6], a.f[7]);
  return a;
}
template <typename HT> __device__ __forceinline__ Acc<4> widen(const uint2 &r) {
  Acc<4> a;
  unpack2<HT>(r.x, a.f[0], a.f[1]); unpack2<HT>(r.y, a.f[2], a.f[3]);
  return a;
}
template <typename HT> __device__ __forceinline__ Acc<1> widen(const uint16_t &r) {
  Acc<1> a;
  a.f[0] = h2f(HT{}, r);
  return a;
}
template <typename HT> __device__ __forceinline__ uint32_t pack2(float lo, float hi) {
  return (uint32_t)f2h(HT{}, lo) | ((uint32_t)f2h(HT{}, hi) << 16);
}
// the one rounding of every output element
template <typename HT> __device__ __forceinline__ void st_row(uint16_t *row, int j, const Acc<8> &a) {
  reinterpret_cast<uint4 *>(row)[j] = make_uint4(pack2<HT>(a.f[0], a.f[1]), pack2<HT>(a.f[2], a.f[3]),
                                                 pack2<HT>(a.f[4], a.f[5]), pack2<HT>(a.f[6], a.f[7]));
}
template <typename HT> __device__ __forceinline__ void st_row(uint16_t *row, int j, const Acc<4> &a) {
  reinterpret_cast<uint2 *>(row)[j] = make_uint2(pack2<HT>(a.f[0], a.f[1]), pack2<HT>(a.f[2], a.f[3]));
}
template <typename HT> __device__ __forceinline__ void st_row(uint16_t *row, int j, const Acc<1> &a) { row[j] = f2h(HT{}, a.f[0]); }

template <int V> __device__ __forceinline__ void azero(Acc<V> &a) {
#pragma unroll
  for (int q = 0; q < V; ++q) a.f[q] = 0.f;
}
template <int V> __device__ __forceinline__ void add_div(Acc<V> &a, const Acc<V> &x, float d) {  // divide, then add
#pragma unroll
  for (int q = 0; q < V; ++q) a.f[q] += x.f[q] / d;
}
template <int V> __device__ __forceinline__ void add_mul(Acc<V> &a, float w, const Acc<V> &x) {
#pragma unroll
  for (int q = 0; q < V; ++q) a.f[q] = fmaf(w, x.f[q], a.f[q]);
}

// Row-tiled 2-D launch of pointvoxel.hip: TX lanes walk the vectors of one row, TY rows per block. A row wider than
// 64 vectors (c up to the reference's 1024) takes more than one pass of the lane row.
struct RowLaunch {
  dim3 block, grid;
  int cv;  // vectors per row
};

template <int V>
RowLaunch row_launch(int64_t n, int c) {
  RowLaunch r;
  r.cv = c / V;
  int tx = 1;
  while (tx < r.cv && tx < 64) tx <<= 1;
  const int ty = 256 / tx;
  r.block = dim3(tx, ty);
  int64_t g = ceil_div(n, ty);
  if (g > 256 * 16) g = 256 * 16;
  if (g < 1) g = 1;
  r.grid = dim3((unsigned)g);
  return r;
}

// R consecutive entries of a run: their R row loads issued together, then added in entry order (divide, then add)
template <typename HT, int V, int R>
__device__ __forceinline__ void vox_rows(Acc<V> &acc, const uint16_t *__restrict__ feats, const int64_t *__restrict__ ord, int c,
                                         int j, float fc) {
  int64_t p[R];
  typename Raw<V>::T r[R];
#pragma unroll
  for (int u = 0; u < R; ++u) p[u] = ord[u];
#pragma unroll
  for (int u = 0; u < R; ++u) r[u] = ld_raw<V>(feats + p[u] * c, j);
#pragma unroll
  for (int u = 0; u < R; ++u) add_div(acc, widen<HT>(r[u]), fc);
}

// the same for K10: entry p = flat position i * 8 + k of (point, corner); weight w8[p], row gout[p >> 3]
template <typename HT, int V, int R>
__device__ __forceinline__ void devox_rows(Acc<V> &acc, const uint16_t *__restrict__ gout, const int64_t *__restrict__ ord,
                                           const float *__restrict__ w8, int c, int j) {
  int64_t p[R];
  float w[R];
  typename Raw<V>::T r[R];
#pragma unroll
  for (int u = 0; u < R; ++u) p[u] = ord[u];
#pragma unroll
  for (int u = 0; u < R; ++u) { w[u] = w8[p[u]]; r[u] = ld_raw<V>(gout + (p[u] >> 3) * c, j); }
#pragma unroll
  for (int u = 0; u < R; ++u) add_mul(acc, w[u], widen<HT>(r[u]));
}

// ---- K7, CSR form: out[v] = sum over the run of v of feats[order[e]] / counts[v] ------------------------------------------
// U independent row loads in flight per lane (2 as the fp32 kernel, or 4: a half row's registers are half as many; what is
// left of a run after the groups of 4 goes as a pair and a single). The loaded rows are added in `order` order whatever U
// is, so both give the same bits.
template <typename HT, int V, int U>
__global__ void __launch_bounds__(256) voxelize_fwd_csr_h_kernel(const uint16_t *__restrict__ feats,
                                                                 const int64_t *__restrict__ order,
                                                                 const int64_t *__restrict__ rowptr,
                                                                 const int32_t *__restrict__ counts, int64_t m, int c, int cv,
                                                                 uint16_t *__restrict__ out) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; v < m; v += (int64_t)gridDim.x * blockDim.y) {
    const int64_t e0 = rowptr[v], e1 = rowptr[v + 1];
    const int32_t cnt = counts[v];
    const float fc = (float)(cnt > 0 ? cnt : 1);
    uint16_t *dst = out + v * c;
    for (int j = threadIdx.x; j < cv; j += blockDim.x) {
      Acc<V> acc;
      azero(acc);
      if (cnt != 0) {
        int64_t e = e0;
        for (; e + U <= e1; e += U) vox_rows<HT, V, U>(acc, feats, order + e, c, j, fc);
        if (U == 4 && e + 2 <= e1) { vox_rows<HT, V, 2>(acc, feats, order + e, c, j, fc); e += 2; }
        if (e < e1) vox_rows<HT, V, 1>(acc, feats, order + e, c, j, fc);
      }
      st_row<HT>(dst, j, acc);
    }
  }
}

// ---- K8: gin[i] = gout[idx[i]] / counts[idx[i]], exact zeros where the point has no voxel --------------------------------
template <typename HT, int V>
__global__ void __launch_bounds__(256) voxelize_bwd_h_kernel(const uint16_t *__restrict__ gout,
                                                             const int32_t *__restrict__ idx,
                                                             const int32_t *__restrict__ counts, int64_t n, int c, int cv,
                                                             uint16_t *__restrict__ gin) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; i < n; i += (int64_t)gridDim.x * blockDim.y) {
    const int32_t pos = idx[i];
    uint16_t *dst = gin + i * c;
    const int32_t cnt = pos >= 0 ? counts[pos] : 0;
    const float fc = (float)(cnt != 0 ? cnt : 1);
    const uint16_t *src = gout + (int64_t)(pos >= 0 ? pos : 0) * c;
    for (int j = threadIdx.x; j < cv; j += blockDim.x) {
      Acc<V> acc;
      azero(acc);
      if (cnt != 0) add_div(acc, widen<HT>(ld_raw<V>(src, j)), fc);
      st_row<HT>(dst, j, acc);
    }
  }
}

// ---- K9: trilinear gather, the 8 corners summed in registers in k = 0..7 order -------------------------------------------
template <typename HT, int V>
__global__ void __launch_bounds__(256) devoxelize_fwd_h_kernel(const uint16_t *__restrict__ feat,
                                                               const int32_t *__restrict__ idx8,
                                                               const float *__restrict__ w8, int64_t n, int c, int cv,
                                                               uint16_t *__restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; i < n; i += (int64_t)gridDim.x * blockDim.y) {
    int32_t id[8];
    float w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { id[k] = idx8[i * 8 + k]; w[k] = w8[i * 8 + k]; }
    uint16_t *dst = out + i * c;
    for (int j = threadIdx.x; j < cv; j += blockDim.x) {
      Acc<V> acc;
      azero(acc);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (id[k] >= 0) add_mul(acc, w[k], widen<HT>(ld_raw<V>(feat + (int64_t)id[k] * c, j)));
      }
      st_row<HT>(dst, j, acc);
    }
  }
}

// ---- K10, CSR form: gfeat[v] = sum over the run of v of w8[order[e]] * gout[order[e] >> 3] --------------------------------
// thread-row form: one row of TX lanes per voxel, U independent row loads in flight, added in `order` order.
template <typename HT, int V, int U>
__global__ void __launch_bounds__(256) devoxelize_bwd_csr_h_kernel(const uint16_t *__restrict__ gout,
                                                                   const int64_t *__restrict__ order,
                                                                   const int64_t *__restrict__ rowptr,
                                                                   const float *__restrict__ w8, int64_t m, int c, int cv,
                                                                   uint16_t *__restrict__ gfeat) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; v < m; v += (int64_t)gridDim.x * blockDim.y) {
    const int64_t e0 = rowptr[v], e1 = rowptr[v + 1];
    uint16_t *dst = gfeat + v * c;
    for (int j = threadIdx.x; j < cv; j += blockDim.x) {
      Acc<V> acc;
      azero(acc);
      int64_t e = e0;
      for (; e + U <= e1; e += U) devox_rows<HT, V, U>(acc, gout, order + e, w8, c, j);
      if (U == 4 && e + 2 <= e1) { devox_rows<HT, V, 2>(acc, gout, order + e, w8, c, j); e += 2; }
      if (e < e1) devox_rows<HT, V, 1>(acc, gout, order + e, w8, c, j);
      st_row<HT>(dst, j, acc);
    }
  }
}

// wave-per-voxel form for NARROW rows (at most 8 vectors: c <= 64 at V = 8, c <= 32 at V = 4) on coarse levels, the shape
// of devoxelize_bwd_csr_narrow_kernel: 8 x-lanes over the row's vectors times 8 entry lanes striding over the voxel's run,
// two independent row loads in flight per lane, the 8 partial rows combined by shuffles in a fixed order (deterministic).
template <typename HT, int V>
__global__ void __launch_bounds__(256) devoxelize_bwd_csr_narrow_h_kernel(const uint16_t *__restrict__ gout,
                                                                          const int64_t *__restrict__ order,
                                                                          const int64_t *__restrict__ rowptr,
                                                                          const float *__restrict__ w8, int64_t m, int c, int cv,
                                                                          uint16_t *__restrict__ gfeat) {
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
        const typename Raw<V>::T r0 = ld_raw<V>(gout + (p0 >> 3) * c, x);
        const typename Raw<V>::T r1 = ld_raw<V>(gout + (p1 >> 3) * c, x);
        add_mul(acc, w0, widen<HT>(r0));
        if (two) add_mul(acc, w1, widen<HT>(r1));   // (not a zero weight: 0 x Inf of a diverged gradient must stay out)
      }
    }
#pragma unroll
    for (int o = 32; o >= 8; o >>= 1) {
#pragma unroll
      for (int q = 0; q < V; ++q) acc.f[q] += __shfl_down(acc.f[q], o, 64);
    }
    if (el == 0 && x < cv) st_row<HT>(gfeat + v * c, x, acc);
  }
}

// Row loads in flight per lane in the two segmented lane-row kernels. Measured on the 12-scan bench batch, bf16
// (profiles/pointvoxel_half_bench.json): 4 loads win where the runs are long -- stride 16 / C 256: voxelize 354 -> 287 us,
// devoxelize backward 806 -> 581 us; stride 4 / C 128: 150 -> 146 and 200 -> 175 us -- and lose on a stride-1 level, where a
// voxel has a handful of entries (C 96 devoxelize backward 184 -> 217 us). m is the proxy for the run length, with the
// threshold the wave-per-voxel form already uses. 0 = this rule; pcs_debug_pointvoxel_h_inflight forces 2 or 4.
int g_inflight = 0;
bool four_loads(int64_t m) { return g_inflight == 4 || (g_inflight == 0 && m <= 400000); }

bool bad_half(int32_t dtype) { return dtype != 1 && dtype != 2; }
bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// halfs per access for rows of c halfs behind these base pointers: 8 (16 B), 4 (8 B) or 1
int vec_width(int c, const void *a, const void *b) {
  if ((c & 7) == 0 && aligned(a, 16) && aligned(b, 16)) return 8;
  if ((c & 3) == 0 && aligned(a, 8) && aligned(b, 8)) return 4;
  return 1;
}

#define PCS_PV_DTYPE(dtype, ...)                                    \
  do {                                                              \
    if ((dtype) == 1) { using HT = B16; __VA_ARGS__; }              \
    else { using HT = H16; __VA_ARGS__; }                           \
  } while (0)

#define PCS_PV_VEC(vw, ...)                                         \
  do {                                                              \
    if ((vw) == 8) { constexpr int V = 8; __VA_ARGS__; }            \
    else if ((vw) == 4) { constexpr int V = 4; __VA_ARGS__; }       \
    else { constexpr int V = 1; __VA_ARGS__; }                      \
  } while (0)

}  // namespace

extern "C" void pcs_debug_pointvoxel_h_inflight(int32_t loads) { g_inflight = (loads == 2 || loads == 4) ? loads : 0; }

extern "C" int pcs_voxelize_fwd_csr_h(const void *feats, const int64_t *order, const int64_t *rowptr, const int32_t *counts,
                                      int64_t m, int32_t c, int32_t dtype, void *out, void *stream) {
  if (m < 0 || c <= 0) { set_error("pcs_voxelize_fwd_csr_h: bad sizes"); return PCS_EINVAL; }
  if (bad_half(dtype)) { set_error("pcs_voxelize_fwd_csr_h: dtype must be 1 (bf16) or 2 (fp16), got %d", (int)dtype); return PCS_EINVAL; }
  if (m == 0) return PCS_OK;
  if (!order || !rowptr || !counts || !out) { set_error("pcs_voxelize_fwd_csr_h: null pointer"); return PCS_EINVAL; }
  hipStream_t st = as_stream(stream);
  const uint16_t *f = reinterpret_cast<const uint16_t *>(feats);
  uint16_t *o = reinterpret_cast<uint16_t *>(out);
  const int vw = vec_width(c, feats, out);
  const bool four = four_loads(m);
  PCS_PV_DTYPE(dtype, PCS_PV_VEC(vw, {
    RowLaunch rl = row_launch<V>(m, c);
    if (four) hipLaunchKernelGGL((voxelize_fwd_csr_h_kernel<HT, V, 4>), rl.grid, rl.block, 0, st, f, order, rowptr, counts, m, c, rl.cv, o);
    else hipLaunchKernelGGL((voxelize_fwd_csr_h_kernel<HT, V, 2>), rl.grid, rl.block, 0, st, f, order, rowptr, counts, m, c, rl.cv, o);
  }));
  return check_launch("pcs_voxelize_fwd_csr_h");
}

extern "C" int pcs_voxelize_bwd_h(const void *gout, const int32_t *idx, const int32_t *counts, int64_t n, int32_t c,
                                  int32_t dtype, void *gin, void *stream) {
  if (n < 0 || c <= 0) { set_error("pcs_voxelize_bwd_h: bad sizes"); return PCS_EINVAL; }
  if (bad_half(dtype)) { set_error("pcs_voxelize_bwd_h: dtype must be 1 (bf16) or 2 (fp16), got %d", (int)dtype); return PCS_EINVAL; }
  if (n == 0) return PCS_OK;
  if (!gout || !idx || !counts || !gin) { set_error("pcs_voxelize_bwd_h: null pointer"); return PCS_EINVAL; }
  hipStream_t st = as_stream(stream);
  const uint16_t *g = reinterpret_cast<const uint16_t *>(gout);
  uint16_t *o = reinterpret_cast<uint16_t *>(gin);
  const int vw = vec_width(c, gout, gin);
  PCS_PV_DTYPE(dtype, PCS_PV_VEC(vw, {
    RowLaunch rl = row_launch<V>(n, c);
    hipLaunchKernelGGL((voxelize_bwd_h_kernel<HT, V>), rl.grid, rl.block, 0, st, g, idx, counts, n, c, rl.cv, o);
  }));
  return check_launch("pcs_voxelize_bwd_h");
}

extern "C" int pcs_devoxelize_fwd_h(const void *feat, const int32_t *idx8, const float *w8, int64_t n, int32_t c,
                                    int32_t dtype, void *out, void *stream) {
  if (n < 0 || c <= 0) { set_error("pcs_devoxelize_fwd_h: bad sizes"); return PCS_EINVAL; }
  if (bad_half(dtype)) { set_error("pcs_devoxelize_fwd_h: dtype must be 1 (bf16) or 2 (fp16), got %d", (int)dtype); return PCS_EINVAL; }
  if (n == 0) return PCS_OK;
  if (!idx8 || !w8 || !out) { set_error("pcs_devoxelize_fwd_h: null pointer"); return PCS_EINVAL; }
  hipStream_t st = as_stream(stream);
  const uint16_t *f = reinterpret_cast<const uint16_t *>(feat);
  uint16_t *o = reinterpret_cast<uint16_t *>(out);
  const int vw = vec_width(c, feat, out);
  PCS_PV_DTYPE(dtype, PCS_PV_VEC(vw, {
    RowLaunch rl = row_launch<V>(n, c);
    hipLaunchKernelGGL((devoxelize_fwd_h_kernel<HT, V>), rl.grid, rl.block, 0, st, f, idx8, w8, n, c, rl.cv, o);
  }));
  return check_launch("pcs_devoxelize_fwd_h");
}

extern "C" int pcs_devoxelize_bwd_csr_h(const void *gout, const int64_t *order, const int64_t *rowptr, const float *w8,
                                        int64_t m, int32_t c, int32_t dtype, void *gfeat, void *stream) {
  if (m < 0 || c <= 0) { set_error("pcs_devoxelize_bwd_csr_h: bad sizes"); return PCS_EINVAL; }
  if (bad_half(dtype)) { set_error("pcs_devoxelize_bwd_csr_h: dtype must be 1 (bf16) or 2 (fp16), got %d", (int)dtype); return PCS_EINVAL; }
  if (m == 0) return PCS_OK;
  if (!gout || !order || !rowptr || !w8 || !gfeat) { set_error("pcs_devoxelize_bwd_csr_h: null pointer"); return PCS_EINVAL; }
  hipStream_t st = as_stream(stream);
  const uint16_t *g = reinterpret_cast<const uint16_t *>(gout);
  uint16_t *o = reinterpret_cast<uint16_t *>(gfeat);
  const int vw = vec_width(c, gout, gfeat);
  // wave-per-voxel form: long runs (coarse levels) of narrow rows; m is the proxy for the run length as in
  // pcs_devoxelize_bwd_csr_f32. A row of up to 8 vectors is 128 bytes at V = 8 (c <= 64), what the fp32 form takes at c <= 32.
  if (vw != 1 && c / vw <= 8 && m <= 400000) {
    int64_t grid = ceil_div(m, 4);
    if (grid > 256 * 64) grid = 256 * 64;
    PCS_PV_DTYPE(dtype, {
      if (vw == 8) hipLaunchKernelGGL((devoxelize_bwd_csr_narrow_h_kernel<HT, 8>), dim3((unsigned)grid), dim3(256), 0, st, g, order, rowptr, w8, m, c, c / 8, o);
      else hipLaunchKernelGGL((devoxelize_bwd_csr_narrow_h_kernel<HT, 4>), dim3((unsigned)grid), dim3(256), 0, st, g, order, rowptr, w8, m, c, c / 4, o);
    });
  } else {
    const bool four = four_loads(m);
    PCS_PV_DTYPE(dtype, PCS_PV_VEC(vw, {
      RowLaunch rl = row_launch<V>(m, c);
      if (four) hipLaunchKernelGGL((devoxelize_bwd_csr_h_kernel<HT, V, 4>), rl.grid, rl.block, 0, st, g, order, rowptr, w8, m, c, rl.cv, o);
      else hipLaunchKernelGGL((devoxelize_bwd_csr_h_kernel<HT, V, 2>), rl.grid, rl.block, 0, st, g, order, rowptr, w8, m, c, rl.cv, o);
    }));
  }
  return check_launch("pcs_devoxelize_bwd_csr_h");
}
