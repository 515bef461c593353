// ReconBlock (DDCM) gate of Cylinder3D -- gfx950, HBM-bound. The reference computes, at the finest level
// (R:pcseg/model/segmentor/voxel/cylinder3d/cylinder_ts.py:337-384),
//     out = x * ( sigmoid(BN0(conv3x1x1(x))) + sigmoid(BN1(conv1x3x1(x))) + sigmoid(BN2(conv1x1x3(x))) )
// as three BatchNorm applies, three sigmoids, two adds and a multiply: about 21 passes over an (N, C) tensor forward and
// about 29 backward. Here, with the three conv outputs a0, a1, a2 given:
//   forward       out = x * ((s0 + s1) + s2),  s_k = 1 / (1 + expf(-bn_k(a_k)))                     4 reads, 1 write
//   bwd stats     [sum g_k | sum g_k * xhat_k], g_k = dy * x * s_k * (1 - s_k), for the three k      5 reads
//   bwd apply     dx_gate = dy * ((s0 + s1) + s2),
//                 da_k = (g_k - sum_g_k / N - xhat_k * sum_gxhat_k / N) * invstd_k * w_k             5 reads, 4 writes
// bn_k(a) = fma(a, sc, sh) with sc = invstd * gamma, sh = beta - mean * sc: the expression of bn_apply_kernel (norm.hip);
// xhat_k = (a - mean) * invstd as the BatchNorm backward passes form it. All arithmetic in fp32 registers, one rounding on
// each store; the sigmoids are recomputed from a_k in backward and never written. Rows move in 16-byte pieces (4 floats or
// 8 halfs per lane), grid-stride over the rows with a capped grid. No atomics: every output element is written exactly once
// and the statistics are two-level with a fixed order (per-workgroup partial rows, then a double reduction), so results
// are deterministic. The 6c-double vector of the statistics is what a data-parallel run all-reduces: one collective for
// the whole block.
#include "row_storage.h"

using namespace pcs;

namespace {

__device__ __forceinline__ float sigmoidf(float t) { return 1.f / (1.f + expf(-t)); }

// the three branches' tensors and per-channel parameters; stat3 = 3 x (mean | invstd), gamma3 / beta3 = 3 x c or NULL
struct Branches {
  const uint4 *a[3];
  const double *stat3;
  const float *gamma3, *beta3;
};

// per-channel constants of branch k for the V channels of piece j
template <int V> struct Chan { float sc[V], sh[V], mean[V], invstd[V]; };
template <int V> __device__ __forceinline__ Chan<V> load_chan(const Branches &b, int k, int c, int j) {
  Chan<V> p;
#pragma unroll
  for (int q = 0; q < V; ++q) {
    const int ch = j * V + q;
    p.invstd[q] = (float)b.stat3[(2 * k + 1) * c + ch];
    p.mean[q] = (float)b.stat3[2 * k * c + ch];
    p.sc[q] = p.invstd[q] * (b.gamma3 ? b.gamma3[k * c + ch] : 1.f);   // bn(x) = fma(x, sc, sh), as bn_apply_kernel forms it
    p.sh[q] = (b.beta3 ? b.beta3[k * c + ch] : 0.f) - p.mean[q] * p.sc[q];
  }
  return p;
}

// rows are addressed in 16-byte pieces: piece j of row r of a (rows, c) tensor sits at uint4 index r * cv + j.
// block = (TX lanes over the pieces of a row, TY rows); grid-stride over the rows
template <typename ET>
__global__ void __launch_bounds__(256) recon_gate_kernel(Branches b, const uint4 *__restrict__ x, int64_t n, int c, int cv,
                                                         uint4 *__restrict__ out) {
  constexpr int V = Piece<ET>::V;
  for (int j = threadIdx.x; j < cv; j += blockDim.x) {
    float sc[3][V], sh[3][V];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const Chan<V> p = load_chan<V>(b, k, c, j);
#pragma unroll
      for (int q = 0; q < V; ++q) { sc[k][q] = p.sc[q]; sh[k][q] = p.sh[q]; }
    }
#pragma unroll 2
    for (int64_t i = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; i < n; i += (int64_t)gridDim.x * blockDim.y) {
      const uint4 r0 = b.a[0][i * cv + j], r1 = b.a[1][i * cv + j], r2 = b.a[2][i * cv + j], rx = x[i * cv + j];
      const Acc<V> a0 = widen(ET{}, r0), a1 = widen(ET{}, r1), a2 = widen(ET{}, r2), xv = widen(ET{}, rx);
      Acc<V> o;
#pragma unroll
      for (int q = 0; q < V; ++q) {
        const float s0 = sigmoidf(fmaf(a0.f[q], sc[0][q], sh[0][q]));
        const float s1 = sigmoidf(fmaf(a1.f[q], sc[1][q], sh[1][q]));
        const float s2 = sigmoidf(fmaf(a2.f[q], sc[2][q], sh[2][q]));
        o.f[q] = xv.f[q] * ((s0 + s1) + s2);
      }
      out[i * cv + j] = narrow(ET{}, o);
    }
  }
}

// partial[blockIdx.x][k][0][ch] = sum g_k, partial[blockIdx.x][k][1][ch] = sum g_k * xhat_k over the rows of this workgroup
template <typename ET>
__global__ void __launch_bounds__(256) recon_gate_partial_kernel(Branches b, const uint4 *__restrict__ dy,
                                                                 const uint4 *__restrict__ x, int64_t n, int c, int cv,
                                                                 float *__restrict__ partial) {
  constexpr int V = Piece<ET>::V;
  extern __shared__ float red[];  // [TY][2][TX * V], one branch at a time
  const int tx = threadIdx.x, ty = threadIdx.y, TX = blockDim.x, TY = blockDim.y;
  const int W = TX * V;
  for (int j0 = 0; j0 < cv; j0 += TX) {   // every thread takes every trip: the barriers below are uniform
    const int j = j0 + tx;
    float s[3][2][V];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int q = 0; q < V; ++q) { s[k][0][q] = 0.f; s[k][1][q] = 0.f; }
    if (j < cv) {
      Chan<V> p[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) p[k] = load_chan<V>(b, k, c, j);
      for (int64_t i = (int64_t)blockIdx.x * TY + ty; i < n; i += (int64_t)gridDim.x * TY) {
        const uint4 rg = dy[i * cv + j], rx = x[i * cv + j];
        const uint4 ra[3] = {b.a[0][i * cv + j], b.a[1][i * cv + j], b.a[2][i * cv + j]};
        const Acc<V> gv = widen(ET{}, rg), xv = widen(ET{}, rx);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const Acc<V> av = widen(ET{}, ra[k]);
#pragma unroll
          for (int q = 0; q < V; ++q) {
            const float sg = sigmoidf(fmaf(av.f[q], p[k].sc[q], p[k].sh[q]));
            const float g = (gv.f[q] * xv.f[q]) * (sg * (1.f - sg));
            s[k][0][q] += g;
            s[k][1][q] += g * ((av.f[q] - p[k].mean[q]) * p[k].invstd[q]);
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int q = 0; q < V; ++q) {
        red[(ty * 2 + 0) * W + tx * V + q] = s[k][0][q];
        red[(ty * 2 + 1) * W + tx * V + q] = s[k][1][q];
      }
      __syncthreads();
      if (ty == 0 && j < cv) {
#pragma unroll
        for (int q = 0; q < V; ++q) {
          float u = 0.f, v = 0.f;
          for (int r = 0; r < TY; ++r) { u += red[(r * 2 + 0) * W + tx * V + q]; v += red[(r * 2 + 1) * W + tx * V + q]; }
          partial[(((int64_t)blockIdx.x * 3 + k) * 2 + 0) * c + j * V + q] = u;
          partial[(((int64_t)blockIdx.x * 3 + k) * 2 + 1) * c + j * V + q] = v;
        }
      }
      __syncthreads();
    }
  }
}

// sums[col] = sum over the nblk partial rows of partial[b][col], col < ncols = 6c, accumulated in double in the FIXED order of
// bn_reduce_kernel (norm.hip): lane ty sums rows ty, ty + 256, ...; groups of 16 lanes in order; the 16 group sums in order.
// f32copy: the same values as floats (the parameter gradients without a conversion launch). A kernel of its own rather than a
// launch of bn_reduce_kernel<float> over 2 x 3c columns (same bits): half the workgroups with twice the loads each took 5.9 us
// against this kernel's 4.9 us per launch (profiles/row_storage_refactor.md), and the pass is pure latency.
__global__ void __launch_bounds__(1024) recon_gate_reduce_kernel(const float *__restrict__ partial, int nblk, int ncols,
                                                                 double *__restrict__ sums, float *__restrict__ f32copy) {
  __shared__ double red[kRedLanes][kRedCh + 1];
  __shared__ double red2[16][kRedCh + 1];
  const int col = blockIdx.x * kRedCh + threadIdx.x;
  double s = 0.0;
  if (col < ncols) {
    float v[4];
    for (int b0 = threadIdx.y; b0 < nblk; b0 += kRedLanes * 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = b0 + kRedLanes * u;
        v[u] = r < nblk ? partial[(int64_t)r * ncols + col] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) s += (double)v[u];
    }
  }
  red[threadIdx.y][threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.y < 16) {
    double a = 0.0;
    for (int r = 0; r < 16; ++r) a += red[threadIdx.y * 16 + r][threadIdx.x];
    red2[threadIdx.y][threadIdx.x] = a;
  }
  __syncthreads();
  if (threadIdx.y == 0 && col < ncols) {
    double t = 0.0;
    for (int r = 0; r < 16; ++r) t += red2[r][threadIdx.x];
    sums[col] = t;
    f32copy[col] = (float)t;
  }
}

struct Grads { uint4 *dx, *da[3]; };

template <typename ET>
__global__ void __launch_bounds__(256) recon_gate_bwd_apply_kernel(Branches b, const uint4 *__restrict__ dy,
                                                                   const uint4 *__restrict__ x,
                                                                   const double *__restrict__ sums2, double count,
                                                                   const double *__restrict__ count_dev, int64_t n, int c,
                                                                   int cv, Grads o) {
  constexpr int V = Piece<ET>::V;
  if (count_dev) count = *count_dev;
  if (!(count > 0.0)) count = 1.0;
  for (int j = threadIdx.x; j < cv; j += blockDim.x) {
    Chan<V> p[3];
    float k1[3][V], k2[3][V];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      p[k] = load_chan<V>(b, k, c, j);
#pragma unroll
      for (int q = 0; q < V; ++q) {
        k1[k][q] = (float)(sums2[2 * k * c + j * V + q] / count);
        k2[k][q] = (float)(sums2[(2 * k + 1) * c + j * V + q] / count);
      }
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; i < n; i += (int64_t)gridDim.x * blockDim.y) {
      const uint4 rg = dy[i * cv + j], rx = x[i * cv + j];
      const uint4 ra[3] = {b.a[0][i * cv + j], b.a[1][i * cv + j], b.a[2][i * cv + j]};
      const Acc<V> gv = widen(ET{}, rg), xv = widen(ET{}, rx);
      float sg[3][V];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const Acc<V> av = widen(ET{}, ra[k]);
        Acc<V> d;
#pragma unroll
        for (int q = 0; q < V; ++q) {
          sg[k][q] = sigmoidf(fmaf(av.f[q], p[k].sc[q], p[k].sh[q]));
          const float g = (gv.f[q] * xv.f[q]) * (sg[k][q] * (1.f - sg[k][q]));
          const float xh = (av.f[q] - p[k].mean[q]) * p[k].invstd[q];
          d.f[q] = (g - k1[k][q] - xh * k2[k][q]) * p[k].sc[q];   // sc = invstd * w
        }
        o.da[k][i * cv + j] = narrow(ET{}, d);
      }
      Acc<V> dx;
#pragma unroll
      for (int q = 0; q < V; ++q) dx.f[q] = gv.f[q] * ((sg[0][q] + sg[1][q]) + sg[2][q]);
      o.dx[i * cv + j] = narrow(ET{}, dx);
    }
  }
}

// one x-lane per 16-byte piece up to 64 (not rounded to a power of two, as the BatchNorm passes); capped grid of 16 workgroups per CU
RowLaunch launch_shape(int dtype, int64_t n, int c) { return row_launch(n, c / (dtype == 0 ? 4 : 8), kRowsExact); }

// the checks every entry shares; PCS_OK with *go = false: nothing to do (n == 0)
int recon_check(const char *what, int dtype, int64_t n, int32_t c, bool *go) {
  *go = false;
  if (n < 0 || c <= 0) { set_error("%s: bad sizes", what); return PCS_EINVAL; }
  if (c % (dtype == 0 ? 4 : 8)) {
    set_error("%s: c = %d is not a multiple of %d (rows move in 16-byte pieces)", what, (int)c, dtype == 0 ? 4 : 8);
    return PCS_EUNSUPPORTED;
  }
  *go = n > 0;
  return PCS_OK;
}

Branches branches(const void *a0, const void *a1, const void *a2, const double *stat3, const float *gamma3, const float *beta3) {
  Branches b;
  b.a[0] = reinterpret_cast<const uint4 *>(a0); b.a[1] = reinterpret_cast<const uint4 *>(a1); b.a[2] = reinterpret_cast<const uint4 *>(a2);
  b.stat3 = stat3; b.gamma3 = gamma3; b.beta3 = beta3;
  return b;
}

int recon_gate_any(const char *what, int dtype, const void *a0, const void *a1, const void *a2, const void *x, const double *stat3,
                   const float *gamma3, const float *beta3, int64_t n, int32_t c, void *out, void *stream) {
  bool go;
  const int rc = recon_check(what, dtype, n, c, &go);
  if (rc != PCS_OK || !go) return rc;
  if (!a0 || !a1 || !a2 || !x || !stat3 || !out) { set_error("%s: null pointer", what); return PCS_EINVAL; }
  if (!aligned(a0, 16) || !aligned(a1, 16) || !aligned(a2, 16) || !aligned(x, 16) || !aligned(out, 16)) {
    set_error("%s: a0, a1, a2, x and out rows must be 16-byte aligned", what);
    return PCS_EUNSUPPORTED;
  }
  if (((uintptr_t)stat3 & 7) || ((uintptr_t)gamma3 & 3) || ((uintptr_t)beta3 & 3)) { set_error("%s: misaligned stat3 / gamma3 / beta3", what); return PCS_EINVAL; }
  const RowLaunch l = launch_shape(dtype, n, c);
  PCS_DTYPE(dtype, hipLaunchKernelGGL(recon_gate_kernel<ET>, l.grid, l.block, 0, as_stream(stream), branches(a0, a1, a2, stat3, gamma3, beta3),
                  reinterpret_cast<const uint4 *>(x), n, c, l.cv, reinterpret_cast<uint4 *>(out)));
  return check_launch(what);
}

int recon_gate_bwd_stats_any(const char *what, int dtype, const void *dy, const void *x, const void *a0, const void *a1,
                             const void *a2, const double *stat3, const float *gamma3, const float *beta3, int64_t n, int32_t c,
                             float *partial_ws, double *sums2, int64_t sums2_doubles, void *stream) {
  bool go;
  const int rc = recon_check(what, dtype, n, c, &go);
  if (rc != PCS_OK || !go) return rc;
  if (!dy || !x || !a0 || !a1 || !a2 || !stat3 || !partial_ws || !sums2) { set_error("%s: null pointer", what); return PCS_EINVAL; }
  if (sums2_doubles < 9 * (int64_t)c) {
    set_error("%s: sums2 must hold 9c doubles (3 x 2c sums + the same 6c values as floats)", what);
    return PCS_EWORKSPACE;
  }
  if (!aligned(dy, 16) || !aligned(x, 16) || !aligned(a0, 16) || !aligned(a1, 16) || !aligned(a2, 16)) {
    set_error("%s: dy, x, a0, a1 and a2 rows must be 16-byte aligned", what);
    return PCS_EUNSUPPORTED;
  }
  if (((uintptr_t)stat3 & 7) || ((uintptr_t)sums2 & 7) || ((uintptr_t)partial_ws & 3) || ((uintptr_t)gamma3 & 3) || ((uintptr_t)beta3 & 3)) {
    set_error("%s: misaligned stat3 / sums2 / partial_ws / gamma3 / beta3", what);
    return PCS_EINVAL;
  }
  const RowLaunch l = launch_shape(dtype, n, c);
  const int V = dtype == 0 ? 4 : 8;
  const size_t lds = (size_t)l.block.y * 2 * l.block.x * V * sizeof(float);   // <= 256 * 2 * 8 * 4 = 16 KB
  hipStream_t st = as_stream(stream);
  PCS_DTYPE(dtype, hipLaunchKernelGGL(recon_gate_partial_kernel<ET>, dim3(kStatBlocks), l.block, lds, st, branches(a0, a1, a2, stat3, gamma3, beta3),
                  reinterpret_cast<const uint4 *>(dy), reinterpret_cast<const uint4 *>(x), n, c, l.cv, partial_ws));
  const int ncols = 6 * c;
  hipLaunchKernelGGL(recon_gate_reduce_kernel, dim3((unsigned)ceil_div(ncols, kRedCh)), dim3(kRedCh, kRedLanes), 0, st, partial_ws,
                     kStatBlocks, ncols, sums2, reinterpret_cast<float *>(sums2 + ncols));
  return check_launch(what);
}

int recon_gate_bwd_apply_any(const char *what, int dtype, const void *dy, const void *x, const void *a0, const void *a1,
                             const void *a2, const double *stat3, const float *gamma3, const float *beta3, const double *sums2,
                             double count, const double *count_dev, int64_t n, int32_t c, void *dx_gate, void *da0, void *da1,
                             void *da2, void *stream) {
  bool go;
  const int rc = recon_check(what, dtype, n, c, &go);
  if (rc != PCS_OK || !go) return rc;   // n == 0 before the count: an empty tensor has none
  if (!dy || !x || !a0 || !a1 || !a2 || !stat3 || !sums2 || !dx_gate || !da0 || !da1 || !da2) { set_error("%s: null pointer", what); return PCS_EINVAL; }
  if (!count_dev && !(count > 0)) { set_error("%s: count must be positive", what); return PCS_EINVAL; }
  if (!aligned(dy, 16) || !aligned(x, 16) || !aligned(a0, 16) || !aligned(a1, 16) || !aligned(a2, 16) || !aligned(dx_gate, 16) ||
      !aligned(da0, 16) || !aligned(da1, 16) || !aligned(da2, 16)) {
    set_error("%s: dy, x, a_k, dx_gate and da_k rows must be 16-byte aligned", what);
    return PCS_EUNSUPPORTED;
  }
  if (((uintptr_t)stat3 & 7) || ((uintptr_t)sums2 & 7) || ((uintptr_t)count_dev & 7) || ((uintptr_t)gamma3 & 3) || ((uintptr_t)beta3 & 3)) {
    set_error("%s: misaligned stat3 / sums2 / count_dev / gamma3 / beta3", what);
    return PCS_EINVAL;
  }
  const RowLaunch l = launch_shape(dtype, n, c);
  Grads o;
  o.dx = reinterpret_cast<uint4 *>(dx_gate);
  o.da[0] = reinterpret_cast<uint4 *>(da0); o.da[1] = reinterpret_cast<uint4 *>(da1); o.da[2] = reinterpret_cast<uint4 *>(da2);
  PCS_DTYPE(dtype, hipLaunchKernelGGL(recon_gate_bwd_apply_kernel<ET>, l.grid, l.block, 0, as_stream(stream), branches(a0, a1, a2, stat3, gamma3, beta3),
                  reinterpret_cast<const uint4 *>(dy), reinterpret_cast<const uint4 *>(x), sums2, count, count_dev, n, c, l.cv, o));
  return check_launch(what);
}

}  // namespace

extern "C" int pcs_recon_gate_f32(const float *a0, const float *a1, const float *a2, const float *x, const double *stat3,
                                  const float *gamma3, const float *beta3, int64_t n, int32_t c, float *out, void *stream) {
  return recon_gate_any("pcs_recon_gate_f32", 0, a0, a1, a2, x, stat3, gamma3, beta3, n, c, out, stream);
}
extern "C" int pcs_recon_gate_h(const void *a0, const void *a1, const void *a2, const void *x, const double *stat3,
                                const float *gamma3, const float *beta3, int64_t n, int32_t c, int32_t dtype, void *out,
                                void *stream) {
  if (bad_half("pcs_recon_gate_h", dtype)) return PCS_EINVAL;
  return recon_gate_any("pcs_recon_gate_h", dtype, a0, a1, a2, x, stat3, gamma3, beta3, n, c, out, stream);
}

extern "C" int pcs_recon_gate_bwd_stats_f32(const float *dy, const float *x, const float *a0, const float *a1, const float *a2,
                                            const double *stat3, const float *gamma3, const float *beta3, int64_t n, int32_t c,
                                            float *partial_ws, double *sums2, int64_t sums2_doubles, void *stream) {
  return recon_gate_bwd_stats_any("pcs_recon_gate_bwd_stats_f32", 0, dy, x, a0, a1, a2, stat3, gamma3, beta3, n, c, partial_ws, sums2,
                                  sums2_doubles, stream);
}
extern "C" int pcs_recon_gate_bwd_stats_h(const void *dy, const void *x, const void *a0, const void *a1, const void *a2,
                                          const double *stat3, const float *gamma3, const float *beta3, int64_t n, int32_t c,
                                          int32_t dtype, float *partial_ws, double *sums2, int64_t sums2_doubles, void *stream) {
  if (bad_half("pcs_recon_gate_bwd_stats_h", dtype)) return PCS_EINVAL;
  return recon_gate_bwd_stats_any("pcs_recon_gate_bwd_stats_h", dtype, dy, x, a0, a1, a2, stat3, gamma3, beta3, n, c, partial_ws, sums2,
                                  sums2_doubles, stream);
}

extern "C" int pcs_recon_gate_bwd_apply_f32(const float *dy, const float *x, const float *a0, const float *a1, const float *a2,
                                            const double *stat3, const float *gamma3, const float *beta3, const double *sums2,
                                            double count, const double *count_dev, int64_t n, int32_t c, float *dx_gate,
                                            float *da0, float *da1, float *da2, void *stream) {
  return recon_gate_bwd_apply_any("pcs_recon_gate_bwd_apply_f32", 0, dy, x, a0, a1, a2, stat3, gamma3, beta3, sums2, count, count_dev,
                                  n, c, dx_gate, da0, da1, da2, stream);
}
extern "C" int pcs_recon_gate_bwd_apply_h(const void *dy, const void *x, const void *a0, const void *a1, const void *a2,
                                          const double *stat3, const float *gamma3, const float *beta3, const double *sums2,
                                          double count, const double *count_dev, int64_t n, int32_t c, int32_t dtype,
                                          void *dx_gate, void *da0, void *da1, void *da2, void *stream) {
  if (bad_half("pcs_recon_gate_bwd_apply_h", dtype)) return PCS_EINVAL;
  return recon_gate_bwd_apply_any("pcs_recon_gate_bwd_apply_h", dtype, dy, x, a0, a1, a2, stat3, gamma3, beta3, sums2, count,
                                  count_dev, n, c, dx_gate, da0, da1, da2, stream);
}
