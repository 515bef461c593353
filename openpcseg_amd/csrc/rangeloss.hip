// The range-view training criterion -- gfx950, two passes over the logits plus a fold, no host read.
// The reference's range segmentors (R:pcseg/model/segmentor/range/fidnet/model/semantic/fidnet.py:62-84, salsanext.py:250-271,
// cenet.py:248-318; the classes in R:pcseg/model/segmentor/range/utils.py:509-724) all run
//   loss = w_ce * mean_pixels(CrossEntropy(reduction='none') + Dice) + w_ls * Lovasz_softmax(ignore=0) + w_bd * BoundaryLoss(theta0=3)
// as three softmax calls, two one-hot builds, two max_pool2d passes, a dozen elementwise and reduction passes and their autograd
// mirror over (B, C, H, W) tensors. Here, for logits (B, C, H, W) NCHW in fp32 / bf16 / fp16 (upcast exactly, fp32 arithmetic,
// double folds) and labels (B, H, W) int64:
//   range_stats_kernel   one workgroup = one 8 x 32 tile of one image. The softmax of the tile plus a one-pixel halo is computed
//                        once into LDS (class-major planes, odd stride); pixels outside the image hold +inf, so the minimum over
//                        the clipped 3 x 3 window needs no bounds test. Leaves the CE sum and, per class, six partial sums
//                        (sum p over valid pixels, count, sum p * onehot, sum pred_b, sum gt_b, sum pred_b * gt_b) in the
//                        workspace, and the probabilities as (B H W, C) rows for pcs_lovasz_softmax_f32 (coalesced from LDS).
//                        pred_b = p - min3x3(p), gt_b = onehot - min3x3(onehot): what max_pool2d(1 - x, 3, 1, 1) - (1 - x) is.
//   range_fold_image_kernel / range_fold_final_kernel   the partials of an image, then the images, summed in double in a fixed
//                        order (no float atomics: the result is a pure function of the input); the five scalars and the
//                        coefficients of the gradient pass: two per class for Dice, two per (image, class) for the boundary term.
//   range_grad_kernel    recomputes the softmax of a tile plus a TWO-pixel halo, the first-minimum position of every 3 x 3
//                        window of the one-pixel halo (one byte per window and class), and gathers
//                          bd_c(q) = coef_c(q) - sum over the centres r around q of coef_c(r) [q is the first minimum of r's window]
//                        with coef_c(r) = a_nc gt_b(r) + b_nc; d logit_c = p_c (g_c - sum_k p_k g_k) + the CE term, rounded once.
// The tie rule is part of the contract: among equal minima the first in row-major order of the clipped window takes the
// gradient (torch's max_pool2d backward). A label outside [0, C) is handled like ignore_index: CE term 0 (still counted in the
// mean's divisor), no one-hot row, left out of Dice's denominator.
#include <math.h>

#include "pcs_common.h"
#include "row_storage.h"

using namespace pcs;

namespace {

constexpr int kBlock = 256;
constexpr int kTW = 32;        // tile width of both passes
constexpr int kTH = 8;         // tile height of the statistics pass (the gradient pass: 8, or 4 where 8 does not fit 64 KB of LDS)
constexpr int kMaxC = 32;
constexpr int kVals = 6;       // per class: sum p (valid pixels), count, sum p onehot, sum pred_b, sum gt_b, sum pred_b gt_b
constexpr int kOutside = -2;   // label slot of a pixel outside the image; -1 = inside with a label outside [0, C)
constexpr size_t kLdsLimit = 64 * 1024;

struct Plan {
  int B, C, H, W, tiles_x, tiles_y, nv;
  int64_t npix, tiles, groups;
  size_t off_img, off_part, bytes;
};

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

int plan_for(const char *what, int B, int C, int H, int W, Plan &p) {
  if (B < 1 || H < 1 || W < 1 || C < 2 || C > kMaxC) {
    set_error("%s: bad sizes (B, H, W >= 1, 2 <= C <= %d), got B %d C %d H %d W %d", what, kMaxC, B, C, H, W);
    return PCS_EINVAL;
  }
  const double elems = (double)B * C * H * W;
  if (elems >= 4294967295.0) {
    set_error("%s: B * C * H * W = %.0f exceeds the 32-bit element index", what, elems);
    return PCS_EINVAL;
  }
  p.B = B; p.C = C; p.H = H; p.W = W;
  p.tiles_x = (W + kTW - 1) / kTW;
  p.tiles_y = (H + kTH - 1) / kTH;
  p.nv = 1 + kVals * C;
  p.npix = (int64_t)B * H * W;
  p.tiles = (int64_t)p.tiles_x * p.tiles_y;
  p.groups = p.tiles * B;
  size_t off = align_up(sizeof(float) * (2 * kMaxC + 2 * (size_t)B * C));   // the coefficients
  p.off_img = off; off = align_up(off + sizeof(double) * (size_t)B * p.nv);
  p.off_part = off; off = align_up(off + sizeof(float) * (size_t)p.groups * p.nv);
  p.bytes = off;
  return PCS_OK;
}

size_t stats_lds_bytes(int C) {
  const int np = (kTW + 2) * (kTH + 2);
  return sizeof(float) * ((size_t)C * (np + 1) + kBlock * kVals) + sizeof(int) * (np + kBlock);
}
size_t grad_lds_bytes(int C, int th) {
  const int np2 = (kTW + 4) * (th + 4), np1 = (kTW + 2) * (th + 2);
  return sizeof(float) * (size_t)C * (np2 | 1) + sizeof(int) * (np2 + np1) + (((size_t)C * np1 + 3) & ~(size_t)3);
}

template <typename ET> __device__ __forceinline__ float load_logit(const typename Elem<ET>::T *p) { return widen(ET{}, *p).f[0]; }
template <typename ET> __device__ __forceinline__ void store_grad(typename Elem<ET>::T *p, float v) { *p = narrow(ET{}, Acc<1>{{v}}); }

// the softmax of halo pixel e of a tile into plane c of P (stride str); label slot -1 / kOutside as above. Returns the CE
// term's log-probability of the label (0 without a valid label).
template <typename ET>
__device__ __forceinline__ float softmax_pixel(const typename Elem<ET>::T *__restrict__ logits, const int64_t *__restrict__ labels,
                                               int n, int C, int H, int W, int gy, int gx, float *P, int str, int e, int *lab) {
  if (gy < 0 || gy >= H || gx < 0 || gx >= W) {
    lab[e] = kOutside;
    for (int c = 0; c < C; ++c) P[c * str + e] = INFINITY;
    return 0.f;
  }
  const int64_t plane = (int64_t)H * W, pix = (int64_t)gy * W + gx;
  const typename Elem<ET>::T *src = logits + (int64_t)n * C * plane + pix;
  const int64_t l64 = labels[(int64_t)n * plane + pix];
  const int l = (l64 >= 0 && l64 < C) ? (int)l64 : -1;
  lab[e] = l;
  float m = -INFINITY, xl = 0.f;
  for (int c = 0; c < C; ++c) {
    const float x = load_logit<ET>(src + c * plane);
    P[c * str + e] = x;
    m = fmaxf(m, x);
    if (c == l) xl = x;
  }
  float s = 0.f;
  for (int c = 0; c < C; ++c) {
    const float ex = expf(P[c * str + e] - m);
    P[c * str + e] = ex;
    s += ex;
  }
  for (int c = 0; c < C; ++c) P[c * str + e] = P[c * str + e] / s;
  return l >= 0 ? (xl - m) - logf(s) : 0.f;
}

// whether a window pixel of the 3 x 3 around slot e (row length hw) inside the image carries another label than l
__device__ __forceinline__ int label_edge(const int *lab, int e, int hw, int l) {
  int edge = 0;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int ln = lab[e + dy * hw + dx];
      edge |= (ln != kOutside && ln != l) ? 1 : 0;
    }
  return edge;
}

template <typename ET>
__global__ void __launch_bounds__(kBlock) range_stats_kernel(const typename Elem<ET>::T *__restrict__ logits,
                                                             const int64_t *__restrict__ labels, const float *__restrict__ cw,
                                                             int C, int H, int W, int tiles_x, int tiles_y, int want_bd,
                                                             float *__restrict__ probas, float *__restrict__ partials) {
  constexpr int HW1 = kTW + 2, NP = HW1 * (kTH + 2), STR = NP + 1;
  extern __shared__ float lds[];
  float *P = lds;                                      // C planes of the tile plus halo
  float *red = P + C * STR;                            // kVals x kBlock
  int *lab = reinterpret_cast<int *>(red + kVals * kBlock);   // NP
  int *info = lab + NP;                                // kBlock: kOutside, or (label + 1) << 1 | edge
  __shared__ float ce_wave[kBlock / kWave];
  const int tid = threadIdx.x;
  int t = blockIdx.x;
  const int x0 = (t % tiles_x) * kTW; t /= tiles_x;
  const int y0 = (t % tiles_y) * kTH;
  const int n = t / tiles_y;

  float ce = 0.f;
  for (int e = tid; e < NP; e += kBlock) {
    const int hy = e / HW1, hx = e - hy * HW1;
    const float logp = softmax_pixel<ET>(logits, labels, n, C, H, W, y0 + hy - 1, x0 + hx - 1, P, STR, e, lab);
    if (hy >= 1 && hy <= kTH && hx >= 1 && hx <= kTW && lab[e] >= 0) ce -= (cw ? cw[lab[e]] : 1.f) * logp;
  }
  for (int o = 32; o > 0; o >>= 1) ce += __shfl_down(ce, o, 64);
  if ((tid & 63) == 0) ce_wave[tid >> 6] = ce;
  __syncthreads();

  if (probas != nullptr) {   // (B H W, C) rows: a tile row is one contiguous run of 32 C floats
    const int run = kTW * C;
    for (int idx = tid; idx < kTH * run; idx += kBlock) {
      const int row = idx / run, rem = idx - row * run;
      const int px = rem / C, c = rem - px * C;
      const int gy = y0 + row, gx = x0 + px;
      if (gy < H && gx < W) probas[(((int64_t)n * H + gy) * W + gx) * C + c] = P[c * STR + (row + 1) * HW1 + px + 1];
    }
  }
  {
    const int ty = tid / kTW, tx = tid - ty * kTW, e = (ty + 1) * HW1 + tx + 1;
    const int l = lab[e];
    info[tid] = l == kOutside ? kOutside : (((l + 1) << 1) | (l >= 0 ? label_edge(lab, e, HW1, l) : 0));
  }
  __syncthreads();

  // thread (class c, part): the pixels part, part + parts, ... of the tile for one class, all six sums in registers
  const int parts = min(kBlock / C, 32);
  const int c = tid / parts, part = tid - c * parts;
  float s[kVals] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c < C) {
    const float *Pc = P + c * STR;
    for (int k = part; k < kTH * kTW; k += parts) {
      const int inf = info[k];
      if (inf == kOutside) continue;
      const int ty = k / kTW, tx = k - ty * kTW, e = (ty + 1) * HW1 + tx + 1;
      const float p = Pc[e];
      float m = p;
      if (want_bd) {
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) m = fminf(m, Pc[e + dy * HW1 + dx]);
      }
      const float pb = p - m;
      const int l = (inf >> 1) - 1;
      if (l >= 0) s[0] += p;
      s[3] += pb;
      if (l == c) {
        s[1] += 1.f;
        s[2] += p;
        if (inf & 1) { s[4] += 1.f; s[5] += pb; }
      }
    }
  }
#pragma unroll
  for (int v = 0; v < kVals; ++v) red[v * kBlock + tid] = s[v];
  __syncthreads();
  float *mine = partials + (int64_t)blockIdx.x * (1 + kVals * C);
  if (tid < kVals * C) {   // (value v, class cc): the parts in ascending order
    const int v = tid / C, cc = tid - v * C;
    float a = 0.f;
    for (int q = 0; q < parts; ++q) a += red[v * kBlock + cc * parts + q];
    mine[1 + cc * kVals + v] = a;
  }
  if (tid == 0) mine[0] = (ce_wave[0] + ce_wave[1]) + (ce_wave[2] + ce_wave[3]);
}

// workgroup n: the partial rows of image n's tiles -> one row of doubles. Wave w takes the values w, w + 4, ...; its lanes stride
// over the tiles and are folded in a fixed shuffle order.
__global__ void __launch_bounds__(kBlock) range_fold_image_kernel(const float *__restrict__ partials, int nv, int64_t tiles,
                                                                  double *__restrict__ img) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float *rows = partials + (int64_t)blockIdx.x * tiles * nv;
  for (int j = wave; j < nv; j += kBlock / kWave) {
    double a = 0.0;
    for (int64_t t = lane; t < tiles; t += kWave) a += (double)rows[t * nv + j];
    for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
    if (lane == 0) img[(int64_t)blockIdx.x * nv + j] = a;
  }
}

// one workgroup: the images in ascending order, the five scalars and the coefficients of the gradient pass
__global__ void __launch_bounds__(kBlock) range_fold_final_kernel(const double *__restrict__ img, int B, int C, double npix, int flags,
                                                                  const float *__restrict__ ls, float w_ce, float w_ls, float w_bd,
                                                                  float *__restrict__ coef, float *__restrict__ terms) {
  __shared__ double sh_d[kMaxC], sh_dice[kMaxC], sh_wave[kBlock / kWave];
  const int tid = threadIdx.x, nv = 1 + kVals * C;
  double da = 0.0, db = 0.0;
  if (tid < C) {
    double sum_p = 0.0, cnt = 0.0, inter = 0.0;
    for (int n = 0; n < B; ++n) {
      const double *row = img + (int64_t)n * nv + 1 + tid * kVals;
      sum_p += row[0]; cnt += row[1]; inter += row[2];
    }
    const double d = sum_p + cnt, den = d + 1e-4;   // _dice_loss_multichannel: eps = 0.0001
    sh_d[tid] = d;
    sh_dice[tid] = 1.0 - 2.0 * inter / den;
    da = -((double)w_ce / C) * 2.0 / den;
    db = ((double)w_ce / C) * 2.0 * inter / (den * den);
  }
  __syncthreads();
  double dsum = 0.0, dice = 0.0;
  for (int c = 0; c < C; ++c) { dsum += sh_d[c]; dice += sh_dice[c]; }
  const bool dice_on = (flags & PCS_RANGE_LOSS_DICE) && dsum != 0.0;   // "only void": the reference returns the zero sum
  if (tid < C) {
    coef[tid] = dice_on ? (float)da : 0.f;
    coef[kMaxC + tid] = dice_on ? (float)db : 0.f;
  }
  const bool bd_on = (flags & PCS_RANGE_LOSS_BOUNDARY) != 0;
  const int nc = B * C;
  const double k = (double)w_bd / nc, e = 1e-7;
  double acc = 0.0;
  for (int i = tid; i < nc; i += kBlock) {
    const double *row = img + (int64_t)(i / C) * nv + 1 + (i % C) * kVals;
    const double S = row[3], G = row[4], I = row[5];
    const double Pr = I / (S + e), R = I / (G + e), den = Pr + R + e;
    acc += 1.0 - 2.0 * Pr * R / den;
    const double dP = 2.0 * R * (R + e) / (den * den), dR = 2.0 * Pr * (Pr + e) / (den * den);
    coef[2 * kMaxC + i] = bd_on ? (float)(-k * (dP / (S + e) + dR / (G + e))) : 0.f;
    coef[2 * kMaxC + nc + i] = bd_on ? (float)(k * dP * I / ((S + e) * (S + e))) : 0.f;
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((tid & 63) == 0) sh_wave[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double ce = 0.0;
    for (int n = 0; n < B; ++n) ce += img[(int64_t)n * nv];
    const float f_ce = (float)(ce / npix);
    const float f_dice = dice_on ? (float)(dice / C) : 0.f;
    const float f_ls = ls != nullptr ? ls[0] : 0.f;
    const float f_bd = bd_on ? (float)(((sh_wave[0] + sh_wave[1]) + (sh_wave[2] + sh_wave[3])) / nc) : 0.f;
    terms[0] = w_ce * (f_ce + f_dice) + w_ls * f_ls + w_bd * f_bd;
    terms[1] = f_ce; terms[2] = f_dice; terms[3] = f_ls; terms[4] = f_bd;
  }
}

// th: the tile height (8 or 4). LDS: C planes of the tile plus a two-pixel halo, the labels of those pixels, label / edge of the
// one-pixel halo, and one byte per (class, one-pixel-halo window): the row-major position 0 .. 8 of the window's first minimum.
template <typename ET>
__global__ void __launch_bounds__(kBlock) range_grad_kernel(const typename Elem<ET>::T *__restrict__ logits,
                                                            const int64_t *__restrict__ labels, const float *__restrict__ cw,
                                                            const float *__restrict__ gls, const float *__restrict__ coef,
                                                            int B, int C, int H, int W, int tiles_x, int tiles_y, int th, int flags,
                                                            float ce_scale, float w_ls, typename Elem<ET>::T *__restrict__ out) {
  const int HW2 = kTW + 4, NP2 = HW2 * (th + 4), STR = NP2 | 1;
  const int HW1 = kTW + 2, NP1 = HW1 * (th + 2);
  extern __shared__ float lds[];
  float *P = lds;
  int *lab = reinterpret_cast<int *>(P + C * STR);   // NP2
  int *info = lab + NP2;                              // NP1: kOutside, or (label + 1) << 1 | edge
  unsigned char *arg = reinterpret_cast<unsigned char *>(info + NP1);   // C x NP1
  const int tid = threadIdx.x;
  int t = blockIdx.x;
  const int x0 = (t % tiles_x) * kTW; t /= tiles_x;
  const int y0 = (t % tiles_y) * th;
  const int n = t / tiles_y;
  const bool bd_on = (flags & PCS_RANGE_LOSS_BOUNDARY) != 0, dice_on = (flags & PCS_RANGE_LOSS_DICE) != 0;

  for (int e = tid; e < NP2; e += kBlock) {
    const int hy = e / HW2, hx = e - hy * HW2;
    softmax_pixel<ET>(logits, labels, n, C, H, W, y0 + hy - 2, x0 + hx - 2, P, STR, e, lab);
  }
  __syncthreads();
  if (bd_on) {
    for (int e1 = tid; e1 < NP1; e1 += kBlock) {
      const int hy = e1 / HW1, hx = e1 - hy * HW1, e2 = (hy + 1) * HW2 + hx + 1;
      const int l = lab[e2];
      info[e1] = l == kOutside ? kOutside : (((l + 1) << 1) | (l >= 0 ? label_edge(lab, e2, HW2, l) : 0));
    }
    for (int idx = tid; idx < C * NP1; idx += kBlock) {
      const int c = idx / NP1, e1 = idx - c * NP1;
      const int hy = e1 / HW1, hx = e1 - hy * HW1, e2 = (hy + 1) * HW2 + hx + 1;
      const float *Pc = P + c * STR + e2;
      float best = INFINITY;
      int bi = 4;
#pragma unroll
      for (int j = 0; j < 9; ++j) {   // row-major, strict <: the first of equal minima
        const float v = Pc[(j / 3 - 1) * HW2 + (j % 3 - 1)];
        if (v < best) { best = v; bi = j; }
      }
      arg[idx] = (unsigned char)bi;
    }
    __syncthreads();
  }

  const int ty = tid / kTW, tx = tid - ty * kTW;
  const int gy = y0 + ty, gx = x0 + tx;
  if (ty >= th || gy >= H || gx >= W) return;
  const int e2 = (ty + 2) * HW2 + tx + 2, e1 = (ty + 1) * HW1 + tx + 1;
  const int l = lab[e2];
  int ninfo[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) ninfo[j] = bd_on ? info[e1 + (j / 3 - 1) * HW1 + (j % 3 - 1)] : kOutside;
  const int64_t plane = (int64_t)H * W, pix = (int64_t)gy * W + gx;
  const float *gl = gls != nullptr ? gls + ((int64_t)n * plane + pix) * C : nullptr;
  const float *bda = coef + 2 * kMaxC + n * C, *bdb = bda + B * C;
  const float wl = l >= 0 ? ce_scale * (cw ? cw[l] : 1.f) : 0.f;

  auto g_of = [&](int c) -> float {
    float g = gl != nullptr ? w_ls * gl[c] : 0.f;
    if (dice_on && l >= 0) g += coef[kMaxC + c] + (l == c ? coef[c] : 0.f);
    if (bd_on) {
      const float a = bda[c], b = bdb[c];
      g += (l == c && (ninfo[4] & 1)) ? a + b : b;
      const unsigned char *ac = arg + c * NP1 + e1;
#pragma unroll
      for (int j = 0; j < 9; ++j) {   // centre r = q + offset j; q sits at position 8 - j of r's window
        const int inf = ninfo[j];
        if (inf != kOutside && ac[(j / 3 - 1) * HW1 + (j % 3 - 1)] == 8 - j) g -= (((inf >> 1) - 1) == c && (inf & 1)) ? a + b : b;
      }
    }
    return g;
  };
  float dot = 0.f;
  for (int c = 0; c < C; ++c) dot += P[c * STR + e2] * g_of(c);
  typename Elem<ET>::T *dst = out + (int64_t)n * C * plane + pix;
  for (int c = 0; c < C; ++c) {
    const float p = P[c * STR + e2];
    store_grad<ET>(dst + c * plane, p * (g_of(c) - dot) + wl * (p - (l == c ? 1.f : 0.f)));
  }
}

bool bad_dtype(const char *what, int32_t dtype) {
  if (dtype >= 0 && dtype <= 2) return false;
  set_error("%s: dtype must be 0 (fp32), 1 (bf16) or 2 (fp16), got %d", what, (int)dtype);
  return true;
}

bool bad_flags(const char *what, int32_t flags) {
  if ((flags & ~(PCS_RANGE_LOSS_DICE | PCS_RANGE_LOSS_BOUNDARY)) == 0) return false;
  set_error("%s: flags may hold PCS_RANGE_LOSS_DICE | PCS_RANGE_LOSS_BOUNDARY only, got %d", what, (int)flags);
  return true;
}

}  // namespace

extern "C" int64_t pcs_range_loss_ws_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
  Plan p;
  if (plan_for("pcs_range_loss_ws_bytes", B, C, H, W, p) != PCS_OK) return -1;
  return (int64_t)p.bytes;
}

extern "C" int pcs_range_loss_stats(const void *logits, int32_t dtype, const int64_t *labels, const float *class_weight, int32_t B,
                                    int32_t C, int32_t H, int32_t W, int32_t flags, float *probas, void *ws, int64_t ws_bytes,
                                    void *stream) {
  Plan p;
  int rc = plan_for("pcs_range_loss_stats", B, C, H, W, p);
  if (rc != PCS_OK) return rc;
  if (bad_dtype("pcs_range_loss_stats", dtype) || bad_flags("pcs_range_loss_stats", flags)) return PCS_EINVAL;
  if (!logits || !labels || !ws) { set_error("pcs_range_loss_stats: null pointer"); return PCS_EINVAL; }
  if (ws_bytes < (int64_t)p.bytes) return ws_too_small("pcs_range_loss_stats", ws_bytes, (int64_t)p.bytes);
  hipStream_t st = as_stream(stream);
  char *base = reinterpret_cast<char *>(ws);
  float *partials = reinterpret_cast<float *>(base + p.off_part);
  double *img = reinterpret_cast<double *>(base + p.off_img);
  const int want_bd = (flags & PCS_RANGE_LOSS_BOUNDARY) ? 1 : 0;
  PCS_DTYPE(dtype, {
    hipLaunchKernelGGL((range_stats_kernel<ET>), dim3((unsigned)p.groups), dim3(kBlock), stats_lds_bytes(C), st,
                       reinterpret_cast<const typename Elem<ET>::T *>(logits), labels, class_weight, C, H, W, p.tiles_x, p.tiles_y,
                       want_bd, probas, partials);
  });
  if ((rc = check_launch("range_stats_kernel")) != PCS_OK) return rc;
  hipLaunchKernelGGL(range_fold_image_kernel, dim3((unsigned)B), dim3(kBlock), 0, st, partials, p.nv, p.tiles, img);
  return check_launch("pcs_range_loss_stats");
}

extern "C" int pcs_range_loss_fold(int32_t B, int32_t C, int32_t H, int32_t W, int32_t flags, const float *lovasz, float w_ce,
                                   float w_ls, float w_bd, float *terms, void *ws, int64_t ws_bytes, void *stream) {
  Plan p;
  int rc = plan_for("pcs_range_loss_fold", B, C, H, W, p);
  if (rc != PCS_OK) return rc;
  if (bad_flags("pcs_range_loss_fold", flags)) return PCS_EINVAL;
  if (!terms || !ws) { set_error("pcs_range_loss_fold: null pointer"); return PCS_EINVAL; }
  if (ws_bytes < (int64_t)p.bytes) return ws_too_small("pcs_range_loss_fold", ws_bytes, (int64_t)p.bytes);
  char *base = reinterpret_cast<char *>(ws);
  hipLaunchKernelGGL(range_fold_final_kernel, dim3(1), dim3(kBlock), 0, as_stream(stream),
                     reinterpret_cast<const double *>(base + p.off_img), B, C, (double)p.npix, flags, lovasz, w_ce, w_ls, w_bd,
                     reinterpret_cast<float *>(base), terms);
  return check_launch("pcs_range_loss_fold");
}

extern "C" int pcs_range_loss_grad(const void *logits, int32_t dtype, const int64_t *labels, const float *class_weight,
                                   const float *lovasz_grad, int32_t B, int32_t C, int32_t H, int32_t W, int32_t flags, float w_ce,
                                   float w_ls, const void *ws, int64_t ws_bytes, void *grad, void *stream) {
  Plan p;
  int rc = plan_for("pcs_range_loss_grad", B, C, H, W, p);
  if (rc != PCS_OK) return rc;
  if (bad_dtype("pcs_range_loss_grad", dtype) || bad_flags("pcs_range_loss_grad", flags)) return PCS_EINVAL;
  if (!logits || !labels || !ws || !grad) { set_error("pcs_range_loss_grad: null pointer"); return PCS_EINVAL; }
  if (ws_bytes < (int64_t)p.bytes) return ws_too_small("pcs_range_loss_grad", ws_bytes, (int64_t)p.bytes);
  const int th = grad_lds_bytes(C, 8) <= kLdsLimit ? 8 : 4;
  const int tiles_y = (H + th - 1) / th;
  const int64_t groups = (int64_t)p.tiles_x * tiles_y * B;
  const float ce_scale = (float)((double)w_ce / (double)p.npix);
  PCS_DTYPE(dtype, {
    hipLaunchKernelGGL((range_grad_kernel<ET>), dim3((unsigned)groups), dim3(kBlock), grad_lds_bytes(C, th), as_stream(stream),
                       reinterpret_cast<const typename Elem<ET>::T *>(logits), labels, class_weight, lovasz_grad,
                       reinterpret_cast<const float *>(ws), B, C, H, W, p.tiles_x, tiles_y, th, flags, ce_scale, w_ls,
                       reinterpret_cast<typename Elem<ET>::T *>(grad));
  });
  return check_launch("pcs_range_loss_grad");
}
