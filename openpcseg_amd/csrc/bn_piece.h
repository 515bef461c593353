// The per-piece body of the fused merge epilogues, pointmerge.hip and rangemerge.hip: one definition of the ARITHMETIC ORDER
// their bit-identity tests pin. bn_apply_kernel (norm.hip) keeps its own statement of the coefficient and mask-word
// expressions: with these functions its register table moved (profiles/bn_rows_refactor.md), and it is the kernel these
// must agree with, held to a float64 reference of its own.
//   gather: the eight corners into fp32 registers from zero, k = 0..7, one fmaf each, a missing corner (index < 0) skipped
//           (devoxelize_fwd_kernel's order);
//   bn(x) = fmaf(x, sc, sh) with sc = invstd * gamma and sh = beta - mean * sc, invstd and mean rounded from double first;
//   gate bit q = [ max(0, bn(x_q)) as the storage type holds it > 0 ]: what a later `y > 0` on the stored tensor sees.
#pragma once
#include "row_storage.h"

namespace pcs {

// piece j of sum over k of w8[i, k] * vox[idx8[i, k]]; rows of cv pieces
template <typename ET>
__device__ __forceinline__ Acc<Piece<ET>::V> gather_corners(const uint4 *__restrict__ vox, const int32_t *__restrict__ idx8,
                                                            const float *__restrict__ w8, int64_t i, int cv, int j) {
  int32_t id[8];
  float w[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { id[k] = idx8[i * 8 + k]; w[k] = w8[i * 8 + k]; }
  Acc<Piece<ET>::V> acc;
  azero(acc);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (id[k] >= 0) add_mul(acc, w[k], widen(ET{}, vox[(int64_t)id[k] * cv + j]));
  }
  return acc;
}

// sc / sh of the V channels from ch0 on; stat = [mean | invstd] of c channels, gamma / beta may be null
template <int V>
__device__ __forceinline__ void bn_coeffs(const double *__restrict__ stat, const float *__restrict__ gamma,
                                          const float *__restrict__ beta, int c, int ch0, float (&sc)[V], float (&sh)[V]) {
#pragma unroll
  for (int q = 0; q < V; ++q) {
    const int ch = ch0 + q;
    const float invstd = (float)stat[c + ch], mean = (float)stat[ch];
    sc[q] = invstd * (gamma ? gamma[ch] : 1.f);
    sh[q] = (beta ? beta[ch] : 0.f) - mean * sc[q];
  }
}

// x <- max(0, bn(x)), unrounded (the caller's sum keeps its one rounding on the store) -> the V gate bits, pcs_bn_apply_*'s
template <typename ET, int V>
__device__ __forceinline__ unsigned bn_relu_gate(Acc<V> &x, const float (&sc)[V], const float (&sh)[V]) {
  unsigned bits = 0;
#pragma unroll
  for (int q = 0; q < V; ++q) {
    float t = fmaf(x.f[q], sc[q], sh[q]);
    if (t < 0.f) t = 0.f;
    bits |= (stored(ET{}, t) > 0.f ? 1u : 0u) << q;
    x.f[q] = t;
  }
  return bits;
}

// 32 / V consecutive lanes, each with the V gate bits of piece `piece` of one row, make one mask word (bn_apply_kernel's
// layout: word = 32 consecutive channels, bit = channel % 32); every lane of the group gets it. It shuffles: EVERY lane of
// the wave must reach the call in the same trip -- outside any branch that depends on the lane -- with the groups aligned
// in the wave; a lane that owns no element passes bits = 0.
template <int V> __device__ __forceinline__ unsigned mask_word(unsigned bits, int piece) {
  constexpr int LPW = 32 / V;
  unsigned m = bits << (V * (piece & (LPW - 1)));
#pragma unroll
  for (int o = 1; o < LPW; o <<= 1) m |= __shfl_xor(m, o, 64);
  return m;
}

}  // namespace pcs
