// Shared by the 16-bit-MFMA fused-convolution code: conv_wave5h.hip (wave-autonomous row-block groups, ticket commit),
// conv_wave6h.hip (weight-stationary ranges) and weights_multi.hip. They read the same prepared weights (MFMA fragment order, pcs_conv_prepare_weights_h) and share the tile epilogue of conv_common.h.
#pragma once
#include "conv_plan.h"

namespace pcs {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x4 mfma_h(Bf16, const uint4 &a, const uint4 &b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_h(Fp16, const uint4 &a, const uint4 &b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

struct ConvArgsH {
  const char *src;    // (n_src, cin) halfs
  const char *Wp;     // prepared weights, fragment order
  const float *bias;  // fp32, may be NULL
  uint16_t *dst;      // (n_dst, cout) halfs
  const int32_t *pairs;
  const int32_t *seg;
  int64_t n_dst;
  int64_t ntiles;
  int cin, cout, K, src_col, ncoltiles, tile_rows, nt16, ns;
  double *stats;  // optional [ntiles][2][cout], as ConvArgs::stats (over the ROUNDED values stored)
  const int32_t *order;  // optional [ntiles]: workgroup slot -> row tile (heaviest first), as ConvArgs::order
  const uint16_t *addend = nullptr;  // optional (n_dst, cout) halfs: added (in fp32, before the rounding) to the output rows
  float act_slope = 1.f;             // LeakyReLU in the write-back, as ConvArgs::act_slope
  const float *post_scale = nullptr, *post_shift = nullptr;  // PCS_EP_POST_AFFINE, as ConvArgs::post_scale (fp32; ONE rounding, on the store)
};

int launch_conv_wave6h(const ConvArgsH &a, const ConvPlan &p, hipStream_t st);   // conv_wave6h.hip

}  // namespace pcs
