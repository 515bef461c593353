// Range-point-voxel merge of RPVNet -- gfx950, HBM-bound. The reference computes, four times per forward
// (R:pcseg/model/segmentor/fusion/rpvnet/rpvnet.py:648-651, 665-668, 683-686, 701-704),
//     z_next.F = voxel_to_point(x, z).F + range_to_point(r, pxpy) + ReLU(BatchNorm(Linear(z.F)))
// as a devoxelize write (K9), a range_sample write, a BatchNorm apply pass and two elementwise adds: about ten passes over an
// (N, C) point tensor. Here the Linear output is read once and the merged rows are written once; the voxel rows are gathered
// as K9 gathers them and the image planes as range_sample_fwd_kernel gathers them.
//     out[i, j]       = ( ( sum over k = 0..7 with idx8[i, k] >= 0 of w8[i, k] * vox[idx8[i, k], j] ) + sample(img[b_i, j], x_i, y_i) ) + third
//     third (bn mode)  = max(0, bn(lin[i, j]))     stat != NULL; mask bit (i, j) = [ bn rounded to the storage type > 0 ],
//                                                  word i * (c / 32) + j / 32, bit j % 32 (bn_apply_kernel's layout)
//     third (add mode) = lin[i, j]                 stat == NULL: lin already holds the finished term (widths that are no multiple of 32)
// Order of the arithmetic (the pieces: bn_piece.h), all in fp32 registers: the corners from zero in k = 0..7 order by fmaf
// (devoxelize_fwd_kernel), the bilinear sample from zero in nw, ne, sw, se order (sample_plane of range_corners.h, the expression
// range_sample_fwd_kernel compiles), acc += sample, bn(x) with the expression of bn_apply_kernel (norm.hip), the third term added
// last, ONE rounding on the store. In fp32 that is bit for bit pcs_devoxelize_fwd_f32, pcs_range_sample_fwd_f32, an add,
// pcs_bn_apply_f32, an add.
// Launch shape: the two kernels composed. A 256-thread workgroup owns 64 consecutive points x a chunk of CH channels.
//   phase 1: wave w samples channels w, w + 4, ... of the chunk with the lanes over the points (corner offsets and weights in
//            registers, every plane read a 4-byte gather out of L2) into a padded LDS tile [point][CH + 4];
//   phase 2: threads cover (row, 16-byte piece): the lin piece first (in flight while the eight vox pieces are gathered), the
//            tile value, the third term, one 16-byte store. bn mode: 8 (fp32) / 4 (16 bits) consecutive lanes make one mask
//            word by __shfl_xor; the shuffles sit outside every `ch < c` branch (a chunk's tail has inactive pieces).
// No atomics; every output element and mask word is written exactly once.
#include "range_corners.h"
#include "bn_piece.h"

using namespace pcs;

namespace {

constexpr int RM_PT = 64;   // points per workgroup

template <typename ET, int CH, bool BN>
__global__ void __launch_bounds__(256) range_point_merge_kernel(const uint4 *__restrict__ vox, const int32_t *__restrict__ idx8,
                                                                const float *__restrict__ w8, const float *__restrict__ img,
                                                                const float *__restrict__ pxpy, int B, int H, int W,
                                                                const uint4 *__restrict__ lin, const double *__restrict__ stat,
                                                                const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                int64_t n, int c, int cv, uint4 *__restrict__ out,
                                                                uint32_t *__restrict__ mask) {
  constexpr int V = Piece<ET>::V;
  constexpr int PV = CH / V;     // pieces of a row inside the chunk: 16 / 8 (fp32), 8 / 4 (16 bits)
  constexpr int LPW = 32 / V;    // lanes per mask word; PV % LPW == 0 and 256 % PV == 0: the groups stay aligned in the wave
  static_assert(PV % LPW == 0 && 256 % PV == 0 && (RM_PT * PV) % 256 == 0, "every thread takes the same trips, in aligned groups");
  __shared__ __attribute__((aligned(16))) float tile[RM_PT][CH + 4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t p0 = (int64_t)blockIdx.x * RM_PT;
  const int c0 = blockIdx.y * CH;
  {
    const int64_t p = p0 + lane;
    Corners cn;
    int b = -1;
    if (p < n) {
      b = frame_of(pxpy[3 * p], B);
      cn = corners_of(pxpy[3 * p + 1], pxpy[3 * p + 2], H, W);
    }
    const int64_t plane = (int64_t)H * W;
    for (int j = wid; j < CH; j += 4) {
      float v = 0.f;
      if (b >= 0 && c0 + j < c)
        v = sample_plane(img + ((int64_t)b * c + c0 + j) * plane, cn);
      tile[lane][j] = v;
    }
  }
  __syncthreads();
  const int pl = threadIdx.x % PV;   // the same piece in every trip (256 % PV == 0)
  const int ch = c0 + V * pl;        // c % V == 0: a piece lies inside the row or outside it, never across its end
  const int j = ch / V;              // piece of the whole row
  float sc[V], sh[V];
  if (BN && ch < c) bn_coeffs<V>(stat, gamma, beta, c, ch, sc, sh);
  for (int t = threadIdx.x; t < RM_PT * PV; t += 256) {
    const int r = t / PV;
    const int64_t i = p0 + r;
    const bool live = i < n && ch < c;
    unsigned bits = 0;
    if (live) {
      const uint4 lr = lin[i * cv + j];  // streamed row first: in flight while the corners are gathered
      Acc<V> acc = gather_corners<ET>(vox, idx8, w8, i, cv, j);
#pragma unroll
      for (int q = 0; q < V; ++q) acc.f[q] += tile[r][V * pl + q];
      Acc<V> y = widen(ET{}, lr);
      if (BN) bits = bn_relu_gate<ET>(y, sc, sh);
#pragma unroll
      for (int q = 0; q < V; ++q) acc.f[q] += y.f[q];
      out[i * cv + j] = narrow(ET{}, acc);
    }
    if (BN) {
      // LPW consecutive lanes of one row make one mask word; a lane outside the row or past n contributes no bit. The call
      // shuffles: it stays here, outside `live`
      const unsigned m = mask_word<V>(bits, pl);
      if (live && (pl & (LPW - 1)) == 0) mask[i * (c >> 5) + (ch >> 5)] = m;   // c % 32 == 0: a word of the row is whole
    }
  }
}

// dtype 0 fp32, 1 bf16, 2 fp16
int range_point_merge_any(const char *what, int dtype, const void *vox, const int32_t *idx8, const float *w8, const float *img,
                          const float *pxpy, int32_t B, int32_t H, int32_t W, const void *lin, const double *stat,
                          const float *gamma, const float *beta, int64_t n, int32_t c, void *out, uint32_t *mask, void *stream) {
  if (n < 0 || c <= 0 || B <= 0 || H <= 0 || W <= 0) { set_error("%s: bad sizes", what); return PCS_EINVAL; }
  const int v = dtype == 0 ? 4 : 8;
  if (c % v) { set_error("%s: c = %d is not a multiple of %d (rows are moved in 16-byte pieces)", what, (int)c, v); return PCS_EUNSUPPORTED; }
  if (stat && (c & 31)) { set_error("%s: bn mode with c = %d, not a multiple of 32 (the ReLU bit mask is made of whole words)", what, (int)c); return PCS_EUNSUPPORTED; }
  if (!stat && (gamma || beta || mask)) { set_error("%s: add mode (stat == NULL) takes no gamma / beta / mask", what); return PCS_EINVAL; }
  if (n == 0) return PCS_OK;
  if (!idx8 || !w8 || !img || !pxpy || !lin || !out || (stat && !mask)) { set_error("%s: null pointer", what); return PCS_EINVAL; }
  if (!aligned(vox, 16) || !aligned(lin, 16) || !aligned(out, 16)) {
    set_error("%s: vox, lin and out rows must be 16-byte aligned", what);
    return PCS_EUNSUPPORTED;
  }
  if (((uintptr_t)mask & 3) || ((uintptr_t)idx8 & 3) || ((uintptr_t)w8 & 3) || ((uintptr_t)img & 3) || ((uintptr_t)pxpy & 3) || ((uintptr_t)stat & 7)) {
    set_error("%s: misaligned mask / idx8 / w8 / img / pxpy / stat", what);
    return PCS_EINVAL;
  }
  const int64_t blocks = ceil_div(n, (int64_t)RM_PT);
  const int ch = c <= 32 ? 32 : 64;
  const int64_t chunks = ceil_div((int64_t)c, (int64_t)ch);
  if (blocks > 0x7FFFFFFF || chunks > 65535) { set_error("%s: grid too large", what); return PCS_EUNSUPPORTED; }
  const dim3 grid((unsigned)blocks, (unsigned)chunks);
  const int cv = c / v;
  hipStream_t st = as_stream(stream);
#define PCS_RM_LAUNCH(CH, BN)                                                                                                      \
  PCS_DTYPE(dtype, hipLaunchKernelGGL((range_point_merge_kernel<ET, CH, BN>), grid, dim3(256), 0, st,                              \
                                      reinterpret_cast<const uint4 *>(vox), idx8, w8, img, pxpy, B, H, W,                          \
                                      reinterpret_cast<const uint4 *>(lin), stat, gamma, beta, n, c, cv,                           \
                                      reinterpret_cast<uint4 *>(out), mask))
  if (stat) { if (ch == 32) PCS_RM_LAUNCH(32, true); else PCS_RM_LAUNCH(64, true); }
  else { if (ch == 32) PCS_RM_LAUNCH(32, false); else PCS_RM_LAUNCH(64, false); }
#undef PCS_RM_LAUNCH
  return check_launch(what);
}

}  // namespace

extern "C" int pcs_range_point_merge_f32(const float *vox, const int32_t *idx8, const float *w8, const float *img, const float *pxpy,
                                         int32_t B, int32_t H, int32_t W, const float *lin, const double *stat, const float *gamma,
                                         const float *beta, int64_t n, int32_t c, float *out, uint32_t *mask, void *stream) {
  return range_point_merge_any("pcs_range_point_merge_f32", 0, vox, idx8, w8, img, pxpy, B, H, W, lin, stat, gamma, beta, n, c, out,
                               mask, stream);
}

extern "C" int pcs_range_point_merge_h(const void *vox, const int32_t *idx8, const float *w8, const float *img, const float *pxpy,
                                       int32_t B, int32_t H, int32_t W, const void *lin, const double *stat, const float *gamma,
                                       const float *beta, int64_t n, int32_t c, int32_t dtype, void *out, uint32_t *mask,
                                       void *stream) {
  if (bad_half("pcs_range_point_merge_h", dtype)) return PCS_EINVAL;
  return range_point_merge_any("pcs_range_point_merge_h", dtype, vox, idx8, w8, img, pxpy, B, H, W, lin, stat, gamma, beta, n, c,
                               out, mask, stream);
}
