// Point-branch merge of SPVCNN -- gfx950, HBM-bound. The reference computes, three times per forward
// (R:pcseg/model/segmentor/fusion/spvcnn/spvcnn.py:417-418, 430-431, 443-444),
//     z_next.F = voxel_to_point(x, z).F + ReLU(BatchNorm(Linear(z.F)))
// as a devoxelize write (K9), a BatchNorm apply pass and an elementwise add: four passes over an (N, C) point tensor.
// Here the Linear output is read once and the merged rows are written once; the voxel rows are gathered as K9 gathers them.
//     out[i, j]       = ( sum over k = 0..7 with idx8[i, k] >= 0 of w8[i, k] * vox[idx8[i, k], j] ) + max(0, bn(lin[i, j]))
//     mask bit (i, j) = [ bn(lin[i, j]) rounded to the storage type > 0 ]          word i * (c / 32) + j / 32, bit j % 32 (bn_apply_kernel's layout)
// Order of the arithmetic (the pieces: bn_piece.h): the corners in fp32 registers from zero in k = 0..7 order
// (devoxelize_fwd_kernel), bn(x) with the expression of bn_apply_kernel (norm.hip), the BatchNorm term added last, ONE
// rounding on the store. In fp32 that is bit for bit what the three separate kernels give; in 16 bits it is one rounding
// where they have three.
// Launch shape of the K9 kernels: a 256-thread workgroup covers 256/TX points, TX lanes x 16 bytes per row, grid-stride
// over the points; the corner indices and weights of a point are loaded once per pass of the lane row (one pass up to
// c = 256 in fp32, 512 in 16 bits). No LDS, no atomics; every output row and mask word is written exactly once.
#include "bn_piece.h"

using namespace pcs;

namespace {

// rows are addressed in 16-byte pieces: piece j of row r of a (rows, c) tensor sits at uint4 index r * cv + j
template <typename ET>
__global__ void __launch_bounds__(256) point_merge_kernel(const uint4 *__restrict__ vox, const int32_t *__restrict__ idx8,
                                                          const float *__restrict__ w8, const uint4 *__restrict__ lin,
                                                          const double *__restrict__ stat, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, int64_t n, int c, int cv,
                                                          uint4 *__restrict__ out, uint32_t *__restrict__ mask) {
  constexpr int V = Piece<ET>::V;
  constexpr int LPW = 32 / V;  // lanes per mask word: 8 (fp32) or 4 (16 bits); cv % LPW == 0 because c % 32 == 0
  for (int j = threadIdx.x; j < cv; j += blockDim.x) {
    float sc[V], sh[V];
    bn_coeffs<V>(stat, gamma, beta, c, j * V, sc, sh);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.y + threadIdx.y; i < n; i += (int64_t)gridDim.x * blockDim.y) {
      const uint4 lr = lin[i * cv + j];  // streamed row first: in flight while the corners are gathered
      Acc<V> acc = gather_corners<ET>(vox, idx8, w8, i, cv, j);
      Acc<V> t = widen(ET{}, lr);
      const unsigned bits = bn_relu_gate<ET>(t, sc, sh);
#pragma unroll
      for (int q = 0; q < V; ++q) acc.f[q] += t.f[q];
      out[i * cv + j] = narrow(ET{}, acc);
      // LPW consecutive lanes of one row make one mask word. The groups are aligned in the wave (blockDim.x is a power
      // of two >= LPW) and all their lanes take the same trips of both loops (cv % LPW == 0).
      const unsigned m = mask_word<V>(bits, j);
      if ((j & (LPW - 1)) == 0) mask[i * (c >> 5) + j / LPW] = m;
    }
  }
}

// dtype 0 fp32, 1 bf16, 2 fp16
int point_merge_any(const char *what, int dtype, const void *vox, const int32_t *idx8, const float *w8, const void *lin,
                    const double *stat, const float *gamma, const float *beta, int64_t n, int32_t c, void *out,
                    uint32_t *mask, void *stream) {
  if (n < 0 || c <= 0) { set_error("%s: bad sizes", what); return PCS_EINVAL; }
  if (c & 31) { set_error("%s: c = %d is not a multiple of 32 (the ReLU bit mask is made of whole words)", what, (int)c); return PCS_EUNSUPPORTED; }
  if (n == 0) return PCS_OK;
  if (!idx8 || !w8 || !lin || !stat || !out || !mask) { set_error("%s: null pointer", what); return PCS_EINVAL; }
  if (!aligned(vox, 16) || !aligned(lin, 16) || !aligned(out, 16)) {
    set_error("%s: vox, lin and out rows must be 16-byte aligned", what);
    return PCS_EUNSUPPORTED;
  }
  if (((uintptr_t)mask & 3) || ((uintptr_t)idx8 & 3) || ((uintptr_t)w8 & 3) || ((uintptr_t)stat & 7)) {
    set_error("%s: misaligned mask / idx8 / w8 / stat", what);
    return PCS_EINVAL;
  }
  const RowLaunch rl = row_launch(n, c / (dtype == 0 ? 4 : 8), kRowsPow2);   // TX >= 4: c >= 32
  PCS_DTYPE(dtype, hipLaunchKernelGGL(point_merge_kernel<ET>, rl.grid, rl.block, 0, as_stream(stream), reinterpret_cast<const uint4 *>(vox),
                                      idx8, w8, reinterpret_cast<const uint4 *>(lin), stat, gamma, beta, n, c, rl.cv,
                                      reinterpret_cast<uint4 *>(out), mask));
  return check_launch(what);
}

}  // namespace

extern "C" int pcs_point_merge_f32(const float *vox, const int32_t *idx8, const float *w8, const float *lin, const double *stat,
                                   const float *gamma, const float *beta, int64_t n, int32_t c, float *out, uint32_t *mask,
                                   void *stream) {
  return point_merge_any("pcs_point_merge_f32", 0, vox, idx8, w8, lin, stat, gamma, beta, n, c, out, mask, stream);
}

extern "C" int pcs_point_merge_h(const void *vox, const int32_t *idx8, const float *w8, const void *lin, const double *stat,
                                 const float *gamma, const float *beta, int64_t n, int32_t c, int32_t dtype, void *out,
                                 uint32_t *mask, void *stream) {
  if (bad_half("pcs_point_merge_h", dtype)) return PCS_EINVAL;
  return point_merge_any("pcs_point_merge_h", dtype, vox, idx8, w8, lin, stat, gamma, beta, n, c, out, mask, stream);
}
