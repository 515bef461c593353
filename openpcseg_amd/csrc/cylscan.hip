// The cylinder dataset's transform of a raw batch on the device -- gfx950, ONE launch, no host read.
// The reference runs it per frame in the dataloader workers with NumPy (R:pcseg/data/dataset/semantickitti/
// semantickitti_cylinder.py:104-160: aug_points, the augmented xyz stored back as float32, cart2polar, the partition), once per
// vote under test-time augmentation (:92-99, ten votes per frame). Here, for every raw row i of frame f and every vote v, with
// the parameter row of (v, f):
//   (x', y', z') = affine_row(x, y, z)          raw_scan.h    -- float64, the order of section 7h, one rounding to float32
//   pol, cell, centre = cyl_cell(x', y', z')    cyl_cell.h    -- the arithmetic of cyl_partition_kernel
//   feat  row v * n + i = [centre (3), rho, phi in degrees, z', x', y', extras...]      (8 + c - 3 floats)
//   coord row v * n + i = cell;  scenes[v * n + i] = v * F + f
// Cells are >= 0 after the clip: no minimum, no ticket, no workspace. Traffic: the scan is read once (4 c B per row) whatever
// the number of votes; per vote 4 (8 + c - 3) + 12 + 8 B are written (56 B at c = 4).
// A workgroup stays inside one frame (the frame is a grid axis), the grid along a frame is sized to the chip, the V parameter
// rows sit in LDS: the row range of a frame, the row load, the staging, the grid and the vote dispatch are raw_scan.h's.
// The store: a feature row is 36 B at c = 4, so a lane that writes its own row issues nine dword stores at a 36-byte stride. Per vote the workgroup's 256 rows are ONE contiguous range of `feat` (and of `coord`): the staged form puts
// the range into LDS (an odd row width falls on distinct banks as it is, an even one is skewed by a pad word per 64) and writes
// it out with consecutive lanes on consecutive addresses -- 16-byte stores over the aligned middle, dwords at the head and the
// tail, because the range starts at (v n + i0) (8 + c - 3) 4 bytes. Two LDS buffers alternate, so a vote costs one barrier.
// PCS_CYLSCAN_STORE (debug / A-B, read once): 0 features and cells staged, 1 every lane stores its own rows, 2 features staged and
// cells direct -- the default: measured on twelve scans x ten votes it is the fastest form beyond the block-to-block spread, and
// within the spread of the other two elsewhere (profiles/cylinder_batch_bench.json).
#include <math.h>
#include <stdlib.h>

#include "cyl_cell.h"
#include "pcs_common.h"
#include "raw_scan.h"

using namespace pcs;

namespace {

constexpr int kBlock = kScanBlock;
constexpr int kMaxExtra = kScanMaxExtra;

enum StoreForm { kStaged = 0, kDirect = 1, kStagedFeat = 2 };

int known_form(int f) { return f == kDirect || f == kStaged ? f : kStagedFeat; }

int store_env() {   // read once
  static const int form = [] {
    const char *v = getenv("PCS_CYLSCAN_STORE");
    return known_form(v ? atoi(v) : kStagedFeat);
  }();
  return form;
}

int g_store_override = -1;   // pcs_debug_cylscan_store: -1 = the environment

template <typename T> struct Vec4;
template <> struct Vec4<float> { using type = float4; };
template <> struct Vec4<int32_t> { using type = int4; };

// `total` words of a workgroup's range go from LDS to dst[0 .. total). The range sits in `stage` at words [shift, shift + total)
// with shift = the word phase of dst inside its 16 bytes (0..3), so word 4 j of the stage and global word dst - shift + 4 j are
// both 16-byte aligned: whole groups j move as one 16-byte store, the words before the first and after the last whole group as
// dwords. SKEW: stage word w lives at LDS word w + (w >> 6) -- one pad word per 64, which spreads rows of an EVEN width over the
// banks (an odd width needs none and reads its groups as one 16-byte LDS load).
template <bool SKEW> __device__ __forceinline__ int stage_at(int w) { return SKEW ? w + (w >> 6) : w; }

template <typename T, bool SKEW>
__device__ __forceinline__ void flush_range(T *__restrict__ dst, const T *stage, int total, int shift, int tid) {
  using V4 = typename Vec4<T>::type;
  const int end = shift + total;
  const int jlo = (shift + 3) >> 2, jhi = end >> 2;   // whole groups: jlo <= j < jhi
  if (jhi > jlo) {
    for (int j = jlo + tid; j < jhi; j += kBlock) {
      V4 q;
      if (SKEW) {   // 4 j .. 4 j + 3 never straddle a multiple of 64: consecutive LDS words, at any phase
        const T *s = stage + stage_at<true>(4 * j);
        q.x = s[0]; q.y = s[1]; q.z = s[2]; q.w = s[3];
      } else {
        q = *reinterpret_cast<const V4 *>(stage + 4 * j);
      }
      *reinterpret_cast<V4 *>(dst + (4 * j - shift)) = q;
    }
    const int head = 4 * jlo - shift, tail0 = 4 * jhi;   // head <= 3 words, tail <= 3 words
    if (tid < head) dst[tid] = stage[stage_at<SKEW>(shift + tid)];
    if (tid < end - tail0) dst[tail0 - shift + tid] = stage[stage_at<SKEW>(tail0 + tid)];
  } else {
    for (int w = shift + tid; w < end; w += kBlock) dst[w - shift] = stage[stage_at<SKEW>(w)];
  }
}

__device__ __forceinline__ int word_phase(const void *p) { return (int)(((uintptr_t)p >> 2) & 3); }

// VB: compiled bound of the vote loop (V <= VB) and of the parameter rows in LDS. ROW16: C == 4 and `pts` 16-byte aligned -- one
// 16-byte load per row, the feature row's width (9) and its LDS layout (linear) known to the compiler.
template <int VB, bool ROW16>
__global__ void __launch_bounds__(kBlock) cyl_scan_kernel(const float *__restrict__ pts, int64_t n, int C,
                                                          const int64_t *__restrict__ frame_offsets, int F,
                                                          const double *__restrict__ params, int V, CylCfg cfg, int form,
                                                          float *__restrict__ feat, int32_t *__restrict__ coord,
                                                          int64_t *__restrict__ scenes) {
  constexpr int kMaxFdim = ROW16 ? 9 : 8 + kMaxExtra;
  constexpr int kStageWords = kBlock * kMaxFdim + 4;   // + 4: the phase shift
  // votes in flight: the general-width instances stay rolled (unrolled, their scalar registers spill)
  constexpr int kUnroll = !ROW16 ? 1 : (VB <= 4 ? VB : 2);
  __shared__ double sp[VB * 8];
  __shared__ CylCfg scfg;   // read from LDS where it is used: 18 doubles held in scalar registers through the loop spill them
  __shared__ __align__(16) float fstage[2][ROW16 ? kStageWords : kStageWords + kStageWords / 64 + 1];   // general width: skewed
  __shared__ __align__(16) int32_t cstage[2][kBlock * 3 + 4];
  const int f = blockIdx.y, tid = threadIdx.x;
  const FrameRows fr = frame_rows(frame_offsets, f, n);
  const int64_t lo = fr.lo, hi = fr.hi;
  if (hi <= lo) return;   // an empty frame writes nothing
  const int64_t want = (hi - lo + kBlock - 1) / kBlock;
  if ((int64_t)blockIdx.x >= want) return;   // the same for the whole workgroup
  stage_params(sp, params, V, F, f);
  if (tid == 0) scfg = cfg;
  __syncthreads();
  const int extras = ROW16 ? 1 : C - 3, fdim = 8 + extras;
  int buf = 0;
  for (int64_t base = lo + (int64_t)blockIdx.x * kBlock; base < hi; base += (int64_t)gridDim.x * kBlock) {
    const int rows = hi - base < kBlock ? (int)(hi - base) : kBlock;   // this round's rows of the workgroup: base .. base + rows
    const bool live = tid < rows;
    RawRow r = {};
    if (live) r = load_raw_row<ROW16>(pts, base + tid, C);
#pragma unroll kUnroll
    for (int v = 0; v < VB; ++v) {
      if (v >= V) continue;   // uniform; a constant trip count, so that the loop unrolls around its barrier
      float fx, fy, fz, pol[3], centre[3];
      int idx[3];
      affine_row(r.x, r.y, r.z, sp + v * 8, fx, fy, fz);
      cyl_cell(fx, fy, fz, scfg, pol, idx, centre);
      const float head[8] = {centre[0], centre[1], centre[2], pol[0], pol[1], pol[2], fx, fy};
      const int64_t row0 = (int64_t)v * n + base;   // first output row of the workgroup's range under this vote
      if (live) scenes[row0 + tid] = (int64_t)v * F + f;
      float *fdst = feat + row0 * fdim;
      int32_t *cdst = coord + row0 * 3;
      if (form == kDirect) {
        if (live) {
          float *o = fdst + (int64_t)tid * fdim;
#pragma unroll
          for (int k = 0; k < 8; ++k) o[k] = head[k];
#pragma unroll
          for (int k = 0; k < kMaxExtra; ++k)
            if (k < extras) o[8 + k] = r.extra[k];
        }
      } else {
        const int w0 = word_phase(fdst) + tid * fdim;   // the row's first word of the staged range
        float *s = fstage[buf];
        if (live) {
#pragma unroll
          for (int k = 0; k < 8; ++k) s[stage_at<!ROW16>(w0 + k)] = head[k];
#pragma unroll
          for (int k = 0; k < kMaxExtra; ++k)
            if (k < extras) s[stage_at<!ROW16>(w0 + 8 + k)] = r.extra[k];
        }
      }
      if (form != kStaged) {
        if (live) { cdst[tid * 3 + 0] = idx[0]; cdst[tid * 3 + 1] = idx[1]; cdst[tid * 3 + 2] = idx[2]; }
      } else {
        int32_t *s = cstage[buf] + word_phase(cdst) + tid * 3;
        if (live) { s[0] = idx[0]; s[1] = idx[1]; s[2] = idx[2]; }
      }
      if (form != kDirect) {   // uniform: the whole workgroup meets the barrier
        __syncthreads();
        flush_range<float, !ROW16>(fdst, fstage[buf], rows * fdim, word_phase(fdst), tid);
        if (form == kStaged) flush_range<int32_t, false>(cdst, cstage[buf], rows * 3, word_phase(cdst), tid);
        buf ^= 1;   // the next vote fills the other buffer: its last readers are a barrier behind
      }
    }
  }
}

}  // namespace

extern "C" void pcs_debug_cylscan_store(int32_t form) { g_store_override = form < 0 ? -1 : known_form(form); }

extern "C" int pcs_cylinder_scan_batch_f32(const float *points, int64_t n, int32_t c, const int64_t *frame_offsets, int32_t num_frames,
                                           const double *params, int32_t num_votes, const double *space_min3,
                                           const double *space_max3, const int32_t *grid3, float *feat, int32_t *coord,
                                           int64_t *scenes, void *stream) {
  if (!scan_sizes_ok(n, num_frames, num_votes) || c < 3 || c > PCS_SCAN_MAX_COLUMNS) {
    set_error("pcs_cylinder_scan_batch_f32: bad args (n >= 0, 3 <= c <= %d, 1 <= votes <= %d, 1 <= frames <= 65535)",
              PCS_SCAN_MAX_COLUMNS, PCS_SCAN_MAX_VOTES);
    return PCS_EINVAL;
  }
  if (!space_min3 || !space_max3 || !grid3) { set_error("pcs_cylinder_scan_batch_f32: null cylinder space"); return PCS_EINVAL; }
  CylCfg cfg;
  if (!cyl_cfg(space_min3, space_max3, grid3, cfg)) {
    set_error("pcs_cylinder_scan_batch_f32: grid must be >= 2 and max > min");
    return PCS_EINVAL;
  }
  if (n == 0) return PCS_OK;
  if (!points || !frame_offsets || !params || !feat || !coord || !scenes) {
    set_error("pcs_cylinder_scan_batch_f32: null pointer");
    return PCS_EINVAL;
  }
  const bool row16 = c == 4 && ((uintptr_t)points & 15) == 0;
  const dim3 grid(vote_grid(n, num_frames, num_votes), num_frames);
  const int form = g_store_override >= 0 ? g_store_override : store_env();
  dispatch_votes(num_votes, row16, [&](auto vb, auto r16) {
    hipLaunchKernelGGL((cyl_scan_kernel<decltype(vb)::value, decltype(r16)::value>), grid, dim3(kBlock), 0, as_stream(stream), points, n,
                       c, frame_offsets, num_frames, params, num_votes, cfg, form, feat, coord, scenes);
  });
  return check_launch("pcs_cylinder_scan_batch_f32");
}
