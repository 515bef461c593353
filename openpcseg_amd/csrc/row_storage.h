// Row storage of the memory-bound kernels: how a feature row sits in memory (fp32, bf16 or fp16), how a piece of it is
// widened to fp32 registers and rounded ONCE on the store, and the row-tiled launch shape those kernels share. The only
// definition of the bf16 rounding and of "the value as stored, read back" (the ReLU gate of the bit masks) in the tree:
// the conv kernels (conv_common.h), norm.hip, pointvoxel.hip, pointmerge.hip, rangemerge.hip, recongate.hip and scatter.hip
// include it.
#pragma once
#include "pcs_common.h"

namespace pcs {

// ---- storage formats (the dtype argument of the C entries: 0 fp32, 1 bf16, 2 fp16); all arithmetic is fp32 -----------------
struct Bf16 {};
struct Fp16 {};
struct Fp32 {};
__device__ __forceinline__ float h2f(Bf16, uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
__device__ __forceinline__ float h2f(Fp16, uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
__device__ __forceinline__ uint16_t f2h(Bf16, float f) {  // round to nearest even; NaN stays NaN
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
__device__ __forceinline__ uint16_t f2h(Fp16, float f) {
  const _Float16 h = (_Float16)f;
  return __builtin_bit_cast(uint16_t, h);
}

// the value a store leaves in memory, read back: what a later `y > 0` sees (fp16 rounds (0, 2^-25] to 0)
__device__ __forceinline__ float stored(Fp32, float f) { return f; }
template <typename HT> __device__ __forceinline__ float stored(HT, float f) { return h2f(HT{}, f2h(HT{}, f)); }

// ---- pieces of a row ------------------------------------------------------------------------------------------------
template <typename ET> struct Elem { using T = uint16_t; };   // one element in memory
template <> struct Elem<Fp32> { using T = float; };
template <typename ET> struct Piece { static constexpr int V = 16 / (int)sizeof(typename Elem<ET>::T); };  // elements per 16 bytes

// V elements as they sit in memory: 16 bytes (4 floats / 8 halfs), 8 bytes (4 halfs) or one element
template <typename ET, int V> struct Raw;
template <> struct Raw<Fp32, 4> { using T = uint4; };
template <> struct Raw<Fp32, 1> { using T = float; };
template <typename HT> struct Raw<HT, 8> { using T = uint4; };
template <typename HT> struct Raw<HT, 4> { using T = uint2; };
template <typename HT> struct Raw<HT, 1> { using T = uint16_t; };

// piece j (of V elements) of the row that starts at `row`
template <typename ET, int V> __device__ __forceinline__ typename Raw<ET, V>::T ld_row(const typename Elem<ET>::T *row, int j) {
  return reinterpret_cast<const typename Raw<ET, V>::T *>(row)[j];
}

// the same V elements in fp32 registers
template <int V> struct Acc { float f[V]; };

__device__ __forceinline__ Acc<4> widen(Fp32, const uint4 &r) {
  Acc<4> a;
  a.f[0] = __uint_as_float(r.x); a.f[1] = __uint_as_float(r.y); a.f[2] = __uint_as_float(r.z); a.f[3] = __uint_as_float(r.w);
  return a;
}
__device__ __forceinline__ Acc<1> widen(Fp32, const float &r) { return Acc<1>{{r}}; }
template <typename HT> __device__ __forceinline__ void unpack2(HT, uint32_t r, float &lo, float &hi) {
  lo = h2f(HT{}, (uint16_t)(r & 0xFFFFu));
  hi = h2f(HT{}, (uint16_t)(r >> 16));
}
template <typename HT> __device__ __forceinline__ Acc<8> widen(HT, const uint4 &r) {
  Acc<8> a;
  unpack2(HT{}, r.x, a.f[0], a.f[1]); unpack2(HT{}, r.y, a.f[2], a.f[3]);
  unpack2(HT{}, r.z, a.f[4], a.f[5]); unpack2(HT{}, r.w, a.f[6], a.f[7]);
  return a;
}
template <typename HT> __device__ __forceinline__ Acc<4> widen(HT, const uint2 &r) {
  Acc<4> a;
  unpack2(HT{}, r.x, a.f[0], a.f[1]); unpack2(HT{}, r.y, a.f[2], a.f[3]);
  return a;
}
template <typename HT> __device__ __forceinline__ Acc<1> widen(HT, const uint16_t &r) { return Acc<1>{{h2f(HT{}, r)}}; }

// and back: the one rounding of an output element
__device__ __forceinline__ uint4 narrow(Fp32, const Acc<4> &a) {
  return make_uint4(__float_as_uint(a.f[0]), __float_as_uint(a.f[1]), __float_as_uint(a.f[2]), __float_as_uint(a.f[3]));
}
__device__ __forceinline__ float narrow(Fp32, const Acc<1> &a) { return a.f[0]; }
template <typename HT> __device__ __forceinline__ uint32_t pack2(HT, float lo, float hi) {
  return (uint32_t)f2h(HT{}, lo) | ((uint32_t)f2h(HT{}, hi) << 16);
}
template <typename HT> __device__ __forceinline__ uint4 narrow(HT, const Acc<8> &a) {
  return make_uint4(pack2(HT{}, a.f[0], a.f[1]), pack2(HT{}, a.f[2], a.f[3]), pack2(HT{}, a.f[4], a.f[5]), pack2(HT{}, a.f[6], a.f[7]));
}
template <typename HT> __device__ __forceinline__ uint2 narrow(HT, const Acc<4> &a) {
  return make_uint2(pack2(HT{}, a.f[0], a.f[1]), pack2(HT{}, a.f[2], a.f[3]));
}
template <typename HT> __device__ __forceinline__ uint16_t narrow(HT, const Acc<1> &a) { return f2h(HT{}, a.f[0]); }

// piece j of the row at `row` <- a, rounded
template <typename ET, int V> __device__ __forceinline__ void st_row(typename Elem<ET>::T *row, int j, const Acc<V> &a) {
  reinterpret_cast<typename Raw<ET, V>::T *>(row)[j] = narrow(ET{}, a);
}

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

// ---- row-tiled launch: TX lanes walk the cv pieces of one row, TY = 256 / TX rows per workgroup, grid-stride over the
// rows with a capped grid. A row wider than 64 pieces takes more than one pass of the lane row.
struct RowPolicy {
  bool pow2;      // TX = the power of two >= cv (shuffle groups stay aligned for any cv), or exactly min(cv, 64): 96
                  // channels = 24 vectors would idle 8 of 32 lanes
  int rows;       // rows a thread row takes before the grid grows
  int max_grid;
};
constexpr RowPolicy kRowsPow2 = {true, 1, 256 * 16};    // point <-> voxel, point merge, scatter
constexpr RowPolicy kRowsExact = {false, 1, 256 * 16};  // ReconBlock gate
constexpr RowPolicy kRowsExact4 = {false, 4, 2048};     // BatchNorm apply passes (unrolled by four rows)

struct RowLaunch {
  dim3 block, grid;
  int cv;  // pieces per row
};
inline RowLaunch row_launch(int64_t n, int cv, RowPolicy p) {
  RowLaunch r;
  r.cv = cv;
  int tx = 1;
  if (p.pow2) { while (tx < cv && tx < 64) tx <<= 1; }
  else if (cv > 1) tx = cv < 64 ? cv : 64;
  const int ty = 256 / tx;
  r.block = dim3(tx, ty);
  int64_t g = ceil_div(n, (int64_t)ty * p.rows);
  if (g > p.max_grid) g = p.max_grid;
  if (g < 1) g = 1;
  r.grid = dim3((unsigned)g);
  return r;
}

inline bool aligned(const void *p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

// the dtype argument of a 16-bit entry. The message texts are part of the C interface: pcs_bn_apply_h and pcs_bn_bwd_apply_h
// (norm.hip) have always printed the text without the value (with_value = false); pcs_bn_stats_h and pcs_bn_bwd_stats_h fold
// the dtype into their one "bad args" check and use is_half() alone
inline bool is_half(int32_t dtype) { return dtype == 1 || dtype == 2; }
inline bool bad_half(const char *what, int32_t dtype, bool with_value = true) {
  if (is_half(dtype)) return false;
  if (with_value) set_error("%s: dtype must be 1 (bf16) or 2 (fp16), got %d", what, (int)dtype);
  else set_error("%s: dtype must be 1 (bf16) or 2 (fp16)", what);
  return true;
}

// runs the statement(s) with `ET` = the storage tag of `DT`
#define PCS_DTYPE(DT, ...)                                      \
  do {                                                          \
    if ((DT) == 0) { using ET = pcs::Fp32; __VA_ARGS__; }       \
    else if ((DT) == 1) { using ET = pcs::Bf16; __VA_ARGS__; }  \
    else { using ET = pcs::Fp16; __VA_ARGS__; }                 \
  } while (0)
// the same with `V` = VW elements per access: a 16-byte piece (4 floats / 8 halfs), 4 elements, or 1
#define PCS_DTYPE_VEC(DT, VW, ...)                                                      \
  PCS_DTYPE(DT, {                                                                       \
    if ((VW) == pcs::Piece<ET>::V) { constexpr int V = pcs::Piece<ET>::V; __VA_ARGS__; } \
    else if ((VW) == 4) { constexpr int V = 4; __VA_ARGS__; }                           \
    else { constexpr int V = 1; __VA_ARGS__; }                                          \
  })

// ---- the two-level statistics of norm.hip and recongate.hip: per-workgroup partial rows, then a fixed-order double reduction --
constexpr int kStatBlocks = 1024;  // partial rows a statistics pass leaves (pcs_bn_num_partials() - 1)
constexpr int kRedCh = 4;          // columns per workgroup of the reduction kernels
constexpr int kRedLanes = 256;     // row lanes per workgroup: lane ty sums rows ty, ty + 256, ... into one double

}  // namespace pcs
