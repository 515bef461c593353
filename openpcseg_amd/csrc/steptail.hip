// The tail of a training step in two launches: gradient norm + overflow flag + loss-scale update, then unscale + clip + SGD.
// The reference ends every voxel / fusion iteration with scaler.unscale_ -> clip_grad_norm_(params, 10) -> scaler.step(SGD(momentum,
// weight_decay, nesterov)) -> scaler.update (R:train.py:367-372, R:pcseg/optim/__init__.py:15-34): torch runs that as ~7 passes over
// every parameter (about 68 B moved per element) behind a Python loop over ~200 tensors. Here one device-resident job table (one job
// per parameter tensor, workgroup -> job by binary search as weights_multi.hip does) serves two kernels that move 24 B per element:
//   steptail_norm_kernel   reads g once (4 B): sum of squares in double, non-finite flag, one partial per workgroup (at most 2048
//                          workgroups sweep the work blocks), and the workgroup that draws the last ticket folds the partials in a
//                          fixed order and writes the 32-byte record of pcseg_hip.h
//                          (and applies GradScaler.update's rule to the device-resident scale / growth tracker);
//   steptail_apply_kernel  reads g, p, buf and writes p, buf (20 B): one rounding per operation, nothing fused, so the result is
//                          the host form (openpcseg_amd.optim.sgd_tail_host) bit for bit whenever the record is the same.
// g is never written: gradients stay as backward left them, scaled and unclipped (torch's unscale_ / clip_grad_norm_ write them).
// No float atomics anywhere: two runs over the same memory give the same bits.
#include <string.h>

#include "pcs_common.h"

using namespace pcs;

namespace {

constexpr int kThreads = 256;
constexpr int kVec = 4;                                    // floats per 16-byte access
constexpr int kNormGrid = 256 * 8;                         // workgroups of the norm launch at most: 8 per CU
constexpr int kIters = PCS_STEP_BLOCK_ELEMS / (kThreads * kVec);
static_assert(kIters * kThreads * kVec == PCS_STEP_BLOCK_ELEMS, "a workgroup's elements are whole 16-byte sweeps");

// pcs_step_job of include/pcseg_hip.h
struct Job {
  float *p;
  const float *g;
  float *buf;
  int64_t numel;
  int32_t group, reserved;
  int64_t first_block;
};
static_assert(sizeof(Job) == sizeof(pcs_step_job), "pcs_step_job layout");

// the job whose block range holds workgroup wb: the last job with first_block <= wb (jobs without elements own no block and are
// never found: the job behind them has the same first_block and sits later in the table)
__device__ __forceinline__ Job find_job(const Job *__restrict__ jobs, int njobs, int64_t wb) {
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].first_block <= wb) lo = mid; else hi = mid - 1;
  }
  return jobs[lo];
}

// The table's pointers come out of memory, so the compiler knows no address space for them and would emit flat accesses; they are
// device allocations, and saying so gives global_load / global_store.
typedef float vfloat4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) vfloat4 gfloat4;
__device__ __forceinline__ gfloat *as_global(float *a) { return (gfloat *)a; }
__device__ __forceinline__ const gfloat *as_global(const float *a) { return (const gfloat *)a; }
__device__ __forceinline__ vfloat4 load4(const gfloat *a) { return *(const gfloat4 *)a; }
__device__ __forceinline__ void store4(gfloat *a, vfloat4 v) { *(gfloat4 *)a = v; }

__device__ __forceinline__ bool aligned16(const void *a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

__device__ __forceinline__ bool non_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) == 0x7F800000u; }

// workspace of the norm launch: [0] ticket (int32, zero between launches), 16 bytes in: one double per workgroup, then one int32
// flag per workgroup -- PCS_STEP_WS_BYTES
__device__ __forceinline__ double *ws_partials(void *ws) { return reinterpret_cast<double *>(reinterpret_cast<char *>(ws) + 16); }
__device__ __forceinline__ int32_t *ws_flags(void *ws, int64_t blocks) { return reinterpret_cast<int32_t *>(ws_partials(ws) + blocks); }

struct NormArgs {
  float max_norm;          // < 0: no clipping
  float *scale;            // device; nullptr: no scaler
  int32_t *growth_tracker; // device, with scale
  double growth, backoff;
  int32_t growth_interval;
};

__global__ void __launch_bounds__(kThreads) steptail_norm_kernel(const Job *__restrict__ jobs, int njobs, int64_t total_blocks, void *ws,
                                                                 NormArgs a, float *__restrict__ record) {
  __shared__ double sh_sum[kThreads / kWave];
  __shared__ int sh_bad[kThreads / kWave];
  __shared__ int sh_last;
  // a workgroup sweeps the work blocks blockIdx.x, blockIdx.x + gridDim.x, ... (one work block = PCS_STEP_BLOCK_ELEMS elements of one
  // job): one partial and one ticket per workgroup, and tickets on one word retire one after the other
  const int64_t groups = gridDim.x;
  double acc = 0.0;
  bool bad = false;
  for (int64_t wb = blockIdx.x; wb < total_blocks; wb += groups) {
    const Job j = find_job(jobs, njobs, wb);
    const int64_t base = (wb - j.first_block) * PCS_STEP_BLOCK_ELEMS;
    const int64_t left = j.numel - base;                    // elements of this work block: 1 .. PCS_STEP_BLOCK_ELEMS
    const int rem = left > PCS_STEP_BLOCK_ELEMS ? PCS_STEP_BLOCK_ELEMS : (left < 0 ? 0 : (int)left);
    const gfloat *g = as_global(j.g) + base;
    if (aligned16(j.g)) {
#pragma unroll
      for (int it = 0; it < kIters; ++it) {
        const int e = (it * kThreads + (int)threadIdx.x) * kVec;
        if (e + kVec <= rem) {
          const vfloat4 v = load4(g + e);
          acc += (double)v.x * (double)v.x; acc += (double)v.y * (double)v.y;
          acc += (double)v.z * (double)v.z; acc += (double)v.w * (double)v.w;
          bad |= non_finite(v.x) | non_finite(v.y) | non_finite(v.z) | non_finite(v.w);
        } else {
          for (int q = e; q < rem; ++q) {                   // the job's ragged end: at most 3 elements of one lane
            const float x = g[q];
            acc += (double)x * (double)x;
            bad |= non_finite(x);
          }
        }
      }
    } else {
      for (int e = threadIdx.x; e < rem; e += kThreads) {
        const float x = g[e];
        acc += (double)x * (double)x;
        bad |= non_finite(x);
      }
    }
  }
  // lanes -> wave -> workgroup, a fixed tree
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) acc += __shfl_down(acc, o, kWave);
  const int any_bad = __any(bad) ? 1 : 0;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (lane == 0) { sh_sum[wave] = acc; sh_bad[wave] = any_bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    int b = 0;
    for (int w = 0; w < kThreads / kWave; ++w) { s += sh_sum[w]; b |= sh_bad[w]; }
    // device-scope relaxed atomic stores are write-through (sc1): once they have left the wave (vmcnt 0) the partial is where
    // every other compute die reads it, so the ticket needs no fence of its own -- a fence per workgroup writes back and
    // invalidates the L2 thousands of times under the streaming loads (measured: 374 us for this kernel with one, per work block)
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(ws_partials(ws)) + blockIdx.x, (unsigned long long)__double_as_longlong(s),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(ws_flags(ws, groups) + blockIdx.x, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    sh_last = __hip_atomic_fetch_add(reinterpret_cast<int *>(ws), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)groups - 1;
  }
  __syncthreads();
  if (!sh_last) return;
  __threadfence();     // once per launch: every other workgroup's ticket, and so its partial, came before
  // the last workgroup: thread t folds partials t, t + 256, ... in index order (device-scope loads, past the caches a die keeps to
  // itself), then the same fixed tree. The order depends on the grid alone, never on which workgroup arrived when.
  double s = 0.0;
  int b = 0;
  for (int64_t i = threadIdx.x; i < groups; i += kThreads) {
    s += __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<unsigned long long *>(ws_partials(ws)) + i, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT));
    b |= __hip_atomic_load(ws_flags(ws, groups) + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) s += __shfl_down(s, o, kWave);
  const int any_b = __any(b != 0) ? 1 : 0;
  __syncthreads();     // sh_sum / sh_bad of the first fold have been read
  if (lane == 0) { sh_sum[wave] = s; sh_bad[wave] = any_b; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  {
#pragma clang fp contract(off)
    double total = 0.0;
    int found = 0;
    for (int w = 0; w < kThreads / kWave; ++w) { total += sh_sum[w]; found |= sh_bad[w]; }
    const float total_norm = (float)sqrt(total);
    float inv_scale = 1.0f;
    if (a.scale) inv_scale = (float)(1.0 / (double)*a.scale);
    const float unscaled = total_norm * inv_scale;
    float coef = 1.0f;
    if (a.max_norm >= 0.0f) {
      // fp32 division by way of double: 53 bits >= 2 * 24 + 2, so the second rounding cannot change the result
      const float c = (float)((double)a.max_norm / (double)(unscaled + 1e-6f));
      coef = c > 1.0f ? 1.0f : c;     // clamp(max=1): a NaN norm stays a NaN coefficient, as in torch
    }
    record[0] = total_norm;
    record[1] = inv_scale;
    record[2] = coef;
    record[3] = found ? 1.0f : 0.0f;
    record[4] = unscaled;
    record[5] = record[6] = record[7] = 0.0f;
    if (a.scale) {   // torch.amp.GradScaler.update (amp_update_scale_): the next step's scale
      if (found) {
        *a.scale = (float)((double)*a.scale * a.backoff);
        *a.growth_tracker = 0;
      } else {
        const int32_t ok = *a.growth_tracker + 1;
        if (ok == a.growth_interval) {
          const float grown = (float)((double)*a.scale * a.growth);
          if (!non_finite(grown)) *a.scale = grown;
          *a.growth_tracker = 0;
        } else {
          *a.growth_tracker = ok;
        }
      }
    }
    *reinterpret_cast<int *>(ws) = 0;   // the ticket of the next launch
  }
}

// pcs_step_hyper by value in the kernel arguments: a per-step change of lr costs no copy
struct Hyper {
  float lr[PCS_STEP_MAX_GROUPS], wd[PCS_STEP_MAX_GROUPS], mu[PCS_STEP_MAX_GROUPS];
  int32_t nesterov[PCS_STEP_MAX_GROUPS];
  int32_t n_groups;
};
static_assert(sizeof(Hyper) == sizeof(pcs_step_hyper), "pcs_step_hyper layout");

struct Group { float inv_scale, coef, neg_lr, wd, mu; bool nesterov; };

// one element; every operation rounds once (no contraction into FMAs), in the order of include/pcseg_hip.h
template <bool kMomentum>
__device__ __forceinline__ void sgd_element(const Group &h, float g, float &p, float &buf) {
#pragma clang fp contract(off)
  const float g1 = g * h.inv_scale;
  const float g2 = g1 * h.coef;
  const float wp = h.wd * p;
  float d = g2 + wp;
  if (kMomentum) {
    const float mb = h.mu * buf;
    buf = mb + d;
    if (h.nesterov) {
      const float nb = h.mu * buf;
      d = d + nb;
    } else {
      d = buf;
    }
  }
  const float u = h.neg_lr * d;
  p = p + u;
}

template <bool kMomentum>
__device__ __forceinline__ void apply_block(const Job &j, const Group &h, int64_t base, int rem) {
  gfloat *p = as_global(j.p) + base;
  const gfloat *g = as_global(j.g) + base;
  gfloat *buf = kMomentum ? as_global(j.buf) + base : nullptr;
  if (aligned16(j.p) && aligned16(j.g) && (!kMomentum || aligned16(j.buf))) {
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int e = (it * kThreads + (int)threadIdx.x) * kVec;
      if (e + kVec <= rem) {
        const vfloat4 gv = load4(g + e);
        vfloat4 pv = load4(p + e);
        vfloat4 bv = kMomentum ? load4(buf + e) : vfloat4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < kVec; ++q) {
          float pe = pv[q], be = bv[q];
          sgd_element<kMomentum>(h, gv[q], pe, be);
          pv[q] = pe;
          bv[q] = be;
        }
        store4(p + e, pv);
        if (kMomentum) store4(buf + e, bv);
      } else {
        for (int q = e; q < rem; ++q) {                     // the job's ragged end, element by element
          float pe = p[q], be = kMomentum ? buf[q] : 0.f;
          sgd_element<kMomentum>(h, g[q], pe, be);
          p[q] = pe;
          if (kMomentum) buf[q] = be;
        }
      }
    }
  } else {
    for (int e = threadIdx.x; e < rem; e += kThreads) {
      float pe = p[e], be = kMomentum ? buf[e] : 0.f;
      sgd_element<kMomentum>(h, g[e], pe, be);
      p[e] = pe;
      if (kMomentum) buf[e] = be;
    }
  }
}

__global__ void __launch_bounds__(kThreads) steptail_apply_kernel(const Job *__restrict__ jobs, int njobs, Hyper hy,
                                                                  const float *__restrict__ record, int skip_on_inf) {
  Group h;
  h.inv_scale = 1.0f;
  h.coef = 1.0f;
  if (record) {
    if (skip_on_inf && record[3] != 0.0f) return;           // an overflowed step: p and buf keep their bits
    h.inv_scale = record[1];
    h.coef = record[2];
  }
  const int64_t wb = blockIdx.x;
  const Job j = find_job(jobs, njobs, wb);
  h.neg_lr = -hy.lr[j.group];
  h.wd = hy.wd[j.group];
  h.mu = hy.mu[j.group];
  h.nesterov = hy.nesterov[j.group] != 0;
  const int64_t base = (wb - j.first_block) * PCS_STEP_BLOCK_ELEMS;
  const int64_t left = j.numel - base;
  const int rem = left > PCS_STEP_BLOCK_ELEMS ? PCS_STEP_BLOCK_ELEMS : (left < 0 ? 0 : (int)left);
  if (j.buf) apply_block<true>(j, h, base, rem);
  else apply_block<false>(j, h, base, rem);
}

bool table_args_ok(const void *jobs_dev, int32_t n_jobs, int64_t total_blocks) {
  return n_jobs >= 0 && total_blocks >= 0 && total_blocks <= 0x7FFFFFFF && (n_jobs == 0 || jobs_dev);
}

}  // namespace

extern "C" int64_t pcs_step_plan(pcs_step_job *jobs_host, int32_t n_jobs, const pcs_step_hyper *hyper) {
  if (n_jobs < 0 || (n_jobs > 0 && !jobs_host) || !hyper || hyper->n_groups < 1 || hyper->n_groups > PCS_STEP_MAX_GROUPS) {
    set_error("pcs_step_plan: bad args (1 .. %d groups)", PCS_STEP_MAX_GROUPS);
    return -1;
  }
  int64_t blocks = 0;
  for (int i = 0; i < n_jobs; ++i) {
    pcs_step_job &j = jobs_host[i];
    if (j.numel < 0 || j.group < 0 || j.group >= hyper->n_groups) {
      set_error("pcs_step_plan: job %d: negative numel or a group outside [0, %d)", i, hyper->n_groups);
      return -1;
    }
    const bool momentum = hyper->mu[j.group] != 0.0f;
    if (j.numel > 0 && (!j.p || !j.g || (momentum && !j.buf) || (!momentum && j.buf))) {
      set_error("pcs_step_plan: job %d: null p / g, or buf that does not go with its group's momentum", i);
      return -1;
    }
    if (((uintptr_t)j.p | (uintptr_t)j.g | (uintptr_t)j.buf) & 3) {
      set_error("pcs_step_plan: job %d: p / g / buf not 4-byte aligned", i);
      return -1;
    }
    j.reserved = 0;
    j.first_block = blocks;
    blocks += ceil_div(j.numel, PCS_STEP_BLOCK_ELEMS);
  }
  if (blocks > 0x7FFFFFFF) { set_error("pcs_step_plan: too many work blocks"); return -1; }
  return blocks;
}

extern "C" int pcs_step_norm(const pcs_step_job *jobs_dev, int32_t n_jobs, int64_t total_blocks, float max_norm, float *scale,
                             int32_t *growth_tracker, double growth_factor, double backoff_factor, int32_t growth_interval,
                             void *ws, int64_t ws_bytes, float *record, void *stream) {
  if (!table_args_ok(jobs_dev, n_jobs, total_blocks) || !record || (scale && !growth_tracker) || max_norm != max_norm) {
    set_error("pcs_step_norm: bad args");
    return PCS_EINVAL;
  }
  if (n_jobs == 0 || total_blocks == 0) {
    set_error("pcs_step_norm: an empty table has no norm (the caller skips the step)");
    return PCS_EINVAL;
  }
  if (!ws || ws_bytes < (int64_t)PCS_STEP_WS_BYTES(total_blocks)) {
    set_error("pcs_step_norm: workspace of %lld bytes, PCS_STEP_WS_BYTES wants %lld", (long long)ws_bytes,
              (long long)PCS_STEP_WS_BYTES(total_blocks));
    return PCS_EWORKSPACE;
  }
  NormArgs a;
  a.max_norm = max_norm;
  a.scale = scale;
  a.growth_tracker = growth_tracker;
  a.growth = growth_factor;
  a.backoff = backoff_factor;
  a.growth_interval = growth_interval;
  const int64_t grid = total_blocks < kNormGrid ? total_blocks : kNormGrid;
  hipLaunchKernelGGL(steptail_norm_kernel, dim3((unsigned)grid), dim3(kThreads), 0, as_stream(stream),
                     reinterpret_cast<const Job *>(jobs_dev), (int)n_jobs, total_blocks, ws, a, record);
  return check_launch("pcs_step_norm");
}

extern "C" int pcs_step_apply(const pcs_step_job *jobs_dev, int32_t n_jobs, int64_t total_blocks, const pcs_step_hyper *hyper,
                              const float *record, int32_t skip_on_inf, void *stream) {
  if (!table_args_ok(jobs_dev, n_jobs, total_blocks) || !hyper || hyper->n_groups < 1 || hyper->n_groups > PCS_STEP_MAX_GROUPS ||
      (skip_on_inf && !record)) {
    set_error("pcs_step_apply: bad args");
    return PCS_EINVAL;
  }
  if (n_jobs == 0 || total_blocks == 0) return PCS_OK;
  Hyper hy;
  static_assert(sizeof(hy) == sizeof(*hyper), "");
  memcpy(&hy, hyper, sizeof(hy));
  hipLaunchKernelGGL(steptail_apply_kernel, dim3((unsigned)total_blocks), dim3(kThreads), 0, as_stream(stream),
                     reinterpret_cast<const Job *>(jobs_dev), (int)n_jobs, hy, record, (int)skip_on_inf);
  return check_launch("pcs_step_apply");
}
