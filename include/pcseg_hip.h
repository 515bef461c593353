/*
 * pcseg_hip.h -- C ABI of libpcseg_hip.so, the MI355X (gfx950) sparse-voxel hot path.
 *
 * This is the drop-in boundary ("B-B" in SURVEY.md section 8b): every entry point below
 * replaces one function of the reference's native module `torchsparse.backend`
 * (TS = /root/reference/package/torchsparse.zip, member prefix torchsparse/), i.e. what the
 * reference's pybind table TS:torchsparse/backend/pybind_cuda.cpp:18-39 binds, plus the
 * rulebook construction that the reference does in Python on top of those functions
 * (TS:torchsparse/nn/functional/conv.py:156-176, downsample.py:11-52).
 *
 * Conventions
 *   - plain C: raw DEVICE pointers + sizes, no torch types, no allocation inside the library.
 *     Scratch memory is caller-provided ("ws"); its size comes from the matching *_ws_bytes().
 *   - every launch goes to the hipStream_t passed as `stream` (void* here so that plain C
 *     callers need no HIP headers). Nothing synchronises the device or the host.
 *   - return value: PCS_OK (0) or a negative PCS_E* code; pcs_last_error() gives the text.
 *   - all tensors are dense row-major; "coords" rows are int32 [x, y, z, batch]
 *     (TS:torchsparse/tensor.py:10-21).
 *   - dtype suffix _f32 = IEEE fp32 storage and fp32 MFMA / FMA arithmetic.
 */
#ifndef PCSEG_HIP_H_
#define PCSEG_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCS_OK 0
#define PCS_EINVAL (-1)   /* bad argument (shape / alignment / null pointer)            */
#define PCS_EWORKSPACE (-2) /* caller workspace too small                                */
#define PCS_ELAUNCH (-3)  /* hipLaunch / hipMemsetAsync failed (pcs_last_error has text) */
#define PCS_EUNSUPPORTED (-4)

/* Still 12 after three additive changes: the `reserved` word of pcs_conv_epilogue became `flags` (PCS_EP_RELU; a zeroed struct
 * means what it meant), the prediction-tail export was added, and pcs_conv_epilogue grew two trailing fields that are read only
 * when the new flag PCS_EP_POST_AFFINE is set. A caller built against the earlier v12 header runs unchanged. */
#define PCS_ABI_VERSION 12

int pcs_abi_version(void);
const char *pcs_last_error(void);

/* ------------------------------------------------------------------------------------------
 * K1  hash_cuda          TS:torchsparse/backend/hash/hash_cuda.cu:10-23,67-73
 * 64-bit FNV-1a over the four uint32 words of a coord row, folded to 60 bits. Bit-exact.
 * coords (n,4) int32 -> out (n,) int64
 */
int pcs_hash(const int32_t *coords, int64_t n, int64_t *out, void *stream);

/* K2  kernel_hash_cuda   TS:torchsparse/backend/hash/hash_cuda.cu:27-55,75-84
 * hash of (coords[:, :3] + offsets[k], coords[:, 3]) for every kernel offset.
 * coords (n,4) int32, offsets (K,3) int32 -> out (K,n) int64, k-major. Bit-exact.
 */
int pcs_kernel_hash(const int32_t *coords, int64_t n, const int32_t *offsets, int32_t K,
                    int64_t *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * K3-K5  hash_query_cuda  TS:torchsparse/backend/others/query_cuda.cu:9-56
 *                         TS:torchsparse/backend/hashmap/hashmap_cuda.cu:8-127
 * The reference builds a 3-function cuckoo table with a host-driven rehash loop on every
 * call. Here: ONE open-addressing (linear probe) table of {key:int64, value:int32}, built
 * by a single kernel with 64-bit CAS, no host round trip. Value = position of the key in
 * `keys`; with duplicate keys the SMALLEST position wins (the reference's CPU twin keeps the
 * first insert, TS:torchsparse/backend/others/query_cpu.cpp:22-26).
 * Table storage is caller-owned: `capacity` slots (power of two, from pcs_hashtable_capacity)
 * laid out as  uint64 key[capacity] | int32 val[capacity]  (pcs_hashtable_bytes).
 */
int64_t pcs_hashtable_capacity(int64_t n);
size_t pcs_hashtable_bytes(int64_t capacity);
int pcs_hashtable_build(const int64_t *keys, int64_t n, void *table, int64_t capacity,
                        void *stream);
/* out[i] = (position of queries[i] in keys) + 1, or 0 when absent -- the reference's
 * backend convention (query_cuda.cu / hashmap_cuda.cu:104-127; Python subtracts 1,
 * TS:torchsparse/nn/functional/query.py:32). */
int pcs_hashtable_query(const void *table, int64_t capacity, const int64_t *queries,
                        int64_t n1, int64_t *out, void *stream);

/* K6  count_cuda  TS:torchsparse/backend/others/count_cuda.cu:10-31
 * out[idx[i]] += 1 for idx[i] >= 0; out (s,) int32 is zeroed inside. */
int pcs_count(const int32_t *idx, int64_t n, int32_t *out, int64_t s, void *stream);

/* ------------------------------------------------------------------------------------------
 * K7/K8  voxelize_forward_cuda / voxelize_backward_cuda
 *        TS:torchsparse/backend/voxelize/voxelize_cuda.cu:12-80
 * fwd: out[idx[i], :] += feats[i, :] / counts[idx[i]]   (divide BEFORE accumulating, as the
 *      reference does); out (m,c) is zeroed inside; rows with idx[i] < 0 are skipped.
 * bwd: gin[i, :] = gout[idx[i], :] / counts[idx[i]]      (0 where idx[i] < 0)
 */
int pcs_voxelize_fwd_f32(const float *feats, const int32_t *idx, const int32_t *counts,
                         int64_t n, int64_t m, int32_t c, float *out, void *stream);
/* The CSR the contention-free forms below run over [v11]: index (n,) int32 = target row of every entry (a voxel per point for
 * K7, a voxel per (point, corner) for K10; < 0 or >= m = no row) -> order (n,) int64 = entry positions sorted by target row,
 * equal rows in ascending position (stable: the summation order of every output row is fixed), entries without a row behind
 * the last row; rowptr (m+1,) int64 = start of each row's run. One radix sort over the bits a row index needs + one binary
 * search per row. ws / ws_bytes from pcs_index_csr_ws_bytes(n, m) (0 on bad sizes); never allocates. */
size_t pcs_index_csr_ws_bytes(int64_t n, int64_t m);
int pcs_index_csr_i32(const int32_t *index, int64_t n, int64_t m, int64_t *order, int64_t *rowptr, void *ws,
                      size_t ws_bytes, void *stream);
/* contention-free forward: order int64 = point rows sorted by voxel (points with idx < 0 outside [rowptr[0], rowptr[m])),
 * rowptr (m+1) int64; every out row written once, deterministic summation order */
int pcs_voxelize_fwd_csr_f32(const float *feats, const int64_t *order, const int64_t *rowptr,
                             const int32_t *counts, int64_t m, int32_t c, float *out, void *stream);
int pcs_voxelize_bwd_f32(const float *gout, const int32_t *idx, const int32_t *counts,
                         int64_t n, int32_t c, float *gin, void *stream);
/* K7 (CSR form) / K8 with 16-bit feature storage, as the reference's AT_DISPATCH_FLOATING_TYPES_AND_HALF instances serve under
 * --amp: feats / out / gout / gin are bf16 (dtype 1) or fp16 (dtype 2) rows, any other dtype is PCS_EINVAL; order, rowptr, idx and
 * counts as in the _f32 entries. Every sum is accumulated in fp32 registers in `order` order (divide, then add) and rounded to
 * storage once (nearest even); every output row is written exactly once, zeros for a voxel without points (fwd) and for a point
 * without a voxel or with a zero count (bwd). 16-byte accesses where c % 8 == 0 and the rows are 16-byte aligned, 8-byte where
 * c % 4 == 0, scalar otherwise. The atomic form pcs_voxelize_fwd_f32 has no 16-bit twin. */
int pcs_voxelize_fwd_csr_h(const void *feats, const int64_t *order, const int64_t *rowptr, const int32_t *counts,
                           int64_t m, int32_t c, int32_t dtype, void *out, void *stream);
int pcs_voxelize_bwd_h(const void *gout, const int32_t *idx, const int32_t *counts, int64_t n, int32_t c,
                       int32_t dtype, void *gin, void *stream);

/* K9/K10  devoxelize_forward_cuda / devoxelize_backward_cuda
 *         TS:torchsparse/backend/devoxelize/devoxelize_cuda.cu:11-98
 * fwd: out[i,:] = sum_{k<8} w[i,k] * feat[idx[i,k],:]  (idx -1 => 0), accumulated in
 *      registers in k = 0..7 order and written once.
 * bwd: gfeat[idx[i,k],:] += w[i,k] * gout[i,:]; gfeat (m,c) is zeroed inside.
 * idx (n,8) int32, w (n,8) fp32.
 */
int pcs_devoxelize_fwd_f32(const float *feat, const int32_t *idx8, const float *w8, int64_t n,
                           int32_t c, float *out, void *stream);
int pcs_devoxelize_bwd_f32(const float *gout, const int32_t *idx8, const float *w8, int64_t n,
                           int64_t m, int32_t c, float *gfeat, void *stream);
/* K9 with 16-bit feature storage: feat / out bf16 (dtype 1) or fp16 (dtype 2), any other dtype is PCS_EINVAL; w8 stays fp32.
 * The 8 corners are accumulated in fp32 registers in k = 0..7 order and rounded to storage once. */
int pcs_devoxelize_fwd_h(const void *feat, const int32_t *idx8, const float *w8, int64_t n, int32_t c,
                         int32_t dtype, void *out, void *stream);
/* K9 merged with the point branch of SPVCNN (additive, still ABI v12):
 *   R:pcseg/model/segmentor/fusion/spvcnn/spvcnn.py:417-418, 430-431, 443-444
 *   `z_next.F = voxel_to_point(x, z).F + ReLU(BatchNorm(Linear(z.F)))` with the Linear output `lin` (n, c) given:
 *     out[i,j]       = ( sum_{k<8, idx8[i,k] >= 0} w8[i,k] * vox[idx8[i,k], j] ) + max(0, bn(lin[i,j]))
 *     mask bit (i,j) = [ bn(lin[i,j]) rounded to the storage type > 0 ]      word i * (c / 32) + j / 32, bit j % 32:
 *                                                what pcs_bn_apply_* writes (the gate of its STORED y) and
 *                                                pcs_bn_bwd_stats_* / pcs_bn_bwd_apply_* read (relu = 1, y = NULL)
 *   stat = mean | invstd (2c doubles), gamma / beta (c floats or NULL) as pcs_bn_apply_* takes them, bn(x) by the same
 *   expression. The corners are accumulated in fp32 registers from zero in k = 0..7 order as pcs_devoxelize_fwd_* does,
 *   the BatchNorm term is added last, one rounding on the store: the fp32 result equals pcs_devoxelize_fwd_f32 +
 *   pcs_bn_apply_f32 + an fp32 add bit for bit. No backward entry: the gradient of `out` is the dy of the BatchNorm
 *   backward passes and the gout of pcs_devoxelize_bwd_csr_*.
 *   c % 32 == 0 and 16-byte-aligned vox / lin / out, else PCS_EUNSUPPORTED; n == 0 is a no-op. _h: vox, lin, out in
 *   bf16 (dtype 1) or fp16 (dtype 2), any other dtype is PCS_EINVAL. */
int pcs_point_merge_f32(const float *vox, const int32_t *idx8, const float *w8, const float *lin, const double *stat,
                        const float *gamma, const float *beta, int64_t n, int32_t c, float *out, uint32_t *mask,
                        void *stream);
int pcs_point_merge_h(const void *vox, const int32_t *idx8, const float *w8, const void *lin, const double *stat,
                      const float *gamma, const float *beta, int64_t n, int32_t c, int32_t dtype, void *out,
                      uint32_t *mask, void *stream);
/* K9 merged with the range and point branches of RPVNet (additive, still ABI v12):
 *   R:pcseg/model/segmentor/fusion/rpvnet/rpvnet.py:648-651, 665-668, 683-686, 701-704
 *   `z_next.F = voxel_to_point(x, z).F + range_to_point(r, pxpy) + ReLU(BatchNorm(Linear(z.F)))`:
 *     out[i,j] = ( ( sum_{k<8, idx8[i,k] >= 0} w8[i,k] * vox[idx8[i,k], j] ) + sample(img[b_i, j], x_i, y_i) ) + third[i,j]
 *   vox (m, c), lin / out (n, c) in the row dtype; img (B, c, H, W) ALWAYS fp32; pxpy (n, 3) fp32 rows (frame, x, y) as
 *   pcs_range_sample_fwd_f32 takes them (bilinear, zero padding, align_corners = False; corners outside the image and frames
 *   that are no integer in [0, B) contribute 0); idx8 / w8 as pcs_point_merge_* takes them.
 *   bn mode  (stat != NULL; c % 32 == 0, mask != NULL): third = max(0, bn(lin)), and the ReLU bit mask is written with the
 *             layout and meaning of pcs_point_merge_* / pcs_bn_apply_* (bit = [bn rounded to the storage type > 0]).
 *   add mode (stat == NULL; gamma, beta, mask must be NULL, else PCS_EINVAL): third = lin, the finished term (widths that are
 *             no multiple of 32).
 *   All arithmetic in fp32 registers: the corners from zero in k = 0..7 order, the sample from zero in nw, ne, sw, se order,
 *   acc += sample, the third term last, one rounding on the store: the fp32 result equals pcs_devoxelize_fwd_f32,
 *   pcs_range_sample_fwd_f32, an fp32 add, pcs_bn_apply_f32 (relu), an fp32 add bit for bit. No backward entry: the gradient
 *   of `out` is the dy of the BatchNorm backward passes, the gout of pcs_devoxelize_bwd_csr_* and (in fp32) of
 *   pcs_range_sample_bwd_csr_f32.
 *   c % 4 == 0 (fp32) / c % 8 == 0 (16 bits), bn mode c % 32 == 0, 16-byte-aligned vox / lin / out, else PCS_EUNSUPPORTED with
 *   nothing launched; n == 0 is a no-op. _h: vox, lin, out in bf16 (dtype 1) or fp16 (dtype 2), any other dtype is PCS_EINVAL. */
int pcs_range_point_merge_f32(const float *vox, const int32_t *idx8, const float *w8, const float *img, const float *pxpy,
                              int32_t B, int32_t H, int32_t W, const float *lin, const double *stat, const float *gamma,
                              const float *beta, int64_t n, int32_t c, float *out, uint32_t *mask, void *stream);
int pcs_range_point_merge_h(const void *vox, const int32_t *idx8, const float *w8, const float *img, const float *pxpy,
                            int32_t B, int32_t H, int32_t W, const void *lin, const double *stat, const float *gamma,
                            const float *beta, int64_t n, int32_t c, int32_t dtype, void *out, uint32_t *mask, void *stream);

/* voxel_to_point map in one pass (R:pcseg/model/segmentor/voxel/minkunet/utils.py:69-105: floor, cat, kernel_hash
 * over the 8 cell corners, hashquery, calc_ti_weights, two transposes): coords (n, coord_ld >= 4) float = x,y,z,..,batch
 * in stride-1 voxel units, table = pcs_hashtable_build over the hashes of the level's voxel coordinates ->
 * idx8 (n,8) int32 (voxel row, -1 absent; corner order of get_kernel_offsets(2, stride)) and w8 (n,8) trilinear
 * weights, the layout pcs_devoxelize_fwd_f32 reads. */
int pcs_corner_map_f32(const float *coords, int32_t coord_ld, int64_t n, int32_t stride, const void *table,
                       int64_t capacity, int32_t *idx8, float *w8, void *stream);

/* K10 without atomics: the same sum as pcs_devoxelize_bwd_f32, as a per-voxel segmented
 * reduction. order (E,) int64 = flat positions i*8+k of the VALID (idx >= 0) entries of idx8,
 * sorted by voxel; rowptr (m+1,) int64 = start of each voxel's run in `order`. Every gfeat row
 * is written once, in `order` order (deterministic). The caller builds order/rowptr once per
 * idx8 (one sort) and reuses them for every backward through the same map. */
int pcs_devoxelize_bwd_csr_f32(const float *gout, const int64_t *order, const int64_t *rowptr,
                               const float *w8, int64_t m, int32_t c, float *gfeat, void *stream);
/* The same with 16-bit feature storage: gout / gfeat bf16 (dtype 1) or fp16 (dtype 2), any other dtype is PCS_EINVAL; w8 fp32.
 * fp32 accumulation in a fixed order (run-to-run identical), one rounding on the store, rows without entries written as zeros.
 * Narrow rows (at most 8 vectors of 8 or 4 halfs) on levels of at most 400 000 voxels take a wave-per-voxel form, everything
 * else one lane row per voxel. The atomic form pcs_devoxelize_bwd_f32 has no 16-bit twin. */
int pcs_devoxelize_bwd_csr_h(const void *gout, const int64_t *order, const int64_t *rowptr, const float *w8,
                             int64_t m, int32_t c, int32_t dtype, void *gfeat, void *stream);
/* Measurement switch (tools/pointvoxel_bench.py), not part of the contract: independent row loads in flight per lane in the
 * segmented lane-row kernels of pcs_voxelize_fwd_csr_h and pcs_devoxelize_bwd_csr_h: 2 or 4 forces that form, any other value
 * restores the default (4 on levels of at most 400 000 voxels, else 2). Same summation order, same bits. */
void pcs_debug_pointvoxel_h_inflight(int32_t loads);

/* calc_ti_weights  TS:torchsparse/nn/functional/devoxelize.py:10-48  (about 25 small torch
 * kernels in the reference, one kernel here). coords (n, coord_ld) fp32 (first 3 columns
 * used), idx_query (8,n) int64 (-1 = miss), -> w (8,n) fp32: trilinear corner weights in
 * get_kernel_offsets(2) order, /scale^3 when scale != 1, zeroed at misses, renormalised by
 * (sum + 1e-8). */
int pcs_ti_weights_f32(const float *coords, int32_t coord_ld, const int64_t *idx_query,
                       int64_t n, float scale, float *w, void *stream);

/* ------------------------------------------------------------------------------------------
 * spdownsample  TS:torchsparse/nn/functional/downsample.py:11-52
 * Step 1 (this call): candidate output coordinates as packed sortable 64-bit keys
 *   key = (batch << 54) | ((x + 2^17) << 36) | ((y + 2^17) << 18) | (z + 2^17)
 * whose ascending order equals the reference's lexicographic order over [b, x, y, z]
 * (downsample.py:49-51). mode 0 = fast branch (downsample.py:25-28): one key per input row,
 * coordinate truncated toward zero to a multiple of sample_stride[d]. mode 1 = general
 * branch (downsample.py:29-45): n*K keys for coords+offsets[k]; rows that fail
 * `% sample_stride == 0` or `>= coords_min` get the key INT64_MAX (sorts last).
 * Step 2: pcs_sort_unique_i64 (v11; or any ascending sort + unique of the caller's). Step 3: pcs_downsample_unpack.
 * *err (device int32, caller-zeroed) is set to 1 if a coordinate does not fit the packing
 * (|x|,|y|,|z| >= 2^17 or batch outside [0, 511]).
 * sample_stride3 is a HOST pointer (three small positive ints); offsets / coords_min3 are
 * device pointers.
 */
int pcs_downsample_pack(const int32_t *coords, int64_t n, const int32_t *sample_stride3,
                        int32_t mode, const int32_t *offsets, int32_t K,
                        const int32_t *coords_min3, int64_t *keys, int32_t *err, void *stream);
int pcs_downsample_unpack(const int64_t *keys, int64_t m, int32_t *coords, void *stream);
/* Step 2 of spdownsample [v11]: out[0 .. m) = the distinct keys in ascending (signed) order -- what the reference's
 * `torch.unique(coords, dim=0)` (downsample.py:47-51) yields on the packed rows. info (device int64[3]) receives everything the
 * host has to read back in one record: info[0] = m, info[1] = the largest key (INT64_MIN when m = 0; INT64_MAX = the general
 * branch's "rejected candidate" sentinel is present and is the last key), info[2] = *err_flag (0 when err_flag is NULL).
 * out holds n keys; ws / ws_bytes from pcs_sort_unique_ws_bytes(n) (never allocates; PCS_EWORKSPACE when too small). */
size_t pcs_sort_unique_ws_bytes(int64_t n);
int pcs_sort_unique_i64(const int64_t *keys, int64_t n, int64_t *out, int64_t *info, const int32_t *err_flag, void *ws,
                        size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Rulebook (kernel map)  TS:torchsparse/nn/functional/conv.py:156-176
 * For every kernel offset k and every query row j (ascending): look up
 * hash(qcoords[j,:3] + offsets[k], qcoords[j,3]) in the table built over hash(ref coords).
 * The reference materialises a (K,N) int64 hash matrix, a (K,N) int64 result matrix, then
 * sum + nonzero. Here the hash is computed in registers and probed immediately:
 *   pass 1  pcs_rulebook_probe : results (K,nq) int32 (ref row or -1) + per-k hit counts
 *   pass 2  pcs_rulebook_fill  : pairs (P,2) int32 = (ref_row, query_row), ordered k-major
 *           then query_row ascending -- exactly the reference's nbmaps order
 *           (conv.py:169-172) -- and koff (K+1) int32 prefix offsets of each k's slice.
 * The same two calls with (query = input coords, ref = output coords, negated offsets)
 * give the input-sorted map used by dgrad / transposed convs.
 * nbsizes (K,) int64 mirrors the reference's `nbsizes` (conv.py:168).
 */
size_t pcs_rulebook_ws_bytes(int64_t nq, int32_t K);
int pcs_rulebook_probe(const int32_t *qcoords, int64_t nq, const int32_t *offsets, int32_t K,
                       const void *table, int64_t capacity, int32_t *results,
                       int64_t *nbsizes, void *ws, size_t ws_bytes, int32_t symmetric, void *stream);
/* symmetric != 0: the caller guarantees a submanifold map -- qcoords are the rows the table was built over, K is odd
 * and offsets[K-1-k] == -offsets[k]. Only the first K/2 offsets are probed; a hit (j + offsets[k] -> i) is also
 * recorded as (i + offsets[K-1-k] -> j) and the centre offset is the identity. Same results, half the probes. */
int pcs_rulebook_fill(const int32_t *results, int64_t nq, int32_t K, const void *ws,
                      int32_t *pairs, int32_t *koff, void *stream);
/* Per (k, tile) segment table for the output-stationary convolution: for tile t of
 * `tile_rows` consecutive destination rows, seg[k*(ntiles+1)+t] is the first pair of offset
 * k (absolute index into pairs) whose destination row >= t*tile_rows.
 * dst_col selects the column of `pairs` that holds the destination row (must be the sorted
 * one, i.e. 1 for maps produced by pcs_rulebook_fill). */
int pcs_rulebook_tile_segments(const int32_t *pairs, const int32_t *koff, int32_t K,
                               int64_t n_dst, int32_t tile_rows, int32_t dst_col,
                               int32_t *seg, void *stream);
/* Heaviest-first order of the row tiles of a segment table (work of a tile = its 16-row MFMA blocks over all
 * offsets): order[i] = the tile the i-th workgroup slot of the fused convolution runs. Workgroups are dispatched in
 * index order, so the light tiles run last and the launch drains evenly (+4..8 % on the deep levels). The order among
 * equally heavy tiles is unspecified; results never depend on the order. */
int pcs_rulebook_tile_order(const int32_t *seg, int32_t K, int64_t ntiles, int32_t *order, void *stream);

/* ------------------------------------------------------------------------------------------
 * F1  convolution_forward_cuda   TS:torchsparse/backend/convolution/convolution_cuda.cu:53-165
 * F2  convolution_backward_cuda  TS:torchsparse/backend/convolution/convolution_cuda.cu:167-278
 * (gather_kernel :14-24, scatter_kernel :27-37, torch::mm_out per offset :149, :259-263)
 *
 * pcs_conv_gather_gemm_f32: output-stationary fused gather-GEMM-accumulate
 *      dst[d, :] = sum over pairs (s, d) of offset k:  src[s, :] @ W[k]      (+ bias)
 * One workgroup owns `tile_rows` consecutive dst rows x a column tile, walks the kernel
 * offsets, gathers the needed src rows into LDS, contracts with W[k] on the fp32 MFMA pipe
 * and accumulates in LDS; every dst row is written exactly once (no atomics, no zero fill
 * needed, deterministic). Used for forward (src = input feats), for dgrad (src = grad_out,
 * W = per-offset transposed weights, input-sorted map) and for transposed convolutions.
 *   src (n_src, cin), W (K, cin, cout), dst (n_dst, cout); pairs (P,2) with the src row in
 *   column src_col and the dst row in column 1-src_col, sorted k-major / dst ascending;
 *   seg from pcs_rulebook_tile_segments with the same tile_rows; bias (cout) or NULL.
 *   tile_rows: a multiple of 16 in [16, 512]; shapes outside the wave kernels (cin % 4 == 0, cin >= 32, cout % 4 == 0,
 *   an even number of 16-column tiles, K <= 32 -- cin % 32 == 0 on the straight-line instance, other widths such as
 *   56 / 112 / 168 / 336 of RPVNet cr 1.75 on the TAIL instance) take 64 or 128 only (PCS_EUNSUPPORTED otherwise).
 * pcs_conv_tile_rows returns the default tile height for (cin, cout); pcs_conv_pick_tile_rows the
 * height for one layer call: with few dst rows (deep strides) the launch is only a few waves of
 * workgroups over the CUs, and the height is chosen so that the last wave is full.
 */
const char *pcs_conv_kernel_revision(void); /* identifies the fused-conv kernels a measurement file was taken on */
int32_t pcs_conv_tile_rows(int32_t cin, int32_t cout);
int32_t pcs_conv_pick_tile_rows(int64_t n_dst, int64_t n_pairs, int32_t K, int32_t cin, int32_t cout);
int32_t pcs_conv_pick_tile_rows_dt(int64_t n_dst, int64_t n_pairs, int32_t K, int32_t cin, int32_t cout,
                                   int32_t dtype); /* dtype 0: fp32 kernels (= the call above), 1 / 2: half kernels */
/* *   bn_partial (may be NULL): [ceil(n_dst / tile_rows)][2][cout] doubles. When given, the write-back also leaves, per
 *   tile and column, sum(x) and sum(x^2) of the rows it stored: the statistics pass of the BatchNorm that follows
 *   the convolution (R:pcseg/model/segmentor/voxel/minkunet/minkunet.py:31-129) costs no extra read of the tensor;
 *   pcs_bn_reduce_partials turns them into the `sums` vector of pcs_bn_finalize_f32. Only for shapes / tile heights
 *   with pcs_conv_emits_bn_partials(...) != 0 (PCS_EUNSUPPORTED otherwise).
 *   tile_order (may be NULL): ceil(n_dst / tile_rows) int32 from pcs_rulebook_tile_order for the same seg; NULL =
 *   tiles in row order (XCD-contiguous ranges). Only the wave kernels (16-byte-granular shapes from 32 input channels
 *   up; every shape of the half kernels) use it.
 */
int32_t pcs_conv_emits_bn_partials(int32_t cin, int32_t cout, int32_t K, int32_t tile_rows, int32_t dtype);
int32_t pcs_conv_uses_tile_order(int32_t cin, int32_t cout, int32_t K, int32_t dtype); /* 1: the shape's kernel reads tile_order */
int pcs_conv_gather_gemm_f32(const float *src, int64_t n_src, int32_t cin, const float *W,
                             int32_t K, int32_t cout, const int32_t *pairs, int32_t src_col,
                             const int32_t *seg, int32_t tile_rows, int64_t n_dst,
                             const float *bias, float *dst, double *bn_partial, const int32_t *tile_order,
                             void *stream);
/* Write-back extras of the fused convolution (all optional; the plain entry = all NULL). Used by the backward pass:
 *   addend : (n_dst, cout) in dst's dtype, added to every output row (dst = conv + bias + addend, in fp32 before any rounding).
 *            dgrad of a convolution whose input also feeds a residual / skip path
 *            (R:pcseg/model/segmentor/voxel/minkunet/minkunet.py:88-129 `relu(net(x) + downsample(x))`): the gradient the skip path
 *            hands back rides in, instead of a separate elementwise sum of the two gradients (what autograd does around
 *            TS:torchsparse/backend/convolution/convolution_cuda.cu:167-278).
 * Shapes the wave kernels do not serve (pcs_conv_supports_epilogue() == 0) return PCS_EUNSUPPORTED when any extra is set.
 * ABI v12: the struct no longer carries the BatchNorm backward-statistics inputs between addend and act_slope.
 * Still v12 (additive): the former `reserved` word is `flags`, same offset and size; a zero-initialised struct means
 * what it meant. Order of the write-back: bias, then addend, then the activation.
 * Still v12 (additive): PCS_EP_POST_AFFINE and the trailing fields post_scale / post_shift. The kernels read the two fields
 * ONLY when the flag is set, so a caller built against the shorter struct (which cannot set bit 16: it was PCS_EINVAL) and a
 * zeroed struct mean what they meant. With the flag the order of the write-back is
 *     v = conv + bias;  v = act(v);  v = v * post_scale[c] + post_shift[c] (fp32);  v = v + addend;  store
 * -- inference of conv -> LeakyReLU -> BatchNorm (+ residual) (R:pcseg/model/segmentor/voxel/cylinder3d/cylinder_ts.py:88-334)
 * with the BatchNorm's running statistics as the affine map: gamma may be negative, so the map does not commute with the
 * activation into the weights. The half kernels round once, on the store. Not together with bn_partial (PCS_EINVAL: statistics
 * of an affine-mapped tensor have no consumer); a null or not 16-byte-aligned post_scale / post_shift is PCS_EINVAL; shapes
 * with pcs_conv_supports_epilogue() == 0 return PCS_EUNSUPPORTED as for the other extras. The bf16x3 entry takes no epilogue. */
#define PCS_EP_RELU 1   /* flags: the activation is ReLU, whatever act_slope holds */
#define PCS_EP_POST_AFFINE 16   /* flags: post_scale / post_shift are read and applied behind the activation, the addend behind them */
typedef struct pcs_conv_epilogue {
  const void *addend;
  float act_slope;   /* LeakyReLU fused into the write-back: dst = v < 0 ? v * act_slope : v, applied before the store and before the
                      * forward BatchNorm statistics (R:pcseg/model/segmentor/voxel/cylinder3d/cylinder_ts.py:88-190: conv -> LeakyReLU
                      * -> BatchNorm1d). 0 is read as 1 (no activation), so a zero-initialised struct is the plain call. */
  int32_t flags;     /* PCS_EP_RELU | PCS_EP_POST_AFFINE; any other bit (2, 4, 8, 32 ...) is PCS_EINVAL. PCS_EP_RELU: the kernels run their LeakyReLU branch with slope
                      * 0 (inference with BatchNorm folded into the weights: conv + bias + residual + ReLU in one launch). A negative
                      * pre-activation therefore gives a zero of either sign (v * 0 = -0.0), and non-finite pre-activations are not
                      * flushed (-inf * 0 = NaN); -0.0 == 0 in every comparison a consumer makes. */
  const float *post_scale;   /* fp32 (cout), 16-byte aligned; read only with PCS_EP_POST_AFFINE */
  const float *post_shift;   /* fp32 (cout), 16-byte aligned; read only with PCS_EP_POST_AFFINE */
} pcs_conv_epilogue;
int pcs_conv_gather_gemm_f32_ex(const float *src, int64_t n_src, int32_t cin, const float *W,
                                int32_t K, int32_t cout, const int32_t *pairs, int32_t src_col,
                                const int32_t *seg, int32_t tile_rows, int64_t n_dst,
                                const float *bias, const pcs_conv_epilogue *ep, float *dst, double *bn_partial,
                                const int32_t *tile_order, void *stream);
int32_t pcs_conv_supports_epilogue(int32_t cin, int32_t cout, int32_t K, int32_t dtype);   /* dtype 0 fp32, 1 / 2 half kernels */

/* dst[k][b][a] = src[k][a][b]: the per-offset transposed weights dgrad contracts with (the reference transposes
 * inside torch::mm_out per offset, convolution_cuda.cu:259-263). */
int pcs_transpose_kab_f32(const float *src, int32_t K, int32_t A, int32_t B, float *dst, void *stream);

/* wgrad:  gW[k] = sum over pairs (a, b) of offset k:  fa[a, :]^T (outer) fb[b, :]
 *   fa (na, ca) rows indexed by pairs column a_col, fb (nb, cb) by the other column;
 *   gW (K, ca, cb). Deterministic two-pass split reduction; ws from pcs_conv_wgrad_ws_bytes.
 *   koff_dev / koff_host: the K+1 prefix offsets of each offset's slice of `pairs`, on the
 *   device (read by the kernels) and on the HOST (the caller has them from the rulebook
 *   build; they size the launch and the workspace). */
size_t pcs_conv_wgrad_ws_bytes(const int32_t *koff_host, int32_t K, int32_t ca, int32_t cb);
int pcs_conv_wgrad_f32(const float *fa, int32_t ca, const float *fb, int32_t cb,
                       const int32_t *pairs, int32_t a_col, const int32_t *koff_dev,
                       const int32_t *koff_host, int32_t K, float *gW, void *ws,
                       size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Cylindrical scatter: torch_scatter.scatter_max(src, index, dim=0) as called by the reference's
 * cylinder front-end (R:tools/utils/common/seg_utils.py:178,
 * R:pcseg/model/segmentor/voxel/cylinder3d/cylinder_ts.py:35). torch_scatter is a third-party,
 * version-unpinned dependency that is not under /root/reference: PARITY UNPINNED (semantics
 * restated: per-voxel channel-wise max, argmax saved for backward, empty voxel -> 0 / -1).
 * Segmented form: order (E,) int64 = point ids sorted by voxel, rowptr (m+1,) int64.
 * (scatter_mean of the same front-end is pcs_voxelize_fwd_f32 with the voxel counts.)
 */
int pcs_scatter_max_fwd_f32(const float *src, const int64_t *order, const int64_t *rowptr, int64_t m,
                            int32_t c, float *out, int32_t *arg, void *stream);
/* gsrc (n,c) is zeroed inside, then gsrc[arg[v,j], j] = gout[v,j]. arg is int32 (point rows < 2^31): as int64 it
 * would be half of the forward kernel's HBM traffic; the Python layer widens it only if the caller reads it. */
int pcs_scatter_max_bwd_f32(const float *gout, const int32_t *arg, int64_t m, int64_t n, int32_t c,
                            float *gsrc, void *stream);

/* K13  map_count_forward   RL:range_utils/src/map_count_gpu.cu:5-14 (RL = R:pcseg/model/segmentor/
 *      fusion/rpvnet/range_lib/): out[b,py,px] += 1 for pxpy rows (b,px,py) inside the image
 *      (the reference checks only px,py >= 0); out (B,H,W) int32 zeroed inside.
 * K14  denselize_forward   RL:range_utils/src/denselize_gpu.cu:5-19: out[b,j,py,px] += feat[i,j] /
 *      count[b,py,px]; out (B,C,H,W) fp32 zeroed inside.
 * K15  denselize_backward  RL:range_utils/src/denselize_gpu.cu:21-34: gfeat[i,j] = gout[b,j,py,px] /
 *      count (0 where the reference would divide by zero / read out of bounds). */
int pcs_map_count(const int32_t *pxpy, int64_t n, int32_t B, int32_t H, int32_t W, int32_t *out,
                  void *stream);
int pcs_denselize_fwd_f32(const float *feat, const int32_t *count_map, const int32_t *pxpy, int64_t n,
                          int32_t B, int32_t C, int32_t H, int32_t W, float *out, void *stream);
/* contention-free forms (C % 4 == 0): order int64 = point rows sorted by pixel ((b*H + py)*W + px; out-of-range
 * points first), rowptr (B*H*W + 1) int64. forward: every out element written once (no memset), NCHW stores in full
 * lines, deterministic. backward: gout read in full lines, one 16-byte-vector row store per point (gfeat zeroed inside). */
int pcs_denselize_fwd_csr_f32(const float *feat, const int64_t *order, const int64_t *rowptr,
                              const int32_t *count_map, int32_t B, int32_t C, int32_t H, int32_t W,
                              float *out, void *stream);
int pcs_denselize_bwd_csr_f32(const float *gout, const int64_t *order, const int64_t *rowptr,
                              const int32_t *count_map, int64_t n, int32_t B, int32_t C, int32_t H, int32_t W,
                              float *gfeat, void *stream);
int pcs_denselize_bwd_f32(const float *gout, const int32_t *count_map, const int32_t *pxpy, int64_t n,
                          int32_t B, int32_t C, int32_t H, int32_t W, float *gfeat, void *stream);

/* ---- range image -> points (ABI v8) --------------------------------------------------------------------------------------
 * Replaces R:pcseg/model/segmentor/fusion/rpvnet/rpvnet.py:31-51 (`resample_grid_stacked` / `range_to_point`: a python loop over
 * frames around torch.nn.functional.grid_sample(mode='bilinear', padding_mode='zeros', align_corners=False)) for all frames in
 * one launch, and its backward (torch's grid_sampler_2d_backward: per-point channel loops of float atomics into NCHW planes,
 * 25 % of an RPVNet step) by an atomic-free segmented pass.
 *   img  (B, C, H, W) fp32;  pxpy (n, 3) fp32 rows (frame, x, y), x / y in [-1, 1];  out (n, C): out[p] = bilinear sample of
 *   frame pxpy[p][0] at ix = ((x + 1) W - 1) / 2, iy = ((y + 1) H - 1) / 2; corners outside the image contribute 0; a row whose
 *   frame is not an integer in [0, B) gives zeros. C % 4 == 0 (16-byte row pieces), else PCS_EUNSUPPORTED.
 *   backward: pcs_range_sample_corners writes, per point and corner (nw, ne, sw, se), the pixel key (b H + y) W + x (or -1) and the
 *   bilinear weight: keys / wts of 4 n entries. The caller sorts the keys (stable) into a CSR over the B H W pixels -- order
 *   (4 n entry ids, the -1 keys first) and rowptr (B H W + 1), once per pxpy and resolution -- and pcs_range_sample_bwd_csr_f32
 *   writes EVERY element of gimg (B, C, H, W): gimg[b, c, y, x] = sum over the pixel's entries of wts[e] * gout[e / 4, c], in
 *   ascending entry order (deterministic); no memset needed. */
int pcs_range_sample_fwd_f32(const float *img, const float *pxpy, int64_t n, int32_t B, int32_t C, int32_t H, int32_t W,
                             float *out, void *stream);
int pcs_range_sample_corners(const float *pxpy, int64_t n, int32_t B, int32_t H, int32_t W, int64_t *keys, float *wts,
                             void *stream);
int pcs_range_sample_bwd_csr_f32(const float *gout, const int64_t *order, const int64_t *rowptr, const float *wts,
                                 int32_t B, int32_t C, int32_t H, int32_t W, float *gimg, void *stream);

/* ------------------------------------------------------------------------------------------
 * Block fusion above the op boundary: training-mode BatchNorm over (N,C)
 * voxel features fused with the residual add and the ReLU that follow it in the reference's
 * blocks (R:pcseg/model/segmentor/voxel/minkunet/minkunet.py:31-129: Conv3d -> (Sync)BatchNorm
 * -> ReLU, and relu(net(x) + downsample(x))). Statistics are two-level and fixed-order
 * (deterministic); `sums` (2c + 1 doubles: sum x | sum x^2 | row count n) is the vector a data-parallel
 * run all-reduces between the stats and the finalize call -- SyncBatchNorm semantics; the global count
 * then reaches finalize / bwd_apply as the DEVICE pointer `count_dev` (= sums + 2c; overrides the host
 * `count` when non-NULL), so no rank ever reads it back --, `sums2` (sum g | sum g*xhat) the one it
 * all-reduces in backward. The forward partial sums are taken about a pivot row and un-shifted in
 * double (E[x^2] - mean^2 on raw fp32 sums cancels when |mean| >> std).
 *   forward : pcs_bn_stats_f32 -> [all-reduce sums, count] -> pcs_bn_finalize_f32 (stat = mean | invstd,
 *             running stats updated with the unbiased variance like nn.BatchNorm1d)
 *             -> pcs_bn_apply_f32: y = act((x - mean) * invstd * w + b [+ res])
 *   backward: pcs_bn_bwd_stats_f32 (g = dy * [y > 0] when relu) -> [all-reduce sums2]
 *             -> pcs_bn_bwd_apply_f32: dx = (g - sum_g/N - xhat * sum_gxhat/N) * invstd * w, dres = g
 *             (dw = sums2[c:], db = sums2[:c]). ABI v7: `sums2` holds 2c doubles FOLLOWED BY the same 2c values as floats
 *             (3c doubles of storage): the parameter gradients in the parameters' dtype without a conversion launch.
 *             ABI v8: the caller states the size of `sums2` in doubles (`sums2_doubles` >= 3c, else PCS_EWORKSPACE) -- a v6 caller's
 *             2c-double buffer fails loudly instead of being overrun. (v8 also drops pcs_conv_ring_enable / pcs_conv_ring_applies:
 *             the experimental ring kernels left the product library.)
 *   single process, statistics from the convolution's write-back: pcs_bn_reduce_partials_finalize = pcs_bn_reduce_partials +
 *             pcs_bn_finalize_f32 (count = n) in one launch (ABI v7; `sums` may be NULL there).
 * partial_ws: pcs_bn_num_partials() * 2 * c floats.
 * mask (optional, c % 32 == 0): n * c/32 words written by the apply pass, bit = [y > 0] of y AS STORED (in fp16 a
 *   pre-activation in (0, 2^-25] stores as 0 and its bit is clear: the mask and the y form of backward always agree, so
 *   a layer's gradient does not depend on whether its width is a multiple of 32); handed to the two backward
 *   passes instead of y (then y may be NULL) -- the ReLU gate costs 1/32 of a tensor read instead of a whole one.
 * n == 0 (an empty tensor; under SyncBN a rank without rows still takes part in the all-reduce): every entry that
 *   takes n returns PCS_OK and the tensor pointers may be NULL -- the stats entries leave sums = 0 with count 0
 *   (sums2 = 0); pcs_bn_reduce_partials(_finalize) accept nrows == 0 with a NULL `partial` (zero sums) and _finalize
 *   reads n == 0 as count 1; the apply entries launch nothing, and pcs_bn_bwd_apply_* return before they look at
 *   `count`. With n > 0 a NULL tensor is PCS_EINVAL, and so is a host `count` that is not positive without a count_dev.
 *   pcs_bn_finalize_f32 takes no n: it wants a positive host `count` or a count_dev, and reads a DEVICE count of 0 as 1.
 */
int32_t pcs_bn_num_partials(void);
int pcs_bn_stats_f32(const float *x, int64_t n, int32_t c, float *partial_ws, double *sums, void *stream);
int pcs_bn_reduce_partials(const double *partial, int64_t nrows, int32_t c, int64_t n, double *sums, void *stream);
int pcs_bn_reduce_partials_finalize(const double *partial, int64_t nrows, int32_t c, int64_t n, double eps, double momentum,
                                    float *running_mean, float *running_var, double *sums, double *stat, void *stream);
int pcs_bn_finalize_f32(const double *sums, double count, const double *count_dev, int32_t c, double eps,
                        double momentum, float *running_mean, float *running_var, double *stat, void *stream);
/* concat fusion (torchsparse.cat([bn_relu(up_conv(x)), skip]), TS:torchsparse/operators.py:10-17 as used by
 * R:pcseg/model/segmentor/voxel/minkunet/minkunet.py:404-416): apply may write y as the left c columns of an (n, ldy)
 * buffer (ldy = row stride in elements, 0 = c) and copy the skip tensor `tail` (n, ctail; may be NULL / 0) into the
 * columns right of it in the same launch; the backward passes then read dy with the row stride lddy (0 = c) straight
 * out of the gradient of that buffer. */
int pcs_bn_apply_f32(const float *x, const float *res, const double *stat, const float *w, const float *b,
                     int64_t n, int32_t c, int32_t relu, float *y, uint32_t *mask, int64_t ldy, const float *tail,
                     int32_t ctail, void *stream);
int pcs_bn_bwd_stats_f32(const float *dy, const float *x, const float *y, const uint32_t *mask, const double *stat,
                         int64_t n, int32_t c, int32_t relu, float *partial_ws, double *sums2, int64_t sums2_doubles,
                         int64_t lddy, void *stream);
int pcs_bn_bwd_apply_f32(const float *dy, const float *x, const float *y, const uint32_t *mask, const double *stat,
                         const double *sums2, double count, const double *count_dev, const float *w, int64_t n,
                         int32_t c, int32_t relu, float *dx, float *dres, int64_t lddy, void *stream);
/* the same four passes over bf16 (dtype 1) / fp16 (dtype 2) feature tensors (x, res, y, dy, dx, dres all in `dtype`):
 * the mixed-precision pipeline of the reference (`--amp`), where the convolutions hand on halfs. Statistics,
 * scale / shift and the arithmetic stay fp32 / double; rows need 8-byte alignment for the vector path. */
int pcs_bn_stats_h(const void *x, int64_t n, int32_t c, int32_t dtype, float *partial_ws, double *sums, void *stream);
int pcs_bn_apply_h(const void *x, const void *res, const double *stat, const float *w, const float *b, int64_t n,
                   int32_t c, int32_t relu, int32_t dtype, void *y, uint32_t *mask, int64_t ldy, const void *tail,
                   int32_t ctail, void *stream);
int pcs_bn_bwd_stats_h(const void *dy, const void *x, const void *y, const uint32_t *mask, const double *stat, int64_t n,
                       int32_t c, int32_t relu, int32_t dtype, float *partial_ws, double *sums2, int64_t sums2_doubles,
                       int64_t lddy, void *stream);
int pcs_bn_bwd_apply_h(const void *dy, const void *x, const void *y, const uint32_t *mask, const double *stat,
                       const double *sums2, double count, const double *count_dev, const float *w, int64_t n,
                       int32_t c, int32_t relu, int32_t dtype, void *dx, void *dres, int64_t lddy, void *stream);
/* pcs_bn_bwd_apply_{f32,h} (dtype 0 / 1 / 2) for a BatchNorm whose INPUT is a LeakyReLU output (conv -> LeakyReLU -> BatchNorm1d,
 * R:pcseg/model/segmentor/voxel/cylinder3d/cylinder_ts.py:88-190): dx leaves multiplied by (x > 0 ? 1 : in_slope), i.e. as the
 * gradient of the activation's input -- torch's leaky_relu_backward pass disappears. */
int pcs_bn_bwd_apply_act(const void *dy, const void *x, const void *y, const uint32_t *mask, const double *stat,
                         const double *sums2, double count, const double *count_dev, const float *w, int64_t n, int32_t c,
                         int32_t relu, int32_t dtype, float in_slope, void *dx, void *dres, int64_t lddy, void *stream);

/* ---- ReconBlock (DDCM) gate of Cylinder3D (additive, still ABI v12) -----------------------------
 *   R:pcseg/model/segmentor/voxel/cylinder3d/cylinder_ts.py:337-384
 *   `out = x * (sigmoid(bn0(conv3x1x1(x))) + sigmoid(bn0_2(conv1x3x1(x))) + sigmoid(bn0_3(conv1x1x3(x))))` with the three conv
 *   outputs a0, a1, a2 (n, c) given. stat3 = 3 x (mean | invstd) (3 x 2c doubles, branch after branch), gamma3 / beta3 =
 *   3 x c floats or NULL; bn_k(a) = fma(a, sc, sh) by the expression of pcs_bn_apply_*, xhat_k = (a - mean_k) * invstd_k.
 *     pcs_recon_gate_*:           out = x * ((s0 + s1) + s2), s_k = 1 / (1 + expf(-bn_k(a_k))); fp32 registers, one rounding
 *                                 on the store, the gates are never written.
 *     pcs_recon_gate_bwd_stats_*: with g_k = dy * x * s_k * (1 - s_k): sums2 = 3 x [sum g_k (c) | sum g_k * xhat_k (c)] as
 *                                 6c doubles FOLLOWED BY the same 6c values as floats (9c doubles of storage, the sums2
 *                                 convention of ABI v7; `sums2_doubles` < 9c is PCS_EWORKSPACE). Two-level, fixed order:
 *                                 bit-identical from run to run. partial_ws: pcs_bn_num_partials() * 6c floats. The 6c doubles
 *                                 are what a data-parallel run all-reduces: one collective for the whole block.
 *     pcs_recon_gate_bwd_apply_*: dx_gate = dy * ((s0 + s1) + s2) (the gradient of x through the product only) and
 *                                 da_k = (g_k - sum_g_k / N - xhat_k * sum_gxhat_k / N) * invstd_k * gamma_k; the sigmoids are
 *                                 recomputed from a_k. count / count_dev as pcs_bn_bwd_apply_* take them.
 *   (dgamma_k = sums2[(2k + 1)c ..], dbeta_k = sums2[2kc ..].) No atomics; every output element is written exactly once.
 *   fp32: c % 4 == 0; _h (all tensors bf16, dtype 1, or fp16, dtype 2; any other dtype is PCS_EINVAL): c % 8 == 0; every row
 *   pointer 16-byte aligned; anything else is PCS_EUNSUPPORTED with nothing launched. n == 0 is a no-op that returns PCS_OK
 *   before any pointer is looked at (nothing is written, sums2 included); a NULL tensor with n > 0 is PCS_EINVAL. */
int pcs_recon_gate_f32(const float *a0, const float *a1, const float *a2, const float *x, const double *stat3,
                       const float *gamma3, const float *beta3, int64_t n, int32_t c, float *out, void *stream);
int pcs_recon_gate_h(const void *a0, const void *a1, const void *a2, const void *x, const double *stat3, const float *gamma3,
                     const float *beta3, int64_t n, int32_t c, int32_t dtype, void *out, void *stream);
int pcs_recon_gate_bwd_stats_f32(const float *dy, const float *x, const float *a0, const float *a1, const float *a2,
                                 const double *stat3, const float *gamma3, const float *beta3, int64_t n, int32_t c,
                                 float *partial_ws, double *sums2, int64_t sums2_doubles, void *stream);
int pcs_recon_gate_bwd_stats_h(const void *dy, const void *x, const void *a0, const void *a1, const void *a2,
                               const double *stat3, const float *gamma3, const float *beta3, int64_t n, int32_t c,
                               int32_t dtype, float *partial_ws, double *sums2, int64_t sums2_doubles, void *stream);
int pcs_recon_gate_bwd_apply_f32(const float *dy, const float *x, const float *a0, const float *a1, const float *a2,
                                 const double *stat3, const float *gamma3, const float *beta3, const double *sums2,
                                 double count, const double *count_dev, int64_t n, int32_t c, float *dx_gate, float *da0,
                                 float *da1, float *da2, void *stream);
int pcs_recon_gate_bwd_apply_h(const void *dy, const void *x, const void *a0, const void *a1, const void *a2,
                               const double *stat3, const float *gamma3, const float *beta3, const double *sums2, double count,
                               const double *count_dev, int64_t n, int32_t c, int32_t dtype, void *dx_gate, void *da0,
                               void *da1, void *da2, void *stream);

/* ---- device-side sparse_quantize ---------------------------------------------------------------
 * Replaces the dataloader-side NumPy voxel dedup TS:torchsparse/utils/quantize.py:9-46
 * (ravel_hash :9-21, sparse_quantize :24-46; called from R:pcseg/data/dataset/semantickitti/
 * semantickitti_voxel.py:112-120) for scans that are already resident in HBM. Contract: voxel =
 * floor(point / voxel_size) evaluated in double like NumPy does, one representative row per voxel =
 * its FIRST occurrence, voxels ordered by ascending ravel hash (row-major index inside the bounding box).
 *   floor: points (n, row_stride >= 3) float32 (is_float = 1), float64 (2) or int32 (0); voxel_size3 = 3 HOST doubles;
 *          coords (n,3) int32 out; bbox = 6 DEVICE int32 {min xyz, max xyz}, preset by the caller to
 *          {INT32_MAX x3, INT32_MIN x3}.
 *   keys:  keys[i] = ((x - xmin) * ey + (y - ymin)) * ez + (z - zmin), int64.
 *   the caller sorts (keys, row) STABLY, then  flags: 1 at the head of every run of equal keys;
 *   the caller scans the flags inclusively (rank), then
 *   emit:  vox (m,3) int32, index (m) int64 = representative row (may be NULL), inverse (n) int64 = voxel of
 *          every row (may be NULL); m = rank[n-1].
 */
int pcs_quantize_floor(const void *points, int32_t is_float, int64_t n, int32_t row_stride,
                       const double *voxel_size3, int32_t *coords, int32_t *bbox, void *stream);
int pcs_quantize_keys(const int32_t *coords, int64_t n, const int32_t *bbox, int64_t *keys, void *stream);
/* The same for a whole collated batch (TS:torchsparse/utils/quantize.py:15-21 per frame + TS:torchsparse/utils/collate.py:11-32):
 * key = ((frame * ex + x - x0) * ey + y - y0) * ez + z - z0 over the BATCH's bounding box bbox = {x0, y0, z0, x1, y1, z1} (device,
 * int32[6]); frames int64 per row. Ascending key = frames in order, inside a frame the reference's ravel-hash order. */
int pcs_quantize_frame_keys(const int32_t *coords, const int64_t *frames, int64_t n, const int32_t *bbox, int64_t *keys, void *stream);
int pcs_quantize_flags(const int64_t *sorted_keys, int64_t n, int32_t *flags, void *stream);
int pcs_quantize_emit(const int32_t *flags, const int64_t *rank, const int64_t *perm, const int32_t *coords,
                      int64_t n, int32_t *vox, int64_t *index, int64_t *inverse, void *stream);

/* ---- device-side dataset transform: augmentation, test-time-augmentation votes, voxel coordinates ----
 * Replaces, for scans resident in HBM, the per-scan NumPy transform of the dataloader workers:
 *   aug_points             R:tools/utils/common/seg_utils.py:43-100 (rotate :56-69, scale :72-75, flip :78-89, jitter :92-98)
 *   get_single_sample      R:pcseg/data/dataset/semantickitti/semantickitti_voxel.py:83-114 (augmented xyz stored as float32 = the
 *                          feature rows; pc_ = round(xyz / voxel_size) as int32; pc_ -= pc_.min(0))
 *   the ten votes of TTA   R:pcseg/data/dataset/semantickitti/semantickitti_voxel.py:62-69
 * transform: points (n, c) fp32 contiguous, 3 <= c <= PCS_SCAN_MAX_COLUMNS, the frames one after the other; frame_offsets
 *   (num_frames + 1) int64 on the device = first row of every frame and n; params (num_votes * num_frames, 8) float64 on the
 *   device, vote-major: row v * num_frames + f = {cos, sin, scale, sx, sy, jx, jy, jz} of vote v of frame f; 1 <= num_votes <=
 *   PCS_SCAN_MAX_VOTES. Per row i of frame f and vote v, in float64 and in this order, no multiply-add fused:
 *     X = x * cos + y * (-sin), Y = x * sin + y * cos, Z = z;  X, Y, Z *= scale;  X *= sx, Y *= sy;  X, Y, Z += jx, jy, jz
 *   feats (num_votes * n, c) fp32: row v * n + i = {float(X), float(Y), float(Z), the other columns unchanged};
 *   coords (num_votes * n, 3) int32: rintf(feats / voxel_size), an IEEE float32 division, ties to even;
 *   mins (num_votes * num_frames, 3) int32: the minimum of coords over the rows of (v, f), written by the call whatever it held
 *   (INT32_MAX for an empty frame); ws: caller scratch of at least the ws_bytes query's size for the same n, num_frames and
 *   num_votes (else PCS_EWORKSPACE), 4-byte aligned, contents irrelevant on entry.
 * shift: coords[v * n + i] -= mins[v * num_frames + frame of i] in place; frames (num_votes * n) int64 = v * num_frames + frame
 *   of i, the scene vector the batch dedup of pcs_quantize_frame_keys takes.
 * Offsets outside [0, n] are clamped: no row outside the arrays is addressed. */
#define PCS_SCAN_MAX_VOTES 16
#define PCS_SCAN_MAX_COLUMNS 8
int64_t pcs_scan_transform_ws_bytes(int64_t n, int32_t num_frames, int32_t num_votes);
int pcs_scan_transform(const float *points, int64_t n, int32_t c, const int64_t *frame_offsets, int32_t num_frames,
                       const double *params, int32_t num_votes, float voxel_size, float *feats, int32_t *coords,
                       int32_t *mins, void *ws, int64_t ws_bytes, void *stream);
int pcs_scan_shift(int32_t *coords, int64_t n, const int64_t *frame_offsets, int32_t num_frames, const int32_t *mins,
                   int32_t num_votes, int64_t *frames, void *stream);

/* Unique keys + inverse map + CSR row pointers from a STABLY sorted key vector (flags from pcs_quantize_flags, rank =
 * their inclusive scan, perm = the sort's row permutation): uniq (m), inverse (n) = run index of every original row,
 * rowptr (m + 1) = first sorted position of every run (rowptr[m] = n). One pass for what initial_voxelize
 * (R:pcseg/model/segmentor/voxel/minkunet/utils.py:16-19) gets from torch.unique + sphashquery + spcount; the sorted
 * order doubles as the CSR of the segmented spvoxelize that follows. */
int pcs_unique_emit(const int32_t *flags, const int64_t *rank, const int64_t *perm, const int64_t *sorted_keys,
                    int64_t n, int64_t *uniq, int64_t *inverse, int64_t *rowptr, void *stream);

/* ---- fp32 convolution on the 16-bit MFMAs ("bf16x3", opt-in) ------------------------------------------
 * The same operator as pcs_conv_gather_gemm_f32 (TS:torchsparse/backend/convolution/convolution_cuda.cu:53-165 in fp32),
 * fp32 features in and out, with every operand split into three bf16 planes and six plane products accumulated in fp32:
 * fp32-grade results (not bit-identical to an fp32 FMA chain), for callers that select it explicitly. gfx950 runs
 * fp32-input MFMAs at 1/16 of the bf16 rate and has no TF32 path.
 *   applies : cin % 8 == 0, cin >= 32, cout % 4 == 0, cout >= 32, K <= 32.
 *   prepare : W (K, A, B) fp32 -> Wp: three planes in MFMA fragment order (transpose = 1: the dgrad weights);
 *             bytes = pcs_conv_prepared_weights_x3_bytes(K, contraction, columns).
 *   conv    : arguments as pcs_conv_gather_gemm_f32 with Wp instead of W; tile_rows as picked for the fp32 kernels.
 */
int pcs_conv_x3_applies(int32_t cin, int32_t cout, int32_t K);
int32_t pcs_conv_x3_column_tiles(int32_t cout);
int32_t pcs_conv_x3_emits_bn_partials(int32_t cin, int32_t cout, int32_t K, int32_t tile_rows);
size_t pcs_conv_prepared_weights_x3_bytes(int32_t K, int32_t ccon, int32_t ccols);
int pcs_conv_prepare_weights_x3(const float *W, int32_t K, int32_t A, int32_t B, int32_t transpose, void *Wp, void *stream);
int pcs_conv_gather_gemm_f32_bf16x3(const float *src, int64_t n_src, int32_t cin, const void *Wp, int32_t K, int32_t cout,
                                    const int32_t *pairs, int32_t src_col, const int32_t *seg, int32_t tile_rows,
                                    int64_t n_dst, const float *bias, float *dst, double *bn_partial,
                                    const int32_t *tile_order, void *stream);

/* ---- half-precision convolution (bf16 / fp16 storage, 16-bit MFMA, fp32 accumulate) --------------
 * The mixed-precision path of the reference: under `--amp` its ops cast their inputs to half
 * (TS:torchsparse/nn/functional/conv.py:19) and convolution_cuda.cu:61,120-127 runs gather / mm / scatter
 * in half. dtype: 1 = bfloat16, 2 = float16 (features, prepared weights and outputs share it).
 * Served shapes: pcs_conv_h_applies(cin, cout, K) != 0 (cin % 8 == 0, cin >= 32, cout % 4 == 0, an even number of
 * 16-column tiles, K <= 32; a last contraction step of 8 / 16 / 24 channels meets zero-padded weight fragments);
 * callers convert other shapes (4/5-channel stems) to fp32 and use the _f32 entries.
 *   prepare : W (K, A, B) fp32 master weights -> Wp, the weights in MFMA fragment order, converted to `dtype`.
 *             transpose = 0: forward (contraction over A = cin, columns B = cout); transpose = 1: dgrad
 *             (contraction over B, columns A). Wp bytes = pcs_conv_prepared_weights_bytes(K, contraction, columns).
 *   conv    : pcs_conv_gather_gemm_f32 with src / dst in halfs and Wp instead of W; bias stays fp32 and is added
 *             in fp32 before the single rounding of the output.
 *   wgrad   : pcs_conv_wgrad_f32 with half operands; accumulated and returned in fp32 (gW, ws as in _f32).
 */
int pcs_conv_h_applies(int32_t cin, int32_t cout, int32_t K);
size_t pcs_conv_prepared_weights_bytes(int32_t K, int32_t contraction, int32_t columns);
int pcs_conv_prepare_weights_h(const float *W, int32_t K, int32_t A, int32_t B, int32_t transpose, int32_t dtype,
                               void *Wp, void *stream);
int pcs_conv_gather_gemm_h(const void *src, int64_t n_src, int32_t cin, const void *Wp, int32_t K, int32_t cout,
                           const int32_t *pairs, int32_t src_col, const int32_t *seg, int32_t tile_rows,
                           int64_t n_dst, const float *bias, void *dst, int32_t dtype, double *bn_partial,
                           const int32_t *tile_order, void *stream);
/* with the write-back extras of pcs_conv_gather_gemm_f32_ex (addend in the storage dtype) */
int pcs_conv_gather_gemm_h_ex(const void *src, int64_t n_src, int32_t cin, const void *Wp, int32_t K, int32_t cout,
                              const int32_t *pairs, int32_t src_col, const int32_t *seg, int32_t tile_rows,
                              int64_t n_dst, const float *bias, const pcs_conv_epilogue *ep, void *dst, int32_t dtype,
                              double *bn_partial, const int32_t *tile_order, void *stream);
/* fp32 operands through the bf16 MFMAs (three-plane split, six products, fp32-grade result); same arguments as _f32 */
int pcs_conv_wgrad_f32_bf16x3(const float *fa, int32_t ca, const float *fb, int32_t cb, const int32_t *pairs,
                              int32_t a_col, const int32_t *koff_dev, const int32_t *koff_host, int32_t K, float *gW,
                              void *ws, size_t ws_bytes, void *stream);
int pcs_conv_wgrad_h(const void *fa, int32_t ca, const void *fb, int32_t cb, const int32_t *pairs, int32_t a_col,
                     const int32_t *koff_dev, const int32_t *koff_host, int32_t K, float *gW, void *ws,
                     size_t ws_bytes, int32_t dtype, void *stream);

/* ---- Cylinder3D front-end on the device -------------------------------
 * Replaces, for scans already resident in HBM, the per-frame NumPy work of
 * R:pcseg/data/dataset/semantickitti/semantickitti_cylinder.py (cart2polar :19-22, cylindrical partition
 * :144-160, voxelize_with_label :31-45) and the eval-time voxel -> point mapping of
 * R:pcseg/model/segmentor/voxel/minkunet/minkunet.py:441-453.
 *   partition : points (n, row_stride >= 3) float32 [x, y, z, extras...]; space_min3 / space_max3 = 3 HOST doubles
 *               (CYLINDER_SPACE_MIN / _MAX: rho, phi in degrees, z), grid3 = 3 HOST ints (CYLINDER_GRID_SIZE).
 *               polar (n,3) float32 [rho, phi_deg, z] (may be NULL); coord (n,3) int32 cell indices
 *               = floor((clip(polar, min, max) - min) / ((max - min) / (grid - 1))) in float64 like NumPy;
 *               feat (n, 8 + row_stride - 3) float32 = [cell centre (3), polar (3), x, y, extras] (may be NULL).
 *   label vote: voxel_labels[v] = first arg-max over classes of #{points i: inverse[i] == v, labels[i] == class},
 *               labels equal to ignore_label (67 in the reference) are not counted; counter_ws = m * num_classes
 *               int32 (zeroed inside); bad_flag = 1 DEVICE int32, set to 1 if a counted label is outside
 *               [0, num_classes) (the reference raises IndexError there).
 *   argmax    : out[i] = first arg-max of logits[inverse ? inverse[i] : i] (m rows of c floats), -1 for an
 *               out-of-range row: `out[cur_inv].argmax(1)` of the reference without the (n, c) intermediate.
 */
int pcs_cylinder_partition_f32(const float *points, int64_t n, int32_t row_stride, const double *space_min3,
                               const double *space_max3, const int32_t *grid3, float *polar, int32_t *coord,
                               float *feat, void *stream);
int pcs_voxel_label_vote(const int64_t *inverse, const int64_t *labels, int64_t n, int64_t m, int32_t num_classes,
                         int64_t ignore_label, int32_t *counter_ws, int32_t *bad_flag, int64_t *voxel_labels,
                         void *stream);
int pcs_rows_argmax_gather_f32(const float *logits, int64_t m, int32_t c, const int64_t *inverse, int64_t n,
                               int64_t *out, void *stream);

/* ---- the cylinder dataset's transform of a raw batch (csrc/cylscan.hip; added under ABI v12, additive) ------------------
 * Replaces, for scans resident in HBM, what R:pcseg/data/dataset/semantickitti/semantickitti_cylinder.py:104-160 does per frame
 * and per vote in the dataloader workers (waymo_cylinder.py is the same code): aug_points (:115-142, R:tools/utils/common/
 * seg_utils.py:43-100) stored back as float32, cart2polar (:144), the degrees (:145), the partition (:146-153) and the point
 * features (:158-160); the ten votes of :92-99 from ONE read of the scan. One launch, no workspace, no host read.
 *   points, frame_offsets, params, num_votes: as pcs_scan_transform (params vote-major, row v * num_frames + f); 3 <= c <=
 *   PCS_SCAN_MAX_COLUMNS, 1 <= num_votes <= PCS_SCAN_MAX_VOTES, 1 <= num_frames <= 65535. space_min3 / space_max3 / grid3:
 *   HOST values as pcs_cylinder_partition_f32 (grid >= 2, max > min, else PCS_EINVAL).
 * Per row i of frame f and vote v, output row v * n + i:
 *   (x', y', z') = the affine map of pcs_scan_transform: float64, that order, no multiply-add fused, one rounding to float32;
 *   [rho, phi in degrees, z'], the cell and its centre = the arithmetic of pcs_cylinder_partition_f32 applied to (x', y', z');
 *   feat (num_votes * n, 8 + c - 3) fp32 = [centre (3), rho, phi, z', x', y', the other columns unchanged];
 *   coord (num_votes * n, 3) int32 = the cell; scenes (num_votes * n) int64 = v * num_frames + f.
 * Offsets outside [0, n] are clamped: nothing outside the num_votes * n rows is addressed; an empty frame writes nothing;
 * n == 0 launches nothing. */
int pcs_cylinder_scan_batch_f32(const float *points, int64_t n, int32_t c, const int64_t *frame_offsets, int32_t num_frames,
                                const double *params, int32_t num_votes, const double *space_min3, const double *space_max3,
                                const int32_t *grid3, float *feat, int32_t *coord, int64_t *scenes, void *stream);

/* ---- the fusion dataset's range view of a collated batch (csrc/rangeproj.hip; added under ABI v12, additive) -------------
 * Replaces, for voxel rows resident in HBM, get_range_image of R:pcseg/data/dataset/semantickitti/semantickitti_fusion.py:64-114
 * (waymo_fusion.py is the same code) and the range_pxpy table of its collates (:198-245): the projection of every scene's
 * deduplicated voxel rows onto an H x W image with a per-scene azimuthal cut, "the last row that hits a pixel wins".
 *   feats (n, c) fp32, c >= 5: [x, y, z, reflectivity, ring, ...]; scenes (n,) int32: the scene of every row, rows of a scene
 *   contiguous and in the collate's order; cuts32 (S,) fp32 ON THE DEVICE: float32((u - 0.5) * 2 pi) of the scene's
 *   np.random.rand() value u, rounded once on the host; S scenes, H >= 2, W >= 2, S * H * W < 2^31, 0 <= n < 2^31.
 * pcs_range_project_f32, per row i (all float32, no multiply-add fused, each operation rounded on its own):
 *   yaw = float32(atan2(double(y), double(-x))) + cuts32[scene];  yaw = remainder(yaw, float32(2 pi)) - float32(pi)  (NumPy's
 *   remainder: fmodf, + float32(2 pi) when negative);  ix = rint(0.5 * (yaw / float32(pi) + 1) * (W - 1)), iy = rint(ring),
 *   ties to even;  pxpy[i] = (float(scene), float(2 (ix / (W - 1) - 0.5)), float(2 (iy / (H - 1) - 0.5))), the last two in
 *   float64 from the rounded integers;  winner[scene][iy][ix] = max(winner[..], i)  (atomic; independent of the order the
 *   atomics retire in, and equal to the reference's last write because a scene's rows ascend).
 *   winner (S * H * W) int32 is set to -1 and bad[0] to 0 by the entry itself (two hipMemsetAsync on `stream`). A row whose
 *   x, y or ring is not finite, whose iy is outside [0, H - 1] or whose scene is outside [0, S) sets bad[0] = 1, writes its
 *   pxpy row and touches no pixel (the reference asserts on a ring > H - 1 and wraps a negative one).
 * pcs_range_image_fill_f32: winner -> image (S, 5, H, W) fp32, pixel-major. A pixel whose winner is w in [0, n):
 *   channel 0 = float32(25 (double(1.0f / depth) - 0.4)), depth = sqrtf((x x + y y) + z z) in float32;
 *   channel 1 = float32(20 (double(reflectivity) - 0.5));  channels 2..4 = x, y, z.  Any other pixel: (-10, -10, 0, 0, 0).
 *   Four pixels per lane and 16-byte stores where W % 4 == 0 and winner / image are 16-byte aligned, one pixel per lane otherwise.
 * pcs_range_project_ws_bytes: the bytes of `winner`, or -1 on sizes the entries refuse. Sizes are checked before any pointer:
 * bad sizes give PCS_EINVAL also with null pointers; n == 0 with valid sizes projects nothing (the winner is still cleared
 * when it is given). Nothing allocates, nothing is read back. */
int64_t pcs_range_project_ws_bytes(int32_t num_scenes, int32_t H, int32_t W);
int pcs_range_project_f32(const float *feats, int64_t n, int32_t c, const int32_t *scenes, const float *cuts32, int32_t num_scenes,
                          int32_t H, int32_t W, int32_t *winner, float *pxpy, int32_t *bad, void *stream);
int pcs_range_image_fill_f32(const int32_t *winner, const float *feats, int64_t n, int32_t c, int32_t num_scenes, int32_t H,
                             int32_t W, float *image, void *stream);

/* ---- the range-view dataset's scan and its KNN label vote (csrc/rangescan.hip; added under ABI v12, additive) -----------------
 * Replaces, for raw scans resident in HBM, LaserScan.do_range_projection + SemLaserScan.do_label_projection of
 * R:pcseg/data/dataset/semantickitti/laserscan.py:174-238, :389-400, prepare_input_label_semantic_with_mask + generate_label of
 * R:pcseg/data/dataset/semantickitti/semantickitti_rv.py:284-334, and KNN.forward of R:pcseg/model/segmentor/range/utils.py:291-341.
 *   points (n, c) fp32, c >= 4: [x, y, z, remission, ...] frame after frame; frame_offsets (F + 1) int64 ON THE DEVICE, ascending
 *   from 0 to n; labels (n) int64 or NULL (the semantic id is label & 0xFFFF); lut (lut_size) int64 ON THE DEVICE or lut_size = 0:
 *   an id below lut_size goes through the table, any other stays; F frames, H >= 1, W >= 1, F * H * W < 2^31, 0 <= n < 2^31.
 *   fov_down_abs, fov_total: float32(|fov_down|) and float32(|fov_down| + |fov_up|) in radians, rounded once on the host.
 * pcs_range_scan_f32, launch 1, per point i of frame f (all float32, no multiply-add fused, each operation rounded on its own,
 * sqrt and divisions correctly rounded):
 *   depth = sqrt((x x + y y) + z z);  yaw = -float32(atan2(double(y), double(x)));  pitch = float32(asin(double(z / depth)));
 *   proj_x[i] = clamp(floor(0.5 (yaw / float32(pi) + 1) W), 0, W - 1);  proj_y[i] = clamp(floor((1 - (pitch + fov_down_abs) /
 *   fov_total) H), 0, H - 1);  unproj_range[i] = depth;  winner[f][proj_y][proj_x] = min(winner[..], float bits of depth << 32 |
 *   index within the frame) (one 64-bit atomic): the pixel goes to the smallest depth, among equal depths to the smallest index,
 *   whatever order the atomics retire in. A row whose x, y, z or depth is not finite, whose depth is zero or whose float32
 *   |z / depth| exceeds 1 (z * z in the subnormals: no pitch) sets bad[0] = 1, gets
 *   proj_x = proj_y = -1 and touches no pixel. winner is set to all ones and bad[0] to 0 by the entry (two hipMemsetAsync).
 * Launch 2, per pixel with winner row r (index idx within its frame):
 *   scan (F, 6, H, W) fp32 = [x / 50, y / 50, z / 3, remission, depth / 80, mask];  label_rv (F, H, W) int64 = the (mapped)
 *   semantic id (0 without labels);  mask_rv (F, H, W) fp32 = mask_hit ? 1 : (idx > 0 ? 1 : 0) (the reference's proj_idx > 0);
 *   proj_idx (F, H, W) int32 = idx.  An empty pixel: x = y = z = remission = depth = -1 before the divisions, mask 0, label 0,
 *   proj_idx -1.
 * pcs_range_scan_ws_bytes: the bytes of `winner` (8 per pixel), or -1 on sizes the entry refuses.
 * pcs_range_knn_vote, one launch, per point i of scene b (point_offset (B + 1) int64 ON THE DEVICE), u = unproj_range[i]:
 *   the search x search window around (proj_y[i], proj_x[i]) of proj_range (B, H, W) fp32 and proj_argmax (B, H, W) int64, range 0
 *   and label 0 outside the image (no azimuthal wrap); a negative range becomes +inf, the centre's range u;
 *   distance_k = |range_k - u| * weights_host[k]  (weights_host: search^2 HOST floats, 1 - the normalised gaussian, row-major;
 *   they travel by value in the kernel arguments); the knn first candidates in ascending (distance, k) vote with their label,
 *   those with distance > cutoff (cutoff > 0) for an extra bin; pred[i] = the class of 1 .. num_class - 1 with the most votes, the
 *   lowest on equal counts (1 when none has any). A label outside [0, num_class), tested on all 64 bits, takes its place among
 *   the nearest and votes for nothing. One point per lane: 0 <= n < 2^31. A point whose pixel is outside
 *   the image (proj_x < 0: the scan's bad rows) gets pred = 0 and is not counted.
 *   hist (num_class, num_class) int64 or NULL: hist[labels[i]][pred[i]] += 1 for labels in [0, num_class); needs labels (n).
 *   Accumulates: integer sums, exact and run-to-run identical.
 *   search in {3, 5, 7}, 1 <= knn <= search^2, cutoff >= 0 (0 = off), 2 <= num_class <= 64: anything else is PCS_EINVAL.
 * Sizes are checked before any pointer: bad sizes give PCS_EINVAL also with null pointers. Nothing allocates, nothing is read back. */
int64_t pcs_range_scan_ws_bytes(int32_t num_frames, int32_t H, int32_t W);
int pcs_range_scan_f32(const float *points, int64_t n, int32_t c, const int64_t *frame_offsets, int32_t num_frames,
                       const int64_t *labels, const int64_t *lut, int32_t lut_size, int32_t H, int32_t W, float fov_down_abs,
                       float fov_total, int32_t mask_hit, void *winner, float *scan, int64_t *label_rv, float *mask_rv,
                       int32_t *proj_idx, int32_t *proj_x, int32_t *proj_y, float *unproj_range, int32_t *bad, void *stream);
int pcs_range_knn_vote(const float *proj_range, const int64_t *proj_argmax, int32_t num_scenes, int32_t H, int32_t W,
                       const float *unproj_range, const int32_t *proj_x, const int32_t *proj_y, int64_t n,
                       const int64_t *point_offset, int32_t search, int32_t knn, float cutoff, const float *weights_host,
                       int32_t num_class, const int64_t *labels, int64_t *hist, int64_t *pred, void *stream);

/* ---- PolarMix / LaserMix of two raw batches (csrc/scanmix.hip; added under ABI v12, additive) ---------------------------
 * Replaces, for scans resident in HBM, the mixing of two scans in R:pcseg/data/dataset/semantickitti/semantickitti.py:117-170
 * (polarmix of PolarMix_semantickitti.py, lasermix_aug of LaserMix_semantickitti.py, get_kitti_points_ringID :86-96).
 *   points1 (n1, 4) fp32 / labels1 (n1) int64 / frame_offsets1 (F + 1) int64: the batch, frame after frame; points2 / labels2 /
 *   frame_offsets2: the partner scans, frame f of one mixes with frame f of the other. n1, n2 >= 0, n1 + 4 n2 < 2^31,
 *   1 <= F <= 65535. Offsets outside [0, n] are clamped: nothing outside the rows is addressed.
 *   plan (F, PCS_MIX_PLAN_STRIDE) float64 ON THE DEVICE, per frame [mode, alpha, beta, swap, paste, T, t_0 .. t_{T-1}, 0 ...]:
 *     mode 0: the mixed frame is scan 1 unchanged (no mixing, and LaserMix as the reference computes it);
 *     mode 1: PolarMix. alpha, beta: the sector's edges as float32 values. A row is inside the sector when swap != 0 and
 *       alpha < yaw < beta, yaw = -float32(atan2(double(y), double(x))), all in float32. paste != 0 appends the instance rows;
 *     mode 2: LaserMix over bands. T <= 5 descending thresholds in radians; band = the number of thresholds with inc <= t,
 *       inc = atan2(double(z), sqrt(double(x)^2 + double(y)^2)), no multiply-add fused.
 *   classes (num_classes) int64 ON THE DEVICE, num_classes <= PCS_MIX_MAX_CLASSES, distinct: the instance classes in paste order.
 *   omega (2, 8) float64 ON THE DEVICE: parameter rows of pcs_scan_transform's affine map, (cos w, sin w, 1, 1, 1, 0, 0, 0).
 * Rows of a mixed frame, in this order (PCS_MIX_BUCKETS counted buckets, each in scan order):
 *   mode 1: bucket 0 = scan 1 outside the sector; bucket 1 = scan 2 inside it; bucket 2 + k = scan 2 with label classes[k];
 *           then buckets 2 .. 9 again under omega row 0, and again under omega row 1 (xyz through the affine map: float64, no
 *           multiply-add fused, one rounding; column 3 and the label copied);
 *   mode 2: bucket b = band b, from scan 1 where b is even, from scan 2 where b is odd;  mode 0: bucket 0 = scan 1.
 * pcs_scan_mix_count: ws (pcs_scan_mix_ws_bytes) <- the per-workgroup bases, totals (F, PCS_MIX_BUCKETS) int32 <- the bucket
 *   sizes, frame_base (F + 1) int64 <- the first mixed row of every frame and, last, the number of mixed rows m (the sum of a
 *   frame's totals, buckets 2 .. 9 counted three times in mode 1). Three launches, no atomics, nothing read back: the caller
 *   reads `totals` (or frame_base[F]) to size the output.
 * pcs_scan_mix_place: the same inputs, ws / totals / frame_base as the count left them -> out_points (m, c_out) fp32, columns
 *   0 .. 3 written (4 <= c_out <= PCS_SCAN_MAX_COLUMNS; 16-byte stores where c_out == 4 and the rows are aligned), out_labels
 *   (m) int64. Every store is checked against m. The order of the output is a pure function of the input.
 * pcs_scan_ring_f32: column 4 of points (m, c >= 5) <- get_kitti_points_ringID per frame of frame_base: proj = 0.5 (yaw /
 *   float32(pi) + 1) in float32 with yaw = -float32(atan2(double(y), double(-x))); row i flags when it is not the first of its
 *   frame, proj[i] < 0.2 and proj[i - 1] > 0.8; ring = min(the flags up to i inside the frame, 63). ws: pcs_scan_ring_ws_bytes(m).
 * Sizes are checked before any pointer: bad sizes give PCS_EINVAL (-1 from the *_ws_bytes queries) also with null pointers. */
#define PCS_MIX_BUCKETS 10
#define PCS_MIX_MAX_CLASSES 8
#define PCS_MIX_PLAN_STRIDE 16
int64_t pcs_scan_mix_ws_bytes(int64_t n1, int64_t n2, int32_t num_frames);
int pcs_scan_mix_count(const float *points1, int64_t n1, const int64_t *frame_offsets1, const float *points2,
                       const int64_t *labels2, int64_t n2, const int64_t *frame_offsets2, int32_t num_frames, const double *plan,
                       const int64_t *classes, int32_t num_classes, void *ws, int64_t ws_bytes, int32_t *totals,
                       int64_t *frame_base, void *stream);
int pcs_scan_mix_place(const float *points1, const int64_t *labels1, int64_t n1, const int64_t *frame_offsets1,
                       const float *points2, const int64_t *labels2, int64_t n2, const int64_t *frame_offsets2,
                       int32_t num_frames, const double *plan, const int64_t *classes, int32_t num_classes, const double *omega,
                       const void *ws, int64_t ws_bytes, const int32_t *totals, const int64_t *frame_base, int64_t m, int32_t c_out,
                       float *out_points, int64_t *out_labels, void *stream);
int64_t pcs_scan_ring_ws_bytes(int64_t m);
int pcs_scan_ring_f32(float *points, int64_t m, int32_t c, const int64_t *frame_base, int32_t num_frames, void *ws,
                      int64_t ws_bytes, void *stream);

/* ---- prediction tail of an evaluation pass (csrc/predict.hip; added under ABI v12, additive) --------------------------
 * The reference's eval tail (R:pcseg/model/segmentor/voxel/minkunet/minkunet.py:436-455, scoring R:infer.py:35-52) for a
 * whole batch in one launch, no host synchronisation. logits: (m, c) rows of the batch, c <= 64. For point i of scene b
 * (the b with point_offset[b] <= i < point_offset[b + 1]): row = row_offset[b] + inverse[i], inverse being the per-SCENE
 * row index of the point. n_scenes = 0 (offsets ignored) = one scene spanning everything: row = inverse ? inverse[i] : i
 * (inverse NULL needs n == m). A row outside its scene's range -- or a point outside every span -- sets bad_flag[0] |= 1
 * (1 device int32, zeroed by the caller, never cleared here), gives pred = -1 and is not counted; the range is checked
 * before any address is formed.
 *   votes (n, c) or NULL : votes[i] += softmax(logits[row]) in fp32, maximum subtracted (the reference's return_tta
 *                          output summed over passes); the score vector is then votes[i], else the logits row;
 *   pred  (n) or NULL    : first arg-max of the score vector (lowest index on ties);
 *   hist  (c, c) or NULL : hist[labels[i]][pred[i]] += 1 for labels in [0, c) (fast_hist's mask); needs labels (n).
 *                          Accumulates (the caller zeroes it once): integer sums, exact and run-to-run identical. */
int pcs_predict_points_f32(const float *logits, int64_t m, int32_t c, const int64_t *inverse, int64_t n,
                           const int64_t *point_offset, const int64_t *row_offset, int32_t n_scenes,
                           const int64_t *labels, float *votes, int64_t *pred, int64_t *hist, int32_t *bad_flag,
                           void *stream);

/* ---- all layers' weight preparation in one launch (ABI v7) ---------------------------------------------------------
 * pcs_transpose_kab_f32 (kind 0: dst (K, B, A) fp32 = per-offset transposed weights for dgrad) and
 * pcs_conv_prepare_weights_h (kind 1 bf16 / 2 fp16: dst = prepared half weights of pcs_conv_prepared_weights_bytes bytes,
 * `transpose` as there) for a whole list of layers: the weights change once per optimizer step, so a training step
 * needs one launch instead of one per layer call (csrc/weights_multi.hip). Element-wise identical to the per-layer calls.
 *   pcs_weights_multi_plan : fills nctt / nt16 / ns / first_block of the HOST job table, returns the launch's work-block
 *                            count (-1 + pcs_last_error on a bad job);
 *   pcs_weights_multi      : jobs_dev = the planned table copied to the device. */
typedef struct {
  const float *src; /* (K, A, B) fp32 master weights */
  void *dst;
  int32_t K, A, B;
  int32_t kind;      /* 0 transpose, 1 prepare bf16, 2 prepare fp16 */
  int32_t transpose; /* kinds 1 / 2: 0 = forward (contract over A), 1 = dgrad (contract over B) */
  int32_t nctt, nt16, ns; /* filled by the plan call */
  int64_t first_block;    /* filled by the plan call */
} pcs_weight_job;
int64_t pcs_weights_multi_plan(pcs_weight_job *jobs_host, int32_t n_jobs);
int pcs_weights_multi(const pcs_weight_job *jobs_dev, int32_t n_jobs, int64_t total_blocks, void *stream);

/* ---- the tail of a training step in two launches (still v12, additive; csrc/steptail.hip) ---------------------------------
 * scaler.unscale_ -> clip_grad_norm_(params, max_norm) -> scaler.step(SGD(momentum, weight_decay, nesterov)) -> scaler.update
 * of R:train.py:367-372 / R:pcseg/optim/__init__.py:15-34 over one job table: a job is one fp32 parameter tensor with its
 * gradient and (with momentum) its momentum buffer. A workgroup covers PCS_STEP_BLOCK_ELEMS elements of one job.
 *   plan  : HOST. Checks the jobs against `hyper` (group index, 4-byte alignment, buf present exactly when the group's
 *           mu != 0, non-null p / g unless numel == 0), fills first_block, returns the work-block count (-1 + pcs_last_error on
 *           a bad job). The planned table is copied to the device by the caller.
 *   norm  : one read of every g. Sum of squares in double; a workgroup sweeps work blocks b, b + grid, ... (grid = min(total_blocks,
 *           2048)), leaves one partial in `ws`, and the workgroup that draws the last ticket folds the partials in a fixed order:
 *           bit-reproducible, no float atomics. Writes `record` (8 DEVICE floats):
 *             [0] total_norm = float(sqrt(double sum)) of the gradients as they are stored (scaled, under a scaler)
 *             [1] inv_scale  = float(1.0 / double(*scale)); 1 when scale == NULL
 *             [2] coef       = min(max_norm / (total_norm * inv_scale + 1e-6f), 1.0f) in fp32, a NaN kept (torch's clamp);
 *                              1 when max_norm < 0 (no clipping)
 *             [3] found_inf  = 1.0f when any gradient value was inf or NaN, else 0.0f
 *             [4] total_norm * inv_scale: the norm of the unscaled gradients, what clip_grad_norm_ returns
 *             [5..7] 0
 *           and then, with scale != NULL, torch.amp.GradScaler.update's rule on the DEVICE words *scale / *growth_tracker:
 *           found_inf -> scale *= backoff, tracker = 0; else ++tracker, and when it equals growth_interval scale *= growth
 *           (kept when the product is not finite) and tracker = 0. The record holds the scale from BEFORE the update.
 *           ws: PCS_STEP_WS_BYTES(total_blocks) bytes whose first 4 are zero before the first launch (the kernel leaves them
 *           zero). An empty table is PCS_EINVAL.
 *   apply : per element, one fp32 rounding per operation, nothing contracted:
 *             g1 = g * inv_scale;  g2 = g1 * coef;  d = g2 + wd * p;
 *             mu != 0:  buf = mu * buf + d;  d = nesterov ? d + mu * buf : buf;
 *             p = p + (-lr) * d
 *           record == NULL: inv_scale = coef = 1 (plain SGD, one launch). skip_on_inf != 0 (a scaler is in play; wants a
 *           record): when found_inf is set nothing is written, p and buf keep their bits. g is NEVER written: unlike torch,
 *           the gradients stay scaled and unclipped. `hyper` is a HOST struct and travels by value in the kernel arguments.
 *           16-byte loads and stores for a job whose p, g, buf are 16-byte aligned, element-wise otherwise and at a job's end. */
#define PCS_STEP_BLOCK_ELEMS 4096
#define PCS_STEP_MAX_GROUPS 8
#define PCS_STEP_WS_BYTES(total_blocks) (16 + 12 * (int64_t)(total_blocks))
typedef struct {
  float *p;
  const float *g;
  float *buf;          /* NULL exactly when the group's mu == 0 */
  int64_t numel;
  int32_t group;       /* index into pcs_step_hyper */
  int32_t reserved;
  int64_t first_block; /* filled by the plan call */
} pcs_step_job;
typedef struct {
  float lr[PCS_STEP_MAX_GROUPS], wd[PCS_STEP_MAX_GROUPS], mu[PCS_STEP_MAX_GROUPS];
  int32_t nesterov[PCS_STEP_MAX_GROUPS];
  int32_t n_groups;
} pcs_step_hyper;
int64_t pcs_step_plan(pcs_step_job *jobs_host, int32_t n_jobs, const pcs_step_hyper *hyper);
int pcs_step_norm(const pcs_step_job *jobs_dev, int32_t n_jobs, int64_t total_blocks, float max_norm, float *scale,
                  int32_t *growth_tracker, double growth_factor, double backoff_factor, int32_t growth_interval, void *ws,
                  int64_t ws_bytes, float *record, void *stream);
int pcs_step_apply(const pcs_step_job *jobs_dev, int32_t n_jobs, int64_t total_blocks, const pcs_step_hyper *hyper,
                   const float *record, int32_t skip_on_inf, void *stream);

/* ---- Lovasz-softmax of the training criterion (the timed step's loss tail) -----------------
 * lovasz_softmax(probas, labels, classes='present', per_image=False, ignore) of
 * R:tools/utils/common/lovasz_losses.py:158-204 (+ lovasz_grad :23-35, flatten_probas :207-228) as the reference's
 * criterion calls it (R:pcseg/loss/__init__.py:106-115), value AND gradient w.r.t. probas, every class in one radix
 * sort instead of a sort / gather / three scans per class (csrc/lovasz.hip).
 *   probas (n, num_class) float32 row-major, labels (n,) int64. has_ignore = 0: every label inside [0, num_class)
 *   counts; has_ignore = 1: points labelled `ignore` (any value, also outside the class range) are dropped. Labels
 *   outside [0, num_class) never count. loss = 1 DEVICE float (0 when no class is present); grad (n, num_class)
 *   float32 = d loss / d probas, every element written (may be NULL: value only).
 *   Ties between equal errors keep point order (what torch's stable descending sort gives the reference).
 *   ws: pcs_lovasz_workspace_bytes(n, num_class, has_ignore, ignore) bytes (-1 + pcs_last_error on bad sizes;
 *   28 B per point and class + the sort's temporaries). num_class <= 60, n * num_class < 2^32 - 1. */
int64_t pcs_lovasz_workspace_bytes(int64_t n, int32_t num_class, int32_t has_ignore, int64_t ignore);
int pcs_lovasz_softmax_f32(const float *probas, const int64_t *labels, int64_t n, int32_t num_class, int32_t has_ignore,
                           int64_t ignore, float *loss, float *grad, void *ws, int64_t ws_bytes, void *stream);

/* ---- the range-view training criterion (csrc/rangeloss.hip; added under ABI v12, additive) ------------
 * What the reference's range segmentors run on their logits every training step
 * (R:pcseg/model/segmentor/range/fidnet/model/semantic/fidnet.py:62-84, salsanext.py:250-271, cenet.py:248-318):
 *   loss = w_ce * mean_pixels(CE + Dice) + w_ls * Lovasz_softmax(ignore) + w_bd * BoundaryLoss(theta0 = 3)
 * with CrossEntropyLoss(reduction='none', weight) / CrossEntropyDiceLoss, DiceLoss._dice_loss_multichannel, BoundaryLoss and
 * one_hot of R:pcseg/model/segmentor/range/utils.py:520-724, value and gradient by the logits.
 *   logits (B, C, H, W) contiguous NCHW, dtype 0 fp32 / 1 bf16 / 2 fp16 (upcast exactly; fp32 arithmetic, double folds);
 *   labels (B, H, W) int64; class_weight (C) fp32 or NULL (= 1): the weight of CrossEntropyLoss; 2 <= C <= 32, B, H, W >= 1,
 *   B * C * H * W < 2^32 - 1. flags: PCS_RANGE_LOSS_DICE (the Dice term is on) | PCS_RANGE_LOSS_BOUNDARY (the boundary term is on).
 *   A label outside [0, C) is handled like ignore_index (the reference raises): CE term 0 but counted in the mean's divisor, no
 *   one-hot row, left out of Dice's denominator. This is the one extension.
 * pcs_range_loss_stats (utils.py:552, :594-608, :689-702; fidnet.py:63, :74, :80): softmax and log-softmax once per pixel; into ws the
 *   CE sum, per class sum p onehot and sum (p + onehot) of Dice, per (image, class) sum pred_b gt_b, sum pred_b, sum gt_b with
 *   pred_b = p - min3x3(p), gt_b = onehot - min3x3(onehot), the window clipped at the image border (max_pool2d(1 - x, 3, 1, 1) -
 *   (1 - x): the padding is minus infinity). probas (B H W, C) fp32 or NULL: the softmax as flatten_probas (utils.py:489-506) lays
 *   it out, the input of pcs_lovasz_softmax_f32. Per-workgroup partials, then a fixed-order sum in double: no float atomics.
 * pcs_range_loss_fold (utils.py:604-624, :705-712; fidnet.py:67, :84): on the device, no host read. lovasz: 1 DEVICE float (the
 *   loss of pcs_lovasz_softmax_f32) or NULL (term off). terms (5) DEVICE floats <- total, ce, dice, ls, bd with total = w_ce (ce +
 *   dice) + w_ls ls + w_bd bd; into ws the coefficients of the gradient pass: per class, with den = D + 1e-4, dDice / dp(x) =
 *   -(1 / C)(2 onehot / den - 2 I / den^2); per (image, class), with P = I / (S + 1e-7), R = I / (G + 1e-7), BF1 = 2 P R / (P + R +
 *   1e-7), d bd / d pred_b(x) = a gt_b(x) + b. Dice is 0 with zero coefficients when every D is zero (utils.py:609-611).
 * pcs_range_loss_grad (the autograd mirror of all of the above): grad (B, C, H, W) in the logits' dtype, every element written,
 *   d logit_c = p_c (g_c - sum_k p_k g_k) + w_ce class_weight[label] (p_c - onehot_c) / (B H W), one rounding, g_c = w_ls
 *   lovasz_grad[pixel][c] + dice_c + bd_c; lovasz_grad (B H W, C) fp32 = the grad of pcs_lovasz_softmax_f32 or NULL. The boundary
 *   term is gathered: bd_c(q) = coef(q) - the coef(r) of every centre r around q whose window has its minimum at q. Among equal
 *   minima the FIRST in row-major order of the clipped window takes the gradient (torch's max_pool2d backward): part of the contract.
 *   flags, class_weight and w_ce as given to the two earlier calls on the same ws.
 * ws: pcs_range_loss_ws_bytes(B, C, H, W) bytes (-1 + pcs_last_error on sizes the entries refuse), contents irrelevant on entry.
 * Sizes are checked before any pointer: bad sizes give PCS_EINVAL also with null pointers. Nothing allocates, nothing is read back;
 * the results are a pure function of the inputs, bit for bit. */
#define PCS_RANGE_LOSS_DICE 1
#define PCS_RANGE_LOSS_BOUNDARY 2
int64_t pcs_range_loss_ws_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
int pcs_range_loss_stats(const void *logits, int32_t dtype, const int64_t *labels, const float *class_weight, int32_t B, int32_t C,
                         int32_t H, int32_t W, int32_t flags, float *probas, void *ws, int64_t ws_bytes, void *stream);
int pcs_range_loss_fold(int32_t B, int32_t C, int32_t H, int32_t W, int32_t flags, const float *lovasz, float w_ce, float w_ls,
                        float w_bd, float *terms, void *ws, int64_t ws_bytes, void *stream);
int pcs_range_loss_grad(const void *logits, int32_t dtype, const int64_t *labels, const float *class_weight, const float *lovasz_grad,
                        int32_t B, int32_t C, int32_t H, int32_t W, int32_t flags, float w_ce, float w_ls, const void *ws,
                        int64_t ws_bytes, void *grad, void *stream);

/* ---- measurement switches (NOT part of the drop-in contract: no reference function stands behind them; results never depend on
 * them; used by tools/convh_ws_ab.py and tools/wgrad_interleave_ab.py to A/B two kernel policies inside one process) -------------
 * pcs_debug_convh_ws: mode -1 = environment (PCS_CONVH_WS, default on), 0 = the 16-bit convolution on conv_os5h only, 1 = the
 *   weight-stationary kernel where the policy picks it, >= 2 = wherever an instance exists; `ru` unused; rs = 1: two-row-block
 *   sub-groups on the two shapes that have both instances.
 * pcs_debug_wgrad_interleave: launch order of the weight-gradient splits, -1 = default (2 for 16-bit operands, 0 for fp32),
 *   0 offset-major, 1 position-major, 2 position-major with every XCD on a contiguous eighth.
 * pcs_debug_conv_plan: host only; the plan the library routes a forward / input-gradient convolution call on -- the one value the
 *   entries launch from and the shape queries answer from. kind 0 = pcs_conv_gather_gemm_f32(_ex), 1 = pcs_conv_gather_gemm_h(_ex),
 *   2 = pcs_conv_gather_gemm_f32_bf16x3; dtype as there; flags: 1 bn_partial given, 2 tile_order given, 4 write-back extras,
 *   8 PCS_EP_POST_AFFINE among them, 16 a tensor off 16 bytes. out = {family (0 not served, 1 conv_block, 2 conv_wave4,
 *   3 conv_wave5, 4 conv_wave5h, 5 conv_wave6h, 6 conv_wave5x), 16-column tiles per column tile, column tiles, threads per
 *   workgroup, TAIL instance, row blocks per group, wave6h row blocks per sub-group, wave6h contraction chunks, nt16, ns of the
 *   prepared weights, LDS bytes, answers (1 emits BatchNorm partials at this height, 2 reads tile_order, 4 takes extras)}. */
void pcs_debug_convh_ws(int32_t mode, int32_t ru, int32_t rs);
void pcs_debug_conv_plan(int32_t kind, int32_t dtype, int32_t cin, int32_t cout, int32_t K, int32_t tile_rows, int32_t flags,
                         int32_t out[12]);
void pcs_debug_wgrad_interleave(int32_t mode);
/* store form of pcs_cylinder_scan_batch_f32 (tools/cylinder_input_bench.py): -1 = environment (PCS_CYLSCAN_STORE, default 2),
 * 0 = features and cells staged in LDS and written as contiguous ranges, 1 = every lane stores its own rows, 2 = features staged,
 * cells direct */
void pcs_debug_cylscan_store(int32_t form);

#ifdef __cplusplus
}
#endif
#endif /* PCSEG_HIP_H_ */
