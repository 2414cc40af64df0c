/*
 * isf_hip.h -- C ABI of libisf_hip.so: the MI355X (gfx950) implementation of IS-Fusion's
 * LiDAR voxelization -> sparse-conv -> BEV hot path (BASELINE.json north_star).
 *
 * Conventions
 *   - extern "C", plain pointers + sizes, no torch/ATen types.  All data pointers are DEVICE pointers
 *     unless the parameter name ends in `_host`.  All tensors are dense, row-major, contiguous.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls are asynchronous on
 *     that stream, except where an output count is returned through a `*_host` pointer: those calls
 *     synchronise the stream once before returning (the reference ops do the same, see each entry).
 *   - Return value: ISF_OK (0) or a negative ISF_ERR_* code; never throws.  isf_last_error() returns a
 *     thread-local message for the last failure.
 *   - Buffers are caller-owned.  Scratch memory (bump arena, side stream, event pool) is one object per
 *     (device, stream) owned by the library, grown on demand with hipMalloc and released by
 *     isf_release_workspace(): calls on different streams are independent; one call at a time per stream.
 *   - No process-global options and no environment switches: precision / diagnostics travel with the call.
 *   - Voxel coordinates are int32 (z, y, x) or (b, z, y, x) exactly like the reference.
 *
 * Each entry cites the reference interface it replaces (paths relative to the reference root).
 */
#ifndef ISF_HIP_H
#define ISF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISF_OK 0
#define ISF_ERR_ARG (-1)         /* bad argument (null pointer, negative size, unsupported shape) */
#define ISF_ERR_HIP (-2)         /* a HIP runtime call failed */
#define ISF_ERR_NOMEM (-3)       /* workspace allocation failed */
#define ISF_ERR_UNSUPPORTED (-4) /* valid request outside what this build implements */
#define ISF_ERR_CAPACITY (-5)    /* caller-provided output capacity too small */

#define ISF_REDUCE_SUM 0
#define ISF_REDUCE_MEAN 1
#define ISF_REDUCE_MAX 2

#define ISF_CONV_SUBM 0   /* SubMConv3d  */
#define ISF_CONV_SPARSE 1 /* SparseConv3d */

typedef void* isf_stream_t; /* hipStream_t */

/* library / runtime ----------------------------------------------------------------------------- */
int isf_version(void);                 /* (major<<16)|(minor<<8)|patch */
const char* isf_last_error(void);      /* message of the last failure on this thread ("" if none) */
int isf_device_count(int* count_host); /* number of visible HIP devices (0 on a CPU-only host) */
int isf_release_workspace(void);       /* free every (device, stream) workspace */
int isf_workspace_bytes(size_t* bytes_host); /* current arena size on the current device */
/* DIAGNOSTIC: every device allocation behind the workspaces of the current device: stream_base_bytes [max_triples][3] =
 * (stream handle, base address, bytes) -- per workspace its blocks, then its two persistent byte maps; *num_triples = how
 * many exist.  tools/graph_fault.py maps a GPU memory-fault address onto them. */
int isf_debug_workspace_blocks(unsigned long long* stream_base_bytes, int max_triples, int* num_triples);
/* DIAGNOSTIC: the library's stable sort on its own (csrc/isf_sort.hip; tests/test_gpu_sort.py).  order [num] = the stable
 * order of keys [num] by their low key_bits bits (1 .. 32) -- bits above them never decide.  after (or NULL): a permutation
 * of 0 .. num-1 from an earlier call; the keys are then taken in that sequence, and order still holds original indices
 * (minor key first, major key after it = lexicographic order).  keys_sorted (or NULL) [num] = keys[order[j]]. */
int isf_debug_stable_sort(const uint32_t* keys, int num, int key_bits, const int32_t* after, int32_t* order,
                          uint32_t* keys_sorted, isf_stream_t stream);

/* A1  dynamic voxelization ------------------------------------------------------------------------
 * replaces voxel_layer.dynamic_voxelize(points, coors, voxel_size, coors_range, NDim=3)
 *   mmdet3d/ops/voxel/src/voxelization.h:83-95, voxelization_cuda.cu:24-61,485-528; caller
 *   mmdet3d/ops/voxel/voxelize.py:52-55.
 * points [P, C>=3] fp32 -> coors [P,3] int32 (z,y,x); rows with any axis outside the grid become
 * (-1,-1,-1) (CPU-path semantics, voxelization_cpu.cpp:8-43).  fp32 arithmetic: floor((p-min)/vs).
 * Asynchronous; no device-wide sync (the reference calls cudaDeviceSynchronize, :524). */
int isf_dynamic_voxelize(const float* points, int num_points, int num_features,
                         const float voxel_size_host[3], const float coors_range_host[6],
                         int32_t* coors, isf_stream_t stream);

/* Batched form used by ISFusionDetector.dynamic_voxelize (detectors/isfusion.py:123-146): samples
 * are concatenated, point_offsets_host[b]..[b+1] delimits sample b; writes coors4 [P,4] (b,z,y,x). */
int isf_dynamic_voxelize_batched(const float* points, const int64_t* point_offsets_host,
                                 int batch_size, int num_features, const float voxel_size_host[3],
                                 const float coors_range_host[6], int32_t* coors4,
                                 isf_stream_t stream);

/* A2  hard (deterministic) voxelization -----------------------------------------------------------
 * replaces voxel_layer.hard_voxelize(points, voxels, coors, num_points_per_voxel, voxel_size,
 *   coors_range, max_points, max_voxels, NDim=3, deterministic=True) -> int voxel_num
 *   voxelization.h:58-81, voxelization_cpu.cpp:45-144, voxelization_cuda.cu:231-373;
 *   caller voxelize.py:56-70 (outputs pre-allocated at max size and ZERO-FILLED by the caller).
 * Voxels in first-appearance order of the points, first max_points points of each in point order,
 * voxels beyond max_voxels dropped.  Writes the prefix [0, voxel_num) of voxels [max_voxels,
 * max_points, C], coors [max_voxels,3], num_points_per_voxel [max_voxels].  Synchronises once to
 * return *voxel_num_host (the reference returns the count to Python as well). */
int isf_hard_voxelize(const float* points, int num_points, int num_features,
                      const float voxel_size_host[3], const float coors_range_host[6],
                      int max_points, int max_voxels, float* voxels, int32_t* coors,
                      int32_t* num_points_per_voxel, int* voxel_num_host, isf_stream_t stream);
/* The same voxelization WITHOUT the host read-back (round 6: device-resident count): the outputs are sized for max_voxels
 * and need NOT be zeroed; rows [0, *voxel_num_device) are written completely (padding slots of a voxel as zeros), the
 * rows behind them are left untouched; *voxel_num_device (device int32) = min(voxels found, max_voxels).  Nothing waits
 * on the host: the caller reads the count when it needs it (the host mirror copies it to pinned memory behind the
 * kernels and slices the outputs after the LiDAR branch has been queued -- detector.ISFusionPtsPath.extract_pts_feat).
 * Replaces the same reference code as isf_hard_voxelize (mmdet3d/ops/voxel/src/voxelization_cuda.cu:231-373), whose
 * `voxel_num` is a host-side .item() (voxelization_cuda.cu:366-371). */
int isf_hard_voxelize_device(const float* points, int num_points, int num_features,
                             const float voxel_size_host[3], const float coors_range_host[6],
                             int max_points, int max_voxels, float* voxels, int32_t* coors,
                             int32_t* num_points_per_voxel, int32_t* voxel_num_device, isf_stream_t stream);

/* The samples of a batch in ONE pass (round 6; replaces the per-sample loop of ISFusionDetector.voxelize,
 * mmdet3d/models/detectors/isfusion.py:148-176: `for res in points: voxel_layer(res)` + cat + F.pad with the sample index):
 * points = the samples one behind the other, sample b = rows [point_offsets_host[b], point_offsets_host[b + 1]) (HOST array of
 * batch_size + 1 entries, batch_size <= 16).  Per sample exactly isf_hard_voxelize_device's result (same voxels, same order,
 * max_voxels each); the samples' voxels are written one behind the other: voxels [rows, max_points, C], coors4 [rows, 4] =
 * (sample, z, y, x), num_points_per_voxel [rows], buffers sized batch_size * max_voxels rows; voxel_num_device
 * [batch_size + 1] = voxels kept per sample, then their sum (= rows written).  Asynchronous, no host read-back. */
int isf_hard_voxelize_batched_device(const float* points, const int64_t* point_offsets_host, int batch_size,
                                     int num_features, const float voxel_size_host[3], const float coors_range_host[6],
                                     int max_points, int max_voxels, float* voxels, int32_t* coors4,
                                     int32_t* num_points_per_voxel, int32_t* voxel_num_device, isf_stream_t stream);

/* A3  DynamicScatter ------------------------------------------------------------------------------
 * replaces voxel_layer.dynamic_point_to_voxel_forward(feats, coors, reduce_type) ->
 *   [reduced_feats, out_coors, coors_map int32, reduce_count int32]
 *   voxelization.h:108-121, scatter_points_cuda.cu:183-239.
 * feats [P,C], coors [P,3] int32 (any row with a negative entry is dropped).  Outputs have capacity
 * P rows; the first *num_voxels_host rows are valid: out_coors sorted lexicographically (the order of
 * at::unique_dim(sorted=true)), coors_map[i] = voxel of point i (-1 if dropped), reduce_count.
 * Synchronises once to return the count. */
int isf_dynamic_point_to_voxel_forward(const float* feats, const int32_t* coors, int num_points,
                                       int num_feats, int reduce_type, float* reduced_feats,
                                       int32_t* out_coors, int32_t* coors_map,
                                       int32_t* reduce_count, int* num_voxels_host,
                                       isf_stream_t stream);

/* DETERMINISTIC ENTRIES (isf_*_det) ---------------------------------------------------------------------------------
 * The library accumulates floats with atomics in four places; an fp32 atomic add rounds per add, so those results depend
 * on the order in which the contributions arrive and differ run to run.  Each of the four has a sibling entry with the
 * SAME ARGUMENT LIST that accumulates exactly, in 64-bit fixed point, and is therefore independent of the arrival order:
 * bit-identical run to run and under any permutation of the contributions.  The mode is a different entry, not an option.
 *   A = a bound of |contribution| from an absmax pass over the call's inputs, A < 2^ex;
 *   N = a bound of the contributions per destination from the call's sizes;
 *   e = 62 - ceil(log2 N) - ex, formed on the device (no host sync);
 *   every contribution c is added as llrint(c * 2^e) (the scaling is exact) with a 64-bit integer atomic add into
 *   accumulators in the library's workspace; a second pass writes float(ldexp(double(S), -e)).
 * Resolution: 2^-(62 - ceil(log2 N)) of 2^ex -- finer than an fp32 sum for every N < 2^38.
 * A == 0 gives zeros.  A NON-FINITE (an inf or a NaN among the inputs A is taken from) makes EVERY ELEMENT of every
 * floating-point output of the call NaN.
 * The float sums that cross RANKS (gradient all-reduce, naiveSyncBN statistics) are made exact the same way, with N = the
 * world size and an integer collective between the passes: "Exact cross-rank sums" (isf_fixed_*_tensors, isf_fixed_sum_rows).
 *
 * isf_dynamic_point_to_voxel_forward_det: isf_dynamic_point_to_voxel_forward (voxelization.h:108-121,
 *   scatter_points_cuda.cu:183-239) with exact sums for reduce sum / mean: A = absmax(feats) (all rows), N = num_points;
 *   the mean is __fdiv_rn(sum, count) as in the default.  reduce max takes the default's path (already order-free).
 *   out_coors, coors_map and reduce_count are the default's. */
int isf_dynamic_point_to_voxel_forward_det(const float* feats, const int32_t* coors, int num_points,
                                           int num_feats, int reduce_type, float* reduced_feats,
                                           int32_t* out_coors, int32_t* coors_map,
                                           int32_t* reduce_count, int* num_voxels_host,
                                           isf_stream_t stream);

/* replaces voxel_layer.dynamic_point_to_voxel_backward(grad_feats, grad_reduced_feats, feats,
 *   reduced_feats, coors_idx, reduce_count, reduce_type)   voxelization.h:123-140,
 *   scatter_points_cuda.cu:241-308.  grad_feats [P,C] is fully overwritten.  Asynchronous. */
int isf_dynamic_point_to_voxel_backward(float* grad_feats, const float* grad_reduced_feats,
                                        const float* feats, const float* reduced_feats,
                                        const int32_t* coors_map, const int32_t* reduce_count,
                                        int num_points, int num_voxels, int num_feats,
                                        int reduce_type, isf_stream_t stream);

/* A4  DynamicVFE.forward (fused) -------------------------------------------------------------------
 * replaces DynamicVFE.forward(features, coors) for the IS-Fusion configuration
 *   (with_cluster_center, with_voxel_center, mode='max', two DynamicVFELayers, eval-mode BN)
 *   mmdet3d/models/voxel_encoders/voxel_encoder.py:453-547, utils.py:129-144.
 * points [P,Cin], coors4 [P,4] (b,z,y,x).  w1 [c1, Cin+6], w2 [c2, 2*c1] in torch Linear layout;
 * scaleN/shiftN = eval BatchNorm1d folded to y = x*scale + shift.  Outputs (capacity P rows):
 * voxel_feats [N,c2], voxel_coors [N,4] sorted by (b,z,y,x) (= per-sample unique_dim order,
 * scatter_points.py:75-96), optional pt2vox [P] (may be NULL).  Synchronises once for the count. */
int isf_dynamic_vfe_forward(const float* points, const int32_t* coors4, int num_points,
                            int in_channels, int batch_size, const float voxel_size_host[3],
                            const float coors_range_host[6], const float* w1, const float* scale1,
                            const float* shift1, int c1, const float* w2, const float* scale2,
                            const float* shift2, int c2, float* voxel_feats, int32_t* voxel_coors,
                            int32_t* pt2vox, int* num_voxels_host, isf_stream_t stream);

/* cfg-1 VFE: HardSimpleVFE.forward(features[M,T,C], num_points[M]) -> [M, num_features]
 *   voxel_encoder.py:28-45.  Asynchronous. */
int isf_hard_simple_vfe(const float* voxels, const int32_t* num_points, int num_voxels,
                        int max_points, int num_point_features, int num_features, float* out,
                        isf_stream_t stream);

/* A5  sparse-conv rulebook --------------------------------------------------------------------------
 * replaces sparse_conv_ext.get_indice_pairs_3d(indices, batch_size, out_shape, spatial_shape, ksize,
 *   stride, padding, dilation, out_padding, subm, transpose) -> [outids, indice_pairs, indice_num]
 *   mmdet3d/ops/bevfusion-ops/spconv/src/all.cc:21-51, include/spconv/spconv_ops.h:27-141,
 *   geometry.h:24-297 (same role: spconv.pytorch / mmcv.ops get_indice_pairs).
 * Native format = output-stationary neighbour table: nbr [K, nbr_stride] int32 with
 * nbr[k*nbr_stride + o] = input row feeding output row o through tap k (-1 if none), tap index
 * k = (kz*Ky + ky)*Kx + kx, in = out*stride - padding + k (cross-correlation, dilation 1).
 * SubM: outputs = inputs in the SAME row order (out_indices may be NULL).  Sparse (strided):
 * out_indices [cap,4] are written sorted by (b,z,y,x) (spconv's GPU path sorts too,
 * spconv_ops.h:130; the CPU path numbers them first-come -- irrelevant after dense()).
 * nbr_stride >= round_up(num_out, 128); the caller provides nbr with K*nbr_stride entries where
 * nbr_stride = isf_nbr_stride(capacity).  Synchronises once for *num_out_host (sparse only). */
int isf_nbr_stride(int num_rows);
int isf_conv_out_shape(const int in_shape_host[3], const int ksize_host[3],
                       const int stride_host[3], const int padding_host[3], int out_shape_host[3]);
int isf_build_rulebook(const int32_t* indices, int num_in, int batch_size,
                       const int spatial_shape_host[3], const int ksize_host[3],
                       const int stride_host[3], const int padding_host[3], int conv_type,
                       int32_t* out_indices, int out_capacity, int32_t* nbr, int nbr_stride,
                       int* num_out_host, isf_stream_t stream);

/* spconv-1 interchange format: indice_pairs [K,2,num_in] (-1 padded) + indice_num [K]
 * (what indice_conv_fp32 consumes, spconv_ops.h:260-271).  Pairs of one tap are ordered by output row. */
int isf_rulebook_to_indice_pairs(const int32_t* nbr, int nbr_stride, int num_out, int num_taps,
                                 int num_in, int32_t* indice_pairs, int32_t* indice_num,
                                 isf_stream_t stream);
int isf_indice_pairs_to_rulebook(const int32_t* indice_pairs, const int32_t* indice_num,
                                 int num_taps, int num_in, int num_out, int32_t* nbr,
                                 int nbr_stride, isf_stream_t stream);

/* A6/A7  sparse convolution forward, fused epilogue ---------------------------------------------------
 * replaces sparse_conv_ext.indice_conv_fp32(features, filters, indice_pairs, indice_num,
 *   num_act_out, inverse, subm)  (spconv_ops.h:260-361; functional.py:22-97) PLUS the
 *   BatchNorm1d(eval) / residual add / ReLU that follow it in SparseSequential / SparseBasicBlock
 *   (ops/sparse_block.py:117-134, sparse_encoder.py:75-104):
 *     y[o,:] = act( (sum_k x[nbr[k][o],:] @ W[k]) * scale + shift + residual[o,:] )
 * features [num_in,Cin]; filters [K,Cin,Cout] = the reference layout [kD,kH,kW,Cin,Cout] (conv.py:100);
 * scale/shift [Cout] (NULL = identity); residual [num_out,Cout] or NULL; relu 0/1; out [num_out,Cout].
 * Each output row is written exactly once (no scatter-add, no atomics).  Asynchronous. */
int isf_sparse_conv_forward(const float* features, int num_in, int c_in, const float* filters,
                            int num_taps, int c_out, const int32_t* nbr, int nbr_stride, int num_out,
                            const float* scale, const float* shift, const float* residual, int relu,
                            float* out, isf_stream_t stream);

/* Same with filters pre-packed by isf_pack_filters (MFMA fragment order); packed size in floats =
 * isf_packed_filter_elems(K, Cin, Cout).  Use this on the hot path: weights are static. */
size_t isf_packed_filter_elems(int num_taps, int c_in, int c_out);
int isf_pack_filters(const float* filters, int num_taps, int c_in, int c_out, float* packed,
                     isf_stream_t stream);
int isf_sparse_conv_forward_packed(const float* features, int num_in, int c_in, const float* packed,
                                   int num_taps, int c_out, const int32_t* nbr, int nbr_stride,
                                   int num_out, const float* scale, const float* shift,
                                   const float* residual, int relu, float* out, isf_stream_t stream);

/* Split-precision ("f16x3") sparse convolution -------------------------------------------------------------
 * Same contract as isf_sparse_conv_forward_packed, evaluated on the f16 matrix cores: operands are carried as
 * hi + lo f16 halves, hi = f16(v), lo = f16(v - hi), products as a_lo*b_hi + a_hi*b_lo + a_hi*b_hi with fp32
 * accumulation.  Weights are scaled by a power of two into [2^12, 2^13) before the split; ACTIVATIONS ARE NOT
 * SCALED, so the accuracy depends on their magnitude (two-sided domain; model: tests/split_model.py):
 *   2^-3 <= |a| < 65504    both halves are normal f16 numbers: 22 significant bits, relative error 2^-22 per
 *                          operand -- the accuracy of an fp32 matmul;
 *   |a| < 2^-3             the lo half is an f16 subnormal: the error is ABSOLUTE, 2^-25 per element (half a
 *                          subnormal step), i.e. relative 2^-25 / |a|; below 2^-14 the hi half is subnormal too;
 *   |a| >= 65520           hi = +inf, lo = -inf: every output that reads the element is NaN (also +-inf and NaN
 *                          inputs).  Loud and confined to those outputs, never finite-wrong; a split-stored
 *                          OUTPUT above the same threshold comes back NaN, not clamped.
 * (model - exact) / max|exact| of a 576-term dot product, N(0,1)*s activations, conv-like weights
 * (tests/test_split_model.py::test_accuracy_table prints it):
 *   max|a|      4.6     0.57    3.6e-2  4.5e-3  5.6e-4  2.8e-4  3.5e-5  4.4e-6  >= 65520
 *   rel. error  9.5e-8  1.8e-7  2.5e-6  2.1e-5  1.8e-4  3.3e-4  2.3e-3  2.0e-2  NaN
 * Activations are exchanged in the SPLIT format:
 * row-major [N, C/32] chunks of 128 bytes, a chunk = 32 channels as 4 x (8 f16 hi) followed by 4 x (8 f16 lo)
 * (same 4 bytes/element as fp32; the 16-byte pieces the four k-group lanes of an MFMA row fetch together are
 * contiguous); isf_f32_to_split / isf_split_to_f32 convert ([N, C] row-major fp32, N*C a multiple of 32).
 * Cin, Cout in {32,64,128,256}.
 * `mode` of isf_sparse_conv_forward_f16x3 (per call; there is no process-wide switch) is a set of ISF_CONV_MODE_* bits
 * (below): 0 = split precision (default);
 * ISF_CONV_MODE_F16 = single-pass f16 (opt-in): the same kernels fetch and multiply only the hi halves -- f16 operands, fp32
 * accumulate, the accuracy of the reference's indice_conv_half under fp16 autocast (BASELINE configs[4]); results are
 * still exchanged in the split format.  TIMING DIAGNOSTICS (tools/conv_knockout.sh; never in production):
 * ISF_CONV_MODE_NO_GATHER = no activation gathers, ISF_CONV_MODE_NO_WEIGHTS = no weight streaming, both = neither,
 * ISF_CONV_MODE_NO_LOOP = no main loop -- the RESULTS ARE GARBAGE, only kernel
 * times are meaningful; ISF_CONV_MODE_NO_SHARING = gather every row (no neighbour sharing): results
 * valid and bit-identical to mode 0, the reference the sharing is tested against; | ISF_CONV_MODE_UNIFORM_TILES (combinable)
 * = uniform row tiles instead
 * of the full / half-tile mix that evens out the row groups per SIMD on launches of a single round of workgroups
 * (results bit-identical: a row's products and their order do not depend on the tile it falls into).
 * Round 5, mode 0 only, results valid and bit-identical, deep (128 / 256-column) shapes: | ISF_CONV_MODE_ONE_BLOCK_4W /
 * _8W = one column block for the 256-column layers (4 x 32-row / 8 x 16-row waves), | ISF_CONV_MODE_STAGGER = staggered
 * issue phases, | ISF_CONV_MODE_R4_ISSUE = round 4's issue phase (index reads inside the step, separate weight-DMA pieces),
 * | ISF_CONV_MODE_TWO_AHEAD = gathered rows two steps ahead -- experiments
 * measured slower than the default, kept as tested opt-ins.
 * Round 6, mode 0 / | ISF_CONV_MODE_UNIFORM_TILES, c_out = 256 (other shapes ignore it): | ISF_CONV_MODE_CHUNK_SPLIT = CHUNK
 * SPLIT -- a tile is computed by two workgroups,
 * each over half of the 32-channel chunks; the second to arrive adds the other's accumulator tile and runs the epilogue.
 * Deterministic, NOT the bits of mode 0 (the sum over chunks becomes (lower half) + (upper half)); measured slower; opt-in.
 * | ISF_CONV_MODE_DEEP (mode 0 / | ISF_CONV_MODE_UNIFORM_TILES): the deep layers' 4-wave launches on isf_spconv_deep.hip
 * (LDS-DMA gathers + one instruction stream per step) -- bit-identical, measured 8 % slower (profiles/r06_deep.txt); opt-in.
 * Workgroup shape (mode 0 / | ISF_CONV_MODE_UNIFORM_TILES; chosen per launch from c_out and num_out, never changes a
 * result): 4 waves x 32 rows and two
 * 128-column blocks for c_out = 256, 8 waves x 32 rows for c_out = 128 from 2048 rows up; launches the tile plan would cut
 * into half tiles only (c_out = 256: num_out <= 96 x CUs; c_out = 128: 2048 <= num_out <= 256 x CUs) run with 16 rows per
 * wave instead.  ISF_CONV_MODE_NO_SHARING keeps the 32-row shapes: the bit-equality reference of
 * that rule too.
 * Bits 64 and 1024 of the same int are hand-overs between the library's own translation units, named in
 * csrc/isf_spconv16.h; callers do not set them. */
#define ISF_CONV_MODE_F16 1               /* single-pass f16: hi halves only, fp32 accumulation */
#define ISF_CONV_MODE_NO_GATHER 2         /* timing knock-out: no activation gathers (results garbage) */
#define ISF_CONV_MODE_NO_WEIGHTS 4        /* timing knock-out: no weight streaming (results garbage; 6 = 2 | 4 = neither) */
#define ISF_CONV_MODE_NO_LOOP 8           /* timing knock-out: no main loop (results garbage) */
#define ISF_CONV_MODE_NO_SHARING 16       /* gather every row, no neighbour sharing (bit-identical) */
#define ISF_CONV_MODE_UNIFORM_TILES 32    /* uniform row tiles, no full / half-tile mix (bit-identical; combinable); in the engine
                                             also equal-row XCD parts for the launches of several rounds */
#define ISF_CONV_MODE_F16_ROWS 256        /* rows are plain f16; accepted only as ISF_CONV_MODE_F16_STORAGE */
#define ISF_CONV_MODE_F16_STORAGE 257     /* ISF_CONV_MODE_F16_ROWS | ISF_CONV_MODE_F16: f16 storage, see below */
#define ISF_CONV_MODE_DMA_PLAN 2048       /* isf_sparse_conv_tile_order: the table is for isf_sparse_conv_forward_dma's plan */
#define ISF_CONV_MODE_ONE_BLOCK_4W 4096   /* 256-column layers as one column block, 4 waves x 32 rows (slower; opt-in) */
#define ISF_CONV_MODE_ONE_BLOCK_8W 8192   /* 256-column layers as one column block, 8 waves x 16 rows (slower; opt-in) */
#define ISF_CONV_MODE_DEEP 32768          /* deep layers' 4-wave launches on isf_spconv_deep.hip (8 % slower; opt-in) */
#define ISF_CONV_MODE_STAGGER 65536       /* staggered issue phases in the deep layers' workgroups (slower; opt-in) */
#define ISF_CONV_MODE_R4_ISSUE 131072     /* round 4's issue phase: the A/B partner of the default (slower; opt-in) */
#define ISF_CONV_MODE_TWO_AHEAD 262144    /* gathered rows two steps ahead (slower; opt-in) */
#define ISF_CONV_MODE_CHUNK_SPLIT 524288  /* two workgroups per tile, half the chunks each (not mode 0's bits; slower; opt-in) */
size_t isf_packed_filter16_bytes(int num_taps, int c_in, int c_out);
int isf_pack_filters_f16x3(const float* filters, int num_taps, int c_in, int c_out, void* packed16,
                           isf_stream_t stream);
/* ... from the per-tap TRANSPOSE: filters_t [num_taps, c_out, c_in] -- e.g. the forward filter when the packed one (c_in x c_out
 * = forward c_out x c_in) is the data gradient's, dX = dY W_k^T: no transposed copy of the weights per layer and step */
/* ... the filters of a DATA GRADIENT with headroom: isf_pack_filters_f16x3_transposed whose inv_scale carries a further
 * 2^-e, e = max(0, ceil(log2 gain) - 5), gain = max over the c_out columns of sum |w|: gradient rows scaled to max |g| < 2^10
 * (isf_grad_to_split) then give split rows |dX| <= 2^15, inside f16's range whatever the filters' magnitude.  room (device
 * float[2]) = {2^e, 2^-e}: multiply the result by room[0] (isf_split_to_f32_scaled2).  Same launches as the plain pack. */
int isf_pack_filters_dx(const float* filters_t, int num_taps, int c_in, int c_out, void* packed16, float* room,
                        isf_stream_t stream);
int isf_pack_filters_f16x3_transposed(const float* filters_t, int num_taps, int c_in, int c_out, void* packed16,
                                      isf_stream_t stream);
int isf_f32_to_split(const float* x, size_t num_elems, void* xs, isf_stream_t stream);
int isf_split_to_f32(const void* xs, size_t num_elems, float* x, isf_stream_t stream);
/* f16 STORAGE (mode ISF_CONV_MODE_F16_STORAGE of isf_sparse_conv_forward_f16x3; isf_encoder_options.precision = 2): features,
 * residual and output rows are plain f16, [N, C] row-major, 2 bytes per element -- the data type of the reference's
 * indice_conv_half / indice_conv_backward_half end to end (mmdet3d/ops/bevfusion-ops/spconv/src/all.cc:35-37; BASELINE
 * configs[4] "fp16, HBM-bound") -- with f16 operands and fp32 accumulation; every layer moves half the activation
 * bytes of the split format.  isf_f32_to_half / isf_half_to_f32 convert (num_elems a multiple of 8). */
int isf_f32_to_half(const float* x, size_t num_elems, void* xh, isf_stream_t stream);
int isf_half_to_f32(const void* xh, size_t num_elems, float* x, isf_stream_t stream);
int isf_sparse_conv_forward_f16x3(const void* features_split, int num_in, int c_in, const void* packed16,
                                  int num_taps, int c_out, const int32_t* nbr, int nbr_stride, int num_out,
                                  const float* scale, const float* shift, const void* residual_split, int relu,
                                  void* out_split, int mode, isf_stream_t stream);
/* TILE ORDER of a launch that is resident in one round of workgroups.  Such a launch ends when its busiest CU does; the
 * tiles a CU gets in launch order (slots j, j + 32, j + 64 of its XCD) add up unevenly because the work of a tile -- the
 * (16-row group, tap) pairs that have a neighbour -- varies ~3x across a LiDAR sweep.  isf_sparse_conv_tile_order counts
 * that work per tile of the launch isf_sparse_conv_forward_f16x3 would make for (c_in, c_out, mode, num_out) and hands
 * the tiles out longest-first to the least-loaded CU with a free slot; `order` (and the scratch `work`) hold at most
 * 8 * 255 ints, *num_entries = how many were written (0: the launch is not a single round -- pass order = NULL).  A
 * table belongs to ONE kernel's launch plan: mode | ISF_CONV_MODE_DMA_PLAN builds it for isf_sparse_conv_forward_dma (whose workgroups per
 * CU, and with them the tiles, differ from isf_sparse_conv_forward_f16x3's on the same shape).
 * One table serves every layer of that channel shape on the rulebook (isf_sparse_encoder_forward builds it per level
 * behind the neighbour table).  isf_sparse_conv_forward_f16x3_ordered = the same convolution with workgroup slot j
 * working on tile order[j]: results bit-identical to isf_sparse_conv_forward_f16x3 (the same tiles compute the same
 * rows).  Replaces nothing in the reference (its gather -> GEMM -> scatter has no tiles); measured in DESIGN.md
 * section 5.1.  isf_sparse_conv_trace: DIAGNOSTIC -- the production launch of a 128 -> 128 or 256 -> 256 layer that also
 * writes 8 int64 per workgroup (trace [trace_capacity_blocks * 8], zero it first; a launch of more workgroups than the
 * buffer holds is refused: 100 MHz time stamps at entry / after the
 * prologue / after the multiply loop / at exit, steps, HW_ID, XCC_ID, first row | half tile << 32); tools/conv_trace.py. */
int isf_sparse_conv_tile_order(const int32_t* nbr, int nbr_stride, int num_taps, int num_out, int c_in, int c_out,
                               int mode, int32_t* work, int32_t* order, int* num_entries, isf_stream_t stream);
int isf_sparse_conv_forward_f16x3_ordered(const void* features_split, int num_in, int c_in, const void* packed16,
                                          int num_taps, int c_out, const int32_t* nbr, int nbr_stride, int num_out,
                                          const float* scale, const float* shift, const void* residual_split, int relu,
                                          void* out_split, int mode, const int32_t* order, isf_stream_t stream);
/* TILE TABLE of a launch that is resident in one round of workgroups (levels 3 / 4: 2.5 tiles per compute unit).  Uniform
 * tiles carry 3x different matrix work (scene density), so the launch ends with its densest CU.  isf_sparse_conv_tile_table
 * deals the 16-row groups of every XCD's row range to that XCD's compute units as contiguous runs of about EQUAL WORK
 * (taps with a neighbour per group) and cuts a CU's run into full tiles plus one remainder tile, slot = where the
 * dispatcher places it: table [parts][workgroups per CU * CUs per XCD][2] = (first group, groups), a buffer of 3072 ints
 * (8 parts x 2 x 192 slots per XCD; a launch that would need more is refused with ISF_ERR_UNSUPPORTED, never written past the
 * buffer); scratch holds 2 * ceil(num_out / 16) ints; *num_ints = ints written (0: the launch is not one round -- use the
 * plain entry).
 * isf_sparse_conv_forward_f16x3_tiled runs the convolution over it: BIT-IDENTICAL results (a row's products and their
 * order do not depend on the tile it falls into); the table belongs to one (c_in, c_out, mode): the workgroup shape depends
 * on all three.  MEASURED SLOWER than uniform tiles + isf_sparse_conv_tile_order on the MI355X (256 -> 256: 1.32 vs 1.265 ms
 * per step; profiles/r04_tile_tables.txt, profiles/EXPERIMENTS.md section 5.4: a tile's time follows its STEP count, not its matrix
 * work), so it is an OPT-IN: isf_sparse_encoder_forward builds the tables with ISF_ENC_DIAG_TILE_TABLES.
 * isf_sparse_conv_tile_table_host: the same arithmetic on the host (tests). */
int isf_sparse_conv_tile_table(const int32_t* nbr, int nbr_stride, int num_taps, int num_out, int c_in, int c_out,
                               int mode, int32_t* scratch, int32_t* table, int* num_ints, isf_stream_t stream);
int isf_sparse_conv_forward_f16x3_tiled(const void* features_split, int num_in, int c_in, const void* packed16,
                                        int num_taps, int c_out, const int32_t* nbr, int nbr_stride, int num_out,
                                        const float* scale, const float* shift, const void* residual_split, int relu,
                                        void* out_split, int mode, const int32_t* table, isf_stream_t stream);
int isf_sparse_conv_tile_table_host(const int32_t* work, int num_groups, int part_groups, int parts, int cus, int wgs_per_cu,
                                    int groups_per_tile, int32_t* tiles, int* fits);
int isf_sparse_conv_trace(const void* features_split, int num_in, int c_in, const void* packed16, int num_taps,
                          int c_out, const int32_t* nbr, int nbr_stride, int num_out, const float* scale,
                          const float* shift, const void* residual_split, int relu, void* out_split,
                          const int32_t* order, long long* trace, int trace_capacity_blocks, int* grid_blocks,
                          isf_stream_t stream);
/* DIAGNOSTIC: isf_sparse_conv_trace plus per-WAVE phase stamps of every step of the multiply loop (shader clock,
 * s_memtime: 1 tick = 1 shader cycle): top of the step / after its s_waitcnt vmcnt(0) / after the barrier / after issuing
 * the next step's loads; the multiply section is what is left until the next top.  This image's rocprofv3 has no
 * thread-trace decoder (--att: "rocprof-trace-decoder library path not found"), so this is the instruction-level account of
 * the dominant kernel.  trace: [*grid_blocks][8] int64 as isf_sparse_conv_trace, then per wave (*waves_per_block per
 * workgroup) *dwords_per_wave uint32: {clock at loop entry lo, hi, HW_ID, steps, tap mask of row group 0, of row group 1,
 * tap mask of the workgroup, clock at loop exit lo} + 4 per step; trace_bytes is checked against the launch (zero the
 * buffer first).  tools/conv_phase_trace.py -> profiles/r05_att_256.txt. */
int isf_sparse_conv_phase_trace(const void* features_split, int num_in, int c_in, const void* packed16, int num_taps,
                                int c_out, const int32_t* nbr, int nbr_stride, int num_out, const float* scale,
                                const float* shift, const void* residual_split, int relu, void* out_split,
                                const int32_t* order, long long* trace, size_t trace_bytes, int* grid_blocks,
                                int* waves_per_block, int* dwords_per_wave, isf_stream_t stream);

/* DIAGNOSTIC: the per-workgroup trace of the NARROW layers' kernel (isf_sparse_conv_forward_dma / _dma_lines; c_in,
 * c_out in {32, 64}): one production launch with 16 int64 per workgroup -- constant-clock (100 MHz) stamps at entry / after
 * the prologue / after the multiply loop / at exit, steps, HW_ID, XCC_ID, first row | half tile << 32, then wave 0's
 * shader-clock cycles summed over the steps: at the per-step vmcnt(0), at the barrier, in the section that reads the
 * transit / weight buffers and issues the next step's loads, in the multiply section; [12], [13]: of the third, the fragment
 * reads' LDS round trip and the index arithmetic + weight run (the rest: the row gathers).  table / mask: the dense neighbour
 * table (mask NULL, taps_per_line ignored) or the line-compressed one.  tools/conv_trace.py --level 0 | 1. */
int isf_sparse_conv_dma_trace(const void* features_split, int num_in, int c_in, const void* packed16, int num_taps,
                              int taps_per_line, int c_out, const int32_t* table, const uint32_t* mask, int nbr_stride,
                              int num_out, const float* scale, const float* shift, const void* residual_split, int relu,
                              void* out_split, long long* trace, int trace_capacity_blocks, int* grid_blocks,
                              isf_stream_t stream);
/* the same launch on a part table (isf_sparse_conv_part_table below): the trace of the equal-work plan */
int isf_sparse_conv_dma_trace_parts(const void* features_split, int num_in, int c_in, const void* packed16, int num_taps,
                                    int taps_per_line, int c_out, const int32_t* table, const uint32_t* mask, int nbr_stride,
                                    int num_out, const float* scale, const float* shift, const void* residual_split, int relu,
                                    void* out_split, const int32_t* part_table, long long* trace, int trace_capacity_blocks,
                                    int* grid_blocks, isf_stream_t stream);
/* EQUAL-WORK PARTS for the launches of several rounds of workgroups (round 7).  A launch that does
 * not fit the chip in one round runs uniform tiles, dealt to the 8 XCDs as 8 (4 with two column blocks) parts of equal
 * ROWS; the steps a tile walks vary 4x with the density of the scene, an XCD cannot give work away, and the launch ends
 * with the XCD that was dealt the most.  isf_sparse_conv_part_table builds, on the device and without a read-back, the
 * PART TABLE of the launch the given kernel would make: the SAME uniform tiles dealt to the XCDs as contiguous runs of
 * equal weight (steps + a measured constant per tile), every run at most `cap` tiles, and inside a run the tiles of the
 * heaviest of four work classes first (tile order inside a class).  Layout: first tile of every part [parts + 1] | class
 * bounds [3] | slots [parts][cap] (tile or -1).  mode: the conv's base mode (0 | ISF_CONV_MODE_F16 |
 * ISF_CONV_MODE_F16_STORAGE), | ISF_CONV_MODE_DMA_PLAN for the LDS-DMA kernel's plan (mask: NULL for a dense table, the
 * tap masks for a line-compressed one).  flags: 1 = treat the launch as one of several rounds whatever its size (tests),
 * 2 = slots in tile order, 4 = the plain plan's equal-row parts (A/B of the order alone).  work: 2 x tiles ints of scratch (the tile weights come first); info: {parts, cap, tiles,
 * table ints}, all 0 when the launch is one round (no table is built: run the plain entry point).
 * isf_sparse_conv_forward_parts runs the launch on the table: every row is computed by the same tile with the same
 * products in the same order -- results BIT-IDENTICAL to the plain entry points, which keep the equal-row plan.
 * isf_sparse_encoder_forward / isf_lidar_branch_forward build these tables for their launches of several rounds. */
int isf_sparse_conv_part_table(const int32_t* table_nbr, const uint32_t* mask, int nbr_stride, int num_taps, int num_out,
                               int c_in, int c_out, int mode, int flags, int32_t* work, int work_capacity, int32_t* part_table,
                               int table_capacity, int* info, isf_stream_t stream);
int isf_sparse_conv_forward_parts(const void* features_split, int num_in, int c_in, const void* packed16, int num_taps,
                                  int taps_per_line, int c_out, const int32_t* table_nbr, const uint32_t* mask, int nbr_stride,
                                  int num_out, const float* scale, const float* shift, const void* residual_split, int relu,
                                  void* out_split, int mode, const int32_t* part_table, isf_stream_t stream);
/* The same convolution for the NARROW layers (c_in, c_out in {32, 64}) with the gathered rows brought in by LDS-DMA
 * (isf_spconv_dma.hip; mode 0 | ISF_CONV_MODE_F16 | ISF_CONV_MODE_F16_STORAGE, | ISF_CONV_MODE_UNIFORM_TILES; order: NULL or isf_sparse_conv_tile_order's table).  A gather instruction of
 * isf_sparse_conv_forward_f16x3 loads straight into the MFMA operand layout -- four different rows = four cache lines per
 * lane quad: 64 address-unit cycles -- and on the narrow layers (few MFMAs per gathered row) the address unit sets the
 * step time.  Here a quad fetches the 64 contiguous bytes of ONE row (16 cycles) into a wave-private LDS transit buffer
 * and the MFMA layout is produced by the LDS read; no neighbour table in LDS, 5-6 workgroups per CU.  Results are
 * BIT-IDENTICAL to isf_sparse_conv_forward_f16x3 (same products in the same order per accumulator);
 * isf_sparse_encoder_forward / isf_lidar_branch_forward run their narrow layers on it (ISF_ENC_DIAG_NARROW_GATHER: gather kernel).
 * Replaces the reference's gather stage (bevfusion-ops/spconv/include/spconv/reordering.cu.h:21-97) for those layers. */
int isf_sparse_conv_forward_dma(const void* features_split, int num_in, int c_in, const void* packed16, int num_taps,
                                int c_out, const int32_t* nbr, int nbr_stride, int num_out, const float* scale,
                                const float* shift, const void* residual_split, int relu, void* out_split, int mode,
                                const int32_t* order, isf_stream_t stream);
/* LINE-COMPRESSED neighbour table (narrow layers).  The taps of one (kz, ky) line of a 3-wide kernel probe x-adjacent cells
 * and rows are sorted by (b, z, y, x), so the neighbours a row has through a line are CONSECUTIVE rows: one int32 per line
 * (the row of the first present neighbour, -1 if none) + one bit per tap say everything the dense table says --
 *   lines [num_taps / taps_per_line][nbr_stride] int32, mask [nbr_stride] uint32 (bit k: tap k present),
 *   nbr[k][o] = mask[o] bit k ? lines[k / tpl][o] + popcount(mask[o] bits of that line below k) : -1
 * -- in 40 bytes per row (3 x 3 x 3) instead of 108: the dense table of a narrow layer is as many bytes per row as a
 * 32-channel activation row, read twice per convolution (tap masks, then indices).  Only tables in rank order qualify
 * (what isf_build_rulebook produces for sorted inputs; isf_rulebook_to_lines sets *not_consecutive_flag (device int, may be
 * NULL) to 1 for any other table).  isf_rulebook_to_lines / isf_lines_to_rulebook convert; isf_sparse_conv_forward_dma_lines
 * = isf_sparse_conv_forward_dma reading the compressed table (a lane keeps its rows' masks in registers and loads one
 * index per LINE): results BIT-IDENTICAL.  isf_sparse_encoder_forward / isf_lidar_branch_forward build the tables of their
 * narrow levels directly in this form (ISF_ENC_DIAG_DENSE_TABLES: dense tables).  taps_per_line = kernel width (1 or 3).
 * Replaces nothing in the reference (its rulebook is pair lists, indice.cu.h:22-203); measured in DESIGN.md section 5.3. */
int isf_rulebook_to_lines(const int32_t* nbr, int nbr_stride, int num_taps, int taps_per_line, int num_out,
                          int32_t* lines, uint32_t* mask, int* not_consecutive_flag, isf_stream_t stream);
int isf_lines_to_rulebook(const int32_t* lines, const uint32_t* mask, int nbr_stride, int num_taps, int taps_per_line,
                          int32_t* nbr, isf_stream_t stream);
int isf_sparse_conv_forward_dma_lines(const void* features_split, int num_in, int c_in, const void* packed16, int num_taps,
                                      int taps_per_line, int c_out, const int32_t* lines, const uint32_t* mask,
                                      int nbr_stride, int num_out, const float* scale, const float* shift,
                                      const void* residual_split, int relu, void* out_split, int mode,
                                      isf_stream_t stream);
/* The same convolution for the 256-COLUMN layers (c_out = 256, c_in in {128, 256}: levels 3 / 4 of the encoder) as ONE
 * WORKGROUP PER COMPUTE UNIT (isf_spconv_cu.hip).  A level-3 launch is 160 rows x 256 columns per CU: cut into 128 x 128
 * tiles it ends with its busiest CU (1.4x the mean work: the density of a LiDAR sweep varies 3x) and every tile streams
 * its own weight stage.  isf_sparse_conv_cu_plan cuts the rows of a rulebook into units of whole 16-row groups with EQUAL
 * matrix work (taps with a neighbour per group; <= 256 rows; cus * r units) -- plan_buf holds
 * isf_sparse_conv_cu_plan_ints(num_out) int32, the plan struct points into it, no host sync (the grid is sized by
 * max_units) -- once per rulebook; isf_sparse_conv_forward_cu runs one workgroup per unit over ALL 256 output columns; the
 * production variant (variant 0 = kCuWavesProd) is FOUR waves, wave w owns columns [64 w, 64 w + 64) (256 accumulator
 * registers = the AGPR half of the file; variants 6 / 7 are the 8-wave x 32-column shape), its weight fragments go
 * global -> VGPR (no LDS, one stream per CU instead of one per tile), the gathered rows come in by LDS-DMA once per CU
 * through a ring of prefetch depth + 1 stages.  Results are
 * BIT-IDENTICAL to isf_sparse_conv_forward_f16x3 (mode 0).  MEASURED SLOWER than the tile kernel on the MI355X (256 -> 256:
 * 1.39 .. 1.50 ms per step against 1.26; profiles/r04_cu_kernel_ab.txt, profiles/EXPERIMENTS.md section 5.2), so it is an OPT-IN:
 * isf_sparse_encoder_forward / isf_lidar_branch_forward run their 256-column layers on it with ISF_ENC_DIAG_CU_KERNEL.  isf_sparse_conv_cu_plan_host / _max_units: the plan
 * arithmetic on the host (tests, tools; no device work): work [num_groups] -> units [max_units][2] = (first group, groups).
 * Replaces the reference's per-tap gather -> GEMM -> scatter-add (spconv_ops.h:260-361) for those layers. */
typedef struct isf_conv_cu_plan {
  const int32_t* group_masks;   /* device [ceil(num_out / 16)] */
  const int32_t* units;         /* device [*num_units][2] */
  const int32_t* num_units;     /* device scalar */
  int max_units;                /* host bound of *num_units */
  int num_out;                  /* rows the plan was built for */
  int variant;                  /* 0 = production.  DIAGNOSTICS: 1 / 2 / 3 = no gathers / no weight loads / neither (TIMING
                                   ONLY, results garbage); 4 / 5 = 4-wave workgroups at prefetch depth 1 / 2 steps, 6 / 7 =
                                   8-wave workgroups at depth 1 / 2 (results valid); round 6, hand-scheduled assembly
                                   multiply phase: 8 = 8 waves, one workgroup per CU; 9 / 10 = two 4-wave workgroups per
                                   CU over units of <= 8 groups at depth 1 / 2 (valid); 11-15 their knock-outs (timing
                                   only).  isf_sparse_conv_cu_plan READS this field: the variant decides the unit shape */
  int cap;                      /* groups per unit the plan was cut for (16 or 8); set by isf_sparse_conv_cu_plan */
} isf_conv_cu_plan;
int isf_sparse_conv_cu_plan_ints(int num_out, size_t* num_ints);
int isf_sparse_conv_cu_plan(const int32_t* nbr, int nbr_stride, int num_taps, int num_out, int32_t* plan_buf,
                            isf_conv_cu_plan* plan, isf_stream_t stream);
int isf_sparse_conv_forward_cu(const void* features_split, int num_in, int c_in, const void* packed16, int num_taps,
                               int c_out, const int32_t* nbr, int nbr_stride, int num_out, const float* scale,
                               const float* shift, const void* residual_split, int relu, void* out_split,
                               const isf_conv_cu_plan* plan, isf_stream_t stream);
int isf_sparse_conv_cu_plan_host(const int32_t* work, int num_groups, int cus, int32_t* units, int max_units,
                                 int* num_units);
int isf_sparse_conv_cu_max_units(int num_groups, int cus);
/* The same convolution with the tile's input rows staged in LDS ("LDS staging of active-voxel tiles"; the reference's
 * gather stage: bevfusion-ops/spconv/include/spconv/reordering.cu.h:21-97 -> staging buffer -> GEMM, spconv_ops.h:300-345).
 * isf_rulebook_stage_tables derives the staging tables of a neighbour table once per rulebook: for every unit of
 * isf_stage_unit_rows() (64) consecutive output rows, ulist [nbr_stride / 64][isf_stage_unit_cap()] = the distinct
 * input rows the unit's taps name (ascending), ucount [nbr_stride / 64] = how many, and slots [num_taps][nbr_stride]
 * (uint16) = the position of nbr[k][o] in its unit's list, 0xFFFF where nbr is -1.  isf_sparse_conv_forward_staged
 * copies the listed rows global -> LDS once per tile and 32-channel chunk (row-coalesced LDS-DMA) and reads the A
 * operands of all taps from LDS; `stage_rows` = LDS rows per 128-row tile (clamped to what 160 KiB hold; list entries
 * beyond a unit's share are gathered from memory, so every value is correct).  Results are bit-identical to
 * isf_sparse_conv_forward_f16x3 (same products, same order).  mode: 0 | ISF_CONV_MODE_F16, | ISF_CONV_MODE_UNIFORM_TILES. */
int isf_stage_unit_rows(void);
int isf_stage_unit_cap(void);
int isf_rulebook_stage_tables(const int32_t* nbr, int nbr_stride, int num_taps, uint16_t* slots, int32_t* ulist,
                              int32_t* ucount, isf_stream_t stream);
int isf_sparse_conv_forward_staged(const void* features_split, int num_in, int c_in, const void* packed16,
                                   int num_taps, int c_out, const uint16_t* slots, int nbr_stride,
                                   const int32_t* ulist, const int32_t* ucount, int num_out, const float* scale,
                                   const float* shift, const void* residual_split, int relu, void* out_split,
                                   int stage_rows, int mode, isf_stream_t stream);
/* A7  SparseConvTensor.dense() + view(N, C*D, H, W) ---------------------------------------------------
 * replaces structure.py:49-59 + sparse_encoder.py:133-136: out[b, c*D+z, y, x] = feats[i,c], zeros
 * elsewhere; out [B, C*D, H, W] is written completely (no separate memset).  Asynchronous. */
int isf_sparse_to_dense_bev(const float* features, const int32_t* indices, int num_rows, int channels,
                            int batch_size, int D, int H, int W, float* out, isf_stream_t stream);

/* A7  whole SparseEncoder.forward in one call -----------------------------------------------------------
 * replaces SparseEncoder.forward(voxel_features, coors, batch_size)
 *   mmdet3d/models/middle_encoders/sparse_encoder.py:107-138 (eval-mode BN folded).
 * A plan is an ordered list of conv layers; SubM layers at one resolution share one rulebook. */
typedef struct isf_conv_layer {
  int conv_type;       /* ISF_CONV_SUBM | ISF_CONV_SPARSE */
  int ksize[3], stride[3], padding[3];
  int c_in, c_out;
  const float* packed; /* device: isf_pack_filters output (fp32 MFMA path) */
  const void* packed16; /* device: isf_pack_filters_f16x3 output, or NULL (then the fp32 path runs) */
  const float* scale;  /* device [c_out] */
  const float* shift;  /* device [c_out] */
  int relu;            /* apply ReLU at the end */
  int residual_from;   /* -2 none; -1 the encoder input; i>=0 output of layer i (added before ReLU) */
} isf_conv_layer;

typedef struct isf_encoder_stats { /* filled on the host after the call (for roofline accounting) */
  int num_layers;
  int num_in[32], num_out[32];
  long long pairs[32]; /* sum over taps of valid (in,out) pairs of layer i */
  float ms[32];        /* hipEvent time of layer i's conv kernel when timing was requested, else 0 */
  int precision;       /* 0 = fp32 MFMA kernels ran, 1 = f16x3 split-precision MFMA kernels ran */
} isf_encoder_stats;

/* per-call options of the two engine entry points (NULL = all defaults; no process-wide state):
 * precision  0 = f16x3 split MFMA when every layer carries packed16, else fp32 MFMA (default); 1 = force the fp32 MFMA
 *            kernels; 2 = f16 storage + single-pass f16 arithmetic (opt-in, the reference's fp16 mode: activations are
 *            f16 rows between the layers, mode ISF_CONV_MODE_F16_STORAGE of isf_sparse_conv_forward_f16x3);
 * diagnostic timing diagnostics of the conv kernels: 0 = off, else a set of ISF_ENC_DIAG_* bits (below).
 *            _NO_GATHER / _NO_WEIGHTS / both / _NO_LOOP / _NO_SHARING, | _UNIFORM_TILES: the conv mode bits of the same
 *            value, see isf_sparse_conv_forward_f16x3;
 *            _LAUNCH_ORDER = tiles in launch order, no isf_sparse_conv_tile_order tables; _NARROW_GATHER = narrow layers on
 *            the gather kernel instead of isf_sparse_conv_forward_dma; _VFE_FP32_ROWS (isf_lidar_branch_forward) = the voxel
 *            encoder writes fp32 rows and a conversion pass makes the split rows, instead of writing them directly;
 *            _CU_KERNEL = the 256-column layers on isf_sparse_conv_forward_cu (one workgroup per CU; opt-in: measured
 *            slower than the tile kernel) -- results bit-identical either way;
 *            | v << ISF_ENC_DIAG_CU_VARIANT_SHIFT = isf_conv_cu_plan.variant v of those layers (timing diagnostics, v < 16);
 *            _DENSE_TABLES = dense neighbour tables for the narrow layers instead of the line-compressed ones -- bit-identical;
 *            _COUNTS_MEMCPY = the encoder's per-level row counts reach the host through hipMemcpyAsync + synchronise
 *            instead of the pinned-memory mailbox (post_int / wait_int) -- bit-identical;
 *            _VOXELIZE_PER_FRAME (isf_lidar_branch_forward) = one dynamic-voxelize launch per frame + a separate byte-map
 *            marking pass instead of the fused voxelize + mark launch -- bit-identical;
 *            _TILE_TABLES = equal-work tile tables for the deep levels instead of uniform tiles + tile order (opt-in:
 *            measured slower) -- bit-identical;
 *            layers run on the gather kernel whenever a diagnostic other than _UNIFORM_TILES is set.
 *            Round 5 (all bit-identical to the default, all measured SLOWER, kept as tested opt-ins):
 *            _ONE_BLOCK_4W / _ONE_BLOCK_8W = the 256-column layers as ONE column block, 4 x 32-row / 8 x 16-row waves
 *            (ISF_CONV_MODE_ONE_BLOCK_4W / _8W); _STAGGER = staggered issue phases inside the deep layers' workgroups
 *            (ISF_CONV_MODE_STAGGER); _TWO_AHEAD = the gathered rows two steps ahead (ISF_CONV_MODE_TWO_AHEAD); _R4_ISSUE =
 *            round 4's issue phase (row-index reads inside the step, four separate weight-DMA pieces;
 *            ISF_CONV_MODE_R4_ISSUE) -- the A/B partner of the default, which reads the
 *            indices one step ahead and stages a wave's weight share as one run.
 *            Round 6: _CHUNK_SPLIT = the 256-column layers with the chunk split (ISF_CONV_MODE_CHUNK_SPLIT): valid,
 *            deterministic, not the default's bits, measured slower (opt-in): 256 -> 256 0.223 -> 0.256 ms per launch,
 *            1 030 -> 980 frames/s (profiles/EXPERIMENTS.md) -- the launch is bound by what its workgroups move through the
 *            CUs' vector-memory paths in total, not by its longest chain (216 steps against an average of 136); a second
 *            prologue per tile and the exchange add to that.
 *            _DEEP = the deep layers on isf_spconv_deep.hip (ISF_CONV_MODE_DEEP; LDS-DMA gathers + one instruction stream
 *            per step): bit-identical, 8 % slower, opt-in.
 *            _BAND_ORDER = the launches of several rounds take their tiles band by band in y (opt-in; bit-identical):
 *            measured slower on the benchmark's scenes (one dominant ground plane per frame: 64 -> 32 0.135 -> 0.154,
 *            32 -> 32 0.27 -> 0.29, 64 -> 64 0.694 -> 0.709 ms per step, profiles/r06_band_order.txt) -- row order already
 *            keeps a plane's y-neighbours together.
 *            _NO_ROW_SORT = the row sort of the deep SubM launches (rows of a tile / a 16-row group with the same tap mask)
 *            off (A/B; bit-identical either way).  _NARROW_ROW_SORT = the row sort for the NARROW layers too (LDS-DMA
 *            kernel, line-compressed tables; opt-in): 33 % fewer tile-taps at level 0 on paper, no gain measured (64 -> 64
 *            0.703 -> 0.719, 32 -> 32 0.272 -> 0.276 ms per step: those layers are bound by their gathers, and like rows are
 *            further apart), profiles/r06_row_sort.txt.  _SORT_KEY_AB = sort key 2 (coarse | in-plane taps) instead of
 *            key 1 (six coarse bits, one radix pass) (A/B).  (Sixteen taps of the planes above / below as the key, two
 *            passes, made the 256-column launches 0.8 % faster, 1.131 vs 1.140 ms per step, and their fabric traffic 37 %
 *            larger, FETCH_SIZE 226 -> 311 MB per launch: finer key groups scatter a tile's rows over the grid -- not kept.)
 *            _NARROW_TILES = the 128-column layers of the large levels on the 4-wave 128-row tile instead of the 8-wave
 *            256-row one (A/B; bit-identical). */
#define ISF_ENC_DIAG_NO_GATHER 2               /* -> ISF_CONV_MODE_NO_GATHER */
#define ISF_ENC_DIAG_NO_WEIGHTS 4              /* -> ISF_CONV_MODE_NO_WEIGHTS */
#define ISF_ENC_DIAG_NO_LOOP 8                 /* -> ISF_CONV_MODE_NO_LOOP */
#define ISF_ENC_DIAG_NO_SHARING 16             /* -> ISF_CONV_MODE_NO_SHARING */
#define ISF_ENC_DIAG_UNIFORM_TILES 32          /* -> ISF_CONV_MODE_UNIFORM_TILES; combines with all others; also: the launches of
                                                  several rounds keep equal-ROW XCD parts (their part tables keep the plain cuts) */
#define ISF_ENC_DIAG_LAUNCH_ORDER 64           /* tiles in launch order, no tile-order tables; also: the part tables of the
                                                  launches of several rounds keep tile order inside a part */
#define ISF_ENC_DIAG_NARROW_GATHER 128         /* narrow layers on the gather kernel, not the LDS-DMA kernel */
#define ISF_ENC_DIAG_VFE_FP32_ROWS 256         /* isf_lidar_branch_forward: fp32 voxel rows + a conversion pass */
#define ISF_ENC_DIAG_CU_KERNEL 512             /* 256-column layers on the one-workgroup-per-CU kernel (slower; opt-in) */
#define ISF_ENC_DIAG_CU_VARIANT_SHIFT 10       /* bits 10-13: isf_conv_cu_plan.variant of the CU kernel */
#define ISF_ENC_DIAG_CU_VARIANT_MASK 15360     /* 15 << ISF_ENC_DIAG_CU_VARIANT_SHIFT */
#define ISF_ENC_DIAG_DENSE_TABLES 16384        /* dense neighbour tables for the narrow layers */
#define ISF_ENC_DIAG_TILE_TABLES 32768         /* equal-work tile tables for the deep levels (slower; opt-in) */
#define ISF_ENC_DIAG_VOXELIZE_PER_FRAME 65536  /* isf_lidar_branch_forward: one voxelize launch per frame */
#define ISF_ENC_DIAG_COUNTS_MEMCPY 131072      /* row counts by hipMemcpyAsync + synchronise, not the mailbox */
#define ISF_ENC_DIAG_ONE_BLOCK_4W 262144       /* -> ISF_CONV_MODE_ONE_BLOCK_4W (256-column layers) */
#define ISF_ENC_DIAG_ONE_BLOCK_8W 524288       /* -> ISF_CONV_MODE_ONE_BLOCK_8W (256-column layers) */
#define ISF_ENC_DIAG_STAGGER 1048576           /* -> ISF_CONV_MODE_STAGGER (deep layers) */
#define ISF_ENC_DIAG_R4_ISSUE 2097152          /* -> ISF_CONV_MODE_R4_ISSUE (deep layers) */
#define ISF_ENC_DIAG_TWO_AHEAD 4194304         /* -> ISF_CONV_MODE_TWO_AHEAD (deep layers) */
#define ISF_ENC_DIAG_DEEP 8388608              /* -> ISF_CONV_MODE_DEEP (deep layers) */
#define ISF_ENC_DIAG_BAND_ORDER 16777216       /* band order for the launches of several rounds (slower; opt-in); its order is
                                                  cut for equal-row parts: no part tables with it */
#define ISF_ENC_DIAG_NO_ROW_SORT 33554432      /* row sort of the deep launches off (A/B) */
#define ISF_ENC_DIAG_NARROW_ROW_SORT 67108864  /* row sort for the narrow layers too (no gain; opt-in); sorted inside equal-row
                                                  parts: the narrow launches keep them (no part tables) */
#define ISF_ENC_DIAG_SORT_KEY_AB 134217728     /* row sort key 2 instead of key 1 (A/B) */
#define ISF_ENC_DIAG_NARROW_TILES 268435456    /* 128-column layers of the large levels on 4-wave tiles (A/B) */
#define ISF_ENC_DIAG_CHUNK_SPLIT 536870912     /* -> ISF_CONV_MODE_CHUNK_SPLIT (256-column layers; opt-in) */
#define ISF_ENC_DIAG_BEV_ONE_PASS (1 << 30)    /* 1073741824: the fp32 BEV map written whole by the final kernel, zeros included,
                                                  instead of zeros early on the geometry stream + occupied 16-cell segments
                                                  last (A/B and bit-identity reference; bit-identical) */
typedef struct isf_encoder_options {
  int precision;
  int diagnostic;
  int stage_rows;  /* LDS-staged input rows per 128-row conv tile (isf_sparse_conv_forward_staged); 0 = the library's
                      per-layer default, -1 = staging off (every layer on the gather kernel) */
  int stage_mask;  /* with stage_rows > 0: bit i = layer i runs staged (tuning); 0 = every layer */
  int bev_format;  /* spatial_features: 0 = fp32 [B, C*D, H, W] (the reference's layout, sparse_encoder.py:137-139);
                      1 = the same map as split-format token matrices, one per 256-channel group: group g at byte offset
                      g * B*H*W * 1024, [B*H*W, 256] in the split activation format (token = (b*H + y)*W + x, channel
                      c*D + z) -- what the fusion encoder's convolutions read (isf_sparse_conv_forward_f16x3 over
                      isf_dense_grid_rulebook): no isf_nchw_to_split pass.  Same byte count; precision 0 only */
} isf_encoder_options;

int isf_sparse_encoder_forward(const float* voxel_features, const int32_t* coors, int num_voxels,
                               int batch_size, const int sparse_shape_host[3],
                               const isf_conv_layer* layers_host, int num_layers,
                               float* spatial_features, /* [B, C_last*D_last, H_last, W_last] */
                               int out_shape_host[4],   /* C*D, H, W and N_last (may be NULL) */
                               isf_encoder_stats* stats_host /* may be NULL */, int time_layers,
                               const isf_encoder_options* options /* may be NULL */, isf_stream_t stream);

/* LiDAR branch in one call: dynamic voxelize + DynamicVFE + SparseEncoder (isfusion.py:103-111) */
typedef struct isf_vfe_params {
  int in_channels, c1, c2;
  const float *w1, *scale1, *shift1, *w2, *scale2, *shift2; /* device */
  float voxel_size[3], coors_range[6];
} isf_vfe_params;

int isf_lidar_branch_forward(const float* points, const int64_t* point_offsets_host, int batch_size,
                             const isf_vfe_params* vfe_host, const int sparse_shape_host[3],
                             const isf_conv_layer* layers_host, int num_layers,
                             float* spatial_features, int out_shape_host[4],
                             isf_encoder_stats* stats_host, int time_layers,
                             const isf_encoder_options* options /* may be NULL */, isf_stream_t stream);

/* The same call over frames that are NOT concatenated: frame_points_host[b] is the device pointer of frame b's
 * [P_b, in_channels] fp32 block (contiguous rows; 4-byte alignment suffices, so a view into a larger buffer will do; may be
 * NULL for a frame without points), point_offsets_host the running sums of the P_b as above.  Saves the caller's
 * concatenation pass (a read and a write of every point).  batch_size <= 8; larger batches: concatenate and call
 * isf_lidar_branch_forward.  Results are bit-identical to the concatenated call. */
int isf_lidar_branch_forward_frames(const float* const* frame_points_host, const int64_t* point_offsets_host, int batch_size,
                                    const isf_vfe_params* vfe_host, const int sparse_shape_host[3],
                                    const isf_conv_layer* layers_host, int num_layers,
                                    float* spatial_features, int out_shape_host[4],
                                    isf_encoder_stats* stats_host, int time_layers,
                                    const isf_encoder_options* options /* may be NULL */, isf_stream_t stream);

/* ===================================================================================================
 * HSF / IGF rows (A8, A10-A14).  Dense 3x3 convolutions around them stay stock
 * PyTorch-ROCm ops (north_star); everything below is what the reference runs through custom CUDA ops
 * or long chains of small torch kernels.
 * =================================================================================================== */

/* nn.Linear with fused epilogue -----------------------------------------------------------------------
 * replaces F.linear + bias + {GELU | ReLU} + residual add + LayerNorm chains of
 *   mmdet3d/models/sst/sst_basic_block_v2.py:104-126 (EncoderLayer), backbones/sst_v2.py:83 (linear0),
 *   middle_encoders/fusion_encoder.py:560-600 (MSDeformAttn projections), :653-674 (decoder layer FFN),
 *   :221-470 (MultiheadAttention in/out projections), :489-496 (Instane2SceneAtt).
 * isf_pack_linear splits weight [out, in] (torch layout) once into f16 hi/lo MFMA fragments.
 * y[r, :] = LN( act( x[r, :] . W^T + bias + row_table[row_table_index[r], :] ) + residual[r, :] )
 *   activation: 0 none, 1 ReLU, 2 GELU(erf);  LN only when ln_gamma != NULL (out_features <= 256).
 * in_features in {32,64,128,256}; out_features % 16 == 0; ldx % 8 == 0. */
size_t isf_packed_linear_bytes(int out_features, int in_features);
int isf_pack_linear(const float* weight, int out_features, int in_features, void* packed, isf_stream_t stream);
/* ... from the transpose: weight_t [in_features, out_features] row-major (the forward weight, for dX = dY W) */
int isf_pack_linear_transposed(const float* weight_t, int out_features, int in_features, void* packed, isf_stream_t stream);
int isf_linear_forward(const float* x, int num_rows, int in_features, int ldx, const void* packed_weight,
                       int out_features, const float* bias, const float* row_table, const int32_t* row_table_index,
                       int activation, const float* residual, const float* ln_gamma, const float* ln_beta,
                       float ln_eps, float* y, int ldy, int x_hw, int residual_hw, int y_hw, isf_stream_t stream);
/* x_hw / residual_hw / y_hw: 0 = row-major [num_rows, C]; hw > 0 = the tensor is channels-first [B, C, hw] with row
 * r = b*hw + pos (a BEV map [B, C, H, W], hw = H*W, hw % 4 == 0): the NCHW <-> token transposes of
 * fusion_encoder.py:1163, sst_v2.py:97-133 and :480-496 happen inside the GEMM's loads / stores. */

/* A10/A11  the attention half of an SST encoder layer in ONE kernel on the matrix cores -------------------------------
 * replaces, for the fusion encoder's dense grids (every cell a token, row = (b*S + y)*S + x), the whole of
 *   WindowAttention.forward + the residual / norm1 of EncoderLayer.forward (models/sst/sst_basic_block_v2.py:41-75,
 *   :104-116) incl. flat2window / window2flat / the position embedding add (ops/sst/sst_ops.py:63-143, 219-268):
 *     y = LayerNorm( x + out_proj( softmax(q k^T / sqrt(hd)) v ) ),  q, k = in_proj(x + pos), v = in_proj(x)
 * x, y [B*S*S, d] fp32; in_proj_bias [3d]; pos_table [window^2, 3d] = pos_embed @ in_proj_weight[:2d]^T (zeros in the
 * v columns); packed = isf_pack_window_block(in_proj_weight [3d, d], out_proj_weight [d, d]); shift as in
 * isf_window_attention_forward.  q, k, v, scores and the attention output never reach memory.  8 heads, 6x6 windows,
 * d = 128 (the 180 x 180 level; the d = 256 level runs linear -> isf_window_attention_forward -> linear, which
 * measured faster there). */
size_t isf_packed_window_block_bytes(int embed_dims);
int isf_pack_window_block(const float* in_proj_weight, const float* out_proj_weight, int embed_dims, int num_heads,
                          void* packed, isf_stream_t stream);
int isf_window_block_forward(const float* x, int batch_size, int grid_size, int embed_dims, int num_heads, int window,
                             int shift, const void* packed, const float* in_proj_bias, const float* pos_table,
                             const float* out_proj_bias, const float* ln_gamma, const float* ln_beta, float ln_eps,
                             float* y, isf_stream_t stream);

/* A10/A11  window attention core on a dense token grid (the unfused form; training uses it) -------------------
 * replaces get_window_coors / flat2window / nn.MultiheadAttention / window2flat of
 *   mmdet3d/ops/sst/sst_ops.py:219-268, 63-143 and models/sst/sst_basic_block_v2.py:41-75
 * for the fusion encoder's dense grids (fusion_encoder.py:1151-1189: every cell is a token, token row =
 * (b*S + y)*S + x).  qkv [B*S*S, 3*d] = (q | k | v) projections (q, k of x + pos, v of x);
 * shift 0: windows aligned at 0, shift 1: windows offset by -window/2 (partial edge windows attend among the
 * cells they hold).  out [B*S*S, d] = softmax(q k^T / sqrt(hd)) v per head, heads concatenated. */
int isf_window_attention_forward(const float* qkv, int batch_size, int grid_size, int embed_dims, int num_heads,
                                 int window, int shift, float* out, isf_stream_t stream);

/* A13/A14  multi-head attention core --------------------------------------------------------------------
 * replaces the softmax(QK^T)V part of multi_head_attention_forward (fusion_encoder.py:371-470; the head's
 * cross attention, transfusion_head_v2.py:104-108): q [B*Lq, ldq], k / v [B*Lk, ldkv] (already projected; head h =
 * columns h*hd..), out [B*Lq, ldo].  head_dim 16 (the IS-Fusion configuration): matrix-core kernel, keys resident in
 * LDS (up to 512 per workgroup; more keys are split and merged); head_dim 32: fp32 vector kernels.  Asynchronous. */
int isf_attention_forward(const float* q, int ldq, const float* k, const float* v, int ldkv, int batch_size,
                          int num_queries, int num_keys, int embed_dims, int num_heads, float* out, int ldo,
                          isf_stream_t stream);
/* ... in TRAINING mode with nn.MultiheadAttention's dropout on the attention probabilities (fusion_encoder.py:458
 * F.dropout(attn_output_weights, p); the IGF modules use p = 0.1, :476, :614): a probability is zeroed with probability
 * dropout_p and the kept ones scaled by 1 / (1 - dropout_p); the row normalisation keeps every term.  The keep / drop
 * decision of (sample * heads + head, query, key) is a counter-based hash of `seed` (MurmurHash3's finaliser over the
 * packed indices; isf_attention_backward_dropout recomputes it from the same seed), so no mask is stored.  dropout_p = 0
 * is isf_attention_forward.  With dropout_p > 0: head_dim 16, any number of keys (more than 512: the 512-key splits and
 * the merge of isf_attention_forward, each split hashing its global key indices), and the hash's index fields bound the
 * sizes: num_queries < 2^24, num_keys < 2^24, batch_size * num_heads < 2^16.  Outside this domain both entries return
 * ISF_ERR_UNSUPPORTED, naming the value, before anything else is looked at. */
int isf_attention_forward_dropout(const float* q, int ldq, const float* k, const float* v, int ldkv, int batch_size,
                                  int num_queries, int num_keys, int embed_dims, int num_heads, float dropout_p,
                                  unsigned long long seed, float* out, int ldo, isf_stream_t stream);

/* A14  per-channel map attention -----------------------------------------------------------------------
 * replaces fusion_encoder.py:497-502: for each of num_maps = B*C maps (size x size, row-major)
 *   out = query_scene + softmax(query_scene . query_ins^T, dim=-1) . query_ins */
int isf_channel_attention_forward(const float* query_scene, const float* query_ins, int num_maps, int size,
                                  float* out, isf_stream_t stream);
/* ... and its gradient (training): replaces what autograd runs behind fusion_encoder.py:495-500 -- the backward of the
 * two torch.matmul calls and of the softmax between them, with the [B, C, size, size] probabilities saved by the forward.
 * Nothing is saved here: per map, with A = query_scene[m], Bm = query_ins[m], G = grad_out[m] (size x size, row-major)
 *   P  = softmax(A Bm^T, dim = -1)                  (recomputed, fp32 MFMA, row maximum subtracted)
 *   gP = G Bm^T
 *   gS = P o (gP - rowsum(gP o P))
 *   gA = G + gS Bm                                   -> grad_query_scene[m]
 *   gB = P^T G + gS^T A                              -> grad_query_ins[m]
 * Domain: the forward's (size % 4 == 0, size <= 192; anything else is ISF_ERR_UNSUPPORTED, checked before any HIP call).
 * Either output may be NULL: the work only it needs is skipped and the other output has the bits of the full call (both
 * NULL: nothing is launched).  Deterministic (no atomics, fixed summation order); map m's result does not depend on
 * num_maps or on the other maps.  Scratch: P and gS of up to 256 maps at a time (2 * 256 * size^2 floats at most, 66 MB
 * at size 180) from the stream's workspace -- more maps are processed in groups of 256 in order, fewer per group if the
 * device cannot provide that much; grad_query_ins = NULL needs none.  Asynchronous. */
int isf_channel_attention_backward(const float* query_scene, const float* query_ins, const float* grad_out,
                                   int num_maps, int size, float* grad_query_scene /* may be NULL */,
                                   float* grad_query_ins /* may be NULL */, isf_stream_t stream);

/* A8  Point-to-Grid sampling ------------------------------------------------------------------------------
 * replaces ISFusionEncoder.img_fv_to_bev + img_point_sampling (fusion_encoder.py:965-1070).
 * pillars [M, slots, pillar_ld] (x, y, z first; zero-padded slots are sampled like the reference does),
 * pillar_coors [M, 4] (b, z, y, x); img_nhwc [B*num_cam, feat_h, feat_w, C]; cam_params [B*num_cam, 20]:
 *   M(3x3) = lidar2img[:3,:3] . inv(lidar_aug[:3,:3]), v(3) = lidar2img[:3,3] - M . lidar_aug[:3,3],
 *   A(2x3) = img_aug[:2,:3], a(2) = img_aug[:2,3]   (host-side 4x4 algebra, see fusion_ops.p2g_camera_params)
 * out [B, C, bev, bev] is written completely (zeros where no pillar). */
int isf_p2g_forward(const float* pillars, int pillar_ld, int slots, const int32_t* pillar_coors, int num_pillars,
                    const float* img_nhwc, int batch_size, int num_cam, int feat_h, int feat_w, int channels,
                    const float* cam_params, int input_h, int input_w, int bev_size, float* out,
                    isf_stream_t stream);
/* ... with the result as ONE split-format token matrix [B*bev*bev, 256] (token = (b*bev + y)*bev + x; channels == 256; the
 * same bytes as the fp32 map, written completely): what conv_fusion reads (dense grid convolution on
 * isf_sparse_conv_forward_f16x3) -- no isf_nchw_to_split pass, and a pillar's 256 values leave the wave as one KiB. */
int isf_p2g_forward_split(const float* pillars, int pillar_ld, int slots, const int32_t* pillar_coors, int num_pillars,
                          const float* img_nhwc, int batch_size, int num_cam, int feat_h, int feat_w, int channels,
                          const float* cam_params, int input_h, int input_w, int bev_size, void* out_split,
                          isf_stream_t stream);

/* A12  instance mining: sigmoid + 3x3 NMS + top-k -------------------------------------------------------
 * replaces fusion_encoder.py:1100-1131.  heatmap [B, K, H, W] logits; classes with bit set in
 * pool1_class_mask use a 1x1 pool (every cell is its own maximum).  top_index [B, k] = flat index % (H*W),
 * top_index_raw [B, k] = flat index over (K, H, W), both in descending score order (ties: ascending index);
 * masked_heatmap [B, K*H*W] optional (NULL to skip). */
int isf_instance_topk(const float* heatmap, int batch_size, int num_classes, int height, int width, int k,
                      unsigned pool1_class_mask, int32_t* top_index, int32_t* top_index_raw, float* masked_heatmap,
                      isf_stream_t stream);

/* A13  multi-scale deformable attention with the op signature of mmcv -----------------------------------------
 * replaces ext_module.ms_deform_attn_forward(value, value_spatial_shapes, value_level_start_index,
 *   sampling_locations, attention_weights, im2col_step)
 *   (mmdet3d/models/middle_encoders/multi_scale_deformable_attn_function.py:118-124; kernel
 *   ms_deform_im2col_cuda.cuh:237-299); im2col_step only blocks the reference's batch loop and has no counterpart.
 * value [B, num_keys, heads, hd]; spatial_shapes [L, 2] int64 (h, w); level_start_index [L] int64;
 * sampling_loc [B, Q, heads, L, P, 2] (x, y) in [0, 1]; attn_weight [B, Q, heads, L, P] (post-softmax);
 * out [B, Q, heads*hd].  Any head_dim / level / point count. */
int isf_ms_deform_attn_forward(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                               const float* sampling_loc, const float* attn_weight, int batch_size, int num_keys,
                               int num_heads, int head_dim, int num_queries, int num_levels, int num_points,
                               float* out, isf_stream_t stream);

/* ... and its backward, with the op's own contract:
 * replaces ext_module.ms_deform_attn_backward(value, value_spatial_shapes, value_level_start_index,
 *   sampling_locations, attention_weights, grad_output, grad_value, grad_sampling_loc, grad_attn_weight, im2col_step)
 *   (multi_scale_deformable_attn_function.py:150-160; kernels ms_deform_im2col_cuda.cuh:301-920).
 * grad_output [B, Q, heads*hd]; grad_value [B, num_keys, heads, hd], grad_sampling_loc [B, Q, heads, L, P, 2] and
 * grad_attn_weight [B, Q, heads, L, P] are ZEROED BY THE CALLER (as the reference does, :142-144) and accumulated
 * into.  isf_msda_backward is the fused single-level form the mirror's InsContextAtt trains through. */
int isf_ms_deform_attn_backward(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                const float* sampling_loc, const float* attn_weight, const float* grad_output,
                                int batch_size, int num_keys, int num_heads, int head_dim, int num_queries,
                                int num_levels, int num_points, float* grad_value, float* grad_sampling_loc,
                                float* grad_attn_weight, isf_stream_t stream);

/* isf_ms_deform_attn_backward with exact accumulation (DETERMINISTIC ENTRIES above; same reference interface,
 * multi_scale_deformable_attn_function.py:150-160).  grad_value: A = absmax(grad_output) * max(1, absmax(attn_weight)),
 * N = num_queries * num_points.  A power-of-two head_dim <= 64 adds each grad_sampling_loc / grad_attn_weight element
 * once (order-free as it is); any other head_dim accumulates them in fixed point too: A = 2 * num_keys *
 * absmax(grad_output) * absmax(value) * max(1, absmax(attn_weight)), N = head_dim.  The three gradients are still
 * ZEROED BY THE CALLER and added to (one fp32 add per element). */
int isf_ms_deform_attn_backward_det(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                    const float* sampling_loc, const float* attn_weight, const float* grad_output,
                                    int batch_size, int num_keys, int num_heads, int head_dim, int num_queries,
                                    int num_levels, int num_points, float* grad_value, float* grad_sampling_loc,
                                    float* grad_attn_weight, isf_stream_t stream);

/* A10  in-group (in-window) indices -------------------------------------------------------------------------
 * replaces TorchEx ingroup_indices.forward(group_inds, out_inds)
 *   (mmdet3d/ops/TorchEx/torchex/src/ingroup_inds/ingroup_inds.cpp:24-54, ingroup_inds_kernel.cu:17-31; called by
 *   get_inner_win_inds_cuda, ops/sst/sst_ops.py:197-211): out_inds[i] = a distinct number in [0, count(group of i))
 *   for every element.  The reference hands the numbers out with atomicAdd (any order); here out_inds[i] is the
 *   number of EARLIER elements of the same group -- one of the reference's possible results, and deterministic.
 * group_inds / out_inds [num] int64 (torch.long, as the reference op takes them). */
int isf_ingroup_indices(const int64_t* group_inds, int num, int64_t* out_inds, isf_stream_t stream);

/* A13  fused single-level form used by the InsContextAtt path -------------------------------------------------
 * replaces MultiScaleDeformableAttnFunction.forward (mmdet3d/ops/.../ms_deform_attn, called at
 * fusion_encoder.py:597) plus the softmax / location arithmetic of :585-596.
 * value [B, H*W, heads*hd]; sampling_offsets [B*Q, heads*P*2]; attention_logits [B*Q, heads*P] (pre-softmax);
 * reference_points [B*Q, 2] (x, y) in [0, 1]; out [B*Q, heads*hd]. */
int isf_msda_forward(const float* value, const float* sampling_offsets, const float* attention_logits,
                     const float* reference_points, int batch_size, int num_queries, int num_heads, int head_dim,
                     int num_points, int height, int width, float* out, isf_stream_t stream);

/* 8f #1  box decoding (detection-head post-processing) ---------------------------------------------------
 * replaces TransFusionHeadV2.get_bboxes with nms_type=None (dense_heads/transfusion_head_v2.py:1278-1312,1344-1418)
 * including TransFusionBBoxCoder.decode(filter=True) (core/bbox/coders/transfusion_bbox_coder.py:39-124).
 * heatmap / query_score [B, classes, ld] (the first num_proposals columns of each row are used; heatmap = logits),
 * query_labels [B, P] int64, center [B,2,ld] (BEV cells), height [B,1,ld], dim [B,3,ld] (log metres), rot [B,2,ld]
 * (sin, cos), vel [B,2,ld] or NULL.  coder = 12 HOST floats: out_size_factor*voxel_size (x, y), pc_range (x, y),
 * post_center_range (6), score_threshold, apply_threshold (0/1; the reference tests `if self.score_threshold:`, so 0.0
 * is not applied).  Outputs, compacted per sample in proposal order: boxes [B, P, 9 | 7 without vel]
 * (x, y, z_bottom, dx, dy, dz, yaw, vx, vy), scores [B, P], labels [B, P] int32, counts [B] = boxes kept. */
int isf_decode_boxes(const float* heatmap, const float* query_score, const int64_t* query_labels, const float* center,
                     const float* height, const float* dim, const float* rot, const float* vel, int batch_size,
                     int num_classes, int num_proposals, int ld, const float* coder, float* boxes, float* scores,
                     int32_t* labels, int32_t* counts, isf_stream_t stream);

/* 8f #1  proposal initialisation / prediction outputs of the detection head ------------------------------------
 * isf_head_query_init replaces the tensor ops of TransFusionHeadV2.forward_single between the top-k and the first
 *   decoder layer (dense_heads/transfusion_head_v2.py:806-842): query_labels = top // HW, query_pos = bev_pos[top % HW],
 *   query = feature column + class_encoding(one_hot(label)), the first layer's self_posembed(query_pos) as a row of a
 *   per-cell table, query + position, and query_heatmap_score = heatmap.gather(top % HW) (:888-890).
 *   top_index / top_raw [B, P] int32 as isf_instance_topk writes them; feat_tok [B*HW, E] token-major;
 *   tok_of_cell [HW] int64 (BEV cell -> token row inside a sample) or NULL = identity; class_table [classes, E] =
 *   class_encoding.weight[:, c] + bias; qpe_table [HW, E] or NULL (then qpe / x are not written); bev_pos [HW, 2];
 *   masked [B, classes * HW] = the suppressed heat-map.  Outputs: query / qpe / x [B*P, E], query_pos [B, P, 2],
 *   top_index64 / query_labels [B, P] int64, query_score [B, classes, P].
 * isf_head_scatter_predictions replaces the per-output transposes of FFN.forward's results (:505-590), `center +=
 *   query_pos` (:883) and `query_pos = center.detach().clone()` (:885): output h = columns [col0[h], col0[h] +
 *   channels[h]) of the token-major block src[h] [B*P, src_ld[h]] -> dst[h] [B, channels[h], P]; center_head (or -1)
 *   gets query_pos [B, P, 2] added and is copied to query_pos_next [B, P, 2] (or NULL).  The four arrays and src / dst
 *   are HOST arrays of num_heads (<= 8) entries.  Both asynchronous. */
int isf_head_query_init(const int32_t* top_index, const int32_t* top_raw, int batch_size, int num_proposals, int hw,
                        int embed, int num_classes, const float* feat_tok, const int64_t* tok_of_cell,
                        const float* class_table, const float* qpe_table, const float* bev_pos, const float* masked,
                        float* query, float* qpe, float* x, float* query_pos, int64_t* top_index64,
                        int64_t* query_labels, float* query_score, isf_stream_t stream);
int isf_head_scatter_predictions(int num_heads, const float* const* src, const int* src_ld, const int* col0,
                                 const int* channels, float* const* dst, int center_head, const float* query_pos,
                                 float* query_pos_next, int batch_size, int num_proposals, isf_stream_t stream);

/* A12/A13  the mined instances' features and positions ---------------------------------------------------------
 * replaces the tensor ops of ISFusionEncoder.instance_fusion after the top-k (middle_encoders/fusion_encoder.py:
 *   1133-1141: x_ins = x_scene.gather(top), query_pos = bev_pos.gather(top)) and InsContextAtt.forward's preamble
 *   (:800-812: positions / bev_size, query_pos_embed, features + embedding).
 * top [B, Q] int32: flat cells y'*S + x' of the TRANSPOSED map (isf_instance_topk on the transposed heat-map);
 * scene [B, E, S, S] in the un-transposed orientation (cell x'*S + y'); qpe_table [S*S, E] = query_pos_embed of every
 * create_2D_grid cell.  Outputs: top64 / cell64 [B, Q] int64 (the transposed / un-transposed cell), tokens, qpe,
 * tokens_pos = tokens + qpe [B*Q, E], query_pos [B, Q, 2] = (x' + .5, y' + .5), ref = query_pos / S.  Asynchronous. */
int isf_instance_gather(const int32_t* top, int batch_size, int num_instances, int bev_size, int embed,
                        const float* scene, const float* qpe_table, int64_t* top64, int64_t* cell64, float* tokens,
                        float* qpe, float* tokens_pos, float* query_pos, float* ref, isf_stream_t stream);

/* 8f #2  sparse convolution backward ------------------------------------------------------------------------
 * replaces sparse_conv_ext.indice_conv_backward_fp32(features, filters, out_bp, indice_pairs, indice_num, inverse,
 *   subm) -> [input_bp, filters_bp]   (spconv_ops.h:363-456; SparseConvFunction.backward, functional.py:38-52).
 * isf_transpose_rulebook: nbr_t [K, nbr_t_stride] with nbr_t[k][j] = o  <=>  nbr[k][o] = j (-1 elsewhere);
 *   nbr_t_stride = isf_nbr_stride(num_in).  Built once per rulebook, shared by the convs that share it.
 * isf_sparse_conv_backward_input: grad_in [num_in, Cin] = sum_k grad_out[nbr_t[k][j], :] @ W[k]^T, every row written
 *   once (the forward kernel over the transposed table; no scatter-add, no atomics).
 * isf_sparse_conv_backward_filter: grad_filters [K, Cin, Cout] = sum_o features[nbr[k][o], :]^T grad_out[o, :]
 *   (fp32 MFMA, deterministic two-pass reduction over row chunks).  filters in the reference layout [K, Cin, Cout].
 * All asynchronous. */
int isf_transpose_rulebook(const int32_t* nbr, int nbr_stride, int num_out, int num_taps, int num_in,
                           int32_t* nbr_t, int nbr_t_stride, isf_stream_t stream);
int isf_sparse_conv_backward_input(const float* grad_out, int num_out, int c_out, const float* filters, int num_taps,
                                   int c_in, const int32_t* nbr_t, int nbr_t_stride, int num_in, float* grad_in,
                                   isf_stream_t stream);
int isf_sparse_conv_backward_filter(const float* features, int num_in, int c_in, const float* grad_out, int num_out,
                                    int c_out, const int32_t* nbr, int nbr_stride, int num_taps,
                                    float* grad_filters, isf_stream_t stream);
/* Round 5: the FILTER gradient on the f16 matrix cores (isf_spconv_wgrad16.hip), the half instantiation of the reference's
 * indice_conv_backward (spconv_ops.h:363-456 with T = half, all.cc:35-51) carried at fp32 accuracy by the f16x3 split.
 * isf_rulebook_pair_lists: the neighbour table -> the spconv-1 interchange format the reference's backward walks,
 *   indice_pairs [K, 2, capacity] (input rows, output rows of a tap's pairs, ordered by output row, -1 padded for at
 *   least 32 entries past the count) + indice_num [K]; capacity = isf_pair_list_capacity(num_in, num_out) (a multiple of
 *   32).  Same content as isf_rulebook_to_indice_pairs (whose second dimension is num_in), built by a two-pass ordered
 *   compaction over 2048-row blocks instead of one workgroup per tap.  Once per rulebook.
 * isf_grad_to_split: grad [n] fp32 -> split rows of grad * s, s = the power of two that brings max|grad| into
 *   [2^9, 2^10) (non-finite entries do not set it); scale_out (device float[2]) = {s, 1 / s}.  Gradients of 1e-6 .. 1e-9
 *   would otherwise lie in f16's subnormal range.  No host sync.
 * isf_grad_rescale: the same scale with fp32 rows out (out = grad * s; the fused linear's dX GEMM splits its input itself):
 *   two launches instead of the nine torch ops of the round-2 form (_lib.pow2_rescale), ~50 calls per training step.
 * isf_split_to_f32_scaled: split rows -> fp32 * *mul (device scalar, NULL = 1): the way back for dX.
 * isf_sparse_conv_backward_filter_f16x3: grad_filters [K, Cin, Cout] = (*grad_inv_scale) * sum over the pairs of tap k of
 *   x[in]^T dY[out], x and dY in the split format (x: what the forward pass stored; dY: isf_grad_to_split), products as
 *   x_lo*g_hi + x_hi*g_lo + x_hi*g_hi on v_mfma_f32_16x16x32_f16 with fp32 accumulation; Cin, Cout in {32, 64, 128, 256};
 *   pair chunks -> partial blocks -> ordered second pass: deterministic.  mode 0 = that (fp32-class); ISF_WGRAD_F16 = SINGLE-PASS
 *   f16: only the hi halves are read and multiplied -- fp16 operands, fp32 accumulation: the arithmetic of the reference's
 *   indice_conv_backward<at::Half>, which is what its sparse convolutions run under autocast (functional.py:24
 *   custom_fwd(cast_inputs=torch.half)); the forward / dX counterpart is ISF_CONV_MODE_F16 of isf_sparse_conv_forward_f16x3 / _dma.
 *   | ISF_WGRAD_FULL_TAPS: every tap's pair list is full (the rulebook of a dense grid, dense_train.py) -- larger reduction chunks (same
 *   sums, chunk boundaries move; still deterministic).  All asynchronous. */
#define ISF_WGRAD_F16 1       /* single-pass f16: hi halves only */
#define ISF_WGRAD_FULL_TAPS 2 /* every tap's pair list is full (dense grid): larger reduction chunks */
int isf_pair_list_capacity(int num_in, int num_out);
int isf_rulebook_pair_lists(const int32_t* nbr, int nbr_stride, int num_out, int num_taps, int capacity,
                            int32_t* indice_pairs, int32_t* indice_num, isf_stream_t stream);
int isf_grad_to_split(const float* grad, size_t num_elems, void* grad_split, float* scale_out, isf_stream_t stream);
int isf_grad_rescale(const float* grad, size_t num_elems, float* out, float* scale_out, isf_stream_t stream);
int isf_split_to_f32_scaled(const void* xs, size_t num_elems, const float* mul, float* x, isf_stream_t stream);
/* ... * *mul * *mul2 (either may be NULL = 1): the gradient's scale and the dX filters' headroom (isf_pack_filters_dx) */
int isf_split_to_f32_scaled2(const void* xs, size_t num_elems, const float* mul, const float* mul2, float* x,
                             isf_stream_t stream);
int isf_sparse_conv_backward_filter_f16x3(const void* features_split, int num_in, int c_in, const void* grad_out_split,
                                          int num_out, int c_out, const int32_t* indice_pairs, const int32_t* indice_num,
                                          int capacity, int num_taps, const float* grad_inv_scale, float* grad_filters,
                                          int mode, isf_stream_t stream);

/* Round 5: BatchNorm1d with BATCH statistics (+ residual, + ReLU) on [N, C] fp32 rows, forward and backward
 * (isf_bn_train.hip) -- the norm / activation of the reference's sparse blocks and DynamicVFE layers in TRAINING mode:
 * nn.BatchNorm1d / naiveSyncBN1d.forward (ops/norm.py:136-211) + ReLU (+ the identity add of SparseBasicBlock,
 * ops/sparse_block.py:117-134), and what autograd derives for them.  channels = 4 * a divisor of 256.
 *   isf_bn1d_stats: stats [2C] = (sum x, sum x^2) per channel (partial sums per block -> ordered second level:
 *     deterministic).  The caller all-reduces stats (and the row count) across ranks for sync-BN.
 *   isf_bn1d_apply: y = relu?(x * gamma * invstd + beta - mean * gamma * invstd + residual?), mean / var from stats /
 *     count; running_mean / running_var (may be NULL) += momentum * (batch - running), the variance unbiased (nn.BatchNorm1d)
 *     or biased (naiveSyncBN1d) by unbiased_running_var; mean_invstd [2C] saved for the backward pass.
 *   isf_bn1d_backward_sums: sums [2C] = (sum g, sum g * xhat), g = grad_y masked by y_relu > 0 (y_relu NULL: no ReLU).
 *   isf_bn1d_backward_apply: grad_x = gamma * invstd * (g - sum_g / count - xhat * sum_gx / count); grad_residual (may be
 *     NULL) = g; grad_gamma = sum_gx, grad_beta = sum_g (may be NULL).  All asynchronous. */
int isf_bn1d_stats(const float* x, int num_rows, int channels, float* stats, isf_stream_t stream);
int isf_bn1d_apply(const float* x, int num_rows, int channels, const float* stats, float count, const float* gamma,
                   const float* beta, float eps, float momentum, int unbiased_running_var, float* running_mean,
                   float* running_var, const float* residual, int relu, float* y, float* mean_invstd, isf_stream_t stream);
/* The same two with the sums taken ABOUT A PIVOT ROW (pivot [C], device; NULL = 0): stats = (sum (x - p), sum (x - p)^2),
 * mean = p + sum / count, var = sumsq / count - (sum / count)^2 -- any pivot gives the same statistics in exact arithmetic,
 * a pivot near the mean (the host mirror passes the batch's first row) keeps fp32 from cancelling when |mean| >> std, as
 * torch's native batch_norm does with its two-pass variance (the single-process nn.BatchNorm1d case; the multi-rank
 * naiveSyncBN keeps pivot NULL = the reference's E[x^2] - E[x]^2 of ops/norm.py:186-190). */
int isf_bn1d_stats_pivot(const float* x, int num_rows, int channels, const float* pivot, float* stats, isf_stream_t stream);
int isf_bn1d_apply_pivot(const float* x, int num_rows, int channels, const float* stats, const float* pivot, float count,
                         const float* gamma, const float* beta, float eps, float momentum, int unbiased_running_var,
                         float* running_mean, float* running_var, const float* residual, int relu, float* y,
                         float* mean_invstd, isf_stream_t stream);
/* ... which also adds 1 to the module's num_batches_tracked (int64 device scalar, NULL = none) inside the same launch */
int isf_bn1d_apply_pivot_counted(const float* x, int num_rows, int channels, const float* stats, const float* pivot, float count,
                                 const float* gamma, const float* beta, float eps, float momentum, int unbiased_running_var,
                                 float* running_mean, float* running_var, long long* num_batches_tracked,
                                 const float* residual, int relu, float* y, float* mean_invstd, isf_stream_t stream);
int isf_bn1d_backward_sums(const float* grad_y, const float* x, const float* y_relu, int num_rows, int channels,
                           const float* mean_invstd, float* sums, isf_stream_t stream);
int isf_bn1d_backward_apply(const float* grad_y, const float* x, const float* y_relu, int num_rows, int channels,
                            const float* mean_invstd, const float* gamma, const float* sums, float count, float* grad_x,
                            float* grad_residual, float* grad_gamma, float* grad_beta, isf_stream_t stream);

/* thin-K linear layer, forward and backward: the first layer of PositionEmbeddingLearned in training mode
 * (fusion_encoder.py:173-189: Conv1d(2 -> E, k = 1) on [B, 2, N] = a linear layer on B * N rows of 2 coordinates).
 * in_features = 2 is far below what isf_linear_forward tiles (K % 32 == 0); padding the coordinates to 32 columns and
 * splitting them into f16 halves would move 16 x the bytes and round positions of up to 180.  Plain fp32 FMA on the
 * vector ALU instead, every sum in one fixed order:
 *   isf_thin_linear_forward: y [M, N] = x [M, K] w^T + b, w [N, K] (nn.Linear layout), b [N] or NULL; per element
 *     b + x_0 w_0 + ... + x_{K-1} w_{K-1}, left to right, one fused multiply-add per term.
 *   isf_thin_linear_parts(M): row chunks the backward reduces over (ceil(M / 128), a function of M alone; 0 for M <= 0);
 *     the caller hands isf_thin_linear_backward a workspace of parts * (K + 1) * N floats.
 *   isf_thin_linear_backward: grad_w [N, K] = grad_y^T x, grad_b [N] = column sums of grad_y (NULL: not computed),
 *     grad_x [M, K] = grad_y w (NULL: not computed; the positions this layer embeds need none).  grad_w / grad_b: one
 *     workgroup per chunk sums its rows in ascending order, a second launch adds the chunks in ascending order -- no
 *     atomics, bit-identical run to run; the longest addition chain is 128 + parts terms.  grad_w NULL: only grad_x.
 *     grad_x: per row, every lane's four columns in ascending order, then a fixed xor tree over the 64 lanes.
 * Domain: 1 <= K <= 8, N % 16 == 0, 16 <= N <= 256; anything else is ISF_ERR_UNSUPPORTED before any launch.  All
 * asynchronous. */
int isf_thin_linear_forward(const float* x, const float* w, const float* b, float* y, int num_rows, int out_features,
                            int in_features, isf_stream_t stream);
int isf_thin_linear_parts(int num_rows);
int isf_thin_linear_backward(const float* grad_y, const float* x, const float* w, float* parts, float* grad_w,
                             float* grad_b, float* grad_x, int num_rows, int out_features, int in_features,
                             isf_stream_t stream);

/* 8f #3  input pre-pass: multi-sweep assembly + augmentation + range filter ---------------------------------
 * replaces, per batch, the dataloader-side numpy / torch code of LoadPointsFromMultiSweeps.__call__
 * (datasets/pipelines/loading.py:860-903), the point side of GlobalRotScaleTransV2 and RandomFlip3DV2
 * (datasets/pipelines/transforms_3d.py:1887-1890, :1171-1183) and PointsRangeFilter (:2012-2025).
 * raw = the sweep files of the batch as loaded (flat float32 [P, 5]: x, y, z, intensity, ring), uploaded untouched.
 * One descriptor per file, grouped by ascending sample, key frame first within a sample (the order of the
 * reference's concatenation).  Output: the kept points of the batch, compacted in input order, float32 [<= P, 5]
 * (capacity P rows), and sample_offsets[batch+1] (rows; device, and host when sample_offsets_host != NULL).
 * The call synchronizes `stream` once. */
typedef struct {
  int64_t first_point;     /* row of the file's first point in raw */
  int32_t num_points;
  int32_t sample;          /* batch index */
  int32_t is_sweep;        /* 0: key frame (time column := 0)   1: previous sweep (pose applied, time := time_lag) */
  int32_t remove_close;    /* sweeps only: drop points with |x| < r and |y| < r before the pose (loading.py:824-844) */
  float close_radius;
  float time_lag;          /* float32(key timestamp - sweep timestamp / 1e6) */
  double rotation[9];      /* sensor2lidar_rotation, row-major; p @ R^T in float64 as numpy does (loading.py:883) */
  double translation[3];   /* sensor2lidar_translation, float64 (loading.py:885) */
} isf_sweep_t;

typedef struct {
  int32_t enabled;
  float rot_mat_T[9];      /* points[:, :3] @ rot_mat_T, float32 (core/points/base_points.py:178) */
  float translation[3];    /* then += translation (:206) */
  float scale;             /* then *= scale (:270) */
  int32_t flip_horizontal; /* then y := -y (core/points/lidar_points.py:31-32) */
  int32_t flip_vertical;   /* and x := -x (:33-34) */
} isf_point_aug_t;

int isf_assemble_points(const float* raw, const isf_sweep_t* sweeps, int num_sweeps, int batch_size,
                        const isf_point_aug_t* aug /* [batch] or NULL */,
                        const float* point_range /* 6 host floats or NULL */, float* points_out,
                        int32_t* sample_offsets, int32_t* sample_offsets_host, isf_stream_t stream);

/* GT-paste, point side: isf_assemble_points with ObjectSampleV2 folded in --------------------------------------------
 * replaces, per batch, ObjectSampleV2.remove_points_in_boxes and the concatenation behind it
 * (datasets/pipelines/transforms_3d.py:1299-1312, :1359-1361), box_np_ops.points_in_rbbox's per-point loop
 * (core/bbox/box_np_ops.py:718-753, numba on one core) and the translate of every sampled object
 * (datasets/pipelines/dbsampler.py:769-777).  isf_assemble_points plus two things:
 *   - a descriptor with is_sweep == ISF_SWEEP_PASTED is a database object: xyz += float32(translation[k]) (one float32
 *     add per coordinate, BasePoints.translate), fifth column kept as stored, no pose, not tested against the boxes.
 *     The caller lists a sample's pasted objects FIRST (points.cat([sampled_points, points]), :1361);
 *   - planes [box_offsets[batch]][6][4] (host, float32): the inward plane equations (n0, n1, n2, d) of each sample's
 *     removal boxes (surface_equ_3d of corner_to_surfaces_3d, box_np_ops.py:404-423, :694-715); box_offsets
 *     [batch + 1] (host).  Key-frame and sweep points are tested AFTER the sensor pose and BEFORE the augmentation and
 *     dropped when, for some box, all six x n0 + y n1 + z n2 + d (float32, left to right, no contraction) are < 0.
 * More than ISF_PASTE_MAX_BOXES boxes on one sample -> ISF_ERR_UNSUPPORTED before any launch.  Augmentation, range
 * filter, compaction, outputs and the single stream synchronisation are isf_assemble_points'. */
#define ISF_SWEEP_PASTED 2
#define ISF_PASTE_MAX_BOXES 64
int isf_assemble_points_paste(const float* raw, const isf_sweep_t* sweeps, int num_sweeps, int batch_size,
                              const isf_point_aug_t* aug /* [batch] or NULL */,
                              const float* point_range /* 6 host floats or NULL */,
                              const float* planes /* host */, const int32_t* box_offsets /* host, [batch + 1] */,
                              float* points_out, int32_t* sample_offsets, int32_t* sample_offsets_host,
                              isf_stream_t stream);

/* GT-paste, image side: in place on the uploaded uint8 views, before isf_image_prepass ---------------------------------
 * replaces, per batch, the far-to-near loop of MMDataBaseSamplerV2.sample_all (datasets/pipelines/dbsampler.py:779-831)
 * with its PIL -> numpy -> PIL round trip of a whole image per object, and paste_obj_v2 (:902-928).  raw holds the
 * views and, behind them, the database patches (uint8 HWC RGB).  One descriptor per view with the range of its
 * operations and their bounding box; a thread owns a pixel and applies the operations that hold it in order, so
 * overlapping rectangles give one deterministic result.  Every byte is numpy's:
 *   ISF_PASTE_MIX    (:814) v = (uint8) trunc(mixup * orig + one_minus_mixup * v) in float64, orig = the byte before
 *                    any operation of this call;
 *   ISF_PASTE_PATCH  (:921-925) v = (uint8) trunc((float32) v * paste_mask) in float64, paste_mask = one_minus_mixup
 *                    inside the mask rectangle and 1 outside; then v += (uint8) trunc((float32)(mixup_f32 * (float32)
 *                    patch) * mask) with uint8 wrap-around.
 * Rectangles are resolved on the host (numpy slice semantics) and lie inside the view.  max_ops_per_view above
 * ISF_PASTE_MAX_OPS -> ISF_ERR_UNSUPPORTED before any launch.  One asynchronous launch, no host wait. */
#define ISF_PASTE_MIX 0
#define ISF_PASTE_PATCH 1
#define ISF_PASTE_MAX_OPS 256
typedef struct {
  int64_t src_offset;      /* byte offset of the view's first pixel in raw */
  int32_t width, height;
  int32_t op_begin, op_end; /* this view's operations, in the order the reference applies them */
  int32_t box_x0, box_y0, box_x1, box_y1; /* bounding box of their rectangles: columns [x0, x1), rows [y0, y1) */
} isf_paste_view_t;

typedef struct {
  int64_t patch_offset;    /* ISF_PASTE_PATCH: byte offset in raw of the patch pixel that lands on (x0, y0) */
  int32_t kind;
  int32_t x0, y0, x1, y1;  /* columns [x0, x1), rows [y0, y1) of the view */
  int32_t mask_x0, mask_y0, mask_x1, mask_y1; /* ISF_PASTE_PATCH: where obj_mask is 1 (view coordinates) */
  int32_t patch_pitch;     /* pixels per patch row */
} isf_paste_op_t;

int isf_image_paste(uint8_t* raw /* device, in place */, const isf_paste_view_t* views /* device */, int num_views,
                    const isf_paste_op_t* ops /* device */, int max_ops_per_view, int max_box_w, int max_box_h,
                    double mixup, double one_minus_mixup, float mixup_f32, isf_stream_t stream);

/* camera input pre-pass: ImageAug3D + ImageNormalize for every view of a batch ---------------------------------------
 * replaces, per batch, the dataloader-side Pillow / torchvision code of ImageAug3D.img_transform
 * (datasets/pipelines/transforms_3d.py:82-112: img.resize(resize_dims) -> img.crop(crop) -> FLIP_LEFT_RIGHT ->
 * img.rotate(rotate)) and ImageNormalize (:25-43: ToTensor + Normalize), as configs/isfusion/isfusion_0075voxel.py:238-352
 * chains them.  raw = the decoded images of the batch (uint8, HWC, RGB, any size per view), uploaded untouched; one
 * descriptor per view.  Output img_out [num_views, 3, out_h, out_w] float32, every element written, bit-exact against
 * Pillow's 8-bit path (resize: antialiased bicubic, horizontal pass rounded to uint8 before the vertical one, 22-bit
 * coefficients; rotate: nearest neighbour in 16.16 fixed point) followed by the 3 x 256 normalise table.
 * tables (int32, device): per resized axis a bounds table [out][2] = (first input index, taps) and a coefficient table
 * [out][ksize] (22 fractional bits), at the descriptor's offsets; an axis that keeps its size uses taps = 1,
 * coefficient 2^22.  A tile whose source box the kernel cannot hold (rot[] that is no rotation, more vertical taps
 * than the ~89 rows it holds: in / out > ~20) is written as NaN.  One asynchronous launch, no host wait. */
typedef struct {
  int64_t src_offset;      /* byte offset of the view's first pixel in raw */
  int32_t src_w, src_h;
  int32_t resize_w, resize_h; /* ImageAug3D resize_dims */
  int32_t crop_x, crop_y;  /* crop[0], crop[1]; the crop is out_w x out_h and may leave the resized image (0 there) */
  int32_t flip;            /* FLIP_LEFT_RIGHT after the crop */
  int32_t rotate;          /* 0: no rotation (rotate % 360 == 0), rot[] unused */
  int32_t rot[6];          /* Pillow's 16.16 affine: (x, y) reads ((rot2 + y rot1 + x rot0) >> 16, (rot5 + y rot4 + x rot3) >> 16) */
  int32_t h_bounds, h_coeffs, h_ksize; /* offsets into tables (in int32) and row length of the coefficient table */
  int32_t v_bounds, v_coeffs, v_ksize;
} isf_image_view_t;

int isf_image_prepass(const uint8_t* raw, const isf_image_view_t* views /* device */, int num_views,
                      const int32_t* tables /* device */, const float* norm_lut /* device, 3 x 256 */, int out_h,
                      int out_w, float* img_out, isf_stream_t stream);

/* 8f #2  Point-to-Grid backward ---------------------------------------------------------------------------------
 * replaces autograd through img_fv_to_bev's F.grid_sample (fusion_encoder.py:1049-1056) + the canvas scatter (:989-1003):
 * grad_out [B, C, bev, bev] -> grad_img_nhwc [B*num_cam, H, W, C] (written completely; fp32 atomics inside).  The
 * other arguments are isf_p2g_forward's.  No gradient flows to points / calibration (not trainable). */
int isf_p2g_backward(const float* pillars, int pillar_ld, int slots, const int32_t* pillar_coors, int num_pillars,
                     int batch_size, int num_cam, int feat_h, int feat_w, int channels, const float* cam_params,
                     int input_h, int input_w, int bev_size, const float* grad_out, float* grad_img_nhwc,
                     isf_stream_t stream);

/* isf_p2g_backward with exact accumulation (DETERMINISTIC ENTRIES; same reference interface, fusion_encoder.py:989-1056):
 * A = absmax(grad_out) (bilinear weights <= 1), N = num_pillars * slots. */
int isf_p2g_backward_det(const float* pillars, int pillar_ld, int slots, const int32_t* pillar_coors, int num_pillars,
                         int batch_size, int num_cam, int feat_h, int feat_w, int channels, const float* cam_params,
                         int input_h, int input_w, int bev_size, const float* grad_out, float* grad_img_nhwc,
                         isf_stream_t stream);

/* Backward of a cell gather, deterministic (used under isfusion_amd.deterministic() in place of autograd's scatter_add):
 * replaces autograd through x_scene.gather(2, top_idx) of get_instance_feat (fusion_encoder.py:1133-1141) and through the
 * proposal-feature gather of TransFusionHeadV2.forward_single (transfusion_head_v2.py:799-803).  index [B, K] int32 cells
 * (a cell may occur more than once: its gradients are summed in ascending entry order, no atomics); channels_last 0:
 * grad_out [B, E, K] -> grad_x [B, E, num_cells]; channels_last 1: grad_out [B, K, E] -> grad_x [B, num_cells, E].
 * grad_x is written completely.  Entries outside [0, num_cells) are ignored.  Asynchronous. */
int isf_gather_cells_backward(const float* grad_out, const int32_t* index, int batch_size, int num_index, int channels,
                              int num_cells, int channels_last, float* grad_x, isf_stream_t stream);

/* 8f #2  multi-scale deformable attention backward (one level) --------------------------------------------------
 * replaces MultiScaleDeformableAttnFunction.backward -> ms_deform_attn_backward (ops/src/cuda/ms_deform_attn_cuda.cu,
 * ms_deform_im2col_cuda.cuh:301-920) plus the backward of the softmax / location arithmetic isf_msda_forward folds in.
 * Same tensors as the forward plus grad_out [B*Q, heads*hd]; outputs grad_value [B, H*W, heads*hd] (zeroed here,
 * fp32 atomics), grad_offsets [B*Q, heads*P*2], grad_logits [B*Q, heads*P].  No gradient for reference_points
 * (the IS-Fusion path feeds constants).  Asynchronous. */
int isf_msda_backward(const float* value, const float* sampling_offsets, const float* attention_logits,
                      const float* reference_points, const float* grad_out, int batch_size, int num_queries,
                      int num_heads, int head_dim, int num_points, int height, int width, float* grad_value,
                      float* grad_offsets, float* grad_logits, isf_stream_t stream);

/* isf_msda_backward with exact accumulation of grad_value (DETERMINISTIC ENTRIES; same reference interface,
 * ms_deform_im2col_cuda.cuh:301-920): A = absmax(grad_out) (softmax and bilinear weights <= 1), N = num_queries *
 * num_points.  grad_offsets / grad_logits are written once, as in the default. */
int isf_msda_backward_det(const float* value, const float* sampling_offsets, const float* attention_logits,
                          const float* reference_points, const float* grad_out, int batch_size, int num_queries,
                          int num_heads, int head_dim, int num_points, int height, int width, float* grad_value,
                          float* grad_offsets, float* grad_logits, isf_stream_t stream);

/* 8f #2  attention backward ------------------------------------------------------------------------------------
 * replaces autograd through nn.MultiheadAttention's softmax(q k^T / sqrt(hd)) v core (sst_basic_block_v2.py:41-75,
 * fusion_encoder.py:371-470) for the layouts of isf_attention_forward / isf_window_attention_forward.  The Lq x Lk
 * probabilities are recomputed (row statistics logsumexp and dO.O), never stored; every gradient row is written
 * once, no atomics.  `out` = the forward result.  head dim 16 (window: 16 or 32).  Asynchronous. */
int isf_attention_backward(const float* q, int ldq, const float* k, const float* v, int ldkv, const float* out,
                           const float* grad_out, int ldo, int batch_size, int num_queries, int num_keys,
                           int embed_dims, int num_heads, float* grad_q, int ldgq, float* grad_k, float* grad_v,
                           int ldgkv, isf_stream_t stream);
/* ... of isf_attention_forward_dropout (same dropout_p, seed and domain; `out` = that call's result).  With dropout_p > 0,
 * more than 512 keys and at most 256 queries (the head's 200 x 32400 cross-attention) dQ is computed by 512-key splits
 * and an ordered merge instead of a wave per query: the same gradients, still no atomics and nothing of size Lq x Lk. */
int isf_attention_backward_dropout(const float* q, int ldq, const float* k, const float* v, int ldkv, const float* out,
                                   const float* grad_out, int ldo, int batch_size, int num_queries, int num_keys,
                                   int embed_dims, int num_heads, float dropout_p, unsigned long long seed, float* grad_q,
                                   int ldgq, float* grad_k, float* grad_v, int ldgkv, isf_stream_t stream);
int isf_window_attention_backward(const float* qkv, const float* grad_out, int batch_size, int grid_size,
                                  int embed_dims, int num_heads, int window, int shift, float* grad_qkv,
                                  isf_stream_t stream);

/* A9 / A15  dense 3x3 BEV convolutions on the sparse-conv kernel ------------------------
 * replaces mmcv ConvModule / nn.Conv2d + BatchNorm2d + ReLU (fusion_encoder.py:862-960, backbones/second.py:126-165,
 * MIOpen Winograd + 2 elementwise kernels per layer).  A dense B x H x W grid is a sparse tensor with every cell
 * active: isf_dense_grid_rulebook writes its neighbour table arithmetically (tap k = ky*kernel_w + kx; with
 * transpose_taps the taps are enumerated (kx, ky), which is the convolution of the SPATIALLY TRANSPOSED map expressed
 * on the un-transposed tokens -- the bev_feats.permute(0,1,3,2) of fusion_encoder.py:1093 costs nothing);
 * isf_sparse_conv_forward_f16x3 then runs Conv + BN + ReLU (+ partial sums of > 256 input channels through its
 * residual input) in one launch.  nbr == NULL only queries out_hw_host.
 * isf_nchw_to_split / isf_split_to_nchw convert between [B, C, hw] fp32 maps and split-format token matrices
 * (token = b*hw + pos); x_channel_offset / channel_offset select a channel slice of the source map / destination
 * rows (<= 256 channels per call). */
int isf_dense_grid_rulebook(int batch_size, int height, int width, int kernel_h, int kernel_w, int stride, int padding,
                            int transpose_taps, int32_t* nbr, int nbr_stride, int out_hw_host[2],
                            isf_stream_t stream);
int isf_nchw_to_split(const float* x, int batch_size, int x_channels, int x_channel_offset, int channels, int hw,
                      void* out_split, int out_channels, int channel_offset, isf_stream_t stream);
int isf_split_to_nchw(const void* x_split, int batch_size, int channels, int hw, float* out, isf_stream_t stream);

/* Detection-head training: targets, Hungarian assignment and losses (isf_head_loss.hip) ------------------------
 * Boxes are [sum G, box_ld] fp32 rows in the LiDARInstance3DBoxes layout (x, y, z_bottom, dx, dy, dz, yaw, vx, vy), the
 * samples' GT concatenated; gt_offsets is a HOST array of batch_size + 1 ints (sample b = rows [off[b], off[b+1])),
 * batch_size <= ISF_HEAD_MAX_BATCH; gt_labels [sum G] int64.  Nothing here synchronises with the host.
 * isf_head_heatmap_targets replaces the per-box loop of get_targets_single (dense_heads/transfusion_head_v2.py:1082-1128)
 *   with gaussian_radius / draw_heatmap_gaussian (core/utils/gaussian.py:6-85): heatmap [B, classes, height, width]
 *   (height = grid_size[1] / out_size_factor, rows indexed by the x cell as the reference's [[1, 0]] swap makes them).
 *   params = 7 HOST floats: voxel_size (x, y), point_cloud_range (x, y), out_size_factor, gaussian_overlap, min_radius.
 * isf_head_assign_cost replaces bbox_coder.decode (:980-994) and HungarianAssigner3D's cost (core/bbox/assigners/
 *   hungarian_assigner.py:106-134): FocalLossCost + BBoxBEVL1Cost + IoU3DCost (BboxOverlaps3D, coordinate='lidar').
 *   Head outputs [B, k, num_layers * num_proposals] (heatmap = logits, vel may be NULL); boxes [B, L*P, 9 | 7] decoded;
 *   cost / iou [B, L, P, gt_stride] (gt_stride >= max G of a sample).  params = 15 HOST floats: out_size_factor *
 *   voxel_size (x, y), pc_range (x, y), point_cloud_range (6), cls / reg / iou weights, focal alpha, gamma.
 * isf_head_assign replaces linear_sum_assignment and the result assembly of :137-156: one workgroup per (sample, layer),
 *   shortest augmenting paths in fp64; G or P above ISF_HEAD_MAX_ASSIGN -> ISF_ERR_UNSUPPORTED.  assigned_gt_inds
 *   [B, L*P] int32 (0 background, k+1 = GT k of the sample), assigned_labels int64 (-1 background), max_overlaps fp32.
 * isf_head_assemble_targets replaces :1036-1080 and the batch reductions of :932-948: labels [B, L*P] int64
 *   (background = num_classes), label_weights fp32, bbox_targets / bbox_weights [B, L*P, code_size]
 *   (TransFusionBBoxCoder.encode, core/bbox/coders/transfusion_bbox_coder.py:24-40), ious = clamp(max_overlaps, 0, 1),
 *   num_pos [1] int32, stats [2] fp32 = (num_pos, matched_ious).  params = 5 HOST floats: out_size_factor * voxel_size
 *   (x, y), pc_range (x, y), pos_weight.
 * Losses (:1170-1276).  Each writes loss [1] (already divided by the avg factor and times loss_weight), scale [1] =
 *   loss_weight / avg_factor and grad = the UNSCALED d loss_element / d input; isf_head_loss_grad_scale then writes
 *   out = grad * scale * grad_output[0] (grad_output device scalar or NULL = 1) for the backward.  Reductions are fixed
 *   order (no float atomics): bit-identical from run to run.
 *   isf_gaussian_focal_loss: GaussianFocalLoss(alpha 2, gamma 4) of clip_sigmoid(logits) vs target, n elements,
 *     avg = max(#(target == 1), 1); partials = 512 doubles of scratch.
 *   isf_sigmoid_focal_loss: sigmoid focal loss of logits [B, classes, ld] columns [offset, offset + P) vs labels /
 *     label_weights [B, ld], avg = max(num_pos[0], 1); grad has the logits' layout (columns outside the slice untouched).
 *   isf_head_l1_loss: L1 of [center 2, height 1, dim 3, rot 2, vel 2] (each [B, k, ld]) vs bbox_targets [B, ld, code],
 *     weight bbox_weights * code_weights (code_size HOST floats), avg = max(num_pos[0], 1); grad [B, code, ld]. */
#define ISF_HEAD_MAX_BATCH 32
#define ISF_HEAD_MAX_ASSIGN 1024
int isf_head_heatmap_targets(const float* gt_boxes, int box_ld, const int64_t* gt_labels, const int* gt_offsets,
                             int batch_size, int num_classes, int height, int width, const float* params,
                             float* heatmap, isf_stream_t stream);
int isf_head_assign_cost(const float* heatmap, const float* center, const float* height, const float* dim,
                         const float* rot, const float* vel, int batch_size, int num_classes, int num_proposals,
                         int num_layers, const float* gt_boxes, int box_ld, const int64_t* gt_labels,
                         const int* gt_offsets, int gt_stride, const float* params, float* boxes, float* cost,
                         float* iou, isf_stream_t stream);
int isf_head_assign(const float* cost, const float* iou, int gt_stride, const int64_t* gt_labels,
                    const int* gt_offsets, int batch_size, int num_proposals, int num_layers, int32_t* assigned_gt_inds,
                    int64_t* assigned_labels, float* max_overlaps, isf_stream_t stream);
int isf_head_assemble_targets(const int32_t* assigned_gt_inds, const float* max_overlaps, const float* gt_boxes,
                              int box_ld, const int64_t* gt_labels, const int* gt_offsets, int batch_size,
                              int num_proposals_total, int num_classes, int code_size, const float* params,
                              int64_t* labels, float* label_weights, float* bbox_targets, float* bbox_weights,
                              float* ious, int32_t* num_pos, float* stats, isf_stream_t stream);
int isf_gaussian_focal_loss(const float* logits, const float* target, size_t n, float loss_weight, double* partials,
                            float* grad, float* loss, float* scale, isf_stream_t stream);
int isf_sigmoid_focal_loss(const float* logits, int batch_size, int num_classes, int num_proposals, int ld,
                           int offset, const int64_t* labels, const float* label_weights, const int32_t* num_pos,
                           float alpha, float gamma, float loss_weight, float* grad, float* loss, float* scale,
                           isf_stream_t stream);
int isf_head_l1_loss(const float* center, const float* height, const float* dim, const float* rot, const float* vel,
                     int batch_size, int num_proposals, int ld, int offset, int code_size, const float* bbox_targets,
                     const float* bbox_weights, const float* code_weights, const int32_t* num_pos, float loss_weight,
                     float* grad, float* loss, float* scale, isf_stream_t stream);
int isf_head_loss_grad_scale(const float* grad, size_t n, const float* scale, const float* grad_output, float* out,
                             isf_stream_t stream);

/* BEV NMS and test-time-augmentation merge (isf_nms.hip) ------------------------------------------------------
 * isf_nms_segmented replaces the NMS branch of TransFusionHeadV2.get_bboxes (dense_heads/transfusion_head_v2.py:
 *   1344-1403: circle_nms, core/post_processing/box3d_nms.py:183-218; nms_gpu, ops/iou3d/iou3d_utils.py:26-57) and the
 *   per-class loop of merge_aug_bboxes_3d (core/post_processing/merge_augs.py:58-86: nms_gpu / nms_normal_gpu,
 *   iou3d_utils.py:60-77, iou3d_kernel.cu nms_kernel / nms_normal_kernel) in ONE launch, one workgroup per segment.
 *   Rows: boxes [num_groups * group_stride, box_ld] (box_format ISF_NMS_BOX_LIDAR: x, y, z_bottom, dx, dy, dz, yaw, ...
 *   as isf_decode_boxes writes them, turned into xyxyr inside as xywhr2xyxyr does; ISF_NMS_BOX_XYXYR: x1, y1, x2, y2, r),
 *   scores [rows], labels [rows] int32 or NULL (then every row is task 0).  Group g = rows [g * group_stride,
 *   g * group_stride + counts[g]) (counts: DEVICE int32 [num_groups], or NULL = all rows); group_stride <=
 *   ISF_NMS_MAX_SEGMENT, else ISF_ERR_UNSUPPORTED before any launch.  Segment (g, t) = the group's rows whose class maps
 *   to task t through task_of_class (HOST, num_classes <= ISF_NMS_MAX_CLASSES entries, -1 = dropped).  Per task (HOST
 *   arrays, num_tasks <= ISF_NMS_MAX_TASKS) a mode and a threshold:
 *     ISF_NMS_KEEP    every row kept, in input order (a task with radius <= 0)
 *     ISF_NMS_ROTATE  nms_gpu: suppressed when the rotated BEV IoU (fp64 overlap, isf_bev.h) > thr
 *     ISF_NMS_NORMAL  nms_normal_gpu: suppressed when the float32 axis-aligned IoU of the xyxy corners > thr
 *     ISF_NMS_CIRCLE  circle_nms on columns 0-1: suppressed when the SQUARED centre distance <= thr (the reference's
 *                     own semantics; it passes the radius as thr)
 *   Within a segment: score descending, equal scores by lower row (the reference's sorts are not stable), then the first
 *   pre_maxsize (< 0: all), greedy suppression, the first post_max_size kept (< 0: all).  Outputs (device, no host
 *   sync): keep [rows] uint8 (1 = kept; rows past a count or of no task 0), keep_index [num_groups * num_tasks,
 *   group_stride] int32 = the kept rows (absolute row numbers) of each segment in kept order, keep_count
 *   [num_groups * num_tasks] int32.  workspace = isf_nms_workspace_size(...) bytes of device scratch (the mask).
 * isf_boxes_iou_bev replaces boxes_iou_bev (iou3d_utils.py:6-23, iou3d_kernel.cu boxes_iou_bev_kernel): boxes_a
 *   [M, 5] / boxes_b [N, 5] xyxyr -> iou [M, N] = overlap / max(area_a + area_b - overlap, 1e-8), areas from the xyxy
 *   corners.
 * isf_bbox_mapping_back replaces bbox3d_mapping_back (core/bbox/transforms.py:5-24) for num_views <=
 *   ISF_NMS_MAX_VIEWS views in place: rows [v * view_stride, v * view_stride + counts[v]) (counts DEVICE or NULL) of
 *   boxes [*, box_ld >= 7]; LiDARInstance3DBoxes.flip (horizontal: columns 1::7 negated, yaw = pi - yaw; vertical:
 *   columns 0::7 negated, yaw = -yaw) then scale(1 / scale_factor[v]) of every column but yaw.  horizontal / vertical
 *   / scale_factor are HOST arrays of num_views. */
#define ISF_NMS_MAX_SEGMENT 1024
#define ISF_NMS_MAX_TASKS 16
#define ISF_NMS_MAX_CLASSES 64
#define ISF_NMS_MAX_VIEWS 16
#define ISF_NMS_KEEP 0
#define ISF_NMS_ROTATE 1
#define ISF_NMS_NORMAL 2
#define ISF_NMS_CIRCLE 3
#define ISF_NMS_BOX_XYXYR 0
#define ISF_NMS_BOX_LIDAR 1
size_t isf_nms_workspace_size(int num_groups, int group_stride, int num_tasks, int pre_maxsize);
int isf_nms_segmented(const float* boxes, int box_ld, int box_format, const float* scores, const int32_t* labels,
                      const int32_t* counts, int num_groups, int group_stride, int num_classes,
                      const int* task_of_class, int num_tasks, const int* task_mode, const float* task_thr,
                      int pre_maxsize, int post_max_size, void* workspace, size_t workspace_bytes, uint8_t* keep,
                      int32_t* keep_index, int32_t* keep_count, isf_stream_t stream);
int isf_boxes_iou_bev(const float* boxes_a, int num_a, const float* boxes_b, int num_b, float* iou,
                      isf_stream_t stream);
int isf_bbox_mapping_back(float* boxes, int box_ld, int num_views, int view_stride, const int32_t* counts,
                          const int* horizontal, const int* vertical, const float* scale_factor, isf_stream_t stream);

/* Camera branch: Swin-T backbone and GeneralizedLSSFPN neck (isf_swin.hip) --------------------------------------
 * isf_swin_gemm replaces every nn.Linear of SwinBlock (WindowMSA.qkv / proj, swin.py:96-103; FFN fc1 + GELU / fc2 +
 *   identity, mmcv FFN), with norm1 / norm2 as a LayerNorm prologue (swin.py:341-356); PatchEmbed's Conv2d(k 4, s 4) +
 *   AdaptivePadding 'corner' (utils/transformer.py:134-258); PatchMerging's nn.Unfold(2, 2) + LayerNorm(4C) + Linear
 *   (utils/transformer.py:260-400); and the neck's F.interpolate(bilinear, align_corners) + torch.cat + 1x1 ConvModule
 *   (generalized_lss.py:83-100).  y = act((A . W^T) * scale + shift) + residual, W packed by isf_pack_linear
 *   ([out_features, k]), A rows generated by the loader (isf_swin_a):
 *     ROWS  : x [num_rows, ldx]; k = channel.  With ln_stats ([num_rows, 2] mean, rstd from isf_swin_row_stats):
 *             a = (x - mean) * rstd * ln_gamma[k] + ln_beta[k].
 *     PATCH : x image [n, c, h, w]; row = (b, oy, ox) of the ceil(h/4) x ceil(w/4) grid; k = ci*16 + ky*4 + kx
 *             (Conv2d weight order), zero past the image (corner padding) and for k >= 16 c (k padded to % 32).
 *     MERGE : x token rows [n*h*w, c]; row = (b, oy, ox) of the ceil(h/2) x ceil(w/2) grid; k = (kh*2 + kw)*c + ci ->
 *             x[b, 2 oy + kh, 2 ox + kw, ci], zero past the grid (corner padding).  nn.Unfold orders the same
 *             elements ci*4 + kh*2 + kw: the caller packs W and gamma / beta in the loader's order.  k = 4 c.
 *     UPCAT : x fine map [n, c, h, w], x2 coarse map [n, c2, h2, w2] (NCHW); row = (b, y, x) of the fine grid;
 *             k < c -> x[b, k, y, x], else the bilinear (align_corners=True) sample of x2 channel k - c.  k = c + c2.
 *   scale / shift: [out_features] or NULL (1 / 0); activation 0 none, 1 ReLU, 2 GELU (erf); residual [num_rows,
 *   out_features] rows or NULL; y rows [num_rows, ldy], or [B, out_features, y_hw] when y_hw > 0.
 * isf_swin_row_stats: mean and rstd = 1 / sqrt(var + eps) (biased variance) of each ROWS / MERGE loader row of k
 *   elements -> stats [num_rows, 2].
 * isf_swin_layernorm replaces nn.LayerNorm of token rows (PatchEmbed.norm; the out_indices norms + view/permute to
 *   NCHW, swin.py:746-763): y rows [num_rows, channels], or [B, channels, y_hw] when y_hw > 0.  x != y.
 * isf_swin_window_attention replaces ShiftWindowMSA + WindowMSA (swin.py:20-283) after the qkv Linear: qkv token rows
 *   [batch*height*width, 3 channels] -> out token rows [batch*height*width, channels] (attention before proj).  Zero
 *   padding to % window (padded cells' q / k / v = qkv_bias, NULL = no bias), torch.roll by -shift, window partition
 *   and reverse are index arithmetic; rel_bias [heads, 49, 49] = relative_position_bias_table[index]; shifted blocks
 *   add -100 between the 3 x 3 regions of the padded grid.  window 7, head dim 32. */
typedef struct isf_swin_a {
  const float* x;
  const float* x2;
  const float* ln_stats;
  const float* ln_gamma;
  const float* ln_beta;
  int mode, ldx, n, c, h, w, c2, h2, w2;
} isf_swin_a;
#define ISF_SWIN_A_ROWS 0
#define ISF_SWIN_A_PATCH 1
#define ISF_SWIN_A_MERGE 2
#define ISF_SWIN_A_UPCAT 3
int isf_swin_gemm(const isf_swin_a* a, int num_rows, int k, const void* packed_weight, int out_features,
                  const float* scale, const float* shift, int activation, const float* residual, float* y, int ldy,
                  int y_hw, isf_stream_t stream);
/* isf_swin_gemm_rowscale: isf_swin_gemm with a per-sample factor on the branch output, for DropPath in training
 *   (mmcv DropPath on ShiftWindowMSA's output, swin.py:251, and on FFN's layers): y = act((A . W^T) * scale + shift) *
 *   row_scale[r / rows_per_sample] + residual.  ROWS loader without the LayerNorm prologue; num_rows is a multiple of
 *   rows_per_sample.  row_scale all 1 gives isf_swin_gemm's result bit for bit; a 0 leaves the residual row. */
int isf_swin_gemm_rowscale(const isf_swin_a* a, int num_rows, int k, const void* packed_weight, int out_features,
                           const float* scale, const float* shift, int activation, const float* residual,
                           const float* row_scale, int rows_per_sample, float* y, int ldy, int y_hw,
                           isf_stream_t stream);
int isf_swin_row_stats(const isf_swin_a* a, int num_rows, int k, float eps, float* stats, isf_stream_t stream);
int isf_swin_layernorm(const float* x, int num_rows, int channels, const float* gamma, const float* beta, float eps,
                       float* y, int y_hw, isf_stream_t stream);
int isf_swin_window_attention(const float* qkv, const float* qkv_bias, const float* rel_bias, int batch, int height,
                              int width, int channels, int heads, int window, int shift, float scale, float* out,
                              isf_stream_t stream);

/* f16 inference mode of the Swin-T backbone (isf_swin.hip, isf_swin_f16.hip) -----------------------------------
 * What the reference computes for SwinTransformer under mmcv's fp16 machinery (auto_fp16 / torch.autocast(float16):
 * half nn.Linear / Conv2d / matmul, swin.py:20-368, utils/transformer.py:134-400), with the residual stream, LayerNorm
 * statistics, softmax, GELU, accumulation and the epilogue arithmetic in fp32.  Every store to an f16 tensor
 * saturates at +-65504 instead of producing inf.
 * isf_pack_linear_f16 replaces weight.half(): weight [out, in] (torch layout, fp32) -> one plane of f16 MFMA
 *   fragments, isf_packed_linear_f16_bytes(out, in) bytes, 16-byte aligned.  out % 16 == 0, in % 32 == 0.
 * isf_swin_gemm_f16 replaces the half nn.Linear / Conv2d of the mode: isf_swin_gemm with ONE matrix instruction per
 *   product.  Same loader, epilogue and argument meanings; packed_weight_f16 from isf_pack_linear_f16.  ROWS, PATCH and
 *   MERGE loaders (no UPCAT), y_hw == 0.  a_is_f16 != 0: a->x (declared const float*) points to _Float16 rows
 *   [num_rows, a->ldx] with a->ldx counted in f16 ELEMENTS (>= k, % 8 == 0, x 16-byte aligned), ROWS loader without
 *   the LayerNorm prologue; else the loader's fp32 values are rounded to f16 after the prologue.  y_is_f16 != 0: y is
 *   f16 rows [num_rows, ldy] (ldy in f16 elements, ROWS loader only), else fp32 rows.
 * isf_swin_window_attention_f16 replaces ShiftWindowMSA + WindowMSA after the half qkv Linear: isf_swin_window_attention
 *   on f16 qkv rows [batch*height*width, 3 channels] -> f16 out rows [batch*height*width, channels], on the matrix
 *   cores.  qkv_bias (fp32, NULL = none) and rel_bias (fp32 [heads, 49, 49]) as there; scores and softmax in fp32, the
 *   probabilities rounded to f16 for the second product.  qkv and qkv_bias 16-byte aligned. */
size_t isf_packed_linear_f16_bytes(int out_features, int in_features);
int isf_pack_linear_f16(const float* weight, int out_features, int in_features, void* packed, isf_stream_t stream);
int isf_swin_gemm_f16(const isf_swin_a* a, int a_is_f16, int num_rows, int k, const void* packed_weight_f16,
                      int out_features, const float* scale, const float* shift, int activation, const float* residual,
                      void* y, int y_is_f16, int ldy, int y_hw, isf_stream_t stream);
int isf_swin_window_attention_f16(const void* qkv, const float* qkv_bias, const float* rel_bias, int batch, int height,
                                  int width, int channels, int heads, int window, int shift, float scale, void* out,
                                  isf_stream_t stream);

/* Backward of the neck's top-down step (isf_swin_train.hip) --------------------------------------------------
 * The 1x1 lateral conv over cat([fine, F.interpolate(coarse, bilinear, align_corners=True)]) (generalized_lss.py:83-100)
 * under autograd: upsample_bilinear2d_backward + cat backward + the conv's wgrad / dgrad.  With output-gradient token
 * rows G [batch*height*width, N]:  dW[:, :C1] = G^T . fine,  dW[:, C1:] = (up^T G)^T . coarse,
 * dcoarse = (up^T G) . W[:, C1:] (isf_swin_gemm, ROWS loader, weight packed by isf_pack_linear_transposed).
 * isf_upsample_rows_adjoint: g2 [batch*height2*width2, channels] = up^T g, the adjoint of the UPCAT loader's bilinear
 *   sample (same float expressions for the taps); gather form, fixed summation order, no atomics.  channels % 4 == 0.
 * isf_rows_weight_grad: dw[n, kk] (row stride ldw) = *inv_scale * sum_r g[r, n] * x[r, kk] for g rows [num_rows,
 *   out_features] and x rows [num_rows, ldx] (x_hw == 0) or an NCHW map [num_rows / x_hw, k, x_hw] (x_hw > 0).  f16
 *   hi/lo split of both operands (g pre-scaled by a power of two, isf_grad_rescale; inv_scale NULL = 1), fp32 accumulate.
 *   workspace: fp32 [num_chunks, out_features, k] with num_chunks = isf_rows_weight_grad_chunks(num_rows, out_features,
 *   k); the chunks' partial sums are added in chunk order: bit-identical run to run. */
int isf_upsample_rows_adjoint(const float* g, int batch, int height, int width, int channels, int height2, int width2,
                              float* g2, isf_stream_t stream);
int isf_rows_weight_grad_chunks(int num_rows, int out_features, int k);
int isf_rows_weight_grad(const float* g, const float* x, int ldx, int x_hw, int num_rows, int out_features, int k,
                         const float* inv_scale, float* workspace, int num_chunks, float* dw, int ldw,
                         isf_stream_t stream);

/* Backward of the Swin-T backbone (isf_swin_train.hip) -------------------------------------------------------
 * What autograd runs under SwinTransformer.forward in training mode.  The matrix products are isf_swin_gemm on the
 * transposed packed weight (dX = dY . W) and isf_rows_weight_grad (dW = dY^T . X); the entries below are the rest.
 * Every reduction over rows, windows or images is two passes -- per-workgroup partial sums over a fixed range, then a
 * sum of the partials in index order -- so results are bit-identical run to run, without float atomics.  Gradient rows
 * arrive pre-scaled by a power of two (isf_grad_rescale); inv_scale (device scalar, NULL = 1) multiplies every
 * parameter gradient an entry writes.
 * isf_swin_operand_rows writes out the operand rows the A loader generates, out [num_rows, k]: ROWS / MERGE (with the
 *   LayerNorm prologue when a->ln_stats is set: the normalised rows X^ of dW = dY^T . X^ for WindowMSA.qkv, swin.py:88,
 *   FFN's first Linear, and PatchMerging.reduction in the loader's q*C + c order, utils/transformer.py:371-384), or
 *   PATCH with k = 16 c (im2col of PatchEmbed.projection, utils/transformer.py:250-252).
 * isf_swin_layernorm_backward differentiates nn.LayerNorm (SwinBlock.norm1 / norm2, swin.py:356-368; PatchEmbed.norm,
 *   utils/transformer.py:255-256; PatchMerging.norm, :383; the out_indices norms, swin.py:756-762) over the loader's
 *   rows x (ROWS or MERGE; a->ln_stats = the forward's (mean, rstd) rows, a->ln_gamma):
 *     dx = rstd (dy gamma - mean_k(dy gamma) - x^ mean_k(dy gamma x^)) + residual_grad,  dgamma = sum_r dy x^,
 *     dbeta = sum_r dy,  with dy read as rows [num_rows, k] or, dy_hw > 0, as an NCHW map [num_rows / dy_hw, k, dy_hw]
 *     (the layout swin.py:759-761 hands the out_indices maps out in) and multiplied by *dy_scale (NULL = 1).
 *   ROWS: dx rows [num_rows, k], residual_grad rows or NULL.  MERGE: dx token rows [n*h*w, c] -- the adjoint of
 *   nn.Unfold(2, 2) with corner padding (utils/transformer.py:368-371): every token lies in one merged row, the
 *   gradient of padded cells is dropped; no residual_grad.  k <= 1536.  workspace: fp32 [num_parts, 2, k],
 *   num_parts = isf_swin_layernorm_backward_parts(num_rows).
 * isf_swin_column_sums: out[c] = *inv_scale * (sum_r g[r, c] + extra[c]) (extra NULL = 0): the bias gradients of
 *   nn.Linear (swin.py:88 and :115, mmcv FFN) and PatchEmbed.projection.  workspace fp32 [num_parts, channels], num_parts =
 *   isf_swin_column_sums_parts(num_rows).
 * isf_swin_gelu_backward differentiates nn.GELU of mmcv FFN (erf form, activation 2 of isf_swin_gemm), in place:
 *   hidden holds the pre-activation z and receives gelu(z), grad holds dL/dgelu and receives dL/dz.
 * isf_swin_scale_rows: out[r, :] = g[r, :] * row_scale[r / rows_per_sample] -- the DropPath factor (swin.py:251, mmcv
 *   FFN) on a branch's incoming gradient; a factor 0 gives exact zeros.
 * isf_swin_window_attention_backward differentiates isf_swin_window_attention (ShiftWindowMSA + WindowMSA after the
 *   qkv Linear, swin.py:79-117 and :178-253) with the forward's geometry: dout [batch*height*width, channels] is the
 *   gradient of the attention output rows; the probabilities are recomputed from qkv.  Writes dqkv [batch*height*
 *   width, 3 channels] (every element), drel_bias [heads, 49, 49] (gradient of the gathered bias, in dout's scale),
 *   dtable [table_rows, heads] = *inv_scale * the sum of drel_bias over rel_index (int64 [49, 49], swin.py:96-100;
 *   dtable NULL = skip) and dqkv_bias_pad [3 channels]: padded cells produce no output but take part as keys and
 *   values with k / v = the qkv bias (the zero padding follows norm1, swin.py:187 after :360), so their dK / dV are gradient
 *   of the qkv bias and of nothing else; in dout's scale, [0, channels) is 0.  workspace: fp32 [num_groups * heads *
 *   (49 * 49 + 64)], num_groups = isf_swin_window_attention_backward_groups(...).  window 7, head dim 32. */
int isf_swin_operand_rows(const isf_swin_a* a, int num_rows, int k, float* out, isf_stream_t stream);
int isf_swin_layernorm_backward_parts(int num_rows);
int isf_swin_layernorm_backward(const isf_swin_a* a, int num_rows, int k, const float* dy, int dy_hw,
                                const float* dy_scale, const float* residual_grad, float* dx, const float* inv_scale,
                                float* workspace, int num_parts, float* dgamma, float* dbeta, isf_stream_t stream);
int isf_swin_column_sums_parts(int num_rows);
int isf_swin_column_sums(const float* g, int num_rows, int channels, const float* extra, const float* inv_scale,
                         float* workspace, int num_parts, float* out, isf_stream_t stream);
int isf_swin_gelu_backward(float* hidden, float* grad, size_t num_elems, isf_stream_t stream);
int isf_swin_scale_rows(const float* g, int num_rows, int channels, const float* row_scale, int rows_per_sample, float* out,
                        isf_stream_t stream);
int isf_swin_window_attention_backward_groups(int batch, int height, int width, int heads);
int isf_swin_window_attention_backward(const float* qkv, const float* qkv_bias, const float* rel_bias,
                                       const int64_t* rel_index, const float* dout, int batch, int height, int width,
                                       int channels, int heads, int window, int shift, float scale,
                                       const float* inv_scale, float* workspace, int num_groups, float* dqkv,
                                       float* drel_bias, float* dtable, int table_rows, float* dqkv_bias_pad,
                                       isf_stream_t stream);

/* Mixed-precision training of the Swin-T backbone (isf_swin.hip, isf_swin_train_f16.hip) ----------------------
 * SwinTransformer.set_precision("mixed"): what the reference trains under torch.autocast(float16) -- half products with
 * fp32 accumulation; fp32 master weights, residual stream, statistics, softmax and parameter gradients; the forward keeps
 * the f16 qkv rows and the f16 attention output.  The forward is the f16 inference mode's plus the entry below; dX = dY . W
 * is isf_swin_gemm_f16 on isf_pack_linear_f16 of the transposed weight; the other backward entries above stay fp32.
 * Gradient rows arrive pre-scaled by a power of two with their largest entry in [2^9, 2^10) (isf_grad_rescale).
 * isf_swin_gemm_f16_rowscale replaces the half nn.Linear followed by DropPath and the identity (WindowMSA.proj with
 *   swin.py:251, the second Linear of mmcv FFN with its DropPath): isf_swin_gemm_f16 with isf_swin_gemm_rowscale's factor,
 *     y = act((A . W^T) * scale + shift) * row_scale[r / rows_per_sample] + residual.
 *   Built for the ROWS loader on f16 A rows (a_is_f16 != 0) without the LayerNorm prologue and fp32 y (y_is_f16 == 0,
 *   y_hw == 0); any other form and a NULL row_scale are refused before a launch.  A factor 1 changes nothing by a bit, a
 *   factor 0 leaves the residual row exactly.
 * isf_rows_weight_grad_f16 replaces autograd's weight gradient of a half nn.Linear (swin.py:88 and :115, mmcv FFN,
 *   PatchMerging.reduction, PatchEmbed.projection as im2col rows): isf_rows_weight_grad with ONE matrix instruction per
 *   product.  g fp32 rows [num_rows, out_features] and x rows [num_rows, ldx] -- fp32, or _Float16 when x_is_f16 != 0 (ldx
 *   in elements of the row type) -- are rounded to f16 in the kernel (nearest even, saturating at +-65504); products are
 *   exact in fp32, accumulation is fp32.  Row-major x only.  workspace, num_chunks, inv_scale, dw / ldw and the
 *   run-to-run bit identity as isf_rows_weight_grad.
 * isf_swin_window_attention_backward_f16 differentiates isf_swin_window_attention_f16 (ShiftWindowMSA + WindowMSA after
 *   the half qkv Linear, swin.py:79-117 and :178-253) on the matrix cores: qkv is _Float16 rows [batch*height*width,
 *   3 channels] as the forward stored them (a padded cell's q / k / v = the f16-rounded qkv_bias), every other argument,
 *   output, scale and the workspace (isf_swin_window_attention_backward_groups) as isf_swin_window_attention_backward.
 *   Scores, softmax, dP - rowsum(P dP), every accumulation and the bias gradient (summed from the unrounded dS) are
 *   fp32; only P, dS and dO are rounded to f16, as operands of the next product.  dO is read as dout * 2^-6 and every
 *   output multiplied by 2^6 (exact): for |dout| < 2^10 and |v| <= 32 (value third of qkv and of qkv_bias) neither dO
 *   nor dS reaches f16's range (|dS 2^-6| < 2^15), and beyond it the operand stores saturate at +-65504 instead of
 *   producing inf.  Entries with |dS 2^-6| < 2^-14 fall into f16's subnormals (absolute error <= 2^-19 in dout's
 *   scale).  Bit-identical run to run. */
int isf_swin_gemm_f16_rowscale(const isf_swin_a* a, int a_is_f16, int num_rows, int k, const void* packed_weight_f16,
                               int out_features, const float* scale, const float* shift, int activation,
                               const float* residual, const float* row_scale, int rows_per_sample, void* y, int y_is_f16,
                               int ldy, int y_hw, isf_stream_t stream);
int isf_rows_weight_grad_f16(const float* g, const void* x, int x_is_f16, int ldx, int num_rows, int out_features, int k,
                             const float* inv_scale, float* workspace, int num_chunks, float* dw, int ldw,
                             isf_stream_t stream);
int isf_swin_window_attention_backward_f16(const void* qkv, const float* qkv_bias, const float* rel_bias,
                                           const int64_t* rel_index, const float* dout, int batch, int height, int width,
                                           int channels, int heads, int window, int shift, float scale,
                                           const float* inv_scale, float* workspace, int num_groups, float* dqkv,
                                           float* drel_bias, float* dtable, int table_rows, float* dqkv_bias_pad,
                                           isf_stream_t stream);

/* Fused AdamW with global-norm gradient clipping (isf_optim.hip) ---------------------------------------------
 * isf_optim_grad_sumsq + isf_optim_adamw replace, together, mmcv OptimizerHook.clip_grads (mmcv/runner/hooks/
 *   optimizer.py: torch.nn.utils.clip_grad_norm_ over every gradient, max_norm, norm_type 2) followed by the step of
 *   torch.optim.AdamW as built by build_optimizer (mmdet3d/apis/train.py:92; torch 2.x _single_tensor_adam with decoupled
 *   weight decay): 2 launches for any number of tensors and param groups, no host sync, no copy.
 * isf_optim_grad_sumsq + isf_optim_adamw(mode ISF_OPTIM_SCALE_GRADS) replace torch.nn.utils.clip_grad_norm_ alone: the
 *   gradients are scaled in place (not written when the coefficient is 1).
 *   tensors: DEVICE int64 [T, 6] = p, g, exp_avg, exp_avg_sq (addresses of contiguous fp32 storage; p / m / v unused in
 *   ISF_OPTIM_SCALE_GRADS), numel, hyperparameter tuple index.  chunks: DEVICE int32 [num_chunks, 2] = tensor, chunk k =
 *   elements [k * ISF_OPTIM_CHUNK, min((k + 1) * ISF_OPTIM_CHUNK, numel)).  Any 4-byte alignment is accepted.
 *   partials: fp64 [num_chunks], one sum of squares per chunk (fixed-order reduction: bit-identical run to run).
 *   isf_optim_adamw: every workgroup reduces the partials in one fixed order, norm = sqrt(sum),
 *   coef = min(1, max_norm / (norm + 1e-6)) (ISF_OPTIM_NO_CLIP: coef = 1, partials / norm_out unused), norm_out[0] =
 *   norm (fp32 device scalar); then per element g' = g * coef and p *= decay; m = lerp(m, g', w1);
 *   v = v * b2 + w2 * g' * g'; p += neg_step_size * m / (sqrt(v) / bc2_sqrt + eps).  .grad is not written (except in
 *   ISF_OPTIM_SCALE_GRADS).  hp: num_hp HOST tuples, passed as kernel arguments while num_hp <= ISF_OPTIM_MAX_HP_ARGS;
 *   above that hp_device (DEVICE, num_hp tuples) is read instead.  Every field is computed on the host in double:
 *   decay = 1 - lr * wd, w1 = 1 - b1, w2 = 1 - b2, neg_step_size = -lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t). */
#define ISF_OPTIM_CHUNK 32768
#define ISF_OPTIM_MAX_HP_ARGS 16
#define ISF_OPTIM_NO_CLIP 0
#define ISF_OPTIM_CLIP 1
#define ISF_OPTIM_SCALE_GRADS 2
typedef struct isf_adamw_hp {
  float decay, w1, b2, w2, eps, neg_step_size, bc2_sqrt, pad;
} isf_adamw_hp;
int isf_optim_grad_sumsq(const int64_t* tensors, const int32_t* chunks, int num_chunks, double* partials,
                         isf_stream_t stream);
int isf_optim_adamw(const int64_t* tensors, const int32_t* chunks, int num_chunks, const isf_adamw_hp* hp, int num_hp,
                    const isf_adamw_hp* hp_device, const double* partials, float max_norm, float* norm_out, int mode,
                    isf_stream_t stream);

/* Exact cross-rank sums (isf_fixed_reduce.hip) -----------------------------------------------------------------
 * The fixed-point sum of the DETERMINISTIC ENTRIES carried across the ranks of a data-parallel job.  A float all-reduce
 *   (DistributedDataParallel's gradient buckets, mmdet3d/apis/train.py:82-86; the [2C] statistic vectors of naiveSyncBN,
 *   mmdet3d/ops/norm.py:12-24,186) rounds after every add, so its bits depend on the collective's algorithm and on the
 *   order of the ranks.  Here each rank turns its contribution into 64-bit integers, the COLLECTIVE SUMS INTEGERS, and
 *   the sum is converted back: the result is a function of the multiset of the ranks' contributions only, whatever the
 *   backend, the algorithm or the rank order.  isf_fixed_absmax_tensors / isf_fixed_pack_tensors /
 *   isf_fixed_finish_tensors are the passes around two integer all-reduces, one launch each for any number of tensors;
 *   isf_fixed_sum_rows is the whole sum for W gathered copies of one short vector.
 *   tensors: DEVICE int64 [T, 3] = address of contiguous fp32 storage (any 4-byte alignment), numel, offset of the
 *   tensor's first element in q.  chunks: DEVICE int32 [num_chunks, 2] = tensor, chunk k = elements
 *   [k * ISF_OPTIM_CHUNK, min((k + 1) * ISF_OPTIM_CHUNK, numel)); one workgroup per chunk.  No host sync, no float atomic.
 * isf_fixed_absmax_tensors: bits [num_tensors] is zeroed, then bits[t] = the largest bit pattern of |x| in tensor t
 *   (integer max: order-free; an inf or a NaN shows as bits[t] >= 0x7f800000).  The caller takes the integer MAX of bits
 *   over the ranks before the next two passes.
 * isf_fixed_pack_tensors: per tensor A = the bound bits[t], A < 2^ex (frexp's exponent), e = 62 - log2_world - ex with
 *   log2_world = ceil(log2(world size)) in [0, 10]; q[offset_t + i] = llrint(ldexp((double)x_i, e)) (int64; the scaling
 *   is exact, |q| <= 2^(62 - log2_world), so the sum over the ranks stays below 2^62).  A == 0 and a non-finite bound
 *   give zeros.  The caller takes the int64 SUM of q over the ranks.
 * isf_fixed_finish_tensors: x_i = (float)(ldexp((double)q[offset_t + i], -e) / divisor), divisor in [1, 1024] (the world
 *   size for a mean, 1 for a sum); EVERY element of a tensor whose bound is not finite becomes NaN.
 * isf_fixed_sum_rows: out[c] = the exact sum over r < W of rows[r * n + c], divided by divisor, W <= ISF_FIXED_MAX_ROWS:
 *   per column the bound over the W values, e = 62 - ceil(log2 W) - ex, the integer sum and the same finish.  A column
 *   that holds a non-finite value gives NaN in that column only.  Independent of the order of the rows. */
#define ISF_FIXED_MAX_ROWS 64
int isf_fixed_absmax_tensors(const int64_t* tensors, const int32_t* chunks, int num_chunks, int num_tensors, uint32_t* bits,
                             isf_stream_t stream);
int isf_fixed_pack_tensors(const int64_t* tensors, const int32_t* chunks, int num_chunks, const uint32_t* bits,
                           int log2_world, int64_t* q, isf_stream_t stream);
int isf_fixed_finish_tensors(const int64_t* tensors, const int32_t* chunks, int num_chunks, const uint32_t* bits,
                             int log2_world, const int64_t* q, double divisor, isf_stream_t stream);
int isf_fixed_sum_rows(const float* rows, int W, int n, double divisor, float* out, isf_stream_t stream);

/* nuScenes detection evaluation: mAP / NDS on the device (isf_eval.hip) ----------------------------------------
 * Together the four stages replace NuScenesDataset._evaluate_single (mmdet3d/datasets/nuscenes_dataset.py:421-476: the
 *   JSON round trip and the nuScenes devkit's DetectionEval on the host) for boxes that are already on the device; the
 *   protocol as built, the frame, the tie rule and the statement on devkit parity are DESIGN.md section 4.0f.  All arithmetic
 *   is fp64 on the fp32 rows.  No stage syncs or copies to the host.
 * isf_eval_attributes replaces the attribute heuristic of _format_bbox (nuscenes_dataset.py:378-397): attrs[i] =
 *   hypot(boxes[i][7], boxes[i][8]) > 0.2 ? moving_attr[label] : still_attr[label] (HOST tables of num_classes attribute
 *   ids, -1 = none); -1 for labels outside [0, num_classes).
 * isf_eval_match replaces the range filter of lidar_nusc_box_to_global (nuscenes_dataset.py:690-697) and the devkit's
 *   greedy matching (accumulate).  Sample s owns prediction rows [pred_off[s], pred_off[s + 1]) (<= max_pred <=
 *   ISF_EVAL_MAX_PRED each) and ground-truth rows [gt_off[s], gt_off[s + 1]) (<= max_gt <= ISF_EVAL_MAX_GT each); the
 *   offsets are DEVICE int32 [num_samples + 1].  Boxes are [rows, 9] (x, y, z_bottom, dx, dy, dz, yaw, vx, vy).  A row
 *   is dropped when pred_valid is 0, its label is outside [0, num_classes), its score is NaN, gt_num_pts (NULL = all
 *   kept) is <= 0, or |(M c)_xy| > class_range[label] with M = lidar2ego[s] (fp64 [4, 4], row major) and c the gravity
 *   centre.  Per sample the kept predictions are ordered by descending score, equal scores by ascending row, and walked
 *   once per distance threshold (HOST dist_ths, num_ths <= ISF_EVAL_MAX_THS): a prediction takes the nearest not yet
 *   taken box of its class (xy centre distance, the lowest row on a tie) when that distance is < the threshold.
 *   Outputs BY POSITION q = pred_off[s] + rank in that order (dropped rows fill the tail of the sample): keys (a uint32
 *   whose ascending order is descending score), cls (the label; num_classes for a dropped row), tp_mask (bit t: TP at
 *   threshold t), conf (the score) and, where bit tp_index is set, errs [rows, 5] = trans, scale, orient (period pi where
 *   half_period[label]), vel, attr (NaN when the box's gt_attrs is < 0 or gt_attrs is NULL).  tp_mask_rows is the mask
 *   by input row.  counts (DEVICE int32 [2 * num_classes], zeroed here) = kept boxes, then kept predictions, per class.
 * isf_eval_order replaces the devkit's sort of a class's predictions by confidence: order [rows] = the positions in the
 *   stable order of (cls, keys), i.e. class by class, descending score, ties by (sample, row).
 * isf_eval_curves replaces the rest of accumulate: per (class, threshold) cumulative TP / FP over the class's segment and
 *   np.interp onto recall_points (DEVICE fp64 [ISF_EVAL_POINTS], computed by the host); at tp_index the cumulative means
 *   of the five errors over the matches and their interpolation onto the confidence curve.  curves [num_classes,
 *   2 * num_ths + 5, ISF_EVAL_POINTS]: precision per threshold, confidence per threshold, the five TP curves.
 * isf_eval_scalars replaces calc_ap, calc_tp, the per-class NaN rules (HOST nan_mask [num_classes], bit m = metric m is
 *   NaN) and DetectionMetrics.serialize's aggregates.  result (fp64): ap [num_classes, num_ths], tp [num_classes, 5],
 *   mean_dist_aps [num_classes], max_recall_ind [num_classes], tp_errors [5], tp_scores [5], mean_ap, nd_score. */
#define ISF_EVAL_MAX_CLASSES 31
#define ISF_EVAL_MAX_PRED 500
#define ISF_EVAL_MAX_GT 1024
#define ISF_EVAL_MAX_THS 4
#define ISF_EVAL_NUM_ERRS 5
#define ISF_EVAL_POINTS 101
int isf_eval_attributes(const int32_t* labels, const float* boxes, int box_ld, long long rows, int num_classes,
                        const int* moving_attr, const int* still_attr, int32_t* attrs, isf_stream_t stream);
int isf_eval_match(const float* pred_boxes, const float* pred_scores, const int32_t* pred_labels, const uint8_t* pred_valid,
                   const int32_t* pred_attrs, const int32_t* pred_off, int max_pred, const float* gt_boxes,
                   const int32_t* gt_labels, const int32_t* gt_attrs, const int32_t* gt_num_pts, const int32_t* gt_off,
                   int max_gt, const double* lidar2ego, int num_samples, int num_classes, const float* class_range,
                   const int* half_period, const double* dist_ths, int num_ths, int tp_index, uint32_t* keys, int32_t* cls,
                   uint8_t* tp_mask, uint8_t* tp_mask_rows, double* conf, double* errs, int32_t* counts, isf_stream_t stream);
int isf_eval_order(const uint32_t* keys, const int32_t* cls, int rows, int num_classes, int32_t* order, isf_stream_t stream);
int isf_eval_curves(const int32_t* order, const uint8_t* tp_mask, const double* conf, const double* errs, const int32_t* counts,
                    const double* recall_points, int rows, int num_classes, int num_ths, int tp_index, double* curves,
                    isf_stream_t stream);
int isf_eval_scalars(const double* curves, int num_classes, int num_ths, int tp_index, const int* nan_mask, double min_recall,
                     double min_precision, double mean_ap_weight, double* result, isf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ISF_HIP_H */
