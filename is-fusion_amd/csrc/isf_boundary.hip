// isf_boundary.hip -- native-op entry points of the reference that the fused HSF / IGF path does not need itself (on a
// dense BEV grid window membership is arithmetic, and InsContextAtt runs the fused single-level kernel in isf_fusion.hip)
// but that a maintainer binding the reference's op layer expects to find:
//   * TorchEx `ingroup_indices.forward(group_inds, out_inds)`  mmdet3d/ops/TorchEx/torchex/src/ingroup_inds/ingroup_inds.cpp:24-54,
//     ingroup_inds_kernel.cu:17-31 (get_inner_win_inds of SST, ops/sst/sst_ops.py:197-211)
//   * mmcv `_ext.ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step)`
//     (models/middle_encoders/multi_scale_deformable_attn_function.py:118-124; kernel ms_deform_im2col_cuda.cuh:237-299)
#include "isf_common.h"
#include "isf_fixed.h"

namespace isf {

// the two sort keys of a group id: its low and its high 32 bits
__global__ void ingroup_split_kernel(const int64_t* __restrict__ ids, int n, uint32_t* __restrict__ lo,
                                     uint32_t* __restrict__ hi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long v = (unsigned long long)ids[i];
  lo[i] = (uint32_t)v;
  hi[i] = (uint32_t)(v >> 32);
}

// order: the elements stably sorted by their id taken as an unsigned 64-bit number.  Equal ids are adjacent and in input
// order, so an element's rank in its group is its position minus the first position of its id: a lower-bound search.
__global__ void ingroup_first_come_kernel(const int64_t* __restrict__ ids, const int32_t* __restrict__ order, int n,
                                          int64_t* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int row = order[j];
  const unsigned long long id = (unsigned long long)ids[row];
  int lo = 0, hi = j;                          // the first position whose id is not below `id` lies in [0, j]
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if ((unsigned long long)ids[order[mid]] < id) lo = mid + 1;
    else hi = mid;
  }
  out[row] = (int64_t)(j - lo);
}

// one thread per (b, q, head, channel): channels of a head are consecutive lanes, so the four bilinear taps of a
// sampling point are coalesced 4*D-byte runs; the (level, point) loop is the reference's (ms_deform_im2col_cuda.cuh:262-296)
__global__ __launch_bounds__(256) void ms_deform_attn_kernel(
    const float* __restrict__ value, const int64_t* __restrict__ spatial_shapes, const int64_t* __restrict__ level_start,
    const float* __restrict__ loc, const float* __restrict__ weight, int B, int S, int M, int D, int Q, int L, int P,
    float* __restrict__ out) {
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)B * Q * M * D;
  if (tid >= total) return;
  const int d = (int)(tid % D);
  const int m = (int)((tid / D) % M);
  const long long bq = tid / ((long long)D * M);
  const int b = (int)(bq / Q);
  const float* wq = weight + (bq * M + m) * (long long)L * P;
  const float* lq = loc + (bq * M + m) * (long long)L * P * 2;
  const size_t vstride = (size_t)M * D;
  float acc = 0.f;
  for (int l = 0; l < L; ++l) {
    const int H = (int)spatial_shapes[2 * l], W = (int)spatial_shapes[2 * l + 1];
    const float* vb = value + ((size_t)b * S + (size_t)level_start[l]) * vstride + (size_t)m * D + d;
    for (int p = 0; p < P; ++p) {
      const float lx = lq[(l * P + p) * 2], ly = lq[(l * P + p) * 2 + 1];
      const float w_im = lx * (float)W - 0.5f, h_im = ly * (float)H - 0.5f;
      if (h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W) {
        const float fh = floorf(h_im), fw = floorf(w_im);
        const int h0 = (int)fh, w0 = (int)fw;
        const float lh = h_im - fh, lw = w_im - fw;
        float s = 0.f;
        if (h0 >= 0 && w0 >= 0) s += (1.f - lh) * (1.f - lw) * vb[((size_t)h0 * W + w0) * vstride];
        if (h0 >= 0 && w0 + 1 <= W - 1) s += (1.f - lh) * lw * vb[((size_t)h0 * W + w0 + 1) * vstride];
        if (h0 + 1 <= H - 1 && w0 >= 0) s += lh * (1.f - lw) * vb[((size_t)(h0 + 1) * W + w0) * vstride];
        if (h0 + 1 <= H - 1 && w0 + 1 <= W - 1) s += lh * lw * vb[((size_t)(h0 + 1) * W + w0 + 1) * vstride];
        acc += wq[l * P + p] * s;
      }
    }
  }
  out[tid] = acc;
}

// backward of ms_deform_attn_kernel with the mmcv op's contract (multi_scale_deformable_attn_function.py:150-160 ->
// ms_deformable_col2im, ms_deform_im2col_cuda.cuh:301-920): grad_value / grad_sampling_loc / grad_attn_weight are
// ZEROED BY THE CALLER and accumulated into.  Same thread mapping as the forward: one thread per (b, q, head,
// channel); the bilinear taps scatter into grad_value with atomics (a value cell is hit by many queries), the location
// and weight gradients of a (query, head, level, point) are first summed over the head's channels inside the wave
// (channels are consecutive lanes: a power-of-two head_dim <= 64 is one shuffle tree) and added once.
// AccV / AccW: where grad_value and (without the tree) grad_weight / grad_loc accumulate -- AccF32 = the caller's arrays,
// AccFixed = isf_ms_deform_attn_backward_det's fixed-point accumulators (isf_fixed.h).  With the tree a weight / location
// gradient receives ONE add onto the caller's zero, which no order can change, so AccW stays AccF32 there.  Bounds of that
// call: grad_value: A = absmax(grad_output) * max(1, absmax(attn_weight)) (the weights are an input here, not a softmax
// of ours), N = Q * P per level; grad_weight / grad_loc without the tree: A = 2 * num_keys (no level side is longer) *
// absmax(grad_output) * absmax(value) * max(1, absmax(attn_weight)), N = head_dim.  Resolution 2^-(62 - ceil(log2 N)) of the power of two above A.
template <bool TREE, class AccV, class AccW>
__global__ __launch_bounds__(256) void ms_deform_attn_backward_kernel(
    const float* __restrict__ value, const int64_t* __restrict__ spatial_shapes, const int64_t* __restrict__ level_start,
    const float* __restrict__ loc, const float* __restrict__ weight, const float* __restrict__ grad_out, int B, int S,
    int M, int D, int Q, int L, int P, AccV grad_value, AccW grad_loc, AccW grad_weight) {
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)B * Q * M * D;
  const bool live = tid < total;
  const long long t = live ? tid : total - 1;            // idle lanes shadow a live one: the shuffles stay uniform
  const int d = (int)(t % D);
  const int m = (int)((t / D) % M);
  const long long bq = t / ((long long)D * M);
  const int b = (int)(bq / Q);
  const long long qm = bq * M + m;
  const float* wq = weight + qm * (long long)L * P;
  const float* lq = loc + qm * (long long)L * P * 2;
  const size_t vstride = (size_t)M * D;
  const float go = live ? grad_out[t] : 0.f;
  for (int l = 0; l < L; ++l) {
    const int H = (int)spatial_shapes[2 * l], W = (int)spatial_shapes[2 * l + 1];
    const size_t vo = ((size_t)b * S + (size_t)level_start[l]) * vstride + (size_t)m * D + d;
    for (int p = 0; p < P; ++p) {
      const float lx = lq[(l * P + p) * 2], ly = lq[(l * P + p) * 2 + 1];
      const float aw = wq[l * P + p];
      const float w_im = lx * (float)W - 0.5f, h_im = ly * (float)H - 0.5f;
      float g_w = 0.f, g_x = 0.f, g_y = 0.f;
      if (h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W) {
        const float fh = floorf(h_im), fw = floorf(w_im);
        const int h0 = (int)fh, w0 = (int)fw;
        const float lh = h_im - fh, lw = w_im - fw, hh = 1.f - lh, hw = 1.f - lw;
        const float tg = go * aw;                          // top_grad * attn_weight
        float v1 = 0.f, v2 = 0.f, v3 = 0.f, v4 = 0.f;
        if (h0 >= 0 && w0 >= 0) {
          const size_t o = vo + ((size_t)h0 * W + w0) * vstride;
          v1 = value[o];
          if (live) grad_value.add(o, hh * hw * tg);
        }
        if (h0 >= 0 && w0 + 1 <= W - 1) {
          const size_t o = vo + ((size_t)h0 * W + w0 + 1) * vstride;
          v2 = value[o];
          if (live) grad_value.add(o, hh * lw * tg);
        }
        if (h0 + 1 <= H - 1 && w0 >= 0) {
          const size_t o = vo + ((size_t)(h0 + 1) * W + w0) * vstride;
          v3 = value[o];
          if (live) grad_value.add(o, lh * hw * tg);
        }
        if (h0 + 1 <= H - 1 && w0 + 1 <= W - 1) {
          const size_t o = vo + ((size_t)(h0 + 1) * W + w0 + 1) * vstride;
          v4 = value[o];
          if (live) grad_value.add(o, lh * lw * tg);
        }
        g_w = go * (hh * hw * v1 + hh * lw * v2 + lh * hw * v3 + lh * lw * v4);
        g_x = (float)W * tg * (-hh * v1 + hh * v2 - lh * v3 + lh * v4);
        g_y = (float)H * tg * (-hw * v1 - lw * v2 + hw * v3 + lw * v4);
      }
      if (TREE) {   // D lanes of one (query, head) are an aligned power-of-two lane group
        for (int s = D >> 1; s >= 1; s >>= 1) {
          g_w += __shfl_xor(g_w, s, 64);
          g_x += __shfl_xor(g_x, s, 64);
          g_y += __shfl_xor(g_y, s, 64);
        }
        if (live && d == 0) {
          grad_weight.add(qm * (long long)L * P + l * P + p, g_w);
          grad_loc.add((qm * (long long)L * P + l * P + p) * 2, g_x);
          grad_loc.add((qm * (long long)L * P + l * P + p) * 2 + 1, g_y);
        }
      } else if (live) {
        grad_weight.add(qm * (long long)L * P + l * P + p, g_w);
        grad_loc.add((qm * (long long)L * P + l * P + p) * 2, g_x);
        grad_loc.add((qm * (long long)L * P + l * P + p) * 2 + 1, g_y);
      }
    }
  }
}

}  // namespace isf

extern "C" {

int isf_ingroup_indices(const int64_t* group_inds, int num, int64_t* out_inds, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num >= 0, ISF_ERR_ARG, "ingroup_indices: bad size");
  if (num == 0) return ISF_OK;
  ISF_REQUIRE(group_inds && out_inds, ISF_ERR_ARG, "ingroup_indices: null pointer");
  hipStream_t st = as_stream(stream);
  Arena& a = arena_for_stream(as_stream(stream));
  ISF_TRY(a.reset());
  uint32_t *lo = nullptr, *hi = nullptr;
  int32_t *by_lo = nullptr, *order = nullptr;
  ISF_TRY(a.alloc_n(&lo, (size_t)num));
  ISF_TRY(a.alloc_n(&hi, (size_t)num));
  ISF_TRY(a.alloc_n(&by_lo, (size_t)num));
  ISF_TRY(a.alloc_n(&order, (size_t)num));
  const dim3 grid(ceil_div(num, 256)), block(256);
  hipLaunchKernelGGL(ingroup_split_kernel, grid, block, 0, st, group_inds, num, lo, hi);
  // stable LSD radix sort, low word first and the high word after it: equal group ids keep their input order, so the
  // position inside a segment is the first-come rank -- one of the numberings the reference's atomicAdd can produce, and
  // always the same one.  (How different ids are ordered among themselves -- here as unsigned numbers -- does not matter.)
  ISF_TRY(stable_sort_u32_impl(a, lo, num, 32, by_lo, st));
  ISF_TRY(stable_sort_u32_impl(a, hi, num, 32, order, st, nullptr, by_lo));
  hipLaunchKernelGGL(ingroup_first_come_kernel, grid, block, 0, st, group_inds, order, num, out_inds);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_ms_deform_attn_forward(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                               const float* sampling_loc, const float* attn_weight, int batch_size, int num_keys,
                               int num_heads, int head_dim, int num_queries, int num_levels, int num_points,
                               float* out, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(batch_size >= 0 && num_keys >= 0 && num_heads > 0 && head_dim > 0 && num_queries >= 0 &&
                  num_levels > 0 && num_points > 0, ISF_ERR_ARG, "ms_deform_attn_forward: bad sizes");
  if (batch_size == 0 || num_queries == 0) return ISF_OK;
  ISF_REQUIRE(value && spatial_shapes && level_start_index && sampling_loc && attn_weight && out, ISF_ERR_ARG,
              "ms_deform_attn_forward: null pointer");
  const long long total = (long long)batch_size * num_queries * num_heads * head_dim;
  hipLaunchKernelGGL(ms_deform_attn_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), value,
                     spatial_shapes, level_start_index, sampling_loc, attn_weight, batch_size, num_keys, num_heads,
                     head_dim, num_queries, num_levels, num_points, out);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_ms_deform_attn_backward(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                const float* sampling_loc, const float* attn_weight, const float* grad_output,
                                int batch_size, int num_keys, int num_heads, int head_dim, int num_queries,
                                int num_levels, int num_points, float* grad_value, float* grad_sampling_loc,
                                float* grad_attn_weight, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(batch_size >= 0 && num_keys >= 0 && num_heads > 0 && head_dim > 0 && num_queries >= 0 &&
                  num_levels > 0 && num_points > 0, ISF_ERR_ARG, "ms_deform_attn_backward: bad sizes");
  if (batch_size == 0 || num_queries == 0) return ISF_OK;
  ISF_REQUIRE(value && spatial_shapes && level_start_index && sampling_loc && attn_weight && grad_output &&
                  grad_value && grad_sampling_loc && grad_attn_weight, ISF_ERR_ARG,
              "ms_deform_attn_backward: null pointer");
  const long long total = (long long)batch_size * num_queries * num_heads * head_dim;
  const bool tree = head_dim <= 64 && (head_dim & (head_dim - 1)) == 0;
  if (tree)
    hipLaunchKernelGGL((ms_deform_attn_backward_kernel<true, AccF32, AccF32>), dim3(ceil_div(total, 256)), dim3(256), 0,
                       as_stream(stream), value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                       grad_output, batch_size, num_keys, num_heads, head_dim, num_queries, num_levels, num_points,
                       AccF32{grad_value}, AccF32{grad_sampling_loc}, AccF32{grad_attn_weight});
  else
    hipLaunchKernelGGL((ms_deform_attn_backward_kernel<false, AccF32, AccF32>), dim3(ceil_div(total, 256)), dim3(256), 0,
                       as_stream(stream), value, spatial_shapes, level_start_index, sampling_loc, attn_weight,
                       grad_output, batch_size, num_keys, num_heads, head_dim, num_queries, num_levels, num_points,
                       AccF32{grad_value}, AccF32{grad_sampling_loc}, AccF32{grad_attn_weight});
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_ms_deform_attn_backward_det(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                    const float* sampling_loc, const float* attn_weight, const float* grad_output,
                                    int batch_size, int num_keys, int num_heads, int head_dim, int num_queries,
                                    int num_levels, int num_points, float* grad_value, float* grad_sampling_loc,
                                    float* grad_attn_weight, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(batch_size >= 0 && num_keys >= 0 && num_heads > 0 && head_dim > 0 && num_queries >= 0 &&
                  num_levels > 0 && num_points > 0, ISF_ERR_ARG, "ms_deform_attn_backward_det: bad sizes");
  if (batch_size == 0 || num_queries == 0) return ISF_OK;
  ISF_REQUIRE(value && spatial_shapes && level_start_index && sampling_loc && attn_weight && grad_output &&
                  grad_value && grad_sampling_loc && grad_attn_weight, ISF_ERR_ARG,
              "ms_deform_attn_backward_det: null pointer");
  hipStream_t st = as_stream(stream);
  const long long total = (long long)batch_size * num_queries * num_heads * head_dim;
  const bool tree = head_dim <= 64 && (head_dim & (head_dim - 1)) == 0;
  const size_t nv = (size_t)batch_size * num_keys * num_heads * head_dim;
  const size_t nw = (size_t)batch_size * num_queries * num_heads * num_levels * num_points;
  Arena& a = arena_for_stream(st);
  ISF_TRY(a.reset());
  unsigned* bits = nullptr;   // [0] grad_output, [1] attn_weight, [2] value
  FixedCtl* ctl = nullptr;    // [0] grad_value, [1] grad_weight / grad_loc
  unsigned long long *accv = nullptr, *accw = nullptr;
  ISF_TRY(fixed_ctl_begin(a, &bits, &ctl, 2, st));
  const size_t nacc = nv + (tree ? 0 : 3 * nw);
  ISF_TRY(a.alloc_n(&accv, nacc));
  accw = accv + nv;
  ISF_HIP_TRY(hipMemsetAsync(accv, 0, nacc * sizeof(unsigned long long), st));
  ISF_TRY(fixed_absmax(grad_output, (size_t)total, bits + 0, st));
  ISF_TRY(fixed_absmax(attn_weight, nw, bits + 1, st));
  ISF_TRY(fixed_ctl(bits, 2, 2u, 0, ceil_log2((long long)num_queries * num_points), ctl, st));
  if (tree) {
    hipLaunchKernelGGL((ms_deform_attn_backward_kernel<true, AccFixed, AccF32>), dim3(ceil_div(total, 256)), dim3(256), 0, st,
                       value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, batch_size, num_keys,
                       num_heads, head_dim, num_queries, num_levels, num_points, AccFixed{accv, ctl},
                       AccF32{grad_sampling_loc}, AccF32{grad_attn_weight});
  } else {
    // the largest level side bounds the location gradients' factor W (H); it is an input on the device, so the bound takes
    // the largest side the key count allows: H, W <= num_keys
    ISF_TRY(fixed_absmax(value, nv, bits + 2, st));
    ISF_TRY(fixed_ctl(bits, 3, 2u, 1 + ceil_log2(num_keys > 1 ? num_keys : 1) + 1, ceil_log2(head_dim), ctl + 1, st));
    hipLaunchKernelGGL((ms_deform_attn_backward_kernel<false, AccFixed, AccFixed>), dim3(ceil_div(total, 256)), dim3(256), 0,
                       st, value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, batch_size,
                       num_keys, num_heads, head_dim, num_queries, num_levels, num_points, AccFixed{accv, ctl},
                       AccFixed{accw + nw, ctl + 1}, AccFixed{accw, ctl + 1});
  }
  ISF_LAUNCH_CHECK();
  ISF_TRY(fixed_finish(accv, ctl, nv, grad_value, true, nullptr, 1, st));
  if (tree) {
    ISF_TRY(fixed_poison(grad_attn_weight, nw, ctl, st));
    return fixed_poison(grad_sampling_loc, nw * 2, ctl, st);
  }
  ISF_TRY(fixed_finish(accw, ctl + 1, nw, grad_attn_weight, true, nullptr, 1, st));
  return fixed_finish(accw + nw, ctl + 1, nw * 2, grad_sampling_loc, true, nullptr, 1, st);
}

}  // extern "C"
