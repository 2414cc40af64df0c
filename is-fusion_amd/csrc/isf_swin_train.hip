// isf_swin_train.hip -- backward of the GeneralizedLSSFPN top-down step (1x1 lateral conv over
// cat([fine, bilinear_up(coarse)])), the training half of isf_swin.hip.
//
// Reference: mmdet3d/models/necks/generalized_lss.py:83-100 under autograd -- upsample_bilinear2d_backward (float atomics),
// cat backward, cuDNN 1x1 wgrad / dgrad.  Upsampling is linear, so with output-gradient rows G [B*H*W, N]:
//   dW[:, :C1] = G^T . fine,   dW[:, C1:] = (up^T G)^T . coarse,   dcoarse = (up^T G) . W[:, C1:]
// and no GEMM samples anything.  Here:
//   isf_upsample_rows_adjoint  G2 = up^T G on token rows, in gather form: one wave per coarse cell sums, in a fixed order,
//                        the fine cells whose forward taps touch it.  The taps (y0, x0, dy, dx, ly, lx) are recomputed
//                        with the float expressions of the forward loader (swin_load_a<UPCAT>, isf_swin.hip).  No atomics.
//   isf_rows_weight_grad dW [N, K] = G^T . X with X token rows [R, K] or an NCHW map [B, K, hw] (contraction index
//                        contiguous per channel).  f16 hi/lo split of both operands, 3 x v_mfma_f32_16x16x32_f16 per
//                        product, fp32 accumulate (as swin_gemm_kernel).  tiling: workgroup 128 (n) x 64 (k) of dW,
//                        4 waves of 32 x 64; the R rows are cut into isf_rows_weight_grad_chunks() chunks (a multiple of
//                        the 32-row MFMA step each) so that tiles x chunks fill the chip; both operands go through a
//                        double-buffered LDS ring (48 KiB) as [hi|lo][8-row group][column] 16-byte slots -- a lane's MFMA
//                        fragment (8 consecutive rows of one column) is one slot.  Partials [chunks, N, K] fp32 are
//                        summed chunk 0, 1, 2, ... by a second launch (times the gradient's inverse power-of-two scale):
//                        bit-identical run to run.
//   dcoarse is isf_swin_gemm (ROWS loader) on G2 with the transposed packed W[:, C1:].
#include "isf_common.h"

namespace isf {

typedef _Float16 wh8 __attribute__((ext_vector_type(8)));
typedef float wf4 __attribute__((ext_vector_type(4)));
typedef float wf8 __attribute__((ext_vector_type(8)));

constexpr int WG_TN = 128;     // dW rows (n) per workgroup
constexpr int WG_TK = 64;      // dW columns (k) per workgroup
constexpr int WG_STEP = 32;    // token rows per MFMA step
constexpr int WG_TARGET = 512; // workgroups a launch aims at (2 per CU)

__device__ __forceinline__ void wg_split8(const wf8 v, wh8& hi, wh8& lo) {
  hi = __builtin_convertvector(v, wh8);
  const wf8 r = v - __builtin_convertvector(hi, wf8);
  lo = __builtin_convertvector(r, wh8);
}

static int wgrad_rows_per_chunk(int R, int N, int K) {
  const int tiles = ceil_div(N, WG_TN) * ceil_div(K, WG_TK);
  const int steps = ceil_div(R, WG_STEP);
  int chunks = ceil_div(WG_TARGET, tiles);
  if (chunks > steps) chunks = steps;
  if (chunks < 1) chunks = 1;
  return ceil_div(steps, chunks) * WG_STEP;
}

// 8 consecutive token rows rb .. rb + 7 (< rend kept, the rest 0) of column `col`
template <bool NCHW>
__device__ __forceinline__ wf8 wg_load8(const float* __restrict__ x, int ld, int hw, int C, int rb, int rend, int col,
                                        bool col_ok) {
  wf8 v = wf8{0, 0, 0, 0, 0, 0, 0, 0};
  if (!col_ok || rb >= rend) return v;
  if (NCHW) {
    const int b = rb / hw, pos = rb - b * hw;
    if (rb + 8 <= rend && pos + 8 <= hw) {
      const float* p = x + ((size_t)b * C + col) * hw + pos;
      if (((uintptr_t)p & 15) == 0) {
        const float4 a = *reinterpret_cast<const float4*>(p);
        const float4 c = *reinterpret_cast<const float4*>(p + 4);
        return wf8{a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = p[j];
      return v;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = rb + j;
      if (r < rend) {
        const int bb = r / hw, pp = r - bb * hw;
        v[j] = x[((size_t)bb * C + col) * hw + pp];
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (rb + j < rend) v[j] = x[(size_t)(rb + j) * ld + col];
  }
  return v;
}

template <bool NCHW>
__global__ __launch_bounds__(256) void rows_wgrad_kernel(const float* __restrict__ g, const float* __restrict__ x, int ldx,
                                                          int x_hw, int R, int N, int K, int rows_per_chunk,
                                                          float* __restrict__ ws) {
  __shared__ uint4 as_[2][2][4][WG_TN];   // [buf][hi|lo][8-row group][n]
  __shared__ uint4 bs_[2][2][4][WG_TK];   // [buf][hi|lo][8-row group][k]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int k0 = blockIdx.x * WG_TK, n0 = blockIdx.y * WG_TN;
  const int rbeg = blockIdx.z * rows_per_chunk;
  const int rend = rbeg + rows_per_chunk < R ? rbeg + rows_per_chunk : R;
  const int steps = (rend - rbeg + WG_STEP - 1) / WG_STEP;
  // loader slots: G two per thread (n = t & 127, row groups 2 (t >> 7) + i), X one (k = t & 63, row group t >> 6)
  const int an = t & 127, ag = (t >> 7) << 1;
  const int bk = t & 63, bg = t >> 6;
  const bool an_ok = n0 + an < N, bk_ok = k0 + bk < K;
  wf8 av[2], bv;
  auto fetch = [&](int s) {
    const int r0 = rbeg + s * WG_STEP;
#pragma unroll
    for (int i = 0; i < 2; ++i) av[i] = wg_load8<false>(g, N, 0, 0, r0 + 8 * (ag + i), rend, n0 + an, an_ok);
    bv = wg_load8<NCHW>(x, ldx, x_hw, K, r0 + 8 * bg, rend, k0 + bk, bk_ok);
  };
  auto commit = [&](int buf) {
    wh8 hi, lo;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      wg_split8(av[i], hi, lo);
      as_[buf][0][ag + i][an] = *reinterpret_cast<const uint4*>(&hi);
      as_[buf][1][ag + i][an] = *reinterpret_cast<const uint4*>(&lo);
    }
    wg_split8(bv, hi, lo);
    bs_[buf][0][bg][bk] = *reinterpret_cast<const uint4*>(&hi);
    bs_[buf][1][bg][bk] = *reinterpret_cast<const uint4*>(&lo);
  };
  wf4 acc[2][4];
#pragma unroll
  for (int gi = 0; gi < 2; ++gi)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[gi][nt] = wf4{0.f, 0.f, 0.f, 0.f};
  fetch(0);
  commit(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const int buf = s & 1;
    const bool more = s + 1 < steps;
    if (more) fetch(s + 1);
    wh8 ah[2], al[2];
#pragma unroll
    for (int gi = 0; gi < 2; ++gi) {
      const int n = wave * 32 + gi * 16 + (lane & 15);
      const uint4 h = as_[buf][0][lane >> 4][n], l = as_[buf][1][lane >> 4][n];
      ah[gi] = *reinterpret_cast<const wh8*>(&h);
      al[gi] = *reinterpret_cast<const wh8*>(&l);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const uint4 bhu = bs_[buf][0][lane >> 4][nt * 16 + (lane & 15)], blu = bs_[buf][1][lane >> 4][nt * 16 + (lane & 15)];
      const wh8 bh = *reinterpret_cast<const wh8*>(&bhu);
      const wh8 bl = *reinterpret_cast<const wh8*>(&blu);
#pragma unroll
      for (int gi = 0; gi < 2; ++gi) {
        acc[gi][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[gi], bh, acc[gi][nt], 0, 0, 0);
        acc[gi][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[gi], bl, acc[gi][nt], 0, 0, 0);
        acc[gi][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[gi], bh, acc[gi][nt], 0, 0, 0);
      }
    }
    if (more) commit(buf ^ 1);   // the other buffer was last read before the previous barrier
    __syncthreads();
  }
  // C/D layout: lane holds rows 16 gi + 4 (lane >> 4) + j of the wave's 32 n, column 16 nt + (lane & 15) of the 64 k
  float* out = ws + (size_t)blockIdx.z * N * K;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int k = k0 + nt * 16 + (lane & 15);
    if (k >= K) continue;
#pragma unroll
    for (int gi = 0; gi < 2; ++gi) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + wave * 32 + gi * 16 + 4 * (lane >> 4) + j;
        if (n < N) out[(size_t)n * K + k] = acc[gi][nt][j];
      }
    }
  }
}

// dW[n, k] = inv_scale * (ws[0] + ws[1] + ... + ws[chunks - 1])[n, k]
__global__ __launch_bounds__(256) void rows_wgrad_reduce_kernel(const float* __restrict__ ws, int chunks, int N, int K,
                                                                 const float* __restrict__ inv_scale,
                                                                 float* __restrict__ dw, int ldw) {
  const size_t total = (size_t)N * K;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += ws[(size_t)c * total + i];
  if (inv_scale) s *= *inv_scale;
  const int n = (int)(i / K), k = (int)(i - (size_t)n * K);
  dw[(size_t)n * ldw + k] = s;
}

// forward taps of fine coordinate d along one axis (the expressions of swin_load_a<UPCAT>): source cells c0 and c0 + dc
// with weights l0 and l1
__device__ __forceinline__ void up_taps(int d, float scale, int in, int& c0, int& dc, float& l0, float& l1) {
  const float f = scale * d;
  c0 = (int)f;
  dc = c0 < in - 1 ? 1 : 0;
  l1 = f - c0;
  l0 = 1.f - l1;
}

// fine coordinates whose taps can touch coarse cell c: [lo, hi] (a superset; the caller tests each one exactly)
__device__ __forceinline__ void up_candidates(int c, float scale, int out, int& lo, int& hi) {
  if (scale <= 0.f) { lo = 0; hi = out - 1; return; }   // out == 1 (or a 1-cell source): every fine cell reads cell 0
  const float inv = 1.f / scale;
  lo = (int)floorf((float)(c - 1) * inv) - 1;
  hi = (int)ceilf((float)(c + 1) * inv) + 1;
  if (lo < 0) lo = 0;
  if (hi > out - 1) hi = out - 1;
}

// one wave per coarse cell (b, Y, X); lane -> 4 channels per 256
__global__ __launch_bounds__(64) void upsample_rows_adjoint_kernel(const float* __restrict__ g, int H, int W, int N, int H2,
                                                                    int W2, float* __restrict__ g2) {
  const int cell = blockIdx.x, b = blockIdx.y;
  const int Y = cell / W2, X = cell - Y * W2;
  const float sy = H > 1 ? (float)(H2 - 1) / (float)(H - 1) : 0.f;
  const float sx = W > 1 ? (float)(W2 - 1) / (float)(W - 1) : 0.f;
  int ylo, yhi, xlo, xhi;
  up_candidates(Y, sy, H, ylo, yhi);
  up_candidates(X, sx, W, xlo, xhi);
  const float* gb = g + (size_t)b * H * W * N;
  float* dst = g2 + ((size_t)b * H2 * W2 + cell) * N;
  for (int c = threadIdx.x * 4; c < N; c += 256) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int y = ylo; y <= yhi; ++y) {
      int y0, dy;
      float ly0, ly1;
      up_taps(y, sy, H2, y0, dy, ly0, ly1);
      const bool ty0 = y0 == Y, ty1 = y0 + dy == Y;
      if (!ty0 && !ty1) continue;
      for (int x = xlo; x <= xhi; ++x) {
        int x0, dx;
        float lx0, lx1;
        up_taps(x, sx, W2, x0, dx, lx0, lx1);
        const bool tx0 = x0 == X, tx1 = x0 + dx == X;
        if (!tx0 && !tx1) continue;
        // the forward value is ly0 (lx0 s00 + lx1 s01) + ly1 (lx0 s10 + lx1 s11): this cell's share of it
        float wgt = 0.f;
        if (ty0 && tx0) wgt += ly0 * lx0;
        if (ty0 && tx1) wgt += ly0 * lx1;
        if (ty1 && tx0) wgt += ly1 * lx0;
        if (ty1 && tx1) wgt += ly1 * lx1;
        const float4 v = *reinterpret_cast<const float4*>(gb + ((size_t)y * W + x) * N + c);
        acc.x = fmaf(wgt, v.x, acc.x);
        acc.y = fmaf(wgt, v.y, acc.y);
        acc.z = fmaf(wgt, v.z, acc.z);
        acc.w = fmaf(wgt, v.w, acc.w);
      }
    }
    *reinterpret_cast<float4*>(dst + c) = acc;
  }
}

}  // namespace isf

extern "C" {

int isf_rows_weight_grad_chunks(int num_rows, int out_features, int k) {
  using namespace isf;
  if (num_rows <= 0 || out_features <= 0 || k <= 0) return 0;
  return ceil_div(num_rows, wgrad_rows_per_chunk(num_rows, out_features, k));
}

int isf_rows_weight_grad(const float* g, const float* x, int ldx, int x_hw, int num_rows, int out_features, int k,
                         const float* inv_scale, float* workspace, int num_chunks, float* dw, int ldw,
                         isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num_rows > 0 && out_features > 0 && k > 0, ISF_ERR_ARG, "rows_weight_grad: bad sizes (rows %d, N %d, K %d)",
              num_rows, out_features, k);
  ISF_REQUIRE(g && x && workspace && dw && ldw >= k, ISF_ERR_ARG, "rows_weight_grad: null pointer or ldw %d < K %d", ldw, k);
  ISF_REQUIRE(x_hw > 0 ? num_rows % x_hw == 0 : ldx >= k, ISF_ERR_ARG,
              "rows_weight_grad: X rows need ldx >= K, an X map needs rows %% hw == 0");
  ISF_REQUIRE(num_chunks == isf_rows_weight_grad_chunks(num_rows, out_features, k), ISF_ERR_ARG,
              "rows_weight_grad: workspace of %d chunks, isf_rows_weight_grad_chunks says %d", num_chunks,
              isf_rows_weight_grad_chunks(num_rows, out_features, k));
  const int rpc = wgrad_rows_per_chunk(num_rows, out_features, k);
  hipStream_t st = as_stream(stream);
  const dim3 grid(ceil_div(k, WG_TK), ceil_div(out_features, WG_TN), num_chunks), block(256);
  ISF_REQUIRE(grid.z <= 65535 && grid.y <= 65535, ISF_ERR_UNSUPPORTED, "rows_weight_grad: grid too large");
  if (x_hw > 0)
    hipLaunchKernelGGL(rows_wgrad_kernel<true>, grid, block, 0, st, g, x, 0, x_hw, num_rows, out_features, k, rpc, workspace);
  else
    hipLaunchKernelGGL(rows_wgrad_kernel<false>, grid, block, 0, st, g, x, ldx, 0, num_rows, out_features, k, rpc,
                       workspace);
  ISF_LAUNCH_CHECK();
  hipLaunchKernelGGL(rows_wgrad_reduce_kernel, dim3(ceil_div((long long)out_features * k, 256)), block, 0, st, workspace,
                     num_chunks, out_features, k, inv_scale, dw, ldw);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_upsample_rows_adjoint(const float* g, int batch, int height, int width, int channels, int height2, int width2,
                              float* g2, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(batch >= 0 && height > 0 && width > 0 && height2 > 0 && width2 > 0 && channels > 0 && channels % 4 == 0,
              ISF_ERR_ARG, "upsample_rows_adjoint: bad sizes (channels %d need %% 4)", channels);
  if (batch == 0) return ISF_OK;
  ISF_REQUIRE(g && g2 && g != g2 && ((uintptr_t)g & 15) == 0 && ((uintptr_t)g2 & 15) == 0, ISF_ERR_ARG,
              "upsample_rows_adjoint: null, aliased or unaligned pointer");
  ISF_REQUIRE(batch <= 65535, ISF_ERR_UNSUPPORTED, "upsample_rows_adjoint: batch %d", batch);
  hipLaunchKernelGGL(upsample_rows_adjoint_kernel, dim3(height2 * width2, batch), dim3(64), 0, as_stream(stream), g, height,
                     width, channels, height2, width2, g2);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

}  // extern "C"
