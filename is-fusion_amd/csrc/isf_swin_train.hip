// isf_swin_train.hip -- the training half of isf_swin.hip: backward of the GeneralizedLSSFPN top-down step (1x1 lateral
// conv over cat([fine, bilinear_up(coarse)])), and, in the second half of the file, the kernels of the Swin-T backbone's
// backward that are not a GEMM: window-attention backward, LayerNorm backward (also the PatchMerging gather adjoint),
// GELU backward, fixed-order column sums, the DropPath factor on gradient rows and the loader's operand rows written out
// (mmdet3d/models/backbones/swin.py and utils/transformer.py under autograd; include/isf_hip.h has the entries).
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

int wgrad_rows_per_chunk(int R, int N, int K) {
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

// ------------------------------------------------------------------------------------------ backbone backward
// Offset in a.x of element k of the loader's operand row r (the index arithmetic of swin_load_a, isf_swin.hip), or -1
// where the loader reads corner padding.
template <int MODE>
__device__ __forceinline__ long long swin_src_offset(const isf_swin_a& a, int r, int k) {
  if (MODE == ISF_SWIN_A_ROWS) {
    return (long long)r * a.ldx + k;
  } else if (MODE == ISF_SWIN_A_MERGE) {
    const int Ho = (a.h + 1) >> 1, Wo = (a.w + 1) >> 1;
    const int b = r / (Ho * Wo), rem = r - b * Ho * Wo, oy = rem / Wo, ox = rem - oy * Wo;
    const int q = k / a.c, ci = k - q * a.c;
    const int y = 2 * oy + (q >> 1), x = 2 * ox + (q & 1);
    return y < a.h && x < a.w ? ((long long)(b * a.h + y) * a.w + x) * a.c + ci : -1;
  } else {   // PATCH
    const int Ho = (a.h + 3) >> 2, Wo = (a.w + 3) >> 2;
    const int b = r / (Ho * Wo), rem = r - b * Ho * Wo, oy = rem / Wo, ox = rem - oy * Wo;
    const int ci = k >> 4, ky = (k >> 2) & 3, kx = k & 3;
    const int y = 4 * oy + ky, x = 4 * ox + kx;
    return ci < a.c && y < a.h && x < a.w ? ((long long)(b * a.c + ci) * a.h + y) * a.w + x : -1;
  }
}

// the loader's operand rows written out: out[r, k] = a(r, k), after the LayerNorm prologue when a.ln_stats is set.
// One wave per row.
template <int MODE>
__global__ __launch_bounds__(256) void swin_operand_rows_kernel(isf_swin_a a, int M, int K, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= M) return;
  const bool ln = a.ln_stats != nullptr;
  const float mean = ln ? a.ln_stats[2 * r] : 0.f, rstd = ln ? a.ln_stats[2 * r + 1] : 1.f;
  for (int k = lane; k < K; k += 64) {
    const long long off = swin_src_offset<MODE>(a, r, k);
    float v = off >= 0 ? a.x[off] : 0.f;
    if (ln) v = (v - mean) * rstd * a.ln_gamma[k] + a.ln_beta[k];
    out[(size_t)r * K + k] = v;
  }
}

constexpr int LNB_T = 24;        // most columns per lane: K <= 64 * 24 = 1536 (PatchMerging's 4 C of the third stage);
                                 // the kernel is built for 2, 3, 6, 12 and 24 (K <= 128, 192, 384, 768, 1536)
constexpr int LNB_PARTS = 4;     // partial dgamma / dbeta rows per chunk: one per wave

// LayerNorm backward over the loader's rows (ROWS, or MERGE: dx lands on the token rows, which is the adjoint of the
// 2 x 2 gather -- every token lies in exactly one merged row, and the gradient of corner padding is dropped).
//   xh = (x - mean) rstd,  g = dy_scale dy,  dxh = g gamma,  dx = rstd (dxh - mean_k(dxh) - xh mean_k(dxh xh)) + residual
// One wave per row: wave w of chunk c takes rows c rows_per_chunk + w, + 4, ...; its column sums of g xh and g go to
// part[4 c + w][0 | 1][K] (summed in that order by swin_ln_bwd_reduce_kernel).
template <int MODE, int NT>
__global__ __launch_bounds__(256) void swin_ln_bwd_kernel(isf_swin_a a, int M, int K, const float* __restrict__ dy,
                                                           int dy_hw, const float* __restrict__ dy_scale,
                                                           const float* __restrict__ res, float* __restrict__ dx,
                                                           int rows_per_chunk, float* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rbeg = blockIdx.x * rows_per_chunk;
  const int rend = rbeg + rows_per_chunk < M ? rbeg + rows_per_chunk : M;
  const float gs = dy_scale ? *dy_scale : 1.f;
  const float invk = 1.f / (float)K;
  float dg[NT], db[NT], gam[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    dg[t] = 0.f;
    db[t] = 0.f;
    const int k = lane + 64 * t;
    gam[t] = k < K ? a.ln_gamma[k] : 0.f;
  }
  for (int r = rbeg + wave; r < rend; r += 4) {
    const float mean = a.ln_stats[2 * r], rstd = a.ln_stats[2 * r + 1];
    const int b = dy_hw ? r / dy_hw : 0, pos = dy_hw ? r - b * dy_hw : 0;
    float xh[NT], dxh[NT];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int k = lane + 64 * t;
      xh[t] = 0.f;
      dxh[t] = 0.f;
      if (k < K) {
        const long long off = swin_src_offset<MODE>(a, r, k);
        const float xv = off >= 0 ? a.x[off] : 0.f;
        const float g = gs * (dy_hw ? dy[((size_t)b * K + k) * dy_hw + pos] : dy[(size_t)r * K + k]);
        xh[t] = (xv - mean) * rstd;
        dxh[t] = g * gam[t];
        s1 += dxh[t];
        s2 += dxh[t] * xh[t];
        dg[t] += g * xh[t];
        db[t] += g;
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      s1 += __shfl_xor(s1, d, 64);
      s2 += __shfl_xor(s2, d, 64);
    }
    const float m1 = s1 * invk, m2 = s2 * invk;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int k = lane + 64 * t;
      if (k < K) {
        float v = rstd * (dxh[t] - m1 - xh[t] * m2);
        if (MODE == ISF_SWIN_A_ROWS) {
          if (res) v += res[(size_t)r * K + k];
          dx[(size_t)r * K + k] = v;
        } else {
          const long long off = swin_src_offset<MODE>(a, r, k);
          if (off >= 0) dx[off] = v;
        }
      }
    }
  }
  float* p = part + (size_t)(blockIdx.x * LNB_PARTS + wave) * 2 * K;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int k = lane + 64 * t;
    if (k < K) {
      p[k] = dg[t];
      p[K + k] = db[t];
    }
  }
}

// out[i] = inv_scale * (sum of part[p][i] over p + extra[i]) for i < width: the fixed-order second pass of the LayerNorm
// backward (width 2 K: dgamma | dbeta) and of the column sums.  16 columns x 16 phases per workgroup: phase q adds the
// parts q, q + 16, ... in that order, then the 16 phase sums are added in phase order -- the same order every run.
__global__ __launch_bounds__(256) void swin_parts_reduce_kernel(const float* __restrict__ part, int nparts, int width,
                                                                 const float* __restrict__ extra,
                                                                 const float* __restrict__ inv_scale,
                                                                 float* __restrict__ out0, float* __restrict__ out1,
                                                                 int split) {
  __shared__ float red[16][16];
  const int col = threadIdx.x & 15, phase = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + col;
  float s = 0.f;
  if (i < width)
    for (int p = phase; p < nparts; p += 16) s += part[(size_t)p * width + i];
  red[phase][col] = s;
  __syncthreads();
  if (phase != 0 || i >= width) return;
  s = red[0][col];
#pragma unroll
  for (int q = 1; q < 16; ++q) s += red[q][col];
  if (extra) s += extra[i];
  if (inv_scale) s *= *inv_scale;
  if (i < split) out0[i] = s;
  else out1[i - split] = s;
}

// column sums of g [M, N]: 64 columns x 4 row phases per workgroup, chunk c of the rows -> part[c][N]
__global__ __launch_bounds__(256) void swin_colsum_kernel(const float* __restrict__ g, int M, int N, int rows_per_chunk,
                                                           float* __restrict__ part) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.y * 64 + lane;
  const int rbeg = blockIdx.x * rows_per_chunk;
  const int rend = rbeg + rows_per_chunk < M ? rbeg + rows_per_chunk : M;
  float s = 0.f;
  if (n < N)
    for (int r = rbeg + wave; r < rend; r += 4) s += g[(size_t)r * N + n];
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && n < N) part[(size_t)blockIdx.x * N + n] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// exact GELU backward in place: z = h[i] (pre-activation) -> h[i] = gelu(z), dh[i] *= gelu'(z)
__global__ __launch_bounds__(256) void swin_gelu_bwd_kernel(float* __restrict__ h, float* __restrict__ dh, size_t n4) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float4 z = reinterpret_cast<float4*>(h)[i], g = reinterpret_cast<float4*>(dh)[i];
  float* zp = reinterpret_cast<float*>(&z);
  float* gp = reinterpret_cast<float*>(&g);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float v = zp[j];
    const float cdf = 0.5f * (1.f + erff(v * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * __expf(-0.5f * v * v);
    zp[j] = v * cdf;
    gp[j] *= cdf + v * pdf;
  }
  reinterpret_cast<float4*>(h)[i] = z;
  reinterpret_cast<float4*>(dh)[i] = g;
}

// out[r, :] = g[r, :] * row_scale[r / rows_per_sample] (the DropPath factor on a branch's gradient)
__global__ __launch_bounds__(256) void swin_scale_rows_kernel(const float* __restrict__ g, size_t n4, int n4_per_sample,
                                                               const float* __restrict__ row_scale,
                                                               float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float s = row_scale[i / n4_per_sample];
  const float4 v = reinterpret_cast<const float4*>(g)[i];
  reinterpret_cast<float4*>(out)[i] = make_float4(v.x * s, v.y * s, v.z * s, v.w * s);
}

constexpr int AB_WS = 7, AB_T = 49, AB_HD = 32;
constexpr int AB_TARGET = 1024;   // workgroups (groups x heads) a launch aims at

int attn_bwd_items_per_group(int batch, int height, int width, int heads) {
  const int total = ceil_div(height, AB_WS) * ceil_div(width, AB_WS) * batch;
  int groups = AB_TARGET / heads;
  if (groups < 1) groups = 1;
  if (groups > total) groups = total;
  return ceil_div(total, groups);
}

// Backward of swin_window_attn_kernel (isf_swin.hip): one wave per (group of windows, head); lane i < 49 is query i in
// the first half of a window's work and key j in the second.  The probabilities are recomputed from qkv with the
// forward's arithmetic.  With dO the gradient of the attention output (0 for a padded query: it produced no output):
//   dP = dO V^T,  dS = P (dP - rowsum(P dP)),  dQ = scale dS K,  dK = dS^T (scale Q),  dV = P^T dO,  dB += dS
// P, dS and the workgroup's dB are 49 x 49 LDS matrices (row stride 49: lane-per-row writes and lane-per-column reads both hit
// 49 different banks).  Padded cells take part as keys and values: their dK / dV belong to the qkv bias and are summed,
// in key order, into the workgroup's 64 pad sums.  The workgroup walks a fixed range of (image, window) items and
// writes its dB [49, 49] and its pad sums once: the sum over groups is the second kernel's, in group order.
__global__ __launch_bounds__(64) void swin_window_attn_bwd_kernel(const float* __restrict__ qkv,
                                                                   const float* __restrict__ qkv_bias,
                                                                   const float* __restrict__ rel_bias,
                                                                   const float* __restrict__ dout, int B, int H, int W,
                                                                   int C, int heads, int shift, float scale,
                                                                   int items_per_group, float* __restrict__ dqkv,
                                                                   float* __restrict__ part_bias,
                                                                   float* __restrict__ part_pad) {
  constexpr int WS = AB_WS, T = AB_T, HD = AB_HD;
  __shared__ __attribute__((aligned(16))) float ks[T][HD];
  __shared__ __attribute__((aligned(16))) float vs[T][HD];
  __shared__ __attribute__((aligned(16))) float qs[T][HD];
  __shared__ __attribute__((aligned(16))) float dos[T][HD];
  __shared__ float pm[T][T], sm[T][T], dbm[T][T];
  __shared__ int lab[T], okc[T];
  const int Hp = (H + WS - 1) / WS * WS, Wp = (W + WS - 1) / WS * WS;
  const int nww = Wp / WS, nwin = (Hp / WS) * nww;
  const int total = nwin * B;
  const int grp = blockIdx.x, h = blockIdx.y;
  const int i = threadIdx.x;
  const int ld = 3 * C;
  const int beg = grp * items_per_group;
  const int end = beg + items_per_group < total ? beg + items_per_group : total;
  if (i < T)
    for (int j = 0; j < T; ++j) dbm[i][j] = 0.f;   // the workgroup's dB; row i is lane i's alone
  float padacc = 0.f;
  const float* rb = rel_bias + ((size_t)h * T + (i < T ? i : 0)) * T;
  for (int item = beg; item < end; ++item) {
    const int b = item / nwin, wi = item - b * nwin;
    const int wy = wi / nww, wx = wi - wy * nww;
    float q[HD], go[HD];
    bool valid = false;
    size_t row = 0;
    if (i < T) {
      const int sy = wy * WS + i / WS, sx = wx * WS + i % WS;
      int py = sy + shift, px = sx + shift;
      if (py >= Hp) py -= Hp;
      if (px >= Wp) px -= Wp;
      valid = py < H && px < W;
      row = ((size_t)b * H + py) * W + px;
      const float* src = valid ? qkv + row * ld : qkv_bias;
      const float* gsrc = dout + row * C + h * HD;
#pragma unroll
      for (int d = 0; d < HD; d += 4) {
        float4 kk = make_float4(0.f, 0.f, 0.f, 0.f), vv = kk, qq = kk, gg = kk;
        if (src) {
          qq = *reinterpret_cast<const float4*>(src + h * HD + d);
          kk = *reinterpret_cast<const float4*>(src + C + h * HD + d);
          vv = *reinterpret_cast<const float4*>(src + 2 * C + h * HD + d);
        }
        if (valid) gg = *reinterpret_cast<const float4*>(gsrc + d);
        q[d] = qq.x * scale; q[d + 1] = qq.y * scale; q[d + 2] = qq.z * scale; q[d + 3] = qq.w * scale;
        go[d] = gg.x; go[d + 1] = gg.y; go[d + 2] = gg.z; go[d + 3] = gg.w;
        *reinterpret_cast<float4*>(&ks[i][d]) = kk;
        *reinterpret_cast<float4*>(&vs[i][d]) = vv;
        *reinterpret_cast<float4*>(&qs[i][d]) = make_float4(q[d], q[d + 1], q[d + 2], q[d + 3]);
        *reinterpret_cast<float4*>(&dos[i][d]) = gg;
      }
      const int ry = sy < Hp - WS ? 0 : (sy < Hp - shift ? 1 : 2);
      const int rx = sx < Wp - WS ? 0 : (sx < Wp - shift ? 1 : 2);
      lab[i] = ry * 3 + rx;
      okc[i] = valid ? 1 : 0;
    }
    const bool any_pad = __ballot(i < T && !valid) != 0ull;
    __syncthreads();
    if (i < T) {
      // the forward's scores and softmax; the row lives in pm[i][.] (this lane's own LDS row)
      const int li = lab[i];
      float m = -INFINITY;
#pragma unroll 7
      for (int j = 0; j < T; ++j) {
        float z = 0.f;
#pragma unroll
        for (int d = 0; d < HD; ++d) z += q[d] * ks[j][d];
        z += rb[j];
        if (shift && lab[j] != li) z += -100.f;
        pm[i][j] = z;
        m = fmaxf(m, z);
      }
      float sum = 0.f;
#pragma unroll 7
      for (int j = 0; j < T; ++j) {
        const float e = __expf(pm[i][j] - m);
        pm[i][j] = e;
        sum += e;
      }
      const float inv = 1.f / sum;
      // rowsum(P dP) = dO . (P V) = dO . O: the forward's output row, recomputed
      float acc[HD];
#pragma unroll
      for (int d = 0; d < HD; ++d) acc[d] = 0.f;
#pragma unroll 7
      for (int j = 0; j < T; ++j) {
        const float pj = pm[i][j] * inv;
        pm[i][j] = pj;
#pragma unroll
        for (int d = 0; d < HD; ++d) acc[d] += pj * vs[j][d];
      }
      float delta = 0.f;
#pragma unroll
      for (int d = 0; d < HD; ++d) { delta += go[d] * acc[d]; acc[d] = 0.f; }
#pragma unroll 7
      for (int j = 0; j < T; ++j) {
        float dp = 0.f;
#pragma unroll
        for (int d = 0; d < HD; ++d) dp += go[d] * vs[j][d];
        const float dsj = pm[i][j] * (dp - delta);
        sm[i][j] = dsj;
        dbm[i][j] += dsj;
#pragma unroll
        for (int d = 0; d < HD; ++d) acc[d] += dsj * ks[j][d];
      }
      if (valid) {
        float* dst = dqkv + row * ld + h * HD;
#pragma unroll
        for (int d = 0; d < HD; d += 4)
          *reinterpret_cast<float4*>(dst + d) =
              make_float4(acc[d] * scale, acc[d + 1] * scale, acc[d + 2] * scale, acc[d + 3] * scale);
      }
    }
    __syncthreads();   // P and dS are in LDS; ks / vs are free from here on
    if (i < T) {
      float dv[HD], dk[HD];
#pragma unroll
      for (int d = 0; d < HD; ++d) { dv[d] = 0.f; dk[d] = 0.f; }
#pragma unroll 7
      for (int ii = 0; ii < T; ++ii) {
        const float pij = pm[ii][i], sij = sm[ii][i];
#pragma unroll
        for (int d = 0; d < HD; ++d) {
          dv[d] += pij * dos[ii][d];
          dk[d] += sij * qs[ii][d];
        }
      }
      float* dstv = valid ? dqkv + row * ld + 2 * C + h * HD : &vs[i][0];
      float* dstk = valid ? dqkv + row * ld + C + h * HD : &ks[i][0];
#pragma unroll
      for (int d = 0; d < HD; d += 4) {
        *reinterpret_cast<float4*>(dstv + d) = make_float4(dv[d], dv[d + 1], dv[d + 2], dv[d + 3]);
        *reinterpret_cast<float4*>(dstk + d) = make_float4(dk[d], dk[d + 1], dk[d + 2], dk[d + 3]);
      }
    }
    if (any_pad) {
      __syncthreads();
      const float* src = i < HD ? &ks[0][i] : &vs[0][i - HD];
      for (int j = 0; j < T; ++j)
        if (!okc[j]) padacc += src[j * HD];
    }
    __syncthreads();   // the next item overwrites every LDS array
  }
  if (i < T) {
    float* dst = part_bias + ((size_t)(grp * heads + h) * T + i) * T;
    for (int j = 0; j < T; ++j) dst[j] = dbm[i][j];
  }
  part_pad[(size_t)(grp * heads + h) * 64 + i] = padacc;
}

// second pass: drel[h, i, j] = sum over groups, in group order; pad[C + 32 h + d] / pad[2 C + 32 h + d] likewise
// (pad[0 .. C) = 0: a padded query has no gradient)
__global__ __launch_bounds__(256) void swin_attn_bwd_reduce_kernel(const float* __restrict__ part_bias,
                                                                    const float* __restrict__ part_pad, int groups,
                                                                    int heads, int C, float* __restrict__ drel,
                                                                    float* __restrict__ pad) {
  const int nb = heads * AB_T * AB_T;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < nb) {
    const int h = i / (AB_T * AB_T), e = i - h * AB_T * AB_T;
    float s = 0.f;
    for (int g = 0; g < groups; ++g) s += part_bias[((size_t)g * heads + h) * AB_T * AB_T + e];
    drel[i] = s;
  } else if (i < nb + 3 * C) {
    const int c = i - nb;
    float s = 0.f;
    if (c >= C) {
      const int part = (c - C) / C, hc = (c - C) - part * C, h = hc / AB_HD, d = hc - h * AB_HD;
      for (int g = 0; g < groups; ++g) s += part_pad[((size_t)g * heads + h) * 64 + part * AB_HD + d];
    }
    pad[c] = s;
  }
}

// dtable[t, h] = inv_scale * sum of drel[h, i, j] over the (i, j) with index[i, j] == t.  One workgroup per (t, h): thread
// u adds its matches among the entries u, u + 256, ... in that order, then the 256 sums go down a fixed tree.
__global__ __launch_bounds__(256) void swin_attn_table_grad_kernel(const float* __restrict__ drel,
                                                                    const long long* __restrict__ index, int heads,
                                                                    const float* __restrict__ inv_scale,
                                                                    float* __restrict__ dtable) {
  __shared__ float red[256];
  const int t = blockIdx.x, h = blockIdx.y, u = threadIdx.x;
  float s = 0.f;
  for (int e = u; e < AB_T * AB_T; e += 256)
    if (index[e] == t) s += drel[(size_t)h * AB_T * AB_T + e];
  red[u] = s;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if (u < d) red[u] += red[u + d];
    __syncthreads();
  }
  if (u == 0) dtable[(size_t)t * heads + h] = inv_scale ? red[0] * *inv_scale : red[0];
}

static int rows_chunk(int M, int min_rows, int max_chunks) {
  int chunks = ceil_div(M, min_rows);
  if (chunks > max_chunks) chunks = max_chunks;
  if (chunks < 1) chunks = 1;
  return ceil_div(M, chunks);
}

// the second passes, shared with the mixed-precision entries of isf_swin_train_f16.hip (same workspace layouts)
int rows_wgrad_reduce(const float* ws, int chunks, int N, int K, const float* inv_scale, float* dw, int ldw,
                      hipStream_t st) {
  hipLaunchKernelGGL(rows_wgrad_reduce_kernel, dim3(ceil_div((long long)N * K, 256)), dim3(256), 0, st, ws, chunks, N, K,
                     inv_scale, dw, ldw);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int swin_attn_bwd_finish(const float* part_bias, const float* part_pad, int groups, int heads, int C, float* drel,
                         float* pad, const int64_t* rel_index, const float* inv_scale, float* dtable, int table_rows,
                         hipStream_t st) {
  hipLaunchKernelGGL(swin_attn_bwd_reduce_kernel, dim3(ceil_div(heads * AB_T * AB_T + 3 * C, 256)), dim3(256), 0, st,
                     part_bias, part_pad, groups, heads, C, drel, pad);
  ISF_LAUNCH_CHECK();
  if (dtable) {
    hipLaunchKernelGGL(swin_attn_table_grad_kernel, dim3(table_rows, heads), dim3(256), 0, st, drel,
                       reinterpret_cast<const long long*>(rel_index), heads, inv_scale, dtable);
    ISF_LAUNCH_CHECK();
  }
  return ISF_OK;
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
  return rows_wgrad_reduce(workspace, num_chunks, out_features, k, inv_scale, dw, ldw, st);
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

static int swin_train_check_a(const isf_swin_a* a, int num_rows, int k, const char* what) {
  using namespace isf;
  ISF_REQUIRE(a && a->x && num_rows > 0 && k > 0, ISF_ERR_ARG, "%s: null operand or bad sizes", what);
  switch (a->mode) {
    case ISF_SWIN_A_ROWS:
      ISF_REQUIRE(a->ldx >= k, ISF_ERR_ARG, "%s: rows need ldx >= K", what);
      break;
    case ISF_SWIN_A_MERGE:
      ISF_REQUIRE(a->n > 0 && a->c > 0 && a->h > 0 && a->w > 0 && k == 4 * a->c &&
                      num_rows == a->n * ((a->h + 1) >> 1) * ((a->w + 1) >> 1),
                  ISF_ERR_ARG, "%s: merge needs K == 4 C and rows == n ceil(h/2) ceil(w/2)", what);
      break;
    case ISF_SWIN_A_PATCH:
      ISF_REQUIRE(a->n > 0 && a->c > 0 && a->h > 0 && a->w > 0 && k == 16 * a->c &&
                      num_rows == a->n * ((a->h + 3) >> 2) * ((a->w + 3) >> 2),
                  ISF_ERR_ARG, "%s: patch needs K == 16 C and rows == n ceil(h/4) ceil(w/4)", what);
      break;
    default:
      ISF_REQUIRE(false, ISF_ERR_UNSUPPORTED, "%s: loader mode %d", what, a->mode);
  }
  ISF_REQUIRE(!a->ln_stats || (a->ln_gamma && a->ln_beta), ISF_ERR_ARG, "%s: LayerNorm prologue needs gamma, beta", what);
  return ISF_OK;
}

int isf_swin_operand_rows(const isf_swin_a* a, int num_rows, int k, float* out, isf_stream_t stream) {
  using namespace isf;
  if (num_rows == 0) return ISF_OK;
  ISF_TRY(swin_train_check_a(a, num_rows, k, "swin_operand_rows"));
  ISF_REQUIRE(out && out != a->x, ISF_ERR_ARG, "swin_operand_rows: null or aliased output");
  ISF_REQUIRE(a->mode != ISF_SWIN_A_PATCH || !a->ln_stats, ISF_ERR_UNSUPPORTED, "swin_operand_rows: patch rows have no prologue");
  const dim3 grid(ceil_div(num_rows, 4)), block(256);
  hipStream_t st = as_stream(stream);
  if (a->mode == ISF_SWIN_A_ROWS)
    hipLaunchKernelGGL(swin_operand_rows_kernel<ISF_SWIN_A_ROWS>, grid, block, 0, st, *a, num_rows, k, out);
  else if (a->mode == ISF_SWIN_A_MERGE)
    hipLaunchKernelGGL(swin_operand_rows_kernel<ISF_SWIN_A_MERGE>, grid, block, 0, st, *a, num_rows, k, out);
  else
    hipLaunchKernelGGL(swin_operand_rows_kernel<ISF_SWIN_A_PATCH>, grid, block, 0, st, *a, num_rows, k, out);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_swin_layernorm_backward_parts(int num_rows) {
  using namespace isf;
  if (num_rows <= 0) return 0;
  return ceil_div(num_rows, rows_chunk(num_rows, 32, 512)) * LNB_PARTS;
}

int isf_swin_layernorm_backward(const isf_swin_a* a, int num_rows, int k, const float* dy, int dy_hw,
                                const float* dy_scale, const float* residual_grad, float* dx, const float* inv_scale,
                                float* workspace, int num_parts, float* dgamma, float* dbeta, isf_stream_t stream) {
  using namespace isf;
  ISF_TRY(swin_train_check_a(a, num_rows, k, "swin_layernorm_backward"));
  ISF_REQUIRE(a->mode != ISF_SWIN_A_PATCH && a->ln_stats, ISF_ERR_ARG,
              "swin_layernorm_backward: rows / merge loader with ln_stats and ln_gamma");
  ISF_REQUIRE(k <= 64 * LNB_T, ISF_ERR_UNSUPPORTED, "swin_layernorm_backward: K %d (at most %d)", k, 64 * LNB_T);
  ISF_REQUIRE(dy && dx && workspace && dgamma && dbeta && dx != dy, ISF_ERR_ARG, "swin_layernorm_backward: null or aliased pointer");
  ISF_REQUIRE(dy_hw >= 0 && (dy_hw == 0 || num_rows % dy_hw == 0), ISF_ERR_ARG,
              "swin_layernorm_backward: rows not a multiple of dy_hw");
  ISF_REQUIRE(!residual_grad || a->mode == ISF_SWIN_A_ROWS, ISF_ERR_UNSUPPORTED,
              "swin_layernorm_backward: a residual gradient needs the rows loader");
  ISF_REQUIRE(num_parts == isf_swin_layernorm_backward_parts(num_rows), ISF_ERR_ARG,
              "swin_layernorm_backward: workspace of %d parts, isf_swin_layernorm_backward_parts says %d", num_parts,
              isf_swin_layernorm_backward_parts(num_rows));
  const int rpc = rows_chunk(num_rows, 32, 512);
  const dim3 grid(num_parts / LNB_PARTS), block(256);
  hipStream_t st = as_stream(stream);
  const int nt = ceil_div(k, 64);
#define ISF_LN_BWD(MODE, NT)                                                                                         \
  hipLaunchKernelGGL((swin_ln_bwd_kernel<MODE, NT>), grid, block, 0, st, *a, num_rows, k, dy, dy_hw, dy_scale,        \
                     residual_grad, dx, rpc, workspace)
#define ISF_LN_BWD_NT(MODE)                   \
  do {                                        \
    if (nt <= 2) ISF_LN_BWD(MODE, 2);         \
    else if (nt <= 3) ISF_LN_BWD(MODE, 3);    \
    else if (nt <= 6) ISF_LN_BWD(MODE, 6);    \
    else if (nt <= 12) ISF_LN_BWD(MODE, 12);  \
    else ISF_LN_BWD(MODE, 24);                \
  } while (0)
  if (a->mode == ISF_SWIN_A_ROWS) ISF_LN_BWD_NT(ISF_SWIN_A_ROWS);
  else ISF_LN_BWD_NT(ISF_SWIN_A_MERGE);
#undef ISF_LN_BWD_NT
#undef ISF_LN_BWD
  ISF_LAUNCH_CHECK();
  hipLaunchKernelGGL(swin_parts_reduce_kernel, dim3(ceil_div(2 * k, 16)), block, 0, st, workspace, num_parts, 2 * k,
                     (const float*)nullptr, inv_scale, dgamma, dbeta, k);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_swin_column_sums_parts(int num_rows) {
  using namespace isf;
  if (num_rows <= 0) return 0;
  return ceil_div(num_rows, rows_chunk(num_rows, 64, 256));
}

int isf_swin_column_sums(const float* g, int num_rows, int channels, const float* extra, const float* inv_scale,
                         float* workspace, int num_parts, float* out, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num_rows > 0 && channels > 0 && g && workspace && out, ISF_ERR_ARG, "swin_column_sums: null pointer or bad sizes");
  ISF_REQUIRE(num_parts == isf_swin_column_sums_parts(num_rows), ISF_ERR_ARG,
              "swin_column_sums: workspace of %d parts, isf_swin_column_sums_parts says %d", num_parts,
              isf_swin_column_sums_parts(num_rows));
  const int rpc = rows_chunk(num_rows, 64, 256);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(swin_colsum_kernel, dim3(num_parts, ceil_div(channels, 64)), dim3(256), 0, st, g, num_rows, channels,
                     rpc, workspace);
  ISF_LAUNCH_CHECK();
  hipLaunchKernelGGL(swin_parts_reduce_kernel, dim3(ceil_div(channels, 16)), dim3(256), 0, st, workspace, num_parts,
                     channels, extra, inv_scale, out, out, channels);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_swin_gelu_backward(float* hidden, float* grad, size_t num_elems, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num_elems % 4 == 0, ISF_ERR_ARG, "swin_gelu_backward: element count must be a multiple of 4");
  if (num_elems == 0) return ISF_OK;
  ISF_REQUIRE(hidden && grad && hidden != grad && ((uintptr_t)hidden & 15) == 0 && ((uintptr_t)grad & 15) == 0, ISF_ERR_ARG,
              "swin_gelu_backward: null, aliased or unaligned pointer");
  const size_t n4 = num_elems / 4;
  hipLaunchKernelGGL(swin_gelu_bwd_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, as_stream(stream), hidden, grad, n4);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_swin_scale_rows(const float* g, int num_rows, int channels, const float* row_scale, int rows_per_sample, float* out,
                        isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num_rows >= 0 && channels > 0 && channels % 4 == 0 && rows_per_sample > 0 && num_rows % rows_per_sample == 0,
              ISF_ERR_ARG, "swin_scale_rows: bad sizes (channels %% 4, rows a multiple of rows_per_sample)");
  if (num_rows == 0) return ISF_OK;
  ISF_REQUIRE(g && row_scale && out && ((uintptr_t)g & 15) == 0 && ((uintptr_t)out & 15) == 0, ISF_ERR_ARG,
              "swin_scale_rows: null or unaligned pointer");
  const size_t n4 = (size_t)num_rows * channels / 4;
  const size_t per = (size_t)rows_per_sample * channels / 4;
  ISF_REQUIRE(per <= 0x7fffffff, ISF_ERR_UNSUPPORTED, "swin_scale_rows: sample too large");
  hipLaunchKernelGGL(swin_scale_rows_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, as_stream(stream), g, n4,
                     (int)per, row_scale, out);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_swin_window_attention_backward_groups(int batch, int height, int width, int heads) {
  using namespace isf;
  if (batch <= 0 || height <= 0 || width <= 0 || heads <= 0) return 0;
  const int total = ceil_div(height, AB_WS) * ceil_div(width, AB_WS) * batch;
  return ceil_div(total, attn_bwd_items_per_group(batch, height, width, heads));
}

int isf_swin_window_attention_backward(const float* qkv, const float* qkv_bias, const float* rel_bias,
                                       const int64_t* rel_index, const float* dout, int batch, int height, int width,
                                       int channels, int heads, int window, int shift, float scale,
                                       const float* inv_scale, float* workspace, int num_groups, float* dqkv,
                                       float* drel_bias, float* dtable, int table_rows, float* dqkv_bias_pad,
                                       isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(batch > 0 && height > 0 && width > 0 && heads > 0, ISF_ERR_ARG, "swin_window_attention_backward: bad sizes");
  ISF_REQUIRE(qkv && rel_bias && dout && workspace && dqkv && drel_bias && dqkv_bias_pad, ISF_ERR_ARG,
              "swin_window_attention_backward: null pointer");
  ISF_REQUIRE(window == 7 && channels == 32 * heads && shift >= 0 && shift < window, ISF_ERR_UNSUPPORTED,
              "swin_window_attention_backward: window 7, head dim 32 only (window %d, C %d, heads %d, shift %d)", window,
              channels, heads, shift);
  ISF_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)qkv_bias & 15) == 0 && ((uintptr_t)dout & 15) == 0 &&
                  ((uintptr_t)dqkv & 15) == 0, ISF_ERR_ARG, "swin_window_attention_backward: unaligned pointer");
  ISF_REQUIRE(!dtable || (rel_index && table_rows > 0), ISF_ERR_ARG,
              "swin_window_attention_backward: the table gradient needs relative_position_index and its row count");
  ISF_REQUIRE(num_groups == isf_swin_window_attention_backward_groups(batch, height, width, heads) && num_groups <= 65535 * 32,
              ISF_ERR_ARG, "swin_window_attention_backward: workspace of %d groups, ..._groups says %d", num_groups,
              isf_swin_window_attention_backward_groups(batch, height, width, heads));
  ISF_REQUIRE(heads <= 65535, ISF_ERR_UNSUPPORTED, "swin_window_attention_backward: heads %d", heads);
  const int ipg = attn_bwd_items_per_group(batch, height, width, heads);
  float* part_bias = workspace;
  float* part_pad = workspace + (size_t)num_groups * heads * AB_T * AB_T;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(swin_window_attn_bwd_kernel, dim3(num_groups, heads), dim3(64), 0, st, qkv, qkv_bias, rel_bias, dout,
                     batch, height, width, channels, heads, shift, scale, ipg, dqkv, part_bias, part_pad);
  ISF_LAUNCH_CHECK();
  return swin_attn_bwd_finish(part_bias, part_pad, num_groups, heads, channels, drel_bias, dqkv_bias_pad, rel_index,
                              inv_scale, dtable, table_rows, st);
}

}  // extern "C"
