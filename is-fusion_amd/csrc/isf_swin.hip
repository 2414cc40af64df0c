// isf_swin.hip -- the camera branch: Swin-T backbone (SwinTransformer) and the GeneralizedLSSFPN top-down step.
//
// Reference: mmdet3d/models/backbones/swin.py (WindowMSA / ShiftWindowMSA / SwinBlock / SwinTransformer),
// models/utils/transformer.py (PatchEmbed, PatchMerging), models/necks/generalized_lss.py -- cuBLAS GEMMs, LayerNorm,
// GELU, F.pad / torch.roll / window partition copies, softmax and F.interpolate + torch.cat.  Here:
//   isf_swin_gemm        K-looped GEMM Y = epi(A . W^T) for every Linear / 4x4 patch conv / 1x1 lateral conv.  The A
//                        loader produces the operand rows on the fly (isf_swin_a.mode):
//                          ROWS   token rows [M, ldx], optional LayerNorm prologue (row stats from isf_swin_row_stats)
//                          PATCH  4 x 4 x Cin patches gathered from the NCHW image (corner zero padding), K padded to 64
//                          MERGE  2 x 2 neighbourhood of the token grid (corner zero padding) + LayerNorm prologue; the
//                                 loader's k order is (kh*2 + kw)*C + c -- contiguous channels -- and the packed weight
//                                 and gamma / beta are permuted to it, so the product equals nn.Unfold's c*4 + kh*2 + kw
//                          UPCAT  [fine NCHW | bilinear(align_corners) upsample of the coarse NCHW] channel concat
//                        epilogue: * scale + shift (bias / folded BN), ReLU or exact GELU, + residual rows, stored as rows
//                        or NCHW.  isf_swin_gemm_rowscale (training, DropPath): the branch output of sample r / rows_per_sample
//                        is multiplied by row_scale[sample] before the residual is added.  arithmetic: f16 hi/lo split of both operands, 3 x v_mfma_f32_16x16x32_f16 per
//                        product, fp32 accumulate (as isf_linear.hip); weights packed by isf_pack_linear.
//                        tiling: workgroup 128 rows x 64 columns, 4 waves of 32 x 64; A (split into hi / lo halves by
//                        the loader) and B staged through a double-buffered LDS ring, one 32-deep K step per stage.
//   isf_swin_gemm_f16    the same kernel template in the f16 inference mode (SwinTransformer.set_precision("f16")): ONE
//                        v_mfma_f32_16x16x32_f16 per product.  The loader converts its fp32 rows (after the LayerNorm
//                        prologue) to f16, or reads f16 rows as they are; the weight is one f16 plane
//                        (isf_pack_linear_f16); accumulation and the epilogue stay fp32; the output rows are fp32 (into
//                        the residual stream) or f16 (qkv, the FFN hidden).  Every store to an f16 tensor saturates at
//                        +-65504 instead of producing inf.  Window attention of this mode: isf_swin_f16.hip.
//                        All four GEMM entries (swin.gemm, swin.gemm_f16_rowscale) end in swin_gemm_launch; swin_gemm_forms is the one
//                        statement of which (loader, LayerNorm, row scale, precision, f16 output) forms are built.
//   isf_swin_row_stats   mean / rstd of the loader's rows (one wave per row, two passes in fp32)
//   isf_swin_layernorm   LayerNorm of token rows, stored as rows or NCHW (patch_norm, the out_indices norms)
//   isf_swin_window_attention  (shifted) window attention on the token-major qkv: padding, cyclic shift, window
//                        partition / reverse are index arithmetic; padded cells' k / v are the qkv bias; relative
//                        position bias table [heads, 49, 49]; -100 between shift regions.  VALU, one wave per
//                        (window, image, head), one query per lane.
#include <stdlib.h>

#include "isf_common.h"
#include "isf_f16.h"

namespace isf {

typedef float sf4 __attribute__((ext_vector_type(4)));
typedef float sf8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void swin_split8(const sf8 v, fh8& hi, fh8& lo) {
  hi = __builtin_convertvector(v, fh8);
  const sf8 r = v - __builtin_convertvector(hi, sf8);
  lo = __builtin_convertvector(r, fh8);
}

__device__ __forceinline__ sf8 ld8(const float* p) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  return sf8{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
}

// 8 consecutive k of operand row r (raw, before the LayerNorm prologue)
template <int MODE>
__device__ __forceinline__ sf8 swin_load_a(const isf_swin_a& a, int r, int k0) {
  sf8 v = sf8{0, 0, 0, 0, 0, 0, 0, 0};
  if (MODE == ISF_SWIN_A_ROWS) {
    v = ld8(a.x + (size_t)r * a.ldx + k0);
  } else if (MODE == ISF_SWIN_A_MERGE) {
    const int Ho = (a.h + 1) >> 1, Wo = (a.w + 1) >> 1;
    const int b = r / (Ho * Wo), rem = r - b * Ho * Wo, oy = rem / Wo, ox = rem - oy * Wo;
    const int q = k0 / a.c, ci = k0 - q * a.c;
    const int y = 2 * oy + (q >> 1), x = 2 * ox + (q & 1);
    if (y < a.h && x < a.w) v = ld8(a.x + ((size_t)(b * a.h + y) * a.w + x) * a.c + ci);
  } else if (MODE == ISF_SWIN_A_PATCH) {
    const int Ho = (a.h + 3) >> 2, Wo = (a.w + 3) >> 2;
    const int b = r / (Ho * Wo), rem = r - b * Ho * Wo, oy = rem / Wo, ox = rem - oy * Wo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + j;
      const int ci = k >> 4, ky = (k >> 2) & 3, kx = k & 3;
      const int y = 4 * oy + ky, x = 4 * ox + kx;
      if (ci < a.c && y < a.h && x < a.w) v[j] = a.x[((size_t)(b * a.c + ci) * a.h + y) * a.w + x];
    }
  } else {   // UPCAT
    const int hw = a.h * a.w;
    const int b = r / hw, pos = r - b * hw, y = pos / a.w, x = pos - y * a.w;
    if (k0 < a.c) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = a.x[((size_t)b * a.c + k0 + j) * hw + pos];
    } else {
      // F.interpolate(bilinear, align_corners=True): src = (in - 1) / (out - 1) * dst, as upsample_bilinear2d computes it
      const float sy = a.h > 1 ? (float)(a.h2 - 1) / (float)(a.h - 1) : 0.f;
      const float sx = a.w > 1 ? (float)(a.w2 - 1) / (float)(a.w - 1) : 0.f;
      const float fy = sy * y, fx = sx * x;
      const int y0 = (int)fy, x0 = (int)fx;
      const int dy = y0 < a.h2 - 1 ? 1 : 0, dx = x0 < a.w2 - 1 ? 1 : 0;
      const float ly1 = fy - y0, ly0 = 1.f - ly1, lx1 = fx - x0, lx0 = 1.f - lx1;
      const int hw2 = a.h2 * a.w2;
      const int p00 = y0 * a.w2 + x0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float* s = a.x2 + ((size_t)b * a.c2 + (k0 - a.c + j)) * hw2 + p00;
        v[j] = ly0 * (lx0 * s[0] + lx1 * s[dx]) + ly1 * (lx0 * s[dy * a.w2] + lx1 * s[dy * a.w2 + dx]);
      }
    }
  }
  return v;
}

struct SwinEpi {
  const float* scale;     // [N] or null (1)
  const float* shift;     // [N] or null (0): bias / folded BN shift
  const float* residual;  // [M, N] rows or null
  int act;                // 0 none, 1 relu, 2 gelu (erf)
  int ldy, y_hw;          // y_hw > 0: y is [B, N, y_hw]
  const float* row_scale; // RS kernels: [num_rows / rows_per_sample] factor on the branch output (DropPath keep / keep_prob)
  int rows_per_sample;
};

constexpr int SW_BM = 128;   // rows per workgroup (columns: 4 tiles of 16)

// thread -> (row, k group) of its two A loads per K step.  Token-row sources: 4 threads per row (one 32-float row
// segment per 4 lanes); NCHW sources: 128 consecutive rows per k group (consecutive lanes read consecutive pixels).
template <int MODE>
__device__ __forceinline__ void swin_a_slot(int t, int i, int& rl, int& kg) {
  if (MODE == ISF_SWIN_A_ROWS || MODE == ISF_SWIN_A_MERGE) { rl = (t >> 2) + 64 * i; kg = t & 3; }
  else { rl = t & 127; kg = ((t >> 7) << 1) + i; }
}

// Operand precision of swin_gemm_kernel.  X3: f16 hi / lo split of both operands, three products (the default mode).
// F16 / F16_ROWS (isf_swin_gemm_f16, the f16 inference mode): one product -- the loader delivers only the hi half of the
// fp32 source (F16), or a.x points to f16 rows [M, ldx] that are staged as they are, 8 elements per 16-byte load
// (F16_ROWS); the weight is one f16 plane (isf_pack_linear_f16, no scale), the LDS ring holds half the bytes per K step.
// Y16: the output rows are f16, stored saturating (sat_f16).  Accumulation and the epilogue arithmetic stay fp32.
enum { SWIN_PREC_X3 = 0, SWIN_PREC_F16 = 1, SWIN_PREC_F16_ROWS = 2 };

template <int MODE, bool LN, bool RS = false, int PREC = SWIN_PREC_X3, bool Y16 = false>
__global__ __launch_bounds__(256) void swin_gemm_kernel(isf_swin_a a, int M, int K, const uint4* __restrict__ wp,
                                                         const float* __restrict__ w_inv_scale, int N, SwinEpi ep,
                                                         float* __restrict__ y) {
  constexpr int NP = PREC == SWIN_PREC_X3 ? 2 : 1;   // operand planes (hi | lo, or hi alone)
  constexpr int TS = 64 * NP;                        // uint4 per packed column tile and K step
  __shared__ uint4 as_[2][NP][4][SW_BM];  // [buf][hi|lo][k group][row]
  __shared__ uint4 bs_[2][4][TS];         // [buf][column tile][hi 0..63 | lo 64..127]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ntiles = N >> 4;
  const int nt0 = blockIdx.x * 4;
  const int R0 = blockIdx.y * SW_BM;
  const int ksteps = K >> 5;
  int rl[2], kg[2], rr[2];
  float mean[2] = {0.f, 0.f}, rstd[2] = {1.f, 1.f};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    swin_a_slot<MODE>(t, i, rl[i], kg[i]);
    rr[i] = R0 + rl[i];
    if (LN && rr[i] < M) { mean[i] = a.ln_stats[2 * rr[i]]; rstd[i] = a.ln_stats[2 * rr[i] + 1]; }
  }
  sf8 av[2];
  uint4 a16[2];   // F16_ROWS: the staged f16 row pieces
  uint4 bv[NP];
  auto fetch = [&](int ks) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int k0 = ks * 32 + kg[i] * 8;
      if constexpr (PREC == SWIN_PREC_F16_ROWS) {
        a16[i] = rr[i] < M ? *reinterpret_cast<const uint4*>(reinterpret_cast<const _Float16*>(a.x) +
                                                             (size_t)rr[i] * a.ldx + k0)
                           : make_uint4(0, 0, 0, 0);
      } else {
        av[i] = rr[i] < M ? swin_load_a<MODE>(a, rr[i], k0) : sf8{0, 0, 0, 0, 0, 0, 0, 0};
        if constexpr (LN && PREC != SWIN_PREC_X3) {
          // The same LayerNorm arithmetic, element by element.  Written as the vector expression below, the compiler
          // emits v_pk_mul_f32 (op_sel:[0,1]) feeding v_pk_fma_f32, and in these instantiations that pair returned
          // gamma * 0 + beta in the low half for lanes 48..63 of about 1 % of the rows once a compute unit ran its
          // second round of workgroups (x, mean, rstd, gamma, beta were read back correct from the same registers;
          // DESIGN 4.0c has the ISA).  The empty asm statements keep the elements out of packed instructions.
          // Seen with hipcc of ROCm 7.2 (AMD clang 22.0.0git) on gfx950; guarded by tests/test_gpu_camera_f16.py::
          // test_layernorm_prologue_f16_is_exact_in_every_round_of_workgroups -- run it after a compiler change.
          if (rr[i] < M) {
            const sf8 g = ld8(a.ln_gamma + k0), be = ld8(a.ln_beta + k0);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              float tn = (av[i][j] - mean[i]) * rstd[i];
              asm volatile("" : "+v"(tn));
              float r = tn * g[j] + be[j];
              asm volatile("" : "+v"(r));
              av[i][j] = r;
            }
          }
        } else if (LN && rr[i] < M) {
          const sf8 g = ld8(a.ln_gamma + k0), be = ld8(a.ln_beta + k0);
          av[i] = (av[i] - mean[i]) * rstd[i] * g + be;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int idx = t + 256 * i;
      const int tile = idx / TS;
      bv[i] = nt0 + tile < ntiles ? wp[((size_t)ks * ntiles + nt0) * TS + idx] : make_uint4(0, 0, 0, 0);
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if constexpr (PREC == SWIN_PREC_X3) {
        fh8 hi, lo;
        swin_split8(av[i], hi, lo);
        as_[buf][0][kg[i]][rl[i]] = *reinterpret_cast<const uint4*>(&hi);
        as_[buf][1][kg[i]][rl[i]] = *reinterpret_cast<const uint4*>(&lo);
      } else if constexpr (PREC == SWIN_PREC_F16) {
        const fh8 hi = __builtin_convertvector(av[i], fh8);
        as_[buf][0][kg[i]][rl[i]] = *reinterpret_cast<const uint4*>(&hi);
      } else {
        as_[buf][0][kg[i]][rl[i]] = a16[i];
      }
      if (i < NP) {
        const int idx = t + 256 * i;
        bs_[buf][idx / TS][idx % TS] = bv[i];
      }
    }
  };
  sf4 acc[2][4];
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[g][nt] = sf4{0.f, 0.f, 0.f, 0.f};
  const int ntv = ntiles - nt0 < 4 ? ntiles - nt0 : 4;   // valid column tiles of this workgroup (uniform)
  fetch(0);
  commit(0);
  __syncthreads();
  for (int ks = 0; ks < ksteps; ++ks) {
    const int buf = ks & 1;
    const bool more = ks + 1 < ksteps;
    if (more) fetch(ks + 1);
    fh8 ah[2], al[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int row = wave * 32 + g * 16 + (lane & 15);
      const uint4 h = as_[buf][0][lane >> 4][row], l = as_[buf][NP - 1][lane >> 4][row];
      ah[g] = *reinterpret_cast<const fh8*>(&h);
      al[g] = *reinterpret_cast<const fh8*>(&l);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      // single-pass modes multiply every column tile: the tiles past N are zeros in LDS, and straight-line MFMAs keep
      // the accumulators where they are
      if (PREC != SWIN_PREC_X3 || nt < ntv) {
        const uint4 bhu = bs_[buf][nt][lane], blu = bs_[buf][nt][TS - 64 + lane];
        const fh8 bh = *reinterpret_cast<const fh8*>(&bhu);
        const fh8 bl = *reinterpret_cast<const fh8*>(&blu);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          if constexpr (PREC == SWIN_PREC_X3) {
            acc[g][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[g], bh, acc[g][nt], 0, 0, 0);
            acc[g][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[g], bl, acc[g][nt], 0, 0, 0);
          }
          acc[g][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[g], bh, acc[g][nt], 0, 0, 0);
        }
      }
    }
    if (more) commit(buf ^ 1);   // the other buffer was last read before the previous barrier
    __syncthreads();
  }
  // C/D layout: lane holds rows 16 g + 4 (lane >> 4) + j of the wave's 32, column 16 nt + (lane & 15)
  const float winv = PREC == SWIN_PREC_X3 ? *w_inv_scale : 1.f;   // the single f16 plane carries no scale
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    if (nt >= ntv) continue;
    const int n = (nt0 + nt) * 16 + (lane & 15);
    const float sc = ep.scale ? ep.scale[n] : 1.f;
    const float sh = ep.shift ? ep.shift[n] : 0.f;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = R0 + wave * 32 + g * 16 + 4 * (lane >> 4) + j;
        if (r >= M) continue;
        float z = (PREC == SWIN_PREC_X3 ? acc[g][nt][j] * winv : acc[g][nt][j]) * sc + sh;
        if (ep.act == 1) z = fmaxf(z, 0.f);
        else if (ep.act == 2) z = 0.5f * z * (1.f + erff(z * 0.70710678118654752440f));
        if (RS) z *= ep.row_scale[r / ep.rows_per_sample];
        if (ep.residual) z += ep.residual[(size_t)r * N + n];
        if constexpr (Y16) {
          reinterpret_cast<_Float16*>(y)[(size_t)r * ep.ldy + n] = sat_f16(z);
        } else if (ep.y_hw) {
          const int b = r / ep.y_hw, pos = r - b * ep.y_hw;
          y[((size_t)b * N + n) * ep.y_hw + pos] = z;
        } else {
          y[(size_t)r * ep.ldy + n] = z;
        }
      }
    }
  }
}

// mean, rstd (biased variance, + eps) of the loader's K-wide rows; one wave per row
template <int MODE>
__global__ __launch_bounds__(256) void swin_row_stats_kernel(isf_swin_a a, int M, int K, float eps,
                                                              float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= M) return;
  float s = 0.f;
  for (int k0 = lane * 8; k0 < K; k0 += 512) {
    const sf8 v = swin_load_a<MODE>(a, r, k0);
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[j];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  const float mean = s / (float)K;
  float q = 0.f;
  for (int k0 = lane * 8; k0 < K; k0 += 512) {
    const sf8 v = swin_load_a<MODE>(a, r, k0);
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float d = v[j] - mean; q += d * d; }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) q += __shfl_xor(q, d, 64);
  if (lane == 0) {
    stats[2 * r] = mean;
    stats[2 * r + 1] = rsqrtf(q / (float)K + eps);
  }
}

// LayerNorm of 64 token rows per workgroup; y_hw > 0 stores [B, C, y_hw] (row r = b * y_hw + pos)
__global__ __launch_bounds__(256) void swin_layernorm_kernel(const float* __restrict__ x, int M, int C,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps,
                                                              float* __restrict__ y, int y_hw) {
  __shared__ float st[64][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int R0 = blockIdx.x * 64;
  for (int rl = wave; rl < 64; rl += 4) {
    const int r = R0 + rl;
    if (r >= M) break;
    const float* xr = x + (size_t)r * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += xr[c];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    const float mean = s / (float)C;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) { const float d = xr[c] - mean; q += d * d; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) q += __shfl_xor(q, d, 64);
    const float rstd = rsqrtf(q / (float)C + eps);
    if (y_hw == 0) {
      for (int c = lane; c < C; c += 64) y[(size_t)r * C + c] = (xr[c] - mean) * rstd * gamma[c] + beta[c];
    } else if (lane == 0) {
      st[rl][0] = mean;
      st[rl][1] = rstd;
    }
  }
  if (y_hw == 0) return;
  __syncthreads();
  const int rows = M - R0 < 64 ? M - R0 : 64;
  for (int idx = threadIdx.x; idx < 64 * C; idx += 256) {
    const int c = idx >> 6, rl = idx & 63;
    if (rl >= rows) continue;
    const int r = R0 + rl, b = r / y_hw, pos = r - b * y_hw;
    y[((size_t)b * C + c) * y_hw + pos] = (x[(size_t)r * C + c] - st[rl][0]) * st[rl][1] * gamma[c] + beta[c];
  }
}

// One wave per (window, image, head); lane i < 49 = query i of the window.  Token i of window (wy, wx) sits at
// (wy*7 + i/7, wx*7 + i%7) of the rolled, padded grid, i.e. at padded cell ((. + shift) mod Hp, (. + shift) mod Wp).
__global__ __launch_bounds__(64) void swin_window_attn_kernel(const float* __restrict__ qkv,
                                                               const float* __restrict__ qkv_bias,
                                                               const float* __restrict__ rel_bias, int H, int W, int C,
                                                               int heads, int shift, float scale,
                                                               float* __restrict__ out) {
  constexpr int WS = 7, T = 49, HD = 32;
  __shared__ float ks[T][HD], vs[T][HD];
  __shared__ int lab[T];
  const int Hp = (H + WS - 1) / WS * WS, Wp = (W + WS - 1) / WS * WS;
  const int nww = Wp / WS;
  const int wy = blockIdx.x / nww, wx = blockIdx.x - wy * nww;
  const int b = blockIdx.y, h = blockIdx.z;
  const int i = threadIdx.x;
  const int ld = 3 * C;
  float q[HD];
  bool valid = false;
  size_t row = 0;
  if (i < T) {
    const int sy = wy * WS + i / WS, sx = wx * WS + i % WS;
    int py = sy + shift, px = sx + shift;
    if (py >= Hp) py -= Hp;
    if (px >= Wp) px -= Wp;
    valid = py < H && px < W;
    row = ((size_t)b * H + py) * W + px;
    // zero padding comes after norm1: a padded cell's q / k / v are the qkv bias
    const float* src = valid ? qkv + row * ld : qkv_bias;
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
      float4 kk = make_float4(0.f, 0.f, 0.f, 0.f), vv = kk, qq = kk;
      if (src) {
        qq = *reinterpret_cast<const float4*>(src + h * HD + d);
        kk = *reinterpret_cast<const float4*>(src + C + h * HD + d);
        vv = *reinterpret_cast<const float4*>(src + 2 * C + h * HD + d);
      }
      q[d] = qq.x * scale; q[d + 1] = qq.y * scale; q[d + 2] = qq.z * scale; q[d + 3] = qq.w * scale;
      *reinterpret_cast<float4*>(&ks[i][d]) = kk;
      *reinterpret_cast<float4*>(&vs[i][d]) = vv;
    }
    // shift regions: slices (0, -ws), (-ws, -shift), (-shift, end) of the rolled padded grid
    const int ry = sy < Hp - WS ? 0 : (sy < Hp - shift ? 1 : 2);
    const int rx = sx < Wp - WS ? 0 : (sx < Wp - shift ? 1 : 2);
    lab[i] = ry * 3 + rx;
  }
  __syncthreads();
  if (i >= T || !valid) return;
  const float* rb = rel_bias + ((size_t)h * T + i) * T;
  const int li = lab[i];
  float s[T];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < T; ++j) {
    float z = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) z += q[d] * ks[j][d];
    z += rb[j];
    if (shift && lab[j] != li) z += -100.f;
    s[j] = z;
    m = fmaxf(m, z);
  }
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < T; ++j) { s[j] = __expf(s[j] - m); sum += s[j]; }
  const float inv = 1.f / sum;
  float o[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) o[d] = 0.f;
#pragma unroll
  for (int j = 0; j < T; ++j)
#pragma unroll
    for (int d = 0; d < HD; ++d) o[d] += s[j] * vs[j][d];
  float* dst = out + row * C + h * HD;
#pragma unroll
  for (int d = 0; d < HD; d += 4)
    *reinterpret_cast<float4*>(dst + d) = make_float4(o[d] * inv, o[d + 1] * inv, o[d + 2] * inv, o[d + 3] * inv);
}

static int swin_a_rows(const isf_swin_a& a, int M) {
  switch (a.mode) {
    case ISF_SWIN_A_ROWS: return M;
    case ISF_SWIN_A_PATCH: return a.n * ((a.h + 3) >> 2) * ((a.w + 3) >> 2);
    case ISF_SWIN_A_MERGE: return a.n * ((a.h + 1) >> 1) * ((a.w + 1) >> 1);
    case ISF_SWIN_A_UPCAT: return a.n * a.h * a.w;
  }
  return -1;
}

static int swin_check_a(const isf_swin_a* a, int M, int K, bool gemm) {
  ISF_REQUIRE(a && a->x, ISF_ERR_ARG, "swin: null A operand");
  ISF_REQUIRE(a->mode >= ISF_SWIN_A_ROWS && a->mode <= ISF_SWIN_A_UPCAT, ISF_ERR_ARG, "swin: bad A mode %d", a->mode);
  ISF_REQUIRE(swin_a_rows(*a, M) == M, ISF_ERR_ARG, "swin: %d rows do not match the A geometry", M);
  ISF_REQUIRE(K > 0 && K % (gemm ? 32 : 8) == 0, ISF_ERR_UNSUPPORTED, "swin: K %d (need %% %d)", K, gemm ? 32 : 8);
  switch (a->mode) {
    case ISF_SWIN_A_ROWS:
      ISF_REQUIRE(a->ldx >= K && a->ldx % 4 == 0 && ((uintptr_t)a->x & 15) == 0, ISF_ERR_ARG,
                  "swin: rows need ldx >= K, ldx %% 4 == 0 (%% 8 for f16 rows, ldx in elements of the row type), "
                  "16-byte aligned x");
      break;
    case ISF_SWIN_A_MERGE:
      ISF_REQUIRE(a->c % 8 == 0 && K == 4 * a->c && ((uintptr_t)a->x & 15) == 0, ISF_ERR_ARG,
                  "swin: merge needs C %% 8 == 0 and K == 4 C");
      break;
    case ISF_SWIN_A_PATCH:
      ISF_REQUIRE(a->c * 16 <= K && K - a->c * 16 < 32, ISF_ERR_ARG, "swin: patch K %d for %d channels", K, a->c);
      break;
    case ISF_SWIN_A_UPCAT:
      ISF_REQUIRE(a->x2 && a->c % 8 == 0 && K == a->c + a->c2 && a->h2 > 0 && a->w2 > 0, ISF_ERR_ARG,
                  "swin: upcat needs C1 %% 8 == 0 and K == C1 + C2");
      break;
  }
  return ISF_OK;
}

// The swin_gemm_kernel instantiations that are built, one row each: swin_gemm_launch looks the call's form up here, and a
// form without a row is ISF_ERR_UNSUPPORTED.  Default mode (X3): ROWS plain / LayerNorm / row scale, MERGE plain /
// LayerNorm, PATCH, UPCAT.  f16 inference mode: ROWS {fp32 rows plain, fp32 rows LayerNorm, f16 rows} x {fp32, f16 out},
// MERGE plain / LayerNorm, PATCH -- the forms SwinTransformer's forward is made of (no DropPath, no UPCAT).  Mixed-precision
// training (isf_swin_gemm_f16_rowscale): ROWS f16 rows with the row scale -> fp32, the proj / fc2 epilogue with DropPath.
// The kernels stand in the code object in row order.
using SwinGemmKernel = void (*)(isf_swin_a, int, int, const uint4*, const float*, int, SwinEpi, float*);
struct SwinGemmForm { int mode; bool ln, rs; int prec; bool y16; SwinGemmKernel kernel; };
template <int MODE, bool LN, bool RS = false, int PREC = SWIN_PREC_X3, bool Y16 = false>
constexpr SwinGemmForm swin_gemm_form() { return {MODE, LN, RS, PREC, Y16, swin_gemm_kernel<MODE, LN, RS, PREC, Y16>}; }
static const SwinGemmForm swin_gemm_forms[] = {
    swin_gemm_form<ISF_SWIN_A_ROWS, false, false, SWIN_PREC_F16_ROWS, true>(),
    swin_gemm_form<ISF_SWIN_A_ROWS, false, false, SWIN_PREC_F16_ROWS, false>(),
    swin_gemm_form<ISF_SWIN_A_ROWS, true, false, SWIN_PREC_F16, true>(),
    swin_gemm_form<ISF_SWIN_A_ROWS, true, false, SWIN_PREC_F16, false>(),
    swin_gemm_form<ISF_SWIN_A_ROWS, false, false, SWIN_PREC_F16, true>(),
    swin_gemm_form<ISF_SWIN_A_ROWS, false, false, SWIN_PREC_F16, false>(),
    swin_gemm_form<ISF_SWIN_A_MERGE, true, false, SWIN_PREC_F16, false>(),
    swin_gemm_form<ISF_SWIN_A_MERGE, false, false, SWIN_PREC_F16, false>(),
    swin_gemm_form<ISF_SWIN_A_PATCH, false, false, SWIN_PREC_F16, false>(),
    swin_gemm_form<ISF_SWIN_A_ROWS, false, true>(),
    swin_gemm_form<ISF_SWIN_A_ROWS, true>(),
    swin_gemm_form<ISF_SWIN_A_ROWS, false>(),
    swin_gemm_form<ISF_SWIN_A_MERGE, true>(),
    swin_gemm_form<ISF_SWIN_A_MERGE, false>(),
    swin_gemm_form<ISF_SWIN_A_PATCH, false>(),
    swin_gemm_form<ISF_SWIN_A_UPCAT, false>(),
    swin_gemm_form<ISF_SWIN_A_ROWS, false, true, SWIN_PREC_F16_ROWS, false>(),
};

}  // namespace isf

extern "C" {

static int swin_gemm_launch(const isf_swin_a* a, int num_rows, int k, const void* packed_weight, int out_features,
                            const float* scale, const float* shift, int activation, const float* residual,
                            const float* row_scale, int rows_per_sample, float* y, int ldy, int y_hw,
                            isf_stream_t stream, int prec = isf::SWIN_PREC_X3, bool y16 = false) {
  using namespace isf;
  ISF_REQUIRE(num_rows >= 0 && out_features > 0 && out_features % 16 == 0, ISF_ERR_ARG,
              "swin_gemm: bad sizes (rows %d, out %d)", num_rows, out_features);
  if (num_rows == 0) return ISF_OK;
  ISF_TRY(swin_check_a(a, num_rows, k, true));
  ISF_REQUIRE(packed_weight && y, ISF_ERR_ARG, "swin_gemm: null pointer");
  const bool ln = a->ln_stats != nullptr;
  ISF_REQUIRE(!ln || (a->ln_gamma && a->ln_beta), ISF_ERR_ARG, "swin_gemm: LayerNorm prologue needs gamma, beta");
  ISF_REQUIRE(y_hw > 0 ? num_rows % y_hw == 0 : ldy >= out_features, ISF_ERR_ARG, "swin_gemm: bad output layout");
  ISF_REQUIRE(activation >= 0 && activation <= 2, ISF_ERR_ARG, "swin_gemm: activation %d", activation);
  ISF_REQUIRE(!row_scale || (rows_per_sample > 0 && num_rows % rows_per_sample == 0), ISF_ERR_ARG,
              "swin_gemm_rowscale: rows %d a multiple of rows_per_sample %d", num_rows, rows_per_sample);
  // the f16 output store knows rows only, and the mode is built for row-major outputs
  ISF_REQUIRE(prec == SWIN_PREC_X3 || y_hw == 0, ISF_ERR_UNSUPPORTED, "swin_gemm_f16: row-major output only");
  ISF_REQUIRE(prec != SWIN_PREC_F16_ROWS || a->ldx % 8 == 0, ISF_ERR_ARG,
              "swin_gemm_f16: f16 A rows need ldx %% 8 == 0 (f16 elements)");
  const SwinGemmForm* form = nullptr;
  for (const SwinGemmForm& f : swin_gemm_forms)
    if (f.mode == a->mode && f.ln == ln && f.rs == (row_scale != nullptr) && f.prec == prec && f.y16 == y16) form = &f;
  ISF_REQUIRE(form, ISF_ERR_UNSUPPORTED,
              "swin_gemm: form not built (loader %d, LayerNorm prologue %d, row scale %d, operand precision %d, f16 "
              "output %d)", a->mode, (int)ln, (int)(row_scale != nullptr), prec, (int)y16);
  const uint4* wp = reinterpret_cast<const uint4*>(packed_weight);
  const float* winv = prec != SWIN_PREC_X3 ? nullptr :
      reinterpret_cast<const float*>(reinterpret_cast<const char*>(packed_weight) + (size_t)out_features * k * 4);
  SwinEpi ep{scale, shift, residual, activation, ldy, y_hw, row_scale, rows_per_sample};
  const dim3 grid(ceil_div(out_features / 16, 4), ceil_div(num_rows, SW_BM)), block(256);
  hipLaunchKernelGGL(form->kernel, grid, block, 0, as_stream(stream), *a, num_rows, k, wp, winv, out_features, ep, y);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_swin_gemm(const isf_swin_a* a, int num_rows, int k, const void* packed_weight, int out_features,
                  const float* scale, const float* shift, int activation, const float* residual, float* y, int ldy,
                  int y_hw, isf_stream_t stream) {
  return swin_gemm_launch(a, num_rows, k, packed_weight, out_features, scale, shift, activation, residual, nullptr, 0, y,
                          ldy, y_hw, stream);
}

int isf_swin_gemm_rowscale(const isf_swin_a* a, int num_rows, int k, const void* packed_weight, int out_features,
                           const float* scale, const float* shift, int activation, const float* residual,
                           const float* row_scale, int rows_per_sample, float* y, int ldy, int y_hw,
                           isf_stream_t stream) {
  ISF_REQUIRE(row_scale, ISF_ERR_ARG, "swin_gemm_rowscale: null row_scale");
  return swin_gemm_launch(a, num_rows, k, packed_weight, out_features, scale, shift, activation, residual, row_scale,
                          rows_per_sample, y, ldy, y_hw, stream);
}

int isf_swin_gemm_f16(const isf_swin_a* a, int a_is_f16, int num_rows, int k, const void* packed_weight_f16,
                      int out_features, const float* scale, const float* shift, int activation, const float* residual,
                      void* y, int y_is_f16, int ldy, int y_hw, isf_stream_t stream) {
  return swin_gemm_launch(a, num_rows, k, packed_weight_f16, out_features, scale, shift, activation, residual, nullptr, 0,
                          reinterpret_cast<float*>(y), ldy, y_hw, stream,
                          a_is_f16 ? isf::SWIN_PREC_F16_ROWS : isf::SWIN_PREC_F16, y_is_f16 != 0);
}

int isf_swin_gemm_f16_rowscale(const isf_swin_a* a, int a_is_f16, int num_rows, int k, const void* packed_weight_f16,
                               int out_features, const float* scale, const float* shift, int activation,
                               const float* residual, const float* row_scale, int rows_per_sample, void* y, int y_is_f16,
                               int ldy, int y_hw, isf_stream_t stream) {
  ISF_REQUIRE(row_scale, ISF_ERR_ARG, "swin_gemm_f16_rowscale: null row_scale");
  return swin_gemm_launch(a, num_rows, k, packed_weight_f16, out_features, scale, shift, activation, residual, row_scale,
                          rows_per_sample, reinterpret_cast<float*>(y), ldy, y_hw, stream,
                          a_is_f16 ? isf::SWIN_PREC_F16_ROWS : isf::SWIN_PREC_F16, y_is_f16 != 0);
}

int isf_swin_row_stats(const isf_swin_a* a, int num_rows, int k, float eps, float* stats, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num_rows >= 0, ISF_ERR_ARG, "swin_row_stats: bad sizes");
  if (num_rows == 0) return ISF_OK;
  ISF_TRY(swin_check_a(a, num_rows, k, false));
  ISF_REQUIRE(stats && (a->mode == ISF_SWIN_A_ROWS || a->mode == ISF_SWIN_A_MERGE), ISF_ERR_ARG,
              "swin_row_stats: rows / merge mode only");
  hipStream_t st = as_stream(stream);
  const dim3 grid(ceil_div(num_rows, 4)), block(256);
  if (a->mode == ISF_SWIN_A_ROWS)
    hipLaunchKernelGGL(swin_row_stats_kernel<ISF_SWIN_A_ROWS>, grid, block, 0, st, *a, num_rows, k, eps, stats);
  else
    hipLaunchKernelGGL(swin_row_stats_kernel<ISF_SWIN_A_MERGE>, grid, block, 0, st, *a, num_rows, k, eps, stats);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_swin_layernorm(const float* x, int num_rows, int channels, const float* gamma, const float* beta, float eps,
                       float* y, int y_hw, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num_rows >= 0 && channels > 0 && y_hw >= 0, ISF_ERR_ARG, "swin_layernorm: bad sizes");
  if (num_rows == 0) return ISF_OK;
  ISF_REQUIRE(x && gamma && beta && y && x != y, ISF_ERR_ARG, "swin_layernorm: null or aliased pointer");
  ISF_REQUIRE(!y_hw || num_rows % y_hw == 0, ISF_ERR_ARG, "swin_layernorm: rows not a multiple of hw");
  hipLaunchKernelGGL(swin_layernorm_kernel, dim3(ceil_div(num_rows, 64)), dim3(256), 0, as_stream(stream), x,
                     num_rows, channels, gamma, beta, eps, y, y_hw);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_swin_window_attention(const float* qkv, const float* qkv_bias, const float* rel_bias, int batch, int height,
                              int width, int channels, int heads, int window, int shift, float scale, float* out,
                              isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(batch >= 0 && height > 0 && width > 0 && heads > 0, ISF_ERR_ARG, "swin_window_attention: bad sizes");
  if (batch == 0) return ISF_OK;
  ISF_REQUIRE(qkv && rel_bias && out, ISF_ERR_ARG, "swin_window_attention: null pointer");
  ISF_REQUIRE(window == 7 && channels == 32 * heads && shift >= 0 && shift < window, ISF_ERR_UNSUPPORTED,
              "swin_window_attention: window 7, head dim 32 only (window %d, C %d, heads %d, shift %d)", window,
              channels, heads, shift);
  const int nw = ceil_div(height, 7) * ceil_div(width, 7);
  hipLaunchKernelGGL(swin_window_attn_kernel, dim3(nw, batch, heads), dim3(64), 0, as_stream(stream), qkv, qkv_bias,
                     rel_bias, height, width, channels, heads, shift, scale, out);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

}  // extern "C"
