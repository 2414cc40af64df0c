// isf_swin_f16.hip -- the f16 inference mode of the Swin-T backbone (SwinTransformer.set_precision("f16")): what is not
// the GEMM (isf_swin_gemm_f16 is swin_gemm_kernel of isf_swin.hip, instantiated for single-pass products; swin.gemm in
// Python).  swin.window_attention picks this file's attention entry when the qkv rows are f16.
//
// Reference: mmdet3d/models/backbones/swin.py (WindowMSA / ShiftWindowMSA) under mmcv's fp16 machinery (auto_fp16 /
// torch.autocast): half qkv, half matmuls, softmax, half attention output.  Here:
//   isf_swin_window_attention_f16  (shifted) window attention on f16 token-major qkv rows, on the matrix cores.  One wave
//                        per (window, image, head).  The index arithmetic restates swin_window_attn_kernel's (isf_swin.hip;
//                        a shared inline helper changed the machine code of both kernels): zero padding to
//                        multiples of 7, cyclic shift, partition / reverse, a padded cell's q / k / v = the qkv bias (and
//                        the cell IS attended to), -100 between shift regions, relative position bias [heads, 49, 49].
//                        The 49 tokens are padded to 64 = 4 tiles of 16; head dim 32 = one K step of
//                        v_mfma_f32_16x16x32_f16.  S^T = K Q^T (16 MFMAs) puts a query on a lane column: lane (col, g) of
//                        tile (kt, qt) holds keys 16 kt + 4 g + j of query 16 qt + col, so the row max / sum are an
//                        in-lane reduction + two __shfl_xor steps and the probabilities are already the B operand of
//                        O^T = V^T P^T: the contraction index of an MFMA may be permuted if both operands agree, so
//                        score tiles 2 p and 2 p + 1 form one 32-deep fragment (position 8 g + jj <-> key 32 p + 4 g +
//                        jj for jj < 4, 32 p + 16 + 4 g + jj - 4 else) and V^T is read from LDS in that order.  The 15
//                        tile-padding keys get -inf (they are not the spatial padding cells).  q and k fragments are
//                        16-byte global loads; only V goes through LDS (transposed on the way in).
//                        Scores, softmax and accumulation are fp32; P is rounded to f16 for the second product; the row
//                        sum keeps the unrounded terms.
//   isf_pack_linear_f16  weight [out, in] fp32 -> one plane of f16 B fragments, [in / 32][out / 16][64 lanes] x 8 f16.
// Every store to an f16 tensor saturates at +-65504 instead of producing inf (sat_f16).
#include "isf_common.h"
#include "isf_f16.h"

namespace isf {

typedef float wf4 __attribute__((ext_vector_type(4)));

constexpr int WA_VT_LD = 68;   // f16 per row of the transposed V tile: 136 bytes, 8-byte aligned reads, 4 g rows 16 banks apart

__device__ __forceinline__ fh8 wa_bias8(const float* p) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  return fh8{sat_f16(a.x), sat_f16(a.y), sat_f16(a.z), sat_f16(a.w), sat_f16(b.x), sat_f16(b.y), sat_f16(b.z), sat_f16(b.w)};
}

// grid ceil(total / 4), 4 waves; item = ((image * windows + window) * heads + head): the waves of a workgroup read
// neighbouring 64-byte pieces of the same qkv rows
__global__ __launch_bounds__(256) void swin_window_attn_f16_kernel(const _Float16* __restrict__ qkv,
                                                                    const float* __restrict__ qkv_bias,
                                                                    const float* __restrict__ rel_bias, int H, int W,
                                                                    int C, int heads, int shift, float scale, int total,
                                                                    _Float16* __restrict__ out) {
  constexpr int WS = 7, T = 49, HD = 32;
  __shared__ __attribute__((aligned(16))) _Float16 vt[4][HD][WA_VT_LD];   // [wave][dim][key]
  __shared__ __attribute__((aligned(16))) int lab_s[4][64];               // shift region of a token; 255: tile padding
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, g = lane >> 4;
  int item = blockIdx.x * 4 + wave;
  const bool live = item < total;            // a surplus wave redoes the last item and stores nothing (no early exit:
  if (!live) item = total - 1;               // the workgroup meets at one barrier)
  const int Hp = (H + WS - 1) / WS * WS, Wp = (W + WS - 1) / WS * WS;
  const int nww = Wp / WS, nw = (Hp / WS) * nww;
  const int h = item % heads, rest = item / heads;
  const int win = rest % nw, b = rest / nw;
  const int wy = win / nww, wx = win - wy * nww;
  // token `lane` of the window: its row of qkv / out, -1 for a spatial padding cell, -2 for tile padding
  int my_row = -2, my_lab = 255;
  if (lane < T) {
    const int sy = wy * WS + lane / WS, sx = wx * WS + lane % WS;
    int py = sy + shift, px = sx + shift;
    if (py >= Hp) py -= Hp;
    if (px >= Wp) px -= Wp;
    my_row = (py < H && px < W) ? (b * H + py) * W + px : -1;
    const int ry = sy < Hp - WS ? 0 : (sy < Hp - shift ? 1 : 2);
    const int rx = sx < Wp - WS ? 0 : (sx < Wp - shift ? 1 : 2);
    my_lab = ry * 3 + rx;
  }
  lab_s[wave][lane] = my_lab;
  // fragments: lane (col, g) holds dims 8 g .. 8 g + 7 of token 16 t + col -- K as the A operand, Q as the B operand
  fh8 qf[4], kf[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int rt = __shfl(my_row, 16 * t + col, 64);
    fh8 q8 = fh8{0, 0, 0, 0, 0, 0, 0, 0}, k8 = q8, v8 = q8;
    if (rt >= 0) {
      const _Float16* src = qkv + (size_t)rt * (3 * C) + h * HD + 8 * g;
      q8 = *reinterpret_cast<const fh8*>(src);
      k8 = *reinterpret_cast<const fh8*>(src + C);
      v8 = *reinterpret_cast<const fh8*>(src + 2 * C);
    } else if (rt == -1 && qkv_bias) {
      // zero padding comes after norm1: a padded cell's q / k / v are the qkv bias, as the qkv GEMM would have stored it
      const float* src = qkv_bias + h * HD + 8 * g;
      q8 = wa_bias8(src);
      k8 = wa_bias8(src + C);
      v8 = wa_bias8(src + 2 * C);
    }
    qf[t] = q8;
    kf[t] = k8;
#pragma unroll
    for (int i = 0; i < 8; ++i) vt[wave][8 * g + i][16 * t + col] = v8[i];
  }
  __syncthreads();
  // S^T[key 16 kt + 4 g + j][query 16 qt + col]
  wf4 s[4][4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int qt = 0; qt < 4; ++qt)
      s[kt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[kt], qf[qt], wf4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
  float inv[4];
#pragma unroll
  for (int qt = 0; qt < 4; ++qt) {
    const int qi = 16 * qt + col;
    const int lq = lab_s[wave][qi];
    const float* rb = rel_bias + ((size_t)h * T + (qi < T ? qi : 0)) * T;   // a tile-padding query is never stored
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const int4 lk4 = *reinterpret_cast<const int4*>(&lab_s[wave][16 * kt + 4 * g]);
      const int lk[4] = {lk4.x, lk4.y, lk4.z, lk4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int key = 16 * kt + 4 * g + j;
        float z = -INFINITY;                         // tile-padding keys are outside the softmax
        if (key < T) {
          z = s[kt][qt][j] * scale + rb[key];
          if (shift && lk[j] != lq) z += -100.f;
        }
        s[kt][qt][j] = z;
        m = fmaxf(m, z);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p = __expf(s[kt][qt][j] - m);
        s[kt][qt][j] = p;
        sum += p;
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    inv[qt] = 1.f / sum;
  }
  // O^T[dim 16 dt + 4 g + j][query 16 qt + col] = sum over p of V^T fragment . P^T fragment (keys in the order above)
  fh8 pf[4][2];
#pragma unroll
  for (int qt = 0; qt < 4; ++qt)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const wf4 a = s[2 * p][qt], c = s[2 * p + 1][qt];
      pf[qt][p] = fh8{(_Float16)a[0], (_Float16)a[1], (_Float16)a[2], (_Float16)a[3],
                      (_Float16)c[0], (_Float16)c[1], (_Float16)c[2], (_Float16)c[3]};
    }
  int rq[4];
#pragma unroll
  for (int qt = 0; qt < 4; ++qt) rq[qt] = __shfl(my_row, 16 * qt + col, 64);
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    fh8 vf[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const _Float16* vr = &vt[wave][16 * dt + col][32 * p + 4 * g];
      const fh4 lo = *reinterpret_cast<const fh4*>(vr), hi = *reinterpret_cast<const fh4*>(vr + 16);
      vf[p] = fh8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      wf4 o = wf4{0.f, 0.f, 0.f, 0.f};
      o = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[0], pf[qt][0], o, 0, 0, 0);
      o = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[1], pf[qt][1], o, 0, 0, 0);
      if (live && rq[qt] >= 0) {
        const fh4 r = fh4{sat_f16(o[0] * inv[qt]), sat_f16(o[1] * inv[qt]), sat_f16(o[2] * inv[qt]),
                          sat_f16(o[3] * inv[qt])};
        *reinterpret_cast<fh4*>(out + (size_t)rq[qt] * C + h * HD + 16 * dt + 4 * g) = r;
      }
    }
  }
}

// one thread per 16-byte lane piece: lane (col, g) of tile (kc, nt) holds w[16 nt + col][32 kc + 8 g .. + 7]
__global__ void pack_linear_f16_kernel(const float* __restrict__ w, int N, int K, uint4* __restrict__ packed) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int ntiles = N >> 4, kcs = K >> 5;
  if (t >= (long long)kcs * ntiles * 64) return;
  const int lane = (int)(t & 63);
  const int nt = (int)((t >> 6) % ntiles);
  const int kc = (int)((t >> 6) / ntiles);
  const float* src = w + (size_t)(16 * nt + (lane & 15)) * K + 32 * kc + 8 * (lane >> 4);
  fh8 v;
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) v[jj] = sat_f16(src[jj]);
  packed[t] = *reinterpret_cast<const uint4*>(&v);
}

}  // namespace isf

extern "C" {

size_t isf_packed_linear_f16_bytes(int out_features, int in_features) {
  return (size_t)out_features * in_features * 2;
}

int isf_pack_linear_f16(const float* weight, int out_features, int in_features, void* packed, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(weight && packed && out_features % 16 == 0 && in_features % 32 == 0 && out_features > 0 && in_features > 0,
              ISF_ERR_ARG, "pack_linear_f16: need out %% 16 == 0 and in %% 32 == 0 (got %d, %d)", out_features,
              in_features);
  ISF_REQUIRE(((uintptr_t)packed & 15) == 0, ISF_ERR_ARG, "pack_linear_f16: packed must be 16-byte aligned");
  const long long total = (long long)(in_features / 32) * (out_features / 16) * 64;
  hipLaunchKernelGGL(pack_linear_f16_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(stream), weight,
                     out_features, in_features, reinterpret_cast<uint4*>(packed));
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_swin_window_attention_f16(const void* qkv, const float* qkv_bias, const float* rel_bias, int batch, int height,
                                  int width, int channels, int heads, int window, int shift, float scale, void* out,
                                  isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(batch >= 0 && height > 0 && width > 0 && heads > 0, ISF_ERR_ARG, "swin_window_attention_f16: bad sizes");
  if (batch == 0) return ISF_OK;
  ISF_REQUIRE(qkv && rel_bias && out, ISF_ERR_ARG, "swin_window_attention_f16: null pointer");
  ISF_REQUIRE(window == 7 && channels == 32 * heads && shift >= 0 && shift < window, ISF_ERR_UNSUPPORTED,
              "swin_window_attention_f16: window 7, head dim 32 only (window %d, C %d, heads %d, shift %d)", window,
              channels, heads, shift);
  ISF_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)out & 7) == 0 && (!qkv_bias || ((uintptr_t)qkv_bias & 15) == 0),
              ISF_ERR_ARG, "swin_window_attention_f16: qkv / qkv_bias need 16-byte, out 8-byte alignment");
  const long long rows = (long long)batch * height * width;
  const long long items = (long long)batch * ceil_div(height, 7) * ceil_div(width, 7) * heads;
  ISF_REQUIRE(rows < (1ll << 31) && items < (1ll << 31), ISF_ERR_UNSUPPORTED,
              "swin_window_attention_f16: %lld rows / %lld (window, head) items exceed 2^31", rows, items);
  hipLaunchKernelGGL(swin_window_attn_f16_kernel, dim3(ceil_div(items, 4)), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const _Float16*>(qkv), qkv_bias, rel_bias, height, width, channels, heads, shift,
                     scale, (int)items, reinterpret_cast<_Float16*>(out));
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

}  // extern "C"
