// isf_swin_train_f16.hip -- the mixed-precision training mode of the Swin-T backbone (SwinTransformer.set_precision("mixed")):
// the two backward kernels that are not the forward's GEMM.  The forward of the mode is the f16 inference mode's
// (isf_swin_gemm_f16, isf_swin_window_attention_f16) with the DropPath factor in the epilogue (isf_swin_gemm_f16_rowscale,
// isf_swin.hip); dX = dY . W is isf_swin_gemm_f16 on the f16 pack of the transposed weight; LayerNorm / GELU backward,
// column sums and the row factor are the fp32 kernels of isf_swin_train.hip.
//
// Reference: mmdet3d/models/backbones/swin.py (WindowMSA / ShiftWindowMSA) and nn.Linear under autograd inside
// torch.autocast(float16): half matmuls with fp32 accumulation, fp32 softmax backward, fp32 parameter gradients.  Here:
//   isf_rows_weight_grad_f16   dW [N, K] = G^T . X as rows_wgrad_kernel (isf_swin_train.hip) computes it -- same tiling
//                        (128 n x 64 k per workgroup, 4 waves of 32 x 64), same chunking of the rows, same fp32 partials
//                        and the same ordered second pass -- with ONE v_mfma_f32_16x16x32_f16 per product: both operands
//                        are rounded to f16 once (saturating), the products of f16 numbers are exact in fp32, so only the
//                        accumulation rounds.  X is fp32 rows or the f16 rows the forward stored.  Half the LDS (24 KiB),
//                        a third of the matrix instructions.
//   isf_swin_window_attention_backward_f16   backward of swin_window_attn_f16_kernel (isf_swin_f16.hip) on the matrix
//                        cores, one wave per (group of windows, head).  The index arithmetic restates the forward's: zero
//                        padding to multiples of 7, cyclic shift, a padded cell's q / k / v = the f16-rounded qkv bias,
//                        -100 between shift regions, the 15 tile-padding keys outside the softmax.  49 tokens -> 64 = 4
//                        tiles of 16, head dim 32 = one K step.  An MFMA output tile puts ONE index on a lane column and
//                        four consecutive values of the other in the lane, and a tile can only be the next product's B
//                        operand over the index it holds in-lane.  dQ contracts over keys, dK and dV over queries, so the
//                        scores are formed in both orientations (the A and B fragments have the same shape: swapping the
//                        operands transposes the tile, no LDS round trip for P or dS):
//                          pass 1, per query tile   S^T = K Q^T, dP^T = V dO^T  (keys in-lane, query = lane column)
//                                  softmax as the forward (fp32, __expf), delta = rowsum(P o dP) = rowsum(dO o O) in fp32,
//                                  dS^T = P o (dP - delta) -> f16 -> dQ^T = K^T dS^T; (max, 1 / sum, delta) per query to LDS
//                          pass 2, per key tile     S = Q K^T, dP = dO V^T      (queries in-lane, key = lane column)
//                                  P and dS again from the stored row statistics -> f16 -> dV^T = dO^T P, dK^T = Q^T dS;
//                                  the UNROUNDED dS is added to the wave's dB accumulators
//                        Q^T, K^T, dO^T fragments come from transposed LDS tiles (as V^T in the forward); the output
//                        tiles are [dim][token], four consecutive dims per lane: one 16-byte store per token.
//                        Reductions: the wave walks a fixed range of (image, window) items; dB lives in 64 accumulator
//                        registers (a 49 x 49 fp32 LDS matrix per wave would cost a read-modify-write of every element
//                        per item; the registers cost nothing and the file has room: one wave per SIMD) and is written
//                        once, as are the padded cells' dK / dV sums (in-lane over items, then a fixed xor tree over the
//                        16 key columns).  Workspace layout and second pass: swin_attn_bwd_finish (isf_swin_train.hip).
//                        Range: dO is multiplied by 2^-6 when it is rounded to f16 and every output by 2^6 (exact), see
//                        AB16_DO_SCALE.  Every conversion to an f16 operand saturates (sat_f16).
// Every cross-window sum is a fixed-order two-pass reduction, as in isf_swin_train.hip.
#include "isf_common.h"
#include "isf_f16.h"

namespace isf {

typedef float tf4 __attribute__((ext_vector_type(4)));
typedef float tf8 __attribute__((ext_vector_type(8)));

constexpr int WG16_TN = 128;    // dW rows (n) per workgroup
constexpr int WG16_TK = 64;     // dW columns (k) per workgroup
constexpr int WG16_STEP = 32;   // token rows per MFMA step

__device__ __forceinline__ fh8 sat_f16x8(const tf8 v) {
  return fh8{sat_f16(v[0]), sat_f16(v[1]), sat_f16(v[2]), sat_f16(v[3]), sat_f16(v[4]), sat_f16(v[5]), sat_f16(v[6]),
             sat_f16(v[7])};
}

// 8 consecutive token rows rb .. rb + 7 (< rend kept, the rest 0) of column `col`, as they are in memory: the rounding to
// f16 waits until the values go to LDS, after the step's matrix instructions, so the loads stay in flight behind them
template <typename T>
__device__ __forceinline__ auto wg16_load8(const T* __restrict__ x, int ld, int rb, int rend, int col, bool col_ok) {
  typedef T tv8 __attribute__((ext_vector_type(8)));
  tv8 v = tv8{0, 0, 0, 0, 0, 0, 0, 0};
  if (!col_ok || rb >= rend) return v;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (rb + j < rend) v[j] = x[(size_t)(rb + j) * ld + col];
  return v;
}
__device__ __forceinline__ uint4 wg16_slot(const tf8 v) {
  const fh8 h = sat_f16x8(v);
  return *reinterpret_cast<const uint4*>(&h);
}
__device__ __forceinline__ uint4 wg16_slot(const fh8 v) { return *reinterpret_cast<const uint4*>(&v); }

// rows_wgrad_kernel's loader, ring and tile walk with one operand plane
template <typename XT>
__global__ __launch_bounds__(256) void rows_wgrad_f16_kernel(const float* __restrict__ g, const XT* __restrict__ x, int ldx,
                                                              int R, int N, int K, int rows_per_chunk,
                                                              float* __restrict__ ws) {
  __shared__ uint4 as_[2][4][WG16_TN];   // [buf][8-row group][n]
  __shared__ uint4 bs_[2][4][WG16_TK];   // [buf][8-row group][k]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int k0 = blockIdx.x * WG16_TK, n0 = blockIdx.y * WG16_TN;
  const int rbeg = blockIdx.z * rows_per_chunk;
  const int rend = rbeg + rows_per_chunk < R ? rbeg + rows_per_chunk : R;
  const int steps = (rend - rbeg + WG16_STEP - 1) / WG16_STEP;
  // loader slots: G two per thread (n = t & 127, row groups 2 (t >> 7) + i), X one (k = t & 63, row group t >> 6)
  const int an = t & 127, ag = (t >> 7) << 1;
  const int bk = t & 63, bg = t >> 6;
  const bool an_ok = n0 + an < N, bk_ok = k0 + bk < K;
  typedef XT xv8 __attribute__((ext_vector_type(8)));
  tf8 av[2];
  xv8 bv;
  auto fetch = [&](int s) {
    const int r0 = rbeg + s * WG16_STEP;
#pragma unroll
    for (int i = 0; i < 2; ++i) av[i] = wg16_load8<float>(g, N, r0 + 8 * (ag + i), rend, n0 + an, an_ok);
    bv = wg16_load8<XT>(x, ldx, r0 + 8 * bg, rend, k0 + bk, bk_ok);
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) as_[buf][ag + i][an] = wg16_slot(av[i]);
    bs_[buf][bg][bk] = wg16_slot(bv);
  };
  tf4 acc[2][4];
#pragma unroll
  for (int gi = 0; gi < 2; ++gi)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[gi][nt] = tf4{0.f, 0.f, 0.f, 0.f};
  fetch(0);
  commit(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const int buf = s & 1;
    const bool more = s + 1 < steps;
    if (more) fetch(s + 1);
    fh8 a[2];
#pragma unroll
    for (int gi = 0; gi < 2; ++gi) {
      const uint4 u = as_[buf][lane >> 4][wave * 32 + gi * 16 + (lane & 15)];
      a[gi] = *reinterpret_cast<const fh8*>(&u);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const uint4 u = bs_[buf][lane >> 4][nt * 16 + (lane & 15)];
      const fh8 b = *reinterpret_cast<const fh8*>(&u);
#pragma unroll
      for (int gi = 0; gi < 2; ++gi) acc[gi][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[gi], b, acc[gi][nt], 0, 0, 0);
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

// ------------------------------------------------------------------------------------- window-attention backward
constexpr int AB16_LD = 68;        // f16 per row of a transposed [dim][token] tile (as WA_VT_LD of the forward)
// dO is rounded to f16 as dO * AB16_DO_SCALE = dO 2^-6.  With |dO| < 2^10 (isf_grad_rescale) and |v| <= 32:
//   |dP| <= 32 max|dO| max|v|,  |dS| = P |dP - sum P dP| <= 2 max|dP|  ->  |dS 2^-6| < 2 * 32 * 2^10 * 2^-6 * 32 = 2^15
// so neither dO (< 2^4) nor dS reaches f16's 65504; dP itself only ever lives in fp32 accumulators.
constexpr float AB16_DO_SCALE = 1.f / 64.f, AB16_OUT_SCALE = 64.f;

__device__ __forceinline__ fh8 ab16_bias8(const float* p) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  return fh8{sat_f16(a.x), sat_f16(a.y), sat_f16(a.z), sat_f16(a.w), sat_f16(b.x), sat_f16(b.y), sat_f16(b.z), sat_f16(b.w)};
}

// contraction positions 8 g + jj of a 32-deep fragment <-> tokens 32 p + 4 g + jj (jj < 4), 32 p + 16 + 4 g + jj - 4 (else):
// two neighbouring output tiles of a lane, and the matching read of a transposed LDS tile
__device__ __forceinline__ fh8 ab16_pair_sat(const tf4 a, const tf4 c) {
  return fh8{sat_f16(a[0]), sat_f16(a[1]), sat_f16(a[2]), sat_f16(a[3]), sat_f16(c[0]), sat_f16(c[1]), sat_f16(c[2]),
             sat_f16(c[3])};
}
__device__ __forceinline__ fh8 ab16_tile_frag(const _Float16* row, int p, int g) {
  const fh4 lo = *reinterpret_cast<const fh4*>(row + 32 * p + 4 * g);
  const fh4 hi = *reinterpret_cast<const fh4*>(row + 32 * p + 16 + 4 * g);
  return fh8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// grid (groups, heads), one wave; group = items [grp * items_per_group, ...) of the (image, window) list
__global__ __launch_bounds__(64) void swin_window_attn_bwd_f16_kernel(const _Float16* __restrict__ qkv,
                                                                       const float* __restrict__ qkv_bias,
                                                                       const float* __restrict__ rel_bias,
                                                                       const float* __restrict__ dout, int B, int H, int W,
                                                                       int C, int heads, int shift, float scale,
                                                                       int items_per_group, float* __restrict__ dqkv,
                                                                       float* __restrict__ part_bias,
                                                                       float* __restrict__ part_pad) {
  constexpr int WS = 7, T = 49, HD = 32;
  __shared__ __attribute__((aligned(16))) _Float16 kT[HD][AB16_LD], qT[HD][AB16_LD], doT[HD][AB16_LD];   // [dim][token]
  __shared__ __attribute__((aligned(16))) int lab_s[64];                  // shift region of a token; 255: tile padding
  __shared__ __attribute__((aligned(16))) float st_m[64], st_inv[64], st_delta[64];   // per query: max, 1 / sum, delta
  const int lane = threadIdx.x, col = lane & 15, g = lane >> 4;
  const int grp = blockIdx.x, h = blockIdx.y;
  const int Hp = (H + WS - 1) / WS * WS, Wp = (W + WS - 1) / WS * WS;
  const int nww = Wp / WS, nwin = (Hp / WS) * nww;
  const int total = nwin * B;
  const int beg = grp * items_per_group;
  const int end = beg + items_per_group < total ? beg + items_per_group : total;
  const size_t ld = (size_t)3 * C;
  const float qk_out = scale * AB16_OUT_SCALE;
  tf4 dbacc[4][4];        // [key tile][query tile]: queries 16 qt + 4 g + j of key 16 kt + col, in dO's f16 scale
  tf4 padk[2], padv[2];   // dims 16 dt + 4 g + j: this lane's padded keys' dK / dV
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) dbacc[kt][qt] = tf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) padk[dt] = padv[dt] = tf4{0.f, 0.f, 0.f, 0.f};
  for (int item = beg; item < end; ++item) {
    const int b = item / nwin, wi = item - b * nwin;
    const int wy = wi / nww, wx = wi - wy * nww;
    // token `lane` of the window: its row of qkv / dout / dqkv, -1 for a spatial padding cell, -2 for tile padding
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
    lab_s[lane] = my_lab;
    // fragments: lane (col, g) holds dims 8 g .. 8 g + 7 of token 16 t + col; A and B operands have this one shape
    fh8 qf[4], kf[4], vf[4], dof[4];
    int rtok[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int rt = __shfl(my_row, 16 * t + col, 64);
      rtok[t] = rt;
      fh8 q8 = fh8{0, 0, 0, 0, 0, 0, 0, 0}, k8 = q8, v8 = q8, d8 = q8;
      if (rt >= 0) {
        const _Float16* src = qkv + (size_t)rt * ld + h * HD + 8 * g;
        q8 = *reinterpret_cast<const fh8*>(src);
        k8 = *reinterpret_cast<const fh8*>(src + C);
        v8 = *reinterpret_cast<const fh8*>(src + 2 * C);
        // a padded query produced no output: its dO stays 0
        const float* gs = dout + (size_t)rt * C + h * HD + 8 * g;
        const float4 a = *reinterpret_cast<const float4*>(gs);
        const float4 c = *reinterpret_cast<const float4*>(gs + 4);
        d8 = sat_f16x8(tf8{a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w} * AB16_DO_SCALE);
      } else if (rt == -1 && qkv_bias) {
        const float* src = qkv_bias + h * HD + 8 * g;
        q8 = ab16_bias8(src);
        k8 = ab16_bias8(src + C);
        v8 = ab16_bias8(src + 2 * C);
      }
      qf[t] = q8;
      kf[t] = k8;
      vf[t] = v8;
      dof[t] = d8;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        kT[8 * g + i][16 * t + col] = k8[i];
        qT[8 * g + i][16 * t + col] = q8[i];
        doT[8 * g + i][16 * t + col] = d8[i];
      }
    }
    __syncthreads();
    // ---- pass 1: keys in-lane.  Tile (kt, qt): keys 16 kt + 4 g + j of query 16 qt + col
    {
      fh8 ktf[2][2];
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int p = 0; p < 2; ++p) ktf[dt][p] = ab16_tile_frag(&kT[16 * dt + col][0], p, g);
#pragma unroll
      for (int qt = 0; qt < 4; ++qt) {
        const int qi = 16 * qt + col;
        const int lq = lab_s[qi];
        const float* rb = rel_bias + ((size_t)h * T + (qi < T ? qi : 0)) * T;   // a tile-padding query has dO = 0
        tf4 s[4], dp[4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[kt], qf[qt], tf4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          dp[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[kt], dof[qt], tf4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        }
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          const int4 lk4 = *reinterpret_cast<const int4*>(&lab_s[16 * kt + 4 * g]);
          const int lk[4] = {lk4.x, lk4.y, lk4.z, lk4.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int key = 16 * kt + 4 * g + j;
            float z = -INFINITY;                         // tile-padding keys are outside the softmax
            if (key < T) {
              z = s[kt][j] * scale + rb[key];
              if (shift && lk[j] != lq) z += -100.f;
            }
            s[kt][j] = z;
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
            const float e = __expf(s[kt][j] - m);
            s[kt][j] = e;
            sum += e;
          }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.f / sum;
        float delta = 0.f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            s[kt][j] *= inv;
            delta += s[kt][j] * dp[kt][j];
          }
        delta += __shfl_xor(delta, 16, 64);
        delta += __shfl_xor(delta, 32, 64);
        if (g == 0) {
          st_m[qi] = m;
          st_inv[qi] = inv;
          st_delta[qi] = delta;
        }
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int j = 0; j < 4; ++j) s[kt][j] *= dp[kt][j] - delta;
        const fh8 ds0 = ab16_pair_sat(s[0], s[1]), ds1 = ab16_pair_sat(s[2], s[3]);
        // dQ^T[dim 16 dt + 4 g + j][query 16 qt + col] = K^T . dS^T
        const int rq = rtok[qt];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          tf4 o = __builtin_amdgcn_mfma_f32_16x16x32_f16(ktf[dt][0], ds0, tf4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          o = __builtin_amdgcn_mfma_f32_16x16x32_f16(ktf[dt][1], ds1, o, 0, 0, 0);
          if (rq >= 0)
            *reinterpret_cast<float4*>(dqkv + (size_t)rq * ld + h * HD + 16 * dt + 4 * g) =
                make_float4(o[0] * qk_out, o[1] * qk_out, o[2] * qk_out, o[3] * qk_out);
        }
      }
    }
    __syncthreads();   // the row statistics are in LDS
    // ---- pass 2: queries in-lane.  Tile (qt, kt): queries 16 qt + 4 g + j of key 16 kt + col
    {
      fh8 qtf[2][2], dotf[2][2];
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          qtf[dt][p] = ab16_tile_frag(&qT[16 * dt + col][0], p, g);
          dotf[dt][p] = ab16_tile_frag(&doT[16 * dt + col][0], p, g);
        }
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const int key = 16 * kt + col;
        const int lk = lab_s[key];
        const int rk = rtok[kt];
        const float* rb = rel_bias + (size_t)h * T * T + (key < T ? key : 0);
        tf4 pr[4], ds[4];
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
          const tf4 s = __builtin_amdgcn_mfma_f32_16x16x32_f16(qf[qt], kf[kt], tf4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          const tf4 dp = __builtin_amdgcn_mfma_f32_16x16x32_f16(dof[qt], vf[kt], tf4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          const float4 m4 = *reinterpret_cast<const float4*>(&st_m[16 * qt + 4 * g]);
          const float4 i4 = *reinterpret_cast<const float4*>(&st_inv[16 * qt + 4 * g]);
          const float4 d4 = *reinterpret_cast<const float4*>(&st_delta[16 * qt + 4 * g]);
          const int4 l4 = *reinterpret_cast<const int4*>(&lab_s[16 * qt + 4 * g]);
          const float mq[4] = {m4.x, m4.y, m4.z, m4.w}, iq[4] = {i4.x, i4.y, i4.z, i4.w};
          const float dq[4] = {d4.x, d4.y, d4.z, d4.w};
          const int lq[4] = {l4.x, l4.y, l4.z, l4.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int q = 16 * qt + 4 * g + j;
            float p = 0.f, d = 0.f;
            if (key < T && q < T) {
              float z = s[j] * scale + rb[q * T];
              if (shift && lq[j] != lk) z += -100.f;
              p = __expf(z - mq[j]) * iq[j];
              d = p * (dp[j] - dq[j]);
            }
            pr[qt][j] = p;
            ds[qt][j] = d;
          }
          dbacc[kt][qt] += ds[qt];   // the bias gradient takes the unrounded dS
        }
        const fh8 p0 = ab16_pair_sat(pr[0], pr[1]), p1 = ab16_pair_sat(pr[2], pr[3]);
        const fh8 ds0 = ab16_pair_sat(ds[0], ds[1]), ds1 = ab16_pair_sat(ds[2], ds[3]);
        // dV^T[dim][key] = dO^T . P,  dK^T[dim][key] = scale Q^T . dS
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          tf4 dv = __builtin_amdgcn_mfma_f32_16x16x32_f16(dotf[dt][0], p0, tf4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          dv = __builtin_amdgcn_mfma_f32_16x16x32_f16(dotf[dt][1], p1, dv, 0, 0, 0);
          tf4 dk = __builtin_amdgcn_mfma_f32_16x16x32_f16(qtf[dt][0], ds0, tf4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          dk = __builtin_amdgcn_mfma_f32_16x16x32_f16(qtf[dt][1], ds1, dk, 0, 0, 0);
          dv *= AB16_OUT_SCALE;
          dk *= qk_out;
          if (rk >= 0) {
            float* dst = dqkv + (size_t)rk * ld + C + h * HD + 16 * dt + 4 * g;
            *reinterpret_cast<float4*>(dst) = make_float4(dk[0], dk[1], dk[2], dk[3]);
            *reinterpret_cast<float4*>(dst + C) = make_float4(dv[0], dv[1], dv[2], dv[3]);
          } else if (rk == -1) {
            // a padded cell's k / v are the qkv bias: its dK / dV are the bias's gradient
            padk[dt] += dk;
            padv[dt] += dv;
          }
        }
      }
    }
    __syncthreads();   // the next item overwrites every LDS array
  }
  float* pb = part_bias + (size_t)(grp * heads + h) * T * T;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    const int key = 16 * kt + col;
#pragma unroll
    for (int qt = 0; qt < 4; ++qt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int q = 16 * qt + 4 * g + j;
        if (key < T && q < T) pb[q * T + key] = dbacc[kt][qt][j] * AB16_OUT_SCALE;
      }
  }
  // the 16 key columns' pad sums down a fixed xor tree; column 0 writes [dK dims 0..31 | dV dims 0..31]
  float* pp = part_pad + (size_t)(grp * heads + h) * 64;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float a = padk[dt][j], c = padv[dt][j];
#pragma unroll
      for (int d = 1; d < 16; d <<= 1) {
        a += __shfl_xor(a, d, 64);
        c += __shfl_xor(c, d, 64);
      }
      if (col == 0) {
        pp[16 * dt + 4 * g + j] = a;
        pp[HD + 16 * dt + 4 * g + j] = c;
      }
    }
}

}  // namespace isf

extern "C" {

int isf_rows_weight_grad_f16(const float* g, const void* x, int x_is_f16, int ldx, int num_rows, int out_features, int k,
                             const float* inv_scale, float* workspace, int num_chunks, float* dw, int ldw,
                             isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num_rows > 0 && out_features > 0 && k > 0, ISF_ERR_ARG,
              "rows_weight_grad_f16: bad sizes (rows %d, N %d, K %d)", num_rows, out_features, k);
  ISF_REQUIRE(g && x && workspace && dw && ldw >= k && ldx >= k, ISF_ERR_ARG,
              "rows_weight_grad_f16: null pointer, ldw %d < K %d or ldx %d < K", ldw, k, ldx);
  ISF_REQUIRE(num_chunks == isf_rows_weight_grad_chunks(num_rows, out_features, k), ISF_ERR_ARG,
              "rows_weight_grad_f16: workspace of %d chunks, isf_rows_weight_grad_chunks says %d", num_chunks,
              isf_rows_weight_grad_chunks(num_rows, out_features, k));
  const int rpc = wgrad_rows_per_chunk(num_rows, out_features, k);
  hipStream_t st = as_stream(stream);
  const dim3 grid(ceil_div(k, WG16_TK), ceil_div(out_features, WG16_TN), num_chunks), block(256);
  ISF_REQUIRE(grid.z <= 65535 && grid.y <= 65535, ISF_ERR_UNSUPPORTED, "rows_weight_grad_f16: grid too large");
  if (x_is_f16)
    hipLaunchKernelGGL(rows_wgrad_f16_kernel<_Float16>, grid, block, 0, st, g, reinterpret_cast<const _Float16*>(x), ldx,
                       num_rows, out_features, k, rpc, workspace);
  else
    hipLaunchKernelGGL(rows_wgrad_f16_kernel<float>, grid, block, 0, st, g, reinterpret_cast<const float*>(x), ldx,
                       num_rows, out_features, k, rpc, workspace);
  ISF_LAUNCH_CHECK();
  return rows_wgrad_reduce(workspace, num_chunks, out_features, k, inv_scale, dw, ldw, st);
}

int isf_swin_window_attention_backward_f16(const void* qkv, const float* qkv_bias, const float* rel_bias,
                                           const int64_t* rel_index, const float* dout, int batch, int height, int width,
                                           int channels, int heads, int window, int shift, float scale,
                                           const float* inv_scale, float* workspace, int num_groups, float* dqkv,
                                           float* drel_bias, float* dtable, int table_rows, float* dqkv_bias_pad,
                                           isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(batch > 0 && height > 0 && width > 0 && heads > 0, ISF_ERR_ARG,
              "swin_window_attention_backward_f16: bad sizes");
  ISF_REQUIRE(qkv && rel_bias && dout && workspace && dqkv && drel_bias && dqkv_bias_pad, ISF_ERR_ARG,
              "swin_window_attention_backward_f16: null pointer");
  ISF_REQUIRE(window == 7 && channels == 32 * heads && shift >= 0 && shift < window, ISF_ERR_UNSUPPORTED,
              "swin_window_attention_backward_f16: window 7, head dim 32 only (window %d, C %d, heads %d, shift %d)",
              window, channels, heads, shift);
  ISF_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)qkv_bias & 15) == 0 && ((uintptr_t)dout & 15) == 0 &&
                  ((uintptr_t)dqkv & 15) == 0, ISF_ERR_ARG, "swin_window_attention_backward_f16: unaligned pointer");
  ISF_REQUIRE(!dtable || (rel_index && table_rows > 0), ISF_ERR_ARG,
              "swin_window_attention_backward_f16: the table gradient needs relative_position_index and its row count");
  ISF_REQUIRE(num_groups == isf_swin_window_attention_backward_groups(batch, height, width, heads) &&
                  num_groups <= 65535 * 32, ISF_ERR_ARG,
              "swin_window_attention_backward_f16: workspace of %d groups, ..._groups says %d", num_groups,
              isf_swin_window_attention_backward_groups(batch, height, width, heads));
  ISF_REQUIRE(heads <= 65535, ISF_ERR_UNSUPPORTED, "swin_window_attention_backward_f16: heads %d", heads);
  ISF_REQUIRE((long long)batch * height * width < (1ll << 31), ISF_ERR_UNSUPPORTED,
              "swin_window_attention_backward_f16: %lld rows exceed 2^31", (long long)batch * height * width);
  const int ipg = attn_bwd_items_per_group(batch, height, width, heads);
  float* part_bias = workspace;
  float* part_pad = workspace + (size_t)num_groups * heads * 49 * 49;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(swin_window_attn_bwd_f16_kernel, dim3(num_groups, heads), dim3(64), 0, st,
                     reinterpret_cast<const _Float16*>(qkv), qkv_bias, rel_bias, dout, batch, height, width, channels,
                     heads, shift, scale, ipg, dqkv, part_bias, part_pad);
  ISF_LAUNCH_CHECK();
  return swin_attn_bwd_finish(part_bias, part_pad, num_groups, heads, channels, drel_bias, dqkv_bias_pad, rel_index,
                              inv_scale, dtable, table_rows, st);
}

}  // extern "C"
