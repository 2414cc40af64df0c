// isf_channel_attn_bwd.hip -- gradient of the A14 per-channel map attention (isf_channel_attn.hip; what autograd runs
// behind fusion_encoder.py:495-500).  Per map, with A = query_scene, Bm = query_ins, G = grad_out (R x R, R = 180):
//   P  = softmax(A Bm^T)          gP = G Bm^T          gS = P o (gP - rowsum(gP o P))
//   gA = G + gS Bm                gB = P^T G + gS^T A
// Two kernels, nothing saved by the forward, no atomics:
//   ROWS  one workgroup per map, Bm resident in LDS exactly as the forward stages it ([192][196] fp32).  A wave takes 16
//         query rows: the forward's GEMM1 forms the S^T tile and -- with the SAME A-operand reads from LDS, grad_out rows
//         in place of query_scene rows as the B operand -- the gP^T tile beside it (two independent accumulator chains
//         per LDS read).  Softmax and the row term D = rowsum(gP o P) happen in registers (4 lanes per row, two
//         shuffles); the gP registers become gS, which is the A operand of the forward's GEMM2 (gS . Bm), + G in the
//         epilogue.  P and gS tiles go to scratch for the second kernel.
//   COLS  gB = [P^T | gS^T] . [G ; A], a K = 2 R product.  No LDS: a wave owns a 64 x 64 output tile as 4 x 4
//         INTERLEAVED 16 x 16 tiles -- a lane's float4 of P[i][j0 + 4 l ..] feeds the four row tiles, its float4 of
//         G[i][w0 + 4 l ..] the four column tiles, so 4 loads of 16 bytes (256 contiguous bytes per row and 16 lanes)
//         feed 32 MFMAs and a lane ends up with 4 consecutive output columns per row (16-byte stores).  The k index of
//         an MFMA is the row i = i4 + (lane >> 4), the same for both operands.
// fp32 MFMA (v_mfma_f32_16x16x4_f32) throughout: exact fp32 products, fixed summation order (two calls give the same
// bits), and no result of a map depends on another map or on the number of maps.
#include "isf_common.h"

#include <algorithm>

namespace isf {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CB_ROWS = 192;    // padded keys (the forward's CA_ROWS)
constexpr int CB_LD = 196;      // LDS row stride (floats): 4 (mod 64), conflict-free row- and column-wise b128 reads
constexpr int CB_GROUP = 256;   // maps per scratch group: one workgroup per CU

// qs / qi / go / ga / pbuf / gsbuf: the GROUP's first map.  ga == nullptr: no gS . Bm; pbuf == nullptr: no scratch writes.
__global__ __launch_bounds__(256, 1) void channel_attention_bwd_rows_kernel(const float* __restrict__ qs,
                                                                            const float* __restrict__ qi,
                                                                            const float* __restrict__ go, int R,
                                                                            float* __restrict__ ga,
                                                                            float* __restrict__ pbuf,
                                                                            float* __restrict__ gsbuf) {
  extern __shared__ __attribute__((aligned(16))) float K[];   // [CB_ROWS][CB_LD]
  const size_t mat = (size_t)blockIdx.x * R * R;
  // stage Bm with zero padding: rows >= R meet p = gS = 0 and must be finite, columns >= R are never stored
  for (int i = threadIdx.x; i < CB_ROWS * (CB_LD / 4); i += 256) {
    const int r = i / (CB_LD / 4), c = (i % (CB_LD / 4)) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < R && c < R) v = *reinterpret_cast<const float4*>(qi + mat + (size_t)r * R + c);
    *reinterpret_cast<float4*>(K + r * CB_LD + c) = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, kg = lane >> 4;
  constexpr int JT = CB_ROWS / 16;   // 12 key tiles
  for (int i0 = wave * 16; i0 < R; i0 += 64) {
    const int irow = i0 + li < R ? i0 + li : R - 1;   // clamped: rows past R repeat row R - 1 and are not stored
    const float* arow = qs + mat + (size_t)irow * R;
    const float* grow = go + mat + (size_t)irow * R;
    // ---- GEMM1 twice over one set of LDS reads: S^T and gP^T tiles [192 keys x 16 queries]
    //      lane (i = li, kg), reg (jt, t)  <->  S[i][j = 16 jt + 4 kg + t]
    f32x4 s[JT], d[JT];
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) s[jt] = d[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int w0 = 0; w0 < R; w0 += 16) {
      const int w = w0 + 4 * kg;
      float4 ba = make_float4(0.f, 0.f, 0.f, 0.f), bg = ba;
      if (w < R) {   // R % 4 == 0
        ba = *reinterpret_cast<const float4*>(arow + w);
        bg = *reinterpret_cast<const float4*>(grow + w);
      }
#pragma unroll
      for (int jt = 0; jt < JT; ++jt) {
        const float4 a = *reinterpret_cast<const float4*>(K + (16 * jt + li) * CB_LD + w);   // zero beyond R
        s[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, ba.x, s[jt], 0, 0, 0);
        d[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bg.x, d[jt], 0, 0, 0);
        s[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, ba.y, s[jt], 0, 0, 0);
        d[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bg.y, d[jt], 0, 0, 0);
        s[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, ba.z, s[jt], 0, 0, 0);
        d[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bg.z, d[jt], 0, 0, 0);
        s[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, ba.w, s[jt], 0, 0, 0);
        d[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bg.w, d[jt], 0, 0, 0);
      }
    }
    // ---- softmax over j for query i = li (the forward's), keys >= R masked out of both tiles
    float m = -INFINITY;
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int j = 16 * jt + 4 * kg + t;
        if (j >= R) {
          s[jt][t] = -INFINITY;
          d[jt][t] = 0.f;
        }
        m = fmaxf(m, s[jt][t]);
      }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        s[jt][t] = __expf(s[jt][t] - m);
        sum += s[jt][t];
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.f / sum;
    // ---- D = rowsum(gP o P), then gS = P o (gP - D) in place of gP
    float dsum = 0.f;
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        s[jt][t] *= inv;
        dsum += d[jt][t] * s[jt][t];
      }
    dsum += __shfl_xor(dsum, 16, 64);
    dsum += __shfl_xor(dsum, 32, 64);
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
      for (int t = 0; t < 4; ++t) d[jt][t] = s[jt][t] * (d[jt][t] - dsum);
    // ---- P and gS tiles to scratch: this lane holds row i0 + li, columns 16 jt + 4 kg .. + 4
    if (pbuf != nullptr && i0 + li < R) {
      float* prow = pbuf + mat + (size_t)(i0 + li) * R;
      float* srow = gsbuf + mat + (size_t)(i0 + li) * R;
#pragma unroll
      for (int jt = 0; jt < JT; ++jt) {
        const int j = 16 * jt + 4 * kg;
        if (j >= R) continue;
        *reinterpret_cast<float4*>(prow + j) = make_float4(s[jt][0], s[jt][1], s[jt][2], s[jt][3]);
        *reinterpret_cast<float4*>(srow + j) = make_float4(d[jt][0], d[jt][1], d[jt][2], d[jt][3]);
      }
    }
    if (ga == nullptr) continue;
    // ---- GEMM2 (the forward's): tile [16 queries x 192 columns] = gS . Bm, three groups of four interleaved column tiles
    f32x4 o[3][4];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int c = 0; c < 4; ++c) o[g][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float p = d[jt][t];
        const float* krow = K + (16 * jt + 4 * kg + t) * CB_LD + 4 * li;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
          const float4 b = *reinterpret_cast<const float4*>(krow + 64 * g);
          o[g][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(p, b.x, o[g][0], 0, 0, 0);
          o[g][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(p, b.y, o[g][1], 0, 0, 0);
          o[g][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(p, b.z, o[g][2], 0, 0, 0);
          o[g][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(p, b.w, o[g][3], 0, 0, 0);
        }
      }
    // ---- epilogue: this lane holds the tile's [i0 + 4 kg + t][64 g + 4 li + c]
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int i = i0 + 4 * kg + t;
      if (i >= R) continue;
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        const int w = 64 * g + 4 * li;
        if (w >= R) continue;
        const float4 r = *reinterpret_cast<const float4*>(go + mat + (size_t)i * R + w);
        *reinterpret_cast<float4*>(ga + mat + (size_t)i * R + w) =
            make_float4(r.x + o[g][0][t], r.y + o[g][1][t], r.z + o[g][2][t], r.w + o[g][3][t]);
      }
    }
  }
}

// One wave per (map, 64 x 64 tile of gB); T = tiles per side; pointers: the GROUP's first map; maps: the group's.
__global__ __launch_bounds__(256) void channel_attention_bwd_cols_kernel(const float* __restrict__ qs,
                                                                         const float* __restrict__ go,
                                                                         const float* __restrict__ pbuf,
                                                                         const float* __restrict__ gsbuf, int R, int T,
                                                                         int maps, float* __restrict__ gb) {
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, kg = lane >> 4;
  const size_t id = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (id >= (size_t)maps * T * T) return;   // wave-uniform; no barrier in this kernel
  const size_t mat = id / (size_t)(T * T) * R * R;
  const int tile = (int)(id % (size_t)(T * T));
  const int j0 = 64 * (tile / T), w0 = 64 * (tile % T);
  const int jc = j0 + 4 * li, wc = w0 + 4 * li;   // this lane's 4 output rows (as A operand) / 4 output columns (as B)
  const bool jok = jc < R, wok = wc < R;          // R % 4 == 0: a float4 is inside or outside as a whole
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = zero;
  // k step = 4 rows i (R % 4 == 0: row i4 + kg always exists); next step's operands are fetched ahead of the MFMAs
  size_t row = mat + (size_t)kg * R;
  f32x4 p = jok ? *reinterpret_cast<const f32x4*>(pbuf + row + jc) : zero;
  f32x4 gs = jok ? *reinterpret_cast<const f32x4*>(gsbuf + row + jc) : zero;
  f32x4 g = wok ? *reinterpret_cast<const f32x4*>(go + row + wc) : zero;
  f32x4 a = wok ? *reinterpret_cast<const f32x4*>(qs + row + wc) : zero;
  for (int i4 = 0; i4 < R; i4 += 4) {
    f32x4 np = zero, ngs = zero, ng = zero, na = zero;
    if (i4 + 4 < R) {
      row += (size_t)4 * R;
      if (jok) {
        np = *reinterpret_cast<const f32x4*>(pbuf + row + jc);
        ngs = *reinterpret_cast<const f32x4*>(gsbuf + row + jc);
      }
      if (wok) {
        ng = *reinterpret_cast<const f32x4*>(go + row + wc);
        na = *reinterpret_cast<const f32x4*>(qs + row + wc);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[r], g[c], acc[r][c], 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(gs[r], a[c], acc[r][c], 0, 0, 0);
    p = np;
    gs = ngs;
    g = ng;
    a = na;
  }
  // this lane holds gB[j0 + 16 kg + 4 t + r][w0 + 4 li + c] in acc[r][c][t]
  if (!wok) return;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = j0 + 16 * kg + 4 * t + r;
      if (j >= R) continue;
      *reinterpret_cast<float4*>(gb + mat + (size_t)j * R + wc) =
          make_float4(acc[r][0][t], acc[r][1][t], acc[r][2][t], acc[r][3][t]);
    }
}

}  // namespace isf

extern "C" int isf_channel_attention_backward(const float* query_scene, const float* query_ins, const float* grad_out,
                                              int num_maps, int size, float* grad_query_scene, float* grad_query_ins,
                                              isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num_maps >= 0 && size > 0, ISF_ERR_ARG, "channel_attention_backward: bad sizes");
  if (num_maps == 0) return ISF_OK;
  if (!grad_query_scene && !grad_query_ins) return ISF_OK;
  ISF_REQUIRE(query_scene && query_ins && grad_out, ISF_ERR_ARG, "channel_attention_backward: null pointer");
  ISF_REQUIRE(size % 4 == 0 && size <= CB_ROWS, ISF_ERR_UNSUPPORTED,
              "channel_attention_backward: map size %d (need %%4 == 0 and <= %d)", size, CB_ROWS);
  hipStream_t st = as_stream(stream);
  const size_t lds = (size_t)CB_ROWS * CB_LD * sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {
    ISF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&channel_attention_bwd_rows_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set = true;
  }
  const size_t map_elems = (size_t)size * size;
  // scratch: P and gS of one group of maps; groups run in order, and a map's result does not depend on its group
  int group = std::min(num_maps, CB_GROUP);
  float* scratch = nullptr;
  if (grad_query_ins) {
    Arena& a = arena_for_stream(st);
    ISF_TRY(a.reset());
    for (;;) {
      const int rc = a.alloc_n(&scratch, 2 * (size_t)group * map_elems);
      if (rc == ISF_OK) break;
      if (rc != ISF_ERR_NOMEM || group == 1) return rc;
      group = (group + 1) / 2;   // the device cannot provide that much: smaller groups
    }
  }
  const int T = ceil_div(size, 64);
  for (int m0 = 0; m0 < num_maps; m0 += group) {
    const int maps = std::min(group, num_maps - m0);
    const size_t off = (size_t)m0 * map_elems;
    float* pbuf = scratch;
    float* gsbuf = scratch ? scratch + (size_t)group * map_elems : nullptr;
    hipLaunchKernelGGL(channel_attention_bwd_rows_kernel, dim3(maps), dim3(256), lds, st, query_scene + off,
                       query_ins + off, grad_out + off, size, grad_query_scene ? grad_query_scene + off : nullptr, pbuf,
                       gsbuf);
    if (grad_query_ins)
      hipLaunchKernelGGL(channel_attention_bwd_cols_kernel, dim3(ceil_div((long long)maps * T * T, 4)), dim3(256), 0, st,
                         query_scene + off, grad_out + off, pbuf, gsbuf, size, T, maps, grad_query_ins + off);
    ISF_LAUNCH_CHECK();
  }
  return ISF_OK;
}
