// isf_encoder.hip -- A7: dense BEV write-out, SparseEncoder.forward and the fused LiDAR branch.
#include "isf_common.h"
#include "isf_spconv_launch.h"   // the conv mode bits that stay inside the library, what a launch's `order` holds

#include <algorithm>

namespace isf {

// ----------------------------------------------------------------------------------------- dense BEV
// out[b, c*D + z, y, x] = feats[row(b,z,y,x), c] or 0.  Dense-stationary: a workgroup owns 64 consecutive
// x cells of one (b, y) line, looks the <= 64*D rows up in the occupancy index, transposes 64x64 blocks
// through LDS and writes 256-B runs; every output element is written exactly once.  ONE PASS (SKIP = false): this kernel
// writes the whole map, zeros included.  TWO PASSES (SKIP = true, the encoder's fp32 map of split rows): the H * W cells of
// a (b, z) plane are cut into SEGMENTS of kBevSeg = 32 cells that are 128-byte lines of the buffer (the cut is shifted by
// where the plane starts in memory: bev_plane_shift; a segment runs across row ends).  A segment without an occupied cell
// is all zeros in every channel of its z and is written by bev_zero_empty_kernel, which the encoder runs on its geometry
// stream beside the convolutions (the occupancy index of the last level exists long before its rows do); this kernel then
// writes the other segments only.  Both kernels decide with bev_segment_empty on the same index bits, so every element
// still has exactly one writer and the two need no order between them.  (Segments of 16 cells aligned to the rows -- 70 %
// of them empty on the benchmark geometry -- were measured first: the two kernels then share 128-byte lines, and the half
// lines cost each of them a whole one: second pass 42 us for 30 % of the bytes, convolutions beside the zero pass +31 us.)
static constexpr int kDenseX = 64;
static constexpr int kBevSeg = 32;           // cells per segment: one 128-byte line of a channel plane
static constexpr int kBevZeroBlocks = 256;   // grid of the zero pass: about one workgroup per CU, it must not crowd the convs

// where the segments of plane (b, z) are cut: the plane's first float (channel c = 0; plane0 = ((b * C) * D + z) * H * W)
// modulo a line.  The planes of the other channels follow at multiples of D * H * W floats: the same cut is line-aligned
// for them too when that is a multiple of 32 (any cut is correct).
__device__ __forceinline__ int bev_plane_shift(const float* out, size_t plane0) {
  return (int)(((reinterpret_cast<uintptr_t>(out) >> 2) + plane0) & (kBevSeg - 1));
}

// segment k of a plane = its cells [32 k - shift, 32 k - shift + 32) that exist (0 <= cell < HW): no occupied one among
// them?  (false for a segment without cells.)  plane_cell0: the plane's first cell in the index; the range may straddle
// two words of it.
__device__ __forceinline__ bool bev_segment_empty(const unsigned long long* __restrict__ bits,
                                                  unsigned long long plane_cell0, int HW, int shift, int k) {
  const int lo = kBevSeg * k - shift < 0 ? 0 : kBevSeg * k - shift;
  const int hi = kBevSeg * k - shift + kBevSeg > HW ? HW : kBevSeg * k - shift + kBevSeg;
  if (lo >= hi) return false;
  const unsigned long long cell0 = plane_cell0 + lo;
  const int len = hi - lo;   // <= 32
  const size_t w = (size_t)(cell0 >> 6);
  const int s = (int)(cell0 & 63);
  unsigned long long m = bits[w] >> s;
  if (s + len > 64) m |= bits[w + 1] << (64 - s);   // (then the range's last cell lies in word w + 1: in bounds)
  m &= (1ull << len) - 1;
  return m == 0;
}

// zero pass of the two-pass map: a workgroup takes (plane, group of 8 segments) units (grid-stride); a wave's lanes are the
// 8 x 8 float4 pieces of the group -- 1 KiB of one channel plane -- and the waves take the channels in turn
__global__ __launch_bounds__(256) void bev_zero_empty_kernel(int B, int C, int D, int HW,
                                                             const unsigned long long* __restrict__ bits,
                                                             float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int groups = ((HW + 2 * kBevSeg - 2) / kBevSeg + 7) / 8;   // covers the segments of any shift
  const long long units = (long long)B * D * groups;
  const bool vec_ok = ((size_t)D * HW) % 4 == 0;   // float4 pieces stay 16-byte aligned in every channel plane
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    const int g = (int)(u % groups);
    const long long bz = u / groups;   // b * D + z
    const int z = (int)(bz % D);
    const size_t plane0 = ((size_t)(bz / D) * C * D + z) * HW;
    const int shift = bev_plane_shift(out, plane0);
    const int k = g * 8 + (lane >> 3);
    const int p0 = kBevSeg * k - shift + 4 * (lane & 7);   // first cell of this lane's piece (pieces are 16-byte aligned)
    if (p0 + 4 <= 0 || p0 >= HW) continue;
    if (!bev_segment_empty(bits, (unsigned long long)bz * HW, HW, shift, k)) continue;
    const bool whole = vec_ok && p0 >= 0 && p0 + 4 <= HW;
    for (int c = wv; c < C; c += 4) {
      float* o = out + plane0 + (size_t)c * D * HW;   // plane (b, c, z)
      if (whole) {
        *reinterpret_cast<float4*>(o + p0) = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (p0 + e >= 0 && p0 + e < HW) o[p0 + e] = 0.f;
      }
    }
  }
}

// the zero pass of out = [B, C * D, H, W] for the index `occ` of (B, D, H, W)
static int bev_zero_empty_impl(const OccIndex& occ, int C, float* out, hipStream_t st) {
  hipLaunchKernelGGL(bev_zero_empty_kernel, dim3(kBevZeroBlocks), dim3(256), 0, st, occ.B, C, occ.D, occ.H * occ.W, occ.bits,
                     out);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

template <int FMT, bool SKIP = false>   // 0 fp32 rows, 1 split rows, 2 f16 rows; SKIP: the empty segments are not written here
__global__ __launch_bounds__(256) void dense_bev_kernel(const void* __restrict__ feats_v, int C, int D,
                                                        int H, int W,
                                                        const unsigned long long* __restrict__ bits,
                                                        const uint32_t* __restrict__ prefix,
                                                        const int32_t* __restrict__ perm,
                                                        float* __restrict__ out) {
  __shared__ float tile[64][kDenseX + 1];
  __shared__ int rows[kDenseX];
  __shared__ int keep[kDenseX + 1];   // SKIP: this x cell's segment is written here; [kDenseX]: any of them
  const int xt = blockIdx.x, y = blockIdx.y, b = blockIdx.z;
  const int x0 = xt * kDenseX;
  const int t = threadIdx.x;
  for (int z = 0; z < D; ++z) {
    __syncthreads();
    if (t < kDenseX) {   // (wave 0, all of it)
      int r = -1;
      bool kp = false;
      const int x = x0 + t;
      if (x < W) {
        r = occ_lookup(bits, prefix, (((unsigned long long)b * D + z) * H + y) * W + x);
        if (r >= 0 && perm) r = perm[r];
        if (SKIP) {
          const int shift = bev_plane_shift(out, ((size_t)b * C * D + z) * H * W);
          kp = !bev_segment_empty(bits, ((unsigned long long)b * D + z) * H * W, H * W, shift, (y * W + x + shift) / kBevSeg);
        }
      }
      rows[t] = r;
      if (SKIP) {
        keep[t] = kp;
        const unsigned long long any = __ballot(kp);
        if (t == 0) keep[kDenseX] = any != 0;
      }
    }
    __syncthreads();
    if (SKIP && !keep[kDenseX]) continue;   // nothing of this z to write here (the same for every thread: the barriers stay aligned)
    for (int c0 = 0; c0 < C; c0 += 64) {
      if (FMT != 0) {
        // split format: row = C/8 units of (hi8 | lo8) f16 (f16 rows: hi8 only); thread -> (row xx = t/8 + 32*j, unit t%8)
        const uint4* fs = reinterpret_cast<const uint4*>(feats_v);
        const int u = t & 7;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int xx = (t >> 3) + 32 * j;
          const int r = rows[xx];
          float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          if (r >= 0 && c0 + u * 8 < C) {
            const size_t o = FMT == 2 ? (size_t)r * (C >> 3) + (c0 >> 3) + u : split_hi_index((size_t)r, C >> 3, (c0 >> 3) + u);
            const uint4 hi = fs[o], lo = FMT == 2 ? make_uint4(0, 0, 0, 0) : fs[o + 4];
            const _Float16* h = reinterpret_cast<const _Float16*>(&hi);
            const _Float16* l = reinterpret_cast<const _Float16*>(&lo);
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = (float)h[q] + (float)l[q];
          }
#pragma unroll
          for (int q = 0; q < 8; ++q) tile[u * 8 + q][xx] = v[q];
        }
      } else {
        // load: thread -> (row xx = t/16 + 16*j, 4 channels c0 + 4*(t%16))
        const float* feats = reinterpret_cast<const float*>(feats_v);
        const int c4 = (t & 15) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int xx = (t >> 4) + 16 * j;
          const int r = rows[xx];
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (r >= 0 && c0 + c4 < C) v = *reinterpret_cast<const float4*>(feats + (size_t)r * C + c0 + c4);
          tile[c4 + 0][xx] = v.x;
          tile[c4 + 1][xx] = v.y;
          tile[c4 + 2][xx] = v.z;
          tile[c4 + 3][xx] = v.w;
        }
      }
      __syncthreads();
      // store: lane -> x, wave -> channel stripe
      const int lane = t & 63, wv = t >> 6;
      if (x0 + lane < W && !(SKIP && !keep[lane])) {
        for (int cc = wv; cc < 64 && c0 + cc < C; cc += 4) {
          const size_t ch = (size_t)(c0 + cc) * D + z;
          out[(((size_t)b * C * D + ch) * H + y) * W + x0 + lane] = tile[cc][lane];
        }
      }
      __syncthreads();
    }
  }
}

int sparse_to_dense_bev_impl(Arena& a, const void* feats, int fmt, const int32_t* indices, int n, int C,
                             int B, int D, int H, int W, float* out, const OccIndex* occ_in, hipStream_t st,
                             bool skip_empty /* split rows of an index: bev_zero_empty_impl writes the empty segments */) {
  ISF_REQUIRE(C % (fmt ? 32 : 4) == 0, ISF_ERR_UNSUPPORTED, "dense: channels %d not a multiple of %d", C,
              fmt ? 32 : 4);
  OccIndex occ;
  const int32_t* perm = nullptr;
  if (occ_in) {
    occ = *occ_in;  // rows already in rank order
  } else {
    ISF_TRY(occ_create(a, &occ, B, D, H, W, st));
    ISF_TRY(occ_mark_coords4(occ, indices, n, st));
    ISF_TRY(occ_scan(a, occ, st));
    int32_t* p = nullptr;
    ISF_TRY(build_perm(a, occ, indices, n, &p, st));
    perm = p;
  }
  dim3 grid(ceil_div(W, kDenseX), H, B);
  ISF_REQUIRE(!skip_empty || (fmt == 1 && occ_in && (long long)H * W < (1ll << 30)), ISF_ERR_ARG,
              "dense: two passes need split rows + index");
  const auto kernel = fmt == 1 ? (skip_empty ? dense_bev_kernel<1, true> : dense_bev_kernel<1>)
                                : (fmt == 2 ? dense_bev_kernel<2> : dense_bev_kernel<0>);
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, feats, C, D, H, W, occ.bits, occ.prefix, perm, out);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

// BEV map of the last level as SPLIT-FORMAT TOKEN MATRICES (isf_encoder_options.bev_format = 1): what the fusion encoder's
// 3 x 3 convolutions read (dense_conv.SplitMap) -- no fp32 [B, C*D, H, W] map, no NCHW -> split pass behind it.  Group g
// (256 channels) = matrix [B*H*W, 256] at out + g * B*H*W * 64 (uint4), token = (b*H + y)*W + x, channel = c*D + z
// (the reference's view(N, C*D, H, W), sparse_encoder.py:137-139).  Thread -> (token, 8-channel unit); every unit written.
__global__ __launch_bounds__(256) void bev_split_kernel(const uint4* __restrict__ fs, int C, int D, int H, int W,
                                                        const unsigned long long* __restrict__ bits,
                                                        const uint32_t* __restrict__ prefix, long long ntok,
                                                        uint4* __restrict__ out) {
  const int upt = C * D / 8;                                   // 8-channel units per token
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= ntok * upt) return;
  const long long tok = t / upt;
  const int j = (int)(t - tok * upt);
  const int hw = H * W;
  const int b = (int)(tok / hw), pos = (int)(tok - (long long)b * hw);
  const int y = pos / W, x = pos - y * W;
  _Float16 hi[8], lo[8];
  if (D == 2) {   // channels 8 j .. 8 j + 7 = (c, z) = (4 j, 0), (4 j, 1), (4 j + 1, 0), ...: four channels of two rows
    const int r0 = occ_lookup(bits, prefix, (((unsigned long long)b * 2 + 0) * H + y) * W + x);
    const int r1 = occ_lookup(bits, prefix, (((unsigned long long)b * 2 + 1) * H + y) * W + x);
    uint2 h0 = make_uint2(0, 0), l0 = h0, h1 = h0, l1 = h0;
    const int uc = j >> 1, e = j & 1;                          // the rows' 8-channel unit, its lower / upper four channels
    if (r0 >= 0) {
      const uint2* p = reinterpret_cast<const uint2*>(fs + split_hi_index((size_t)r0, C >> 3, uc));
      h0 = p[e];
      l0 = p[8 + e];                                           // lo piece: 4 uint4 = 8 uint2 further
    }
    if (r1 >= 0) {
      const uint2* p = reinterpret_cast<const uint2*>(fs + split_hi_index((size_t)r1, C >> 3, uc));
      h1 = p[e];
      l1 = p[8 + e];
    }
    const _Float16 *a0 = reinterpret_cast<const _Float16*>(&h0), *a1 = reinterpret_cast<const _Float16*>(&h1);
    const _Float16 *b0 = reinterpret_cast<const _Float16*>(&l0), *b1 = reinterpret_cast<const _Float16*>(&l1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      hi[2 * q] = a0[q]; hi[2 * q + 1] = a1[q];
      lo[2 * q] = b0[q]; lo[2 * q + 1] = b1[q];
    }
  } else {
    for (int q = 0; q < 8; ++q) {
      const int ch = 8 * j + q, c = ch / D, z = ch - c * D;
      const int r = occ_lookup(bits, prefix, (((unsigned long long)b * D + z) * H + y) * W + x);
      hi[q] = lo[q] = (_Float16)0.f;
      if (r >= 0) {
        const _Float16* p = reinterpret_cast<const _Float16*>(fs + split_hi_index((size_t)r, C >> 3, c >> 3));
        hi[q] = p[c & 7];
        lo[q] = p[32 + (c & 7)];                               // 4 uint4 = 32 halves further
      }
    }
  }
  const int g = j >> 5, ju = j & 31;                           // 256-channel group, unit inside it
  uint4* o = out + (size_t)g * ntok * 64 + split_hi_index((size_t)tok, 32, ju);
  o[0] = *reinterpret_cast<const uint4*>(hi);
  o[4] = *reinterpret_cast<const uint4*>(lo);
}

int sparse_to_bev_split_impl(const void* feats_split, int C, int B, int D, int H, int W, const OccIndex& occ, void* out,
                             hipStream_t st) {
  ISF_REQUIRE(C % 32 == 0 && (C * D) % 256 == 0, ISF_ERR_UNSUPPORTED,
              "bev (split token matrices): %d x %d channels are not whole 256-channel groups", C, D);
  const long long ntok = (long long)B * H * W, total = ntok * (C * D / 8);
  hipLaunchKernelGGL(bev_split_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, st, reinterpret_cast<const uint4*>(feats_split),
                     C, D, H, W, occ.bits, occ.prefix, ntok, reinterpret_cast<uint4*>(out));
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

__global__ void check_rank_order_kernel(const int32_t* __restrict__ coors4, int n, int B, int D, int H, int W,
                                        const unsigned long long* __restrict__ bits,
                                        const uint32_t* __restrict__ prefix, int* __restrict__ flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int4 c = reinterpret_cast<const int4*>(coors4)[i];
  int r = -1;
  if (c.x >= 0 && c.y >= 0 && c.z >= 0 && c.w >= 0 && c.x < B && c.y < D && c.z < H && c.w < W)
    r = occ_lookup(bits, prefix, (((unsigned long long)c.x * D + c.y) * H + c.z) * W + c.w);
  if (r != i) *flag = 1;
}

__global__ void gather_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ perm, int n, int C,
                                   float* __restrict__ xs) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)n * C) return;
  xs[t] = x[(size_t)perm[t / C] * C + (t % C)];
}

// ----------------------------------------------------------------------------------------- encoder
struct StageTables {
  uint16_t* slots = nullptr;
  int32_t* ulist = nullptr;
  int32_t* ucount = nullptr;
};

// ONE NEIGHBOUR TABLE and everything derived from it, all built behind it on the geometry stream.  The SubM convs of a
// level with one kernel size share LevelState::subm, a strided conv has a table of its own; NbrTable{} is the reset.
struct NbrTable {
  int32_t* nbr = nullptr;   // [K][stride]
  int stride = 0, rows = 0;
  int ks[3] = {0, 0, 0};
  const uint32_t* lmask = nullptr;   // non-null: nbr is LINE-COMPRESSED (lines [ks0 * ks1][stride]) with these tap masks
  StageTables stage;                 // staging tables (slots == nullptr: not built)
  const int32_t* order = nullptr;    // tile order / tile table / part table of an (order_cin -> order_cout) launch, or nullptr
  int order_cin = 0, order_cout = 0;
  int order_kind = kOrderPerm;       // kOrderPerm | kOrderTable | kOrderParts
  ConvCuPlan cu;                     // unit plan for the one-workgroup-per-CU kernel (n_out == 0: not built)
  const int32_t* rowmap = nullptr;   // ROW SORT (conv_row_sort_impl): position -> row, or nullptr
  const int32_t* nbr_sorted = nullptr;      // nbr by position
  const uint32_t* lmask_sorted = nullptr;   // lmask by position
  int sort_part_rows = 0;            // the launch plan's rows per part the sort was cut for
  int pair_slot = 0;                 // the table's pair total lives in pair_counts[pair_slot]
  int K() const { return ks[0] * ks[1] * ks[2]; }
};

struct LevelState {
  int shape[3] = {0, 0, 0};
  int n = 0;                        // active rows (host)
  const int32_t* coors = nullptr;   // [n,4] sorted
  OccIndex occ;
  bool has_occ = false;
  NbrTable subm;                    // the level's shared SubM table (nbr == nullptr: none yet)
};

static int ensure_occ(Arena& a, LevelState& L, int B, hipStream_t st) {
  if (L.has_occ) return ISF_OK;
  ISF_TRY(occ_create(a, &L.occ, B, L.shape[0], L.shape[1], L.shape[2], st));
  ISF_TRY(occ_mark_coords4(L.occ, L.coors, L.n, st));
  ISF_TRY(occ_scan(a, L.occ, st));
  L.has_occ = true;
  return ISF_OK;
}

// isf_encoder_options.diagnostic: what each bit selects, and what was measured with it, is recorded beside its ISF_ENC_DIAG_*
// name in include/isf_hip.h.  decode_encoder_options decodes it once per call.
static constexpr int kKnockoutBits = ISF_ENC_DIAG_NO_GATHER | ISF_ENC_DIAG_NO_WEIGHTS | ISF_ENC_DIAG_NO_LOOP | ISF_ENC_DIAG_NO_SHARING;
static constexpr int kDeepOptBits = ISF_CONV_MODE_STAGGER | ISF_CONV_MODE_R4_ISSUE | ISF_CONV_MODE_TWO_AHEAD | ISF_CONV_MODE_DEEP | kConvModeNarrowTiles;
static constexpr struct { int diag, mode; } kDiagToConvMode[] = {
    {ISF_ENC_DIAG_NO_GATHER, ISF_CONV_MODE_NO_GATHER},       {ISF_ENC_DIAG_NO_WEIGHTS, ISF_CONV_MODE_NO_WEIGHTS},
    {ISF_ENC_DIAG_NO_LOOP, ISF_CONV_MODE_NO_LOOP},           {ISF_ENC_DIAG_NO_SHARING, ISF_CONV_MODE_NO_SHARING},
    {ISF_ENC_DIAG_UNIFORM_TILES, ISF_CONV_MODE_UNIFORM_TILES}, {ISF_ENC_DIAG_CHUNK_SPLIT, ISF_CONV_MODE_CHUNK_SPLIT},
    {ISF_ENC_DIAG_ONE_BLOCK_4W, ISF_CONV_MODE_ONE_BLOCK_4W}, {ISF_ENC_DIAG_ONE_BLOCK_8W, ISF_CONV_MODE_ONE_BLOCK_8W},
    {ISF_ENC_DIAG_STAGGER, ISF_CONV_MODE_STAGGER},           {ISF_ENC_DIAG_R4_ISSUE, ISF_CONV_MODE_R4_ISSUE},
    {ISF_ENC_DIAG_TWO_AHEAD, ISF_CONV_MODE_TWO_AHEAD},       {ISF_ENC_DIAG_DEEP, ISF_CONV_MODE_DEEP},
    {ISF_ENC_DIAG_NARROW_TILES, kConvModeNarrowTiles}};
// every bit the engine entry points know: the table's, the encoder's own, isf_lidar_branch_forward's two
static constexpr int kEncDiagKnown =
    kKnockoutBits | ISF_ENC_DIAG_UNIFORM_TILES | ISF_ENC_DIAG_CHUNK_SPLIT | ISF_ENC_DIAG_ONE_BLOCK_4W | ISF_ENC_DIAG_ONE_BLOCK_8W |
    ISF_ENC_DIAG_STAGGER | ISF_ENC_DIAG_R4_ISSUE | ISF_ENC_DIAG_TWO_AHEAD | ISF_ENC_DIAG_DEEP | ISF_ENC_DIAG_NARROW_TILES |
    ISF_ENC_DIAG_LAUNCH_ORDER | ISF_ENC_DIAG_NARROW_GATHER | ISF_ENC_DIAG_CU_KERNEL | ISF_ENC_DIAG_CU_VARIANT_MASK |
    ISF_ENC_DIAG_DENSE_TABLES | ISF_ENC_DIAG_TILE_TABLES | ISF_ENC_DIAG_COUNTS_MEMCPY | ISF_ENC_DIAG_BAND_ORDER | ISF_ENC_DIAG_NO_ROW_SORT |
    ISF_ENC_DIAG_NARROW_ROW_SORT | ISF_ENC_DIAG_SORT_KEY_AB | ISF_ENC_DIAG_VFE_FP32_ROWS | ISF_ENC_DIAG_VOXELIZE_PER_FRAME |
    ISF_ENC_DIAG_BEV_ONE_PASS;
static constexpr int kSortMinRows = 4096;   // (configs[2] at B = 2: 7.05 ms sorted from 4 096 rows up, 7.10 from 32 768, 7.10 unsorted)

// f16x3 split MFMA when every layer was packed for it (and precision 1 does not override it), else fp32 MFMA
static bool encoder_use16(const isf_conv_layer* layers, int num_layers, int precision) {
  bool use16 = precision != 1;
  for (int i = 0; i < num_layers; ++i)
    use16 = use16 && layers[i].packed16 && sparse_conv_f16x3_supported(layers[i].c_in, layers[i].c_out);
  return use16;
}

// isf_encoder_options, decoded and validated once per call
struct EncoderKnobs {
  int precision = 0;
  int dg = 0;          // timing diagnostic of the conv kernels (they exist on the gather kernel only)
  int conv_mode = 0;   // what every layer's launch starts from: a knock-out or f16 storage, | uniform tiles
  int one_block = 0;   // for the 256-column layers
  int deep_opts = 0;   // for 128 columns and more
  bool chunk_split = false;
  bool tile_order = true, dma_gather = true, line_tables = true, mailbox = true, row_sort = true;   // defaults a bit switches off
  bool tile_tables = false, band_order = false, narrow_sort = false, cu_units = false;               // opt-ins
  int sort_key = 1;    // conv_row_sort_impl: 1 = six coarse bits (one radix pass), 2 = coarse | in-plane taps
  int cu_variant = 0, cu_cap = 16;   // isf_conv_cu_plan.variant and its unit shape
  int stage_opt = 0;   // stage_rows: LDS rows a layer of stage_mask stages (0 and -1: the gather kernels)
  unsigned stage_mask = 0;
  int bev_format = 0;
  bool use16 = false;          // encoder_use16
  bool f16io = false;          // f16 rows between the layers
  bool fp32_class = false;     // the split-precision kernels proper: the only ones the variants apply to
  bool bev_two_pass = false;   // the fp32 BEV map of split rows in two passes (dense_bev_kernel): zeros early, on the geometry stream
};

static int decode_encoder_options(const isf_encoder_options* opt, const isf_conv_layer* layers, int num_layers, bool fp32_map,
                                  EncoderKnobs* knobs) {
  EncoderKnobs k;
  const int diagnostic = opt ? opt->diagnostic : 0;
  k.precision = opt ? opt->precision : 0;
  k.dg = diagnostic & kKnockoutBits;
  ISF_REQUIRE(k.precision >= 0 && k.precision <= 2 && diagnostic >= 0 && (diagnostic & ~kEncDiagKnown) == 0 &&
                  (k.dg == 0 || conv_mode_is_knockout(k.dg) || k.dg == ISF_ENC_DIAG_NO_SHARING) && !(k.precision == 2 && k.dg != 0),
              ISF_ERR_ARG, "sparse_encoder: options (precision %d, diagnostic %d)", k.precision, diagnostic);
  int translated = 0;
  for (const auto& t : kDiagToConvMode)
    if (diagnostic & t.diag) translated |= t.mode;
  k.f16io = k.precision == 2;
  k.fp32_class = k.dg == 0 && !k.f16io;
  k.conv_mode = (k.f16io ? ISF_CONV_MODE_F16_STORAGE : k.dg) | (translated & ISF_CONV_MODE_UNIFORM_TILES);
  k.one_block = translated & (ISF_CONV_MODE_ONE_BLOCK_4W | ISF_CONV_MODE_ONE_BLOCK_8W);
  k.deep_opts = translated & kDeepOptBits;
  k.chunk_split = (translated & ISF_CONV_MODE_CHUNK_SPLIT) && k.fp32_class && k.one_block == 0 && k.deep_opts == 0;
  auto on = [&](int bit) { return (diagnostic & bit) != 0; };
  k.tile_order = !on(ISF_ENC_DIAG_LAUNCH_ORDER);
  k.dma_gather = !on(ISF_ENC_DIAG_NARROW_GATHER);
  k.line_tables = !on(ISF_ENC_DIAG_DENSE_TABLES);
  k.mailbox = !on(ISF_ENC_DIAG_COUNTS_MEMCPY);
  k.row_sort = !on(ISF_ENC_DIAG_NO_ROW_SORT);
  k.tile_tables = on(ISF_ENC_DIAG_TILE_TABLES);
  k.band_order = on(ISF_ENC_DIAG_BAND_ORDER);
  k.narrow_sort = on(ISF_ENC_DIAG_NARROW_ROW_SORT);
  k.cu_units = on(ISF_ENC_DIAG_CU_KERNEL);
  k.sort_key = on(ISF_ENC_DIAG_SORT_KEY_AB) ? 2 : 1;
  k.cu_variant = (diagnostic & ISF_ENC_DIAG_CU_VARIANT_MASK) >> ISF_ENC_DIAG_CU_VARIANT_SHIFT;
  k.cu_cap = conv_cu_variant_cap(k.cu_variant);
  k.stage_opt = opt ? opt->stage_rows : 0;
  k.stage_mask = opt ? (unsigned)opt->stage_mask : 0u;
  k.bev_format = opt ? opt->bev_format : 0;
  ISF_REQUIRE(k.stage_opt >= -1, ISF_ERR_ARG, "sparse_encoder: stage_rows %d", k.stage_opt);
  ISF_REQUIRE(num_layers > 0 && num_layers <= 32, ISF_ERR_ARG, "sparse_encoder: %d layers (1..32)", num_layers);
  k.use16 = encoder_use16(layers, num_layers, k.precision);
  k.bev_two_pass = !on(ISF_ENC_DIAG_BEV_ONE_PASS) && k.use16 && !k.f16io && k.bev_format == 0 && fp32_map;
  *knobs = k;
  return ISF_OK;
}

// what ONE LAYER runs on, decided on the host from the knobs, the layer list and the row count of the layer's table
struct LayerPlan {
  int K = 0, nx = 0;
  int srows = 0;            // LDS rows this layer stages (0 = a gather kernel)
  bool cu = false;          // 256-column layers: one workgroup per CU over units of equal work (isf_spconv_cu.hip)
  bool dma = false;         // narrow layers: LDS-DMA gathers (isf_spconv_dma.hip)
  int layer_mode = 0;       // the conv mode on the tile kernel, as the launch and everything planned for it see it
  bool parts_ok = false;    // equal-work parts when the launch runs in several rounds
  bool want_order = false;  // build_tile_order: a tile order / table, or a part table
  bool lines = false;       // a table this layer builds is line-compressed
  bool sort = false;        // ROW SORT (round 6): the rows are computed in the order of their tap masks
  int sort_key = 1;
  bool sort_full_key = false;   // a line-compressed table of the input level: all 27 mask bits decide
  int part_rows = 0;        // sort: rows per part of this layer's launch plan
};

static int plan_layer(const EncoderKnobs& kn, const isf_conv_layer* layers, int i, int num_layers, int rows, LayerPlan* plan) {
  const isf_conv_layer& ly = layers[i];
  const bool subm = ly.conv_type == ISF_CONV_SUBM;
  LayerPlan p;
  p.K = ly.ksize[0] * ly.ksize[1] * ly.ksize[2];
  p.nx = ly.ksize[2];
  // the timing diagnostics and ISF_CONV_MODE_NO_SHARING exist on the gather kernel only: no staging, no LDS-DMA
  if (kn.use16 && kn.fp32_class && kn.stage_opt > 0 && sparse_conv_f16x3_supported(ly.c_in, ly.c_out) &&
      (kn.stage_mask == 0 || ((kn.stage_mask >> i) & 1u)))
    p.srows = kn.stage_opt;
  p.cu = kn.use16 && kn.cu_units && p.srows == 0 && kn.conv_mode == 0 && sparse_conv_cu_supported(ly.c_in, ly.c_out);
  const bool plan_ok = kn.use16 && p.srows == 0 && !p.cu;   // the tile kernel or the LDS-DMA kernel
  p.layer_mode = kn.conv_mode | (kn.fp32_class && ly.c_out >= 128 ? kn.deep_opts : 0) |
                 (kn.chunk_split && plan_ok && ly.c_out == 256 && ly.c_in >= 128 ? ISF_CONV_MODE_CHUNK_SPLIT : 0);
  p.dma = kn.use16 && kn.dma_gather && p.srows == 0 && kn.dg == 0 && sparse_conv_dma_supported(ly.c_in, ly.c_out);
  // the uniform-tiles diagnostic keeps the equal-row parts (with the launch-order diagnostic: no table at all), and so do
  // the opt-ins whose tables are cut for them (narrow row sort, band order)
  p.parts_ok = plan_ok && kn.dg == 0 && !((kn.conv_mode & ISF_CONV_MODE_UNIFORM_TILES) && !kn.tile_order) && !kn.band_order &&
               !(p.dma && kn.narrow_sort) && (p.dma || (p.layer_mode & (ISF_CONV_MODE_DEEP | ISF_CONV_MODE_CHUNK_SPLIT)) == 0);
  p.want_order = (plan_ok && kn.tile_order) || p.parts_ok;
  // a table may be line-compressed when every layer that reads it runs the LDS-DMA kernel: for a SubM table, all the SubM
  // layers of this level with the same kernel (up to the next strided conv); for a strided conv, itself
  p.lines = p.dma && kn.line_tables && kn.stage_opt <= 0 && (p.nx == 1 || p.nx == 3) && ly.ksize[0] * ly.ksize[1] <= 9;
  for (int j = i; p.lines && subm && j < num_layers && layers[j].conv_type == ISF_CONV_SUBM; ++j) {
    const isf_conv_layer& q = layers[j];
    if (q.ksize[0] == ly.ksize[0] && q.ksize[1] == ly.ksize[1] && q.ksize[2] == ly.ksize[2] &&
        !sparse_conv_dma_supported(q.c_in, q.c_out))
      p.lines = false;
  }
  // row sort: deep layers on the tile kernel; SubM layers on the LDS-DMA kernel (full or line-compressed table) as an opt-in.
  // (The f16-storage mode too: the sort only renames positions; its epilogue reads / writes through the row map.)  A strided
  // conv sorts its own table (its rows want 10 of 27 taps, in many patterns: -12 % tile-taps, -26 % MFMA blocks at level 3
  // on the benchmark geometry, profiles/r06_row_sort.txt) with the one-pass key.
  const bool sort_mode_ok = kn.dg == 0 && kn.one_block == 0 && (kn.deep_opts & ~kConvModeNarrowTiles) == 0;
  const bool sortable = kn.row_sort && plan_ok && p.K == 27 && sort_mode_ok && rows >= kSortMinRows;
  p.sort = sortable && (subm ? (p.dma ? kn.narrow_sort : ly.c_out >= 128) : (!p.dma && ly.c_out >= 128));
  p.sort_key = subm ? kn.sort_key : 1;
  p.sort_full_key = true;   // the input level's rows have few, varied neighbours (6 of 27 on the benchmark geometry)
  for (int j = 0; j < i; ++j) p.sort_full_key = p.sort_full_key && layers[j].conv_type == ISF_CONV_SUBM;
  if (p.sort) {
    Conv16LaunchInfo info;
    ISF_TRY(conv16_launch_info(p.dma ? kConvKernelDma : kConvKernelTile, ly.c_in, ly.c_out, rows, p.dma ? kn.conv_mode : p.layer_mode,
                               &info));
    p.part_rows = info.part_rows;
  }
  *plan = p;
  return ISF_OK;
}

// a level sorted for one launch plan serves only the layers whose plan is cut the same way; the others keep the plain table
static bool sort_applies(const NbrTable& t, const LayerPlan& p) {
  return p.sort && t.rowmap && p.part_rows == t.sort_part_rows;
}

// staging tables of a neighbour table (isf_spconv_stage.hip)
static int build_stage_tables(Arena& a, NbrTable& t, hipStream_t sg) {
  const int units = t.stride / isf_stage_unit_rows();
  ISF_TRY(a.alloc_n(&t.stage.slots, (size_t)t.K() * t.stride));
  ISF_TRY(a.alloc_n(&t.stage.ulist, (size_t)units * isf_stage_unit_cap()));
  ISF_TRY(a.alloc_n(&t.stage.ucount, (size_t)units));
  return stage_tables_impl(t.nbr, t.stride, t.K(), t.stage.slots, t.stage.ulist, t.stage.ucount, sg);
}

// row sort of a neighbour table for the launch plan of `p`; the plain table stays
static int build_row_sort(Arena& a, NbrTable& t, const LayerPlan& p, hipStream_t sg) {
  int32_t *rm = nullptr, *ns = nullptr;
  ISF_TRY(a.alloc_n(&rm, (size_t)t.stride));
  if (t.lmask) {
    const int nl = t.ks[0] * t.ks[1];
    uint32_t* lms = nullptr;
    ISF_TRY(a.alloc_n(&ns, (size_t)nl * t.stride));
    ISF_TRY(a.alloc_n(&lms, (size_t)t.stride));
    ISF_TRY(conv_row_sort_lines_impl(a, t.nbr, t.lmask, t.stride, nl, t.rows, p.part_rows, p.sort_full_key, rm, ns, lms, sg));
    t.lmask_sorted = lms;
  } else {
    ISF_TRY(a.alloc_n(&ns, (size_t)t.K() * t.stride));
    ISF_TRY(conv_row_sort_impl(a, t.nbr, t.stride, t.K(), t.rows, p.part_rows, rm, ns, sg, p.sort_key));
  }
  t.rowmap = rm;
  t.nbr_sorted = ns;
  t.sort_part_rows = p.part_rows;
  return ISF_OK;
}

// tile order / tile table of layer `ly`'s launch over a neighbour table (the sorted one when the sort applies).  A launch
// of the tile kernel that is resident in one round gets a TILE TABLE (conv16_table_part: the groups dealt to the compute
// units by equal work; kOrderTable, run the conv with mode | kConvModeTileTable); the LDS-DMA kernel's launches keep the
// permutation of uniform tiles (conv16_tile_order_impl).  A launch of SEVERAL ROUNDS (uniform tiles) gets a PART TABLE
// (conv16_part_table_impl: equal-work XCD parts, heavy tiles first -- in tile order without kn.tile_order; kOrderParts, run
// the conv with mode | kConvModePartTable) when p.parts_ok.  t.order stays nullptr when none applies.
static int build_tile_order(Arena& a, NbrTable& t, const LayerPlan& p, const EncoderKnobs& kn, const isf_conv_layer& ly,
                            const LevelState& out /* the level of the table's rows */, hipStream_t sg) {
  const bool sorted = sort_applies(t, p);
  const int32_t* nbr = sorted ? t.nbr_sorted : t.nbr;
  const uint32_t* lmask = sorted && t.lmask ? t.lmask_sorted : t.lmask;
  const int K = t.K(), stride = t.stride, n_out = t.rows, mode = p.layer_mode;
  t.order = nullptr;
  t.order_kind = kOrderPerm;
  t.order_cin = ly.c_in;
  t.order_cout = ly.c_out;
  const ConvKernel kernel = p.dma ? kConvKernelDma : kConvKernelTile;
  Conv16LaunchInfo info;
  if (p.parts_ok && n_out > 0) {   // the launch's uniform plan: several rounds?
    ISF_TRY(conv16_launch_info(kernel, ly.c_in, ly.c_out, n_out, mode | ISF_CONV_MODE_UNIFORM_TILES, &info));
    if (conv16_parts_apply(info)) {
      const int parts = conv16_order_parts(info), T = conv16_parts_tiles(info.full, parts);
      int32_t *work = nullptr, *table = nullptr;
      ISF_TRY(a.alloc_n(&work, (size_t)2 * T));
      ISF_TRY(a.alloc_n(&table, (size_t)conv16_part_table_ints(parts, conv16_parts_cap(T, parts))));
      ISF_TRY(conv16_part_table_impl(nbr, lmask, stride, K, n_out, ly.c_in, ly.c_out, info, !kn.tile_order, work, table, sg,
                                     (mode & ISF_CONV_MODE_UNIFORM_TILES) != 0));
      t.order = table;
      t.order_kind = kOrderParts;
      return ISF_OK;
    }
  }
  if (!kn.tile_order) return ISF_OK;
  ISF_TRY(conv16_launch_info(kernel, ly.c_in, ly.c_out, n_out, mode, &info));
  if (!p.dma && kn.tile_tables && !lmask && conv16_table_applies(info) && n_out >= 16 * info.cus_per_xcd) {
    const int ng = ceil_div(n_out, 16);
    int32_t *masks = nullptr, *work = nullptr, *table = nullptr;
    ISF_TRY(a.alloc_n(&masks, (size_t)ng));
    ISF_TRY(a.alloc_n(&work, (size_t)ng));
    ISF_TRY(a.alloc_n(&table, (size_t)conv16_table_ints(info)));
    ISF_TRY(conv_group_masks_impl(nbr, stride, K, n_out, masks, work, sg));
    ISF_TRY(conv16_tile_table_impl(work, n_out, info, table, sg));
    t.order = table;
    t.order_kind = kOrderTable;
    return ISF_OK;
  }
  if (!conv16_order_applies(info)) {
    // a launch of several rounds: its tiles band by band in y (conv16_band_order_kernel), so that the rows the dz = +-1
    // taps gather are still in the XCD's L2
    if (kn.band_order && conv16_band_order_applies(info)) {
      int32_t* ord = nullptr;
      ISF_TRY(a.alloc_n(&ord, (size_t)conv16_order_parts(info) * conv16_order_tiles(info)));
      ISF_TRY(conv16_band_order_impl(out.coors, n_out, info, std::max(8, out.shape[1] / 45), ord, sg));
      t.order = ord;
    }
    return ISF_OK;
  }
  const size_t n = (size_t)conv16_order_parts(info) * conv16_order_tiles(info);
  int32_t *work = nullptr, *ord = nullptr;
  ISF_TRY(a.alloc_n(&work, n));
  ISF_TRY(a.alloc_n(&ord, n));
  ISF_TRY(conv16_tile_order_impl(nbr, stride, K, n_out, info, work, ord, sg, lmask));
  t.order = ord;
  return ISF_OK;
}

// unit plan of a neighbour table (isf_spconv_cu.hip)
static int build_cu_plan(Arena& a, NbrTable& t, int cap, hipStream_t sg) {
  int32_t* buf = nullptr;
  ISF_TRY(a.alloc_n(&buf, conv_cu_plan_ints(t.rows)));
  return conv_cu_plan_impl(t.nbr, t.stride, t.K(), t.rows, buf, &t.cu, sg, cap);
}

// the neighbour table of layer `ly`: rows of level `out` (SubM: out is in), neighbours in level `in`, whose index exists
static int build_nbr_table(Arena& a, const LevelState& in, const LevelState& out, const isf_conv_layer& ly, bool lines,
                           int pair_slot, unsigned long long* pair_count, hipStream_t sg, NbrTable* t) {
  const bool subm = ly.conv_type == ISF_CONV_SUBM;
  *t = NbrTable{};
  t->stride = isf_nbr_stride(out.n);
  t->rows = out.n;
  for (int j = 0; j < 3; ++j) t->ks[j] = ly.ksize[j];
  t->pair_slot = pair_slot;   // resolved after the final sync
  if (lines) {
    uint32_t* lm = nullptr;
    ISF_TRY(a.alloc_n(&t->nbr, (size_t)ly.ksize[0] * ly.ksize[1] * t->stride));
    ISF_TRY(a.alloc_n(&lm, (size_t)t->stride));
    ISF_TRY(launch_nbr_lines(a, out.coors, out.n, in.shape, ly.ksize, ly.stride, ly.padding, subm, in.occ, t->nbr, lm, t->stride,
                             pair_count, sg));
    t->lmask = lm;
  } else {
    ISF_TRY(a.alloc_n(&t->nbr, (size_t)t->K() * t->stride));
    ISF_TRY(launch_nbr(a, out.coors, out.n, in.shape, ly.ksize, ly.stride, ly.padding, subm, in.occ, nullptr, t->nbr, t->stride,
                       pair_count, sg));
  }
  return ISF_OK;
}

// Build what the launch of `p` needs behind the table and does not have yet, on the geometry stream: staging tables, row
// sort, tile order / table / part table (again when the launch shape changes), unit plan.  Everything is built on first
// need: a later layer of the level may be the first to stage, to sort or to run the unit kernel.  *enqueued: anything?
static int prepare_table(Arena& a, NbrTable& t, const LayerPlan& p, const EncoderKnobs& kn, const isf_conv_layer& ly,
                         const LevelState& out, hipStream_t sg, bool* enqueued) {
  *enqueued = false;
  if (p.srows > 0 && !t.stage.slots) {
    ISF_TRY(build_stage_tables(a, t, sg));
    *enqueued = true;
  }
  if (p.sort && !t.rowmap) {   // (sorted for another plan already: this layer keeps the plain table)
    ISF_TRY(build_row_sort(a, t, p, sg));
    *enqueued = true;
  }
  if (p.want_order && (t.order_cin != ly.c_in || t.order_cout != ly.c_out)) {
    ISF_TRY(build_tile_order(a, t, p, kn, ly, out, sg));
    *enqueued = true;
  }
  if (p.cu && t.cu.n_out == 0 && t.rows > 0) {
    ISF_TRY(build_cu_plan(a, t, kn.cu_cap, sg));
    *enqueued = true;
  }
  return ISF_OK;
}

// the output level of the strided conv `ly` over level L: its index, its row count (a host wait) and its coordinates
static int open_next_level(Arena& a, LevelState& L, const isf_conv_layer& ly, int i, int B, bool mailbox, hipStream_t sg,
                           LevelState* next) {
  LevelState Nx;
  ISF_TRY(ensure_occ(a, L, B, sg));
  ISF_TRY(isf_conv_out_shape(L.shape, ly.ksize, ly.stride, ly.padding, Nx.shape));
  ISF_REQUIRE(Nx.shape[0] > 0 && Nx.shape[1] > 0 && Nx.shape[2] > 0, ISF_ERR_ARG, "sparse_encoder: layer %d output shape empty", i);
  ISF_TRY(occ_create(a, &Nx.occ, B, Nx.shape[0], Nx.shape[1], Nx.shape[2], sg));
  ISF_TRY(launch_mark_out(L.coors, L.n, L.shape, ly.ksize, ly.stride, ly.padding, Nx.occ, sg));
  ISF_TRY(occ_scan(a, Nx.occ, sg));
  if (mailbox) {                               // host wait without a copy command (post_int / wait_int)
    unsigned ticket = 0;
    ISF_TRY(post_int(a, Nx.occ.total, sg, &ticket));
    ISF_TRY(wait_int(a, ticket, sg, &Nx.n));
  } else {
    ISF_TRY(read_int(Nx.occ.total, &Nx.n, sg));  // host sync: sizes the next level's buffers / grids
  }
  Nx.has_occ = true;
  int32_t* nc = nullptr;
  ISF_TRY(a.alloc_n(&nc, (size_t)std::max(Nx.n, 1) * 4));
  if (Nx.n > 0) ISF_TRY(occ_compact_coords4(Nx.occ, nc, sg));
  Nx.coors = nc;
  *next = Nx;
  return ISF_OK;
}

// layer i's convolution y = conv(x) on the kernel its plan names, over the table and what prepare_table built for it
static int run_layer_conv(const EncoderKnobs& kn, const LayerPlan& p, const isf_conv_layer& ly, int i, const NbrTable& t,
                          const void* x, int n_in, const void* res, void* y, hipStream_t st) {
  const bool sorted = sort_applies(t, p);   // positions instead of rows: the sorted table + the row map
  const uint32_t* lmask = sorted && t.lmask ? t.lmask_sorted : t.lmask;
  ISF_REQUIRE(!lmask || p.dma, ISF_ERR_UNSUPPORTED, "sparse_encoder: layer %d cannot read a line-compressed table", i);
  const int32_t* nbr = sorted ? t.nbr_sorted : t.nbr;
  const int n_out = t.rows;
  ConvCall call = conv_call(x, ly.c_in, ly.packed16, p.K, ly.c_out, nbr, t.stride, n_out, ly.scale, ly.shift, res, ly.relu, y,
                            kn.conv_mode, st);
  if (p.srows > 0) return sparse_conv_forward_staged_impl(call, t.stage.slots, t.stage.ulist, t.stage.ucount, p.srows);
  if (p.cu && n_out > 0) {
    ConvCuPlan units = t.cu;
    units.variant = kn.cu_variant;
    return sparse_conv_forward_cu_impl(call, units);
  }
  if (kn.use16) {   // the LDS-DMA kernel or the tile kernel, on the order / table and the row sort built for this launch
    const int order_bit = order_mode_bit(p.want_order ? t.order_kind : kOrderPerm);
    call.order = p.want_order ? t.order : nullptr;
    call.rowmap = sorted ? t.rowmap : nullptr;
    if (p.dma) {
      call.mode = kn.conv_mode | order_bit;
      call.lmask = lmask;
      call.nx = p.nx;
      return sparse_conv_forward_dma_impl(call);
    }
    call.mode = p.layer_mode | order_bit | (ly.c_out == 256 && kn.fp32_class ? kn.one_block : 0);
    return sparse_conv_forward_f16x3_impl(call);
  }
  const float *xf = reinterpret_cast<const float*>(x), *rf = reinterpret_cast<const float*>(res);
  float* yf = reinterpret_cast<float*>(y);
  if (sparse_conv_mfma_supported(ly.c_in, ly.c_out))
    return sparse_conv_forward_packed_impl(xf, n_in, ly.c_in, ly.packed, p.K, ly.c_out, nbr, t.stride, n_out, ly.scale, ly.shift, rf,
                                           ly.relu, yf, st);
  return sparse_conv_forward_generic_impl(xf, ly.c_in, ly.packed, p.K, ly.c_out, nbr, t.stride, n_out, ly.scale, ly.shift, rf,
                                          ly.relu, yf, st);
}

int sparse_encoder_forward_impl(Arena& a, const float* x0, const int32_t* coors0, int n0, int B,
                                const int shape0[3], const OccIndex* occ0, const isf_conv_layer* layers,
                                int num_layers, float* spatial_features, int out_shape[4],
                                isf_encoder_stats* stats, int time_layers, const isf_encoder_options* opt,
                                hipStream_t st, hipEvent_t geometry_ready = nullptr,
                                const void* x0_split = nullptr /* x0 already in the split format (DynamicVFE wrote it) */) {
  EncoderKnobs kn;
  ISF_TRY(decode_encoder_options(opt, layers, num_layers, spatial_features != nullptr, &kn));
  // Geometry (occupancy indexes, output sets, neighbour tables: small integer kernels + the host syncs that size
  // the next level) runs on a side stream and overlaps the convolutions of the previous level on `st`; a
  // convolution waits for the event recorded behind what prepare_table built for it.  `sg` first waits for everything
  // the caller enqueued on `st` -- or only for `geometry_ready`, the point where the VFE's coordinates are final.
  hipStream_t sg = nullptr;
  ISF_TRY(side_stream(a, &sg));
  if (geometry_ready) ISF_HIP_TRY(hipStreamWaitEvent(sg, geometry_ready, 0));   // coords final: overlap the VFE tail too
  else ISF_TRY(stream_wait_stream(a, sg, st));
  LevelState L;
  for (int j = 0; j < 3; ++j) L.shape[j] = shape0[j];
  L.n = n0;
  L.coors = coors0;
  if (occ0) { L.occ = *occ0; L.has_occ = true; }
  bool bev_zeroed = false;
  const void* outputs[32];
  int out_rows[32];
  const void* x = x0;
  ISF_REQUIRE(!x0_split || (kn.use16 && !kn.f16io), ISF_ERR_ARG, "sparse_encoder: split input without the split kernels");
  if (x0_split) {
    x = x0_split;
  } else if (kn.use16) {  // inter-layer activations live in the split (hi8|lo8 f16) format: same bytes as fp32
    void* xs0 = nullptr;
    ISF_TRY(a.alloc(&xs0, (size_t)std::max(n0, 1) * layers[0].c_in * 4));
    if (kn.f16io) ISF_TRY(f32_to_half_impl(x0, (size_t)n0 * layers[0].c_in, xs0, st));
    else ISF_TRY(f32_to_split_impl(x0, (size_t)n0 * layers[0].c_in, xs0, st));
    x = xs0;
  }
  const void* x_in0 = x;
  unsigned long long* pair_counts = nullptr;   // per-rulebook pair totals: statistics only (8 + 1 launches a caller without
  if (stats) {                                   // `stats` does not pay for)
    ISF_TRY(a.alloc_n(&pair_counts, 32));
    ISF_HIP_TRY(hipMemsetAsync(pair_counts, 0, 32 * sizeof(unsigned long long), sg));
  }
  std::vector<hipEvent_t> ev;
  if (time_layers && stats) {
    ev.resize((size_t)num_layers * 2);
    for (auto& e : ev) ISF_HIP_TRY(hipEventCreate(&e));
  }
  int c_last = layers[0].c_in;
  for (int i = 0; i < num_layers; ++i) {
    const isf_conv_layer& ly = layers[i];
    const int K = ly.ksize[0] * ly.ksize[1] * ly.ksize[2];
    ISF_REQUIRE(K >= 1 && K <= 27, ISF_ERR_UNSUPPORTED, "sparse_encoder: layer %d has %d taps", i, K);
    ISF_REQUIRE(ly.c_in == c_last, ISF_ERR_ARG, "sparse_encoder: layer %d expects %d channels, got %d", i, ly.c_in, c_last);
    const int n_in = L.n;
    unsigned long long* pair_count = stats ? pair_counts + i : nullptr;
    // plan the layer and get its table: the level's shared SubM table (built on a miss), or a strided conv's own
    LayerPlan p;
    NbrTable own;
    NbrTable* t = &L.subm;
    bool fresh = true;
    if (ly.conv_type == ISF_CONV_SUBM) {
      ISF_TRY(plan_layer(kn, layers, i, num_layers, L.n, &p));
      fresh = !(t->nbr && t->ks[0] == ly.ksize[0] && t->ks[1] == ly.ksize[1] && t->ks[2] == ly.ksize[2]);
      if (fresh) {
        ISF_TRY(ensure_occ(a, L, B, sg));
        ISF_TRY(build_nbr_table(a, L, L, ly, p.lines, i, pair_count, sg, t));
      }
    } else {
      LevelState Nx;
      ISF_TRY(open_next_level(a, L, ly, i, B, kn.mailbox, sg, &Nx));
      ISF_TRY(plan_layer(kn, layers, i, num_layers, Nx.n, &p));
      t = &own;
      ISF_TRY(build_nbr_table(a, L, Nx, ly, p.lines, i, pair_count, sg, t));
      L = Nx;
    }
    bool enqueued = false;
    ISF_TRY(prepare_table(a, *t, p, kn, ly, L, sg, &enqueued));
    if (fresh || enqueued) ISF_TRY(stream_wait_stream(a, st, sg));   // the convolution waits for its table
    if (stats) stats->pairs[i] = -(long long)t->pair_slot - 1;   // pairs live in pair_counts[pair_slot]
    const int n_out = t->rows;
    if (kn.bev_two_pass && i == num_layers - 1 && (long long)L.shape[1] * L.shape[2] < (1ll << 30)) {
      // L is the output level and the last convolution no longer waits for `sg`: the zero segments of the map are written
      // beside the convolutions still queued on `st` (a strided last layer has built the index above; the buffer is free:
      // `sg` started behind everything the caller had queued on `st`); the join before dense_bev_kernel covers this launch
      ISF_TRY(ensure_occ(a, L, B, sg));
      ISF_TRY(bev_zero_empty_impl(L.occ, ly.c_out, spatial_features, sg));
      bev_zeroed = true;
    }
    void* y = nullptr;
    ISF_TRY(a.alloc(&y, (size_t)std::max(n_out, 1) * ly.c_out * 4));
    const void* res = nullptr;
    if (ly.residual_from == -1) res = x_in0;
    else if (ly.residual_from >= 0) {
      ISF_REQUIRE(ly.residual_from < i && out_rows[ly.residual_from] == n_out, ISF_ERR_ARG,
                  "sparse_encoder: layer %d residual source %d incompatible", i, ly.residual_from);
      res = outputs[ly.residual_from];
    }
    if (!ev.empty()) ISF_HIP_TRY(hipEventRecord(ev[2 * i], st));
    ISF_TRY(run_layer_conv(kn, p, ly, i, *t, x, n_in, res, y, st));
    if (!ev.empty()) ISF_HIP_TRY(hipEventRecord(ev[2 * i + 1], st));
    outputs[i] = y;
    out_rows[i] = n_out;
    if (stats) { stats->num_in[i] = n_in; stats->num_out[i] = n_out; stats->ms[i] = 0.f; }
    x = y;
    c_last = ly.c_out;
  }
  // dense BEV of the last level
  ISF_TRY(ensure_occ(a, L, B, sg));
  ISF_TRY(stream_wait_stream(a, st, sg));
  if (kn.bev_format == 1) {   // split-format token matrices (same byte count as the fp32 map)
    ISF_REQUIRE(kn.use16 && !kn.f16io, ISF_ERR_UNSUPPORTED, "sparse_encoder: bev_format 1 needs the split-precision path");
    ISF_TRY(sparse_to_bev_split_impl(x, c_last, B, L.shape[0], L.shape[1], L.shape[2], L.occ, spatial_features, st));
  } else {
    ISF_REQUIRE(kn.bev_format == 0, ISF_ERR_ARG, "sparse_encoder: bev_format %d (0 fp32 map, 1 split token matrices)",
                kn.bev_format);
    ISF_TRY(sparse_to_dense_bev_impl(a, x, kn.use16 ? (kn.f16io ? 2 : 1) : 0, L.coors, L.n, c_last, B, L.shape[0], L.shape[1],
                                     L.shape[2], spatial_features, &L.occ, st, bev_zeroed));
  }
  if (stats) stats->precision = kn.use16 ? 1 : 0;
  if (out_shape) { out_shape[0] = c_last * L.shape[0]; out_shape[1] = L.shape[1]; out_shape[2] = L.shape[2]; out_shape[3] = L.n; }
  if (stats) {
    unsigned long long h_pairs[32];
    ISF_HIP_TRY(hipMemcpyAsync(h_pairs, pair_counts, sizeof(h_pairs), hipMemcpyDeviceToHost, st));
    ISF_HIP_TRY(hipStreamSynchronize(st));
    stats->num_layers = num_layers;
    for (int i = 0; i < num_layers; ++i)
      if (stats->pairs[i] < 0) stats->pairs[i] = (long long)h_pairs[-(stats->pairs[i] + 1)];
    for (int i = 0; i < num_layers && !ev.empty(); ++i)
      ISF_HIP_TRY(hipEventElapsedTime(&stats->ms[i], ev[2 * i], ev[2 * i + 1]));
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  return ISF_OK;
}

}  // namespace isf

extern "C" {

int isf_sparse_to_dense_bev(const float* features, const int32_t* indices, int num_rows, int channels,
                            int batch_size, int D, int H, int W, float* out, isf_stream_t stream) {
  ISF_REQUIRE(num_rows >= 0 && channels > 0 && batch_size > 0 && D > 0 && H > 0 && W > 0 && out, ISF_ERR_ARG,
              "sparse_to_dense_bev: bad arguments");
  ISF_REQUIRE(num_rows == 0 || (features && indices), ISF_ERR_ARG, "sparse_to_dense_bev: null pointer");
  isf::Arena& a = isf::arena_for_stream(isf::as_stream(stream));
  ISF_TRY(a.reset());
  return isf::sparse_to_dense_bev_impl(a, features, 0, indices, num_rows, channels, batch_size, D, H, W, out,
                                       nullptr, isf::as_stream(stream));
}

int isf_sparse_encoder_forward(const float* voxel_features, const int32_t* coors, int num_voxels,
                               int batch_size, const int sparse_shape_host[3],
                               const isf_conv_layer* layers_host, int num_layers, float* spatial_features,
                               int out_shape_host[4], isf_encoder_stats* stats_host, int time_layers,
                               const isf_encoder_options* options, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num_voxels > 0 && batch_size > 0 && sparse_shape_host && layers_host && spatial_features &&
                  voxel_features && coors && num_layers > 0,
              ISF_ERR_ARG, "sparse_encoder_forward: bad arguments");
  hipStream_t st = as_stream(stream);
  Arena& a = arena_for_stream(as_stream(stream));
  ISF_TRY(a.reset());
  // The kernels want rows in rank ((b,z,y,x)-sorted) order, which is what DynamicVFE emits.  Verify it on
  // the device; arbitrary / duplicated input rows (e.g. the reference's shape test feeds random coords)
  // are re-ranked once: x_sorted[rank(coord_i)] = x[i] (a duplicate coordinate keeps one of its rows).
  OccIndex occ0;
  ISF_TRY(occ_create(a, &occ0, batch_size, sparse_shape_host[0], sparse_shape_host[1], sparse_shape_host[2], st));
  ISF_TRY(occ_mark_coords4(occ0, coors, num_voxels, st));
  ISF_TRY(occ_scan(a, occ0, st));
  int* flag = nullptr;
  ISF_TRY(a.alloc_n(&flag, 64));
  ISF_HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), st));
  hipLaunchKernelGGL(check_rank_order_kernel, dim3(ceil_div(num_voxels, 256)), dim3(256), 0, st, coors,
                     num_voxels, occ0.B, occ0.D, occ0.H, occ0.W, occ0.bits, occ0.prefix, flag);
  ISF_LAUNCH_CHECK();
  int h[2] = {0, 0};
  ISF_HIP_TRY(hipMemcpyAsync(&h[0], flag, sizeof(int), hipMemcpyDeviceToHost, st));
  ISF_HIP_TRY(hipMemcpyAsync(&h[1], occ0.total, sizeof(int), hipMemcpyDeviceToHost, st));
  ISF_HIP_TRY(hipStreamSynchronize(st));
  const float* x = voxel_features;
  const int32_t* c = coors;
  int n = num_voxels;
  if (h[0] != 0 || h[1] != num_voxels) {
    n = h[1];
    ISF_REQUIRE(n > 0, ISF_ERR_ARG, "sparse_encoder_forward: no coordinate inside sparse_shape");
    int32_t* perm = nullptr;
    ISF_TRY(build_perm(a, occ0, coors, num_voxels, &perm, st));
    int32_t* cs = nullptr;
    float* xs = nullptr;
    const int C = layers_host[0].c_in;
    ISF_TRY(a.alloc_n(&cs, (size_t)n * 4));
    ISF_TRY(a.alloc_n(&xs, (size_t)n * C));
    ISF_TRY(occ_compact_coords4(occ0, cs, st));
    hipLaunchKernelGGL(gather_rows_kernel, dim3(ceil_div((long long)n * C, 256)), dim3(256), 0, st,
                       voxel_features, perm, n, C, xs);
    ISF_LAUNCH_CHECK();
    x = xs;
    c = cs;
  }
  return sparse_encoder_forward_impl(a, x, c, n, batch_size, sparse_shape_host, &occ0, layers_host, num_layers,
                                     spatial_features, out_shape_host, stats_host, time_layers, options, st);
}

// the LiDAR branch over B frames: one concatenated block (`points`) or one block per frame (`frame_points`, B <= kVoxMaxBatch)
static int lidar_branch_impl(const float* points, const float* const* frame_points, const int64_t* point_offsets_host,
                             int batch_size, const isf_vfe_params* vfe_host, const int sparse_shape_host[3],
                             const isf_conv_layer* layers_host, int num_layers, float* spatial_features,
                             int out_shape_host[4], isf_encoder_stats* stats_host, int time_layers,
                             const isf_encoder_options* options, isf_stream_t stream) {
  using namespace isf;
  hipStream_t st = as_stream(stream);
  Arena& a = arena_for_stream(as_stream(stream));
  ISF_TRY(a.reset());
  const int64_t P64 = point_offsets_host[batch_size];
  ISF_REQUIRE(P64 > 0 && P64 < (1ll << 31), ISF_ERR_ARG, "lidar_branch_forward: bad point count");
  const int P = (int)P64;
  const int Cin = vfe_host->in_channels;
  int32_t* coors4 = nullptr;
  ISF_TRY(a.alloc_n(&coors4, (size_t)P * 4));
  // batches of up to 8 frames: one frame table {offsets, base pointers} for every kernel that reads points, and the frames
  // are voxelized inside the byte-map marking launch of the VFE (one launch instead of B + 1 and one pass over the
  // coordinates less); ISF_ENC_DIAG_VOXELIZE_PER_FRAME and larger batches: one dynamic_voxelize launch per frame
  const bool table = batch_size <= kVoxMaxBatch;
  VoxBatch vb = table ? VoxBatch() : vox_one_block(points, P);   // (larger batches: concatenated, one block)
  if (table) vb.B = batch_size;
  const bool fused_vox = table && !(options && (options->diagnostic & ISF_ENC_DIAG_VOXELIZE_PER_FRAME));
  for (int b = 0; b < batch_size; ++b) {
    const int64_t lo = point_offsets_host[b], hi = point_offsets_host[b + 1];
    ISF_REQUIRE(hi >= lo, ISF_ERR_ARG, "lidar_branch_forward: bad offsets");
    const float* base = frame_points ? frame_points[b] : points + lo * Cin;
    ISF_REQUIRE(base || hi == lo, ISF_ERR_ARG, "lidar_branch_forward: frame %d has no points pointer", b);
    if (table) {
      vb.off[b] = lo;
      vb.off[b + 1] = hi;
      vb.base[b] = base;
    }
    if (!fused_vox && hi > lo)
      ISF_TRY(dynamic_voxelize_impl(base, (int)(hi - lo), Cin, vfe_host->voxel_size, vfe_host->coors_range, coors4 + lo * 4,
                                    4, 1, b, st));
  }
  float* vf = nullptr;
  int32_t* vc = nullptr;
  ISF_TRY(a.alloc_n(&vf, (size_t)P * vfe_host->c2));
  ISF_TRY(a.alloc_n(&vc, (size_t)P * 4));
  int n0 = 0;
  OccIndex occ0;
  hipEvent_t coords_ready = nullptr;
  // the voxel rows go straight into the split format the first convolution reads (whole rows from the VFE's segmented
  // max, the rows cut by a wave boundary from a fix-up pass): no [N, 64] fp32 -> split conversion pass in between
  void* vf_split = nullptr;
  const bool split_kernels = (options ? options->precision : 0) == 0 && num_layers > 0 && num_layers <= 32 &&
                             encoder_use16(layers_host, num_layers, 0);   // fp32-class f16x3 arithmetic on split rows
  if (split_kernels && vfe_host->c2 == layers_host[0].c_in &&
      !(options && (options->diagnostic & ISF_ENC_DIAG_VFE_FP32_ROWS)))   // fp32 rows + the conversion pass (same bits)
    ISF_TRY(a.alloc(&vf_split, (size_t)P * vfe_host->c2 * 4));
  ISF_TRY(dynamic_vfe_impl(a, nullptr, coors4, P, Cin, batch_size, vfe_host->voxel_size, vfe_host->coors_range,
                           vfe_host->w1, vfe_host->scale1, vfe_host->shift1, vfe_host->c1, vfe_host->w2,
                           vfe_host->scale2, vfe_host->shift2, vfe_host->c2, vf, vc, nullptr, &n0, &occ0,
                           sparse_shape_host[0], st, &coords_ready, vf_split, fused_vox ? &vb : nullptr, &vb));
  ISF_REQUIRE(n0 > 0, ISF_ERR_ARG, "lidar_branch_forward: no point falls inside the voxel grid");
  const bool occ_ok = occ0.D == sparse_shape_host[0] && occ0.H == sparse_shape_host[1] &&
                      occ0.W == sparse_shape_host[2];
  return sparse_encoder_forward_impl(a, vf, vc, n0, batch_size, sparse_shape_host, occ_ok ? &occ0 : nullptr,
                                     layers_host, num_layers, spatial_features, out_shape_host, stats_host,
                                     time_layers, options, st, occ_ok ? coords_ready : nullptr, vf_split);
}

int isf_lidar_branch_forward(const float* points, const int64_t* point_offsets_host, int batch_size,
                             const isf_vfe_params* vfe_host, const int sparse_shape_host[3],
                             const isf_conv_layer* layers_host, int num_layers, float* spatial_features,
                             int out_shape_host[4], isf_encoder_stats* stats_host, int time_layers,
                             const isf_encoder_options* options, isf_stream_t stream) {
  ISF_REQUIRE(points && point_offsets_host && batch_size > 0 && vfe_host && sparse_shape_host && layers_host &&
                  spatial_features,
              ISF_ERR_ARG, "lidar_branch_forward: bad arguments");
  return lidar_branch_impl(points, nullptr, point_offsets_host, batch_size, vfe_host, sparse_shape_host, layers_host,
                           num_layers, spatial_features, out_shape_host, stats_host, time_layers, options, stream);
}

int isf_lidar_branch_forward_frames(const float* const* frame_points_host, const int64_t* point_offsets_host, int batch_size,
                                    const isf_vfe_params* vfe_host, const int sparse_shape_host[3],
                                    const isf_conv_layer* layers_host, int num_layers, float* spatial_features,
                                    int out_shape_host[4], isf_encoder_stats* stats_host, int time_layers,
                                    const isf_encoder_options* options, isf_stream_t stream) {
  ISF_REQUIRE(frame_points_host && point_offsets_host && batch_size > 0 && vfe_host && sparse_shape_host && layers_host &&
                  spatial_features,
              ISF_ERR_ARG, "lidar_branch_forward_frames: bad arguments");
  ISF_REQUIRE(batch_size <= isf::kVoxMaxBatch, ISF_ERR_UNSUPPORTED,
              "lidar_branch_forward_frames: %d frames (at most %d; concatenate larger batches)", batch_size, isf::kVoxMaxBatch);
  return lidar_branch_impl(nullptr, frame_points_host, point_offsets_host, batch_size, vfe_host, sparse_shape_host,
                           layers_host, num_layers, spatial_features, out_shape_host, stats_host, time_layers, options, stream);
}

}  // extern "C"
