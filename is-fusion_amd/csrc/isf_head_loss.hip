// isf_head_loss.hip -- training targets, Hungarian assignment and losses of TransFusionHeadV2
// (mmdet3d/models/dense_heads/transfusion_head_v2.py:910-1276, core/bbox/assigners/hungarian_assigner.py:85-156).
//
// The reference runs this stage per sample in Python: a per-box loop that draws Gaussians, a host copy of the cost
// matrix for scipy's linear_sum_assignment, and .item() calls for the average factors -- each a host sync.  Here every
// step is a kernel on the caller's stream, counts and average factors stay on the device, and every reduction is done in
// a fixed order (per-thread partials, then a tree), so two identical calls give bit-identical results.
//
//   heat-map targets   one thread per 4 pixels of one (sample, class) plane; the sample's boxes of that class in LDS;
//                      pixels combine with max, so no atomics and the result does not depend on box order
//   assignment cost    one thread per (proposal, GT) pair: decode (isf_box.h) + focal / BEV-L1 / 3D-IoU costs
//   assignment         one workgroup per (sample, decoder layer): shortest augmenting paths (Jonker-Volgenant, the
//                      variant scipy implements) in fp64 over the fp32 cost; per-column state in LDS
//   target assembly    one workgroup for the batch (B x L x P proposals), writes num_pos / matched_ious on the device
//   losses             each kernel writes the loss and the UNSCALED per-element gradient plus the device scalar
//                      loss_weight / avg_factor; the backward multiplies by that scalar and the incoming gradient
#include "isf_common.h"
#include "isf_box.h"
#include "isf_bev.h"

// float arithmetic below restates torch float32 op sequences: keep every product and sum separately rounded
#pragma clang fp contract(off)

namespace isf {
namespace {

constexpr int kMaxBatch = ISF_HEAD_MAX_BATCH;
constexpr int kLsaMax = ISF_HEAD_MAX_ASSIGN;   // max(P, G) of one assignment problem
constexpr int kThreads = 256;
constexpr int kPartials = 256;                  // blocks of the first reduction stage (fixed: the order never changes)

struct Offsets {
  int off[kMaxBatch + 1];
};

struct HeatmapParams {
  float vx, vy, ox, oy, osf, overlap;
  int min_radius;
};

struct CostParams {
  float cell_x, cell_y, org_x, org_y;
  float pcr[6];
  float w_cls, w_reg, w_iou, alpha, gamma;
};

// ------------------------------------------------------------------------------------------------ block reductions
__device__ double block_sum(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];   // waves in order
  return s;
}

// ------------------------------------------------------------------------------------------------ heat-map targets
// core/utils/gaussian.py:55-85 with the float32 operation order of torch (scalars rounded to float32 first)
__device__ float gaussian_radius_f32(float height, float width, float min_overlap) {
  const float s1 = (float)(1.0 - (double)min_overlap), s2 = (float)(1.0 + (double)min_overlap);
  const float b1 = height + width;
  const float c1 = width * height * s1 / s2;
  const float r1 = (b1 + sqrtf(b1 * b1 - 4.f * c1)) / 2.f;
  const float b2 = 2.f * (height + width);
  const float c2 = s1 * width * height;
  const float r2 = (b2 + sqrtf(b2 * b2 - 16.f * c2)) / 2.f;
  const float b3 = (float)(-2.0 * (double)min_overlap) * (height + width);
  const float c3 = (float)((double)min_overlap - 1.0) * width * height;
  const float r3 = (b3 + sqrtf(b3 * b3 - (float)(16.0 * (double)min_overlap) * c3)) / 2.f;
  return fminf(r1, fminf(r2, r3));
}

__global__ __launch_bounds__(kThreads) void heatmap_targets_kernel(const float* __restrict__ gt, int box_ld,
                                                                  const int64_t* __restrict__ labels, Offsets offs,
                                                                  int C, int H, int W, HeatmapParams prm,
                                                                  float* __restrict__ heatmap) {
  __shared__ int s_row[kThreads], s_col[kThreads], s_rad[kThreads];
  const int strips = (H * W + 4 * kThreads - 1) / (4 * kThreads);
  const int strip = blockIdx.x % strips, c = (blockIdx.x / strips) % C, b = blockIdx.x / (strips * C);
  float val[4] = {0.f, 0.f, 0.f, 0.f};
  const int g0 = offs.off[b], g1 = offs.off[b + 1];
  for (int k0 = g0; k0 < g1; k0 += kThreads) {
    const int k = k0 + threadIdx.x;
    int rad = -1, row = 0, col = 0;
    if (k < g1 && labels[k] == c) {
      const float* box = gt + (size_t)k * box_ld;
      // transfusion_head_v2.py:1089-1126: width along x, length along y, in feature-map cells
      const float width = box[3] / prm.vx / prm.osf, length = box[4] / prm.vy / prm.osf;
      if (width > 0.f && length > 0.f) {
        rad = max(prm.min_radius, (int)gaussian_radius_f32(length, width, prm.overlap));
        const float cx = (box[0] - prm.ox) / prm.vx / prm.osf, cy = (box[1] - prm.oy) / prm.vy / prm.osf;
        // center_int[[1, 0]] (:1122-1124): draw_heatmap_gaussian's x (column) is coor_y, its y (row) is coor_x
        row = (int)cx;
        col = (int)cy;
      }
    }
    __syncthreads();
    s_rad[threadIdx.x] = rad;
    s_row[threadIdx.x] = row;
    s_col[threadIdx.x] = col;
    __syncthreads();
    const int n = min(kThreads, g1 - k0);
    for (int q = 0; q < 4; ++q) {
      const int pix = (strip * 4 + q) * kThreads + threadIdx.x;
      if (pix >= H * W) continue;
      const int i = pix / W, j = pix % W;
      for (int t = 0; t < n; ++t) {
        const int r = s_rad[t];
        if (r < 0) continue;
        const int dy = i - s_row[t], dx = j - s_col[t];
        if (dy < -r || dy > r || dx < -r || dx > r) continue;
        // gaussian_2d((2r+1, 2r+1), sigma=(2r+1)/6) in float64, entries below eps * max (max = 1) cut to 0, then float32
        const double sigma = (double)(2 * r + 1) / 6.0;
        const double h = exp(-((double)dx * dx + (double)dy * dy) / (2.0 * sigma * sigma));
        const float g = h < 2.220446049250313e-16 ? 0.f : (float)h;
        val[q] = fmaxf(val[q], g);
      }
    }
  }
  float* out = heatmap + ((size_t)b * C + c) * H * W;
  for (int q = 0; q < 4; ++q) {
    const int pix = (strip * 4 + q) * kThreads + threadIdx.x;
    if (pix < H * W) out[pix] = val[q];
  }
}

// ------------------------------------------------------------------------------------------------ 3D IoU
// bev_overlap: isf_bev.h (shared with the rotated NMS)

// BboxOverlaps3D(coordinate='lidar') = LiDARInstance3DBoxes.overlaps (core/bbox/structures/base_box3d.py:388-442):
// BEV overlap x height overlap / union, bottom-centre boxes
__device__ double iou3d(const float* a, const float* b) {
  const double top = fmin((double)a[2] + a[5], (double)b[2] + b[5]), bot = fmax((double)a[2], (double)b[2]);
  const double oh = fmax(top - bot, 0.0);
  const double o3 = bev_overlap(a, b) * oh;
  const double va = (double)a[3] * a[4] * a[5], vb = (double)b[3] * b[4] * b[5];
  return o3 / fmax(va + vb - o3, 1e-8);
}

__global__ __launch_bounds__(kThreads) void assign_cost_kernel(
    const float* __restrict__ heatmap, const float* __restrict__ center, const float* __restrict__ height,
    const float* __restrict__ dim, const float* __restrict__ rot, const float* __restrict__ vel, int C, int P, int ld,
    const float* __restrict__ gt, int box_ld, const int64_t* __restrict__ labels, Offsets offs, int gs, CostParams prm,
    float* __restrict__ boxes, float* __restrict__ cost, float* __restrict__ iou) {
  const int b = blockIdx.z, l = blockIdx.y;
  const int G = offs.off[b + 1] - offs.off[b];
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  const int code = vel ? 9 : 7;
  const int p = G > 0 ? idx / G : idx, g = G > 0 ? idx % G : 0;
  if (p >= P) return;
  const int col = l * P + p;
  float box[9];
  decode_box(center + (size_t)b * 2 * ld, height + (size_t)b * ld, dim + (size_t)b * 3 * ld, rot + (size_t)b * 2 * ld,
             vel ? vel + (size_t)b * 2 * ld : nullptr, ld, col, prm.cell_x, prm.cell_y, prm.org_x, prm.org_y, box);
  if (g == 0) {
    float* o = boxes + ((size_t)b * ld + col) * code;
    for (int a = 0; a < code; ++a) o[a] = box[a];
  }
  if (G == 0) return;
  const int k = offs.off[b] + g;
  const float* gbox = gt + (size_t)k * box_ld;
  const int lab = (int)labels[k];
  // FocalLossCost on cls_pred[0].T (mmdet/core/bbox/match_costs/match_cost.py, FocalLossCost.__call__)
  float cls = 0.f;
  if (lab >= 0 && lab < C) {
    const float x = heatmap[((size_t)b * C + lab) * ld + col];
    const float s = 1.f / (1.f + expf(-x));
    const float eps = 1e-12f;
    const float neg = -logf(1.f - s + eps) * (1.f - prm.alpha) * powf(s, prm.gamma);
    const float pos = -logf(s + eps) * prm.alpha * powf(1.f - s, prm.gamma);
    cls = (pos - neg) * prm.w_cls;
  }
  // BBoxBEVL1Cost (hungarian_assigner.py:27-38): L1 distance of the centres normalised by point_cloud_range
  const float sx = prm.pcr[3] - prm.pcr[0], sy = prm.pcr[4] - prm.pcr[1];
  const float reg = (fabsf((box[0] - prm.pcr[0]) / sx - (gbox[0] - prm.pcr[0]) / sx) +
                     fabsf((box[1] - prm.pcr[1]) / sy - (gbox[1] - prm.pcr[1]) / sy)) * prm.w_reg;
  const float ov = (float)iou3d(box, gbox);
  const size_t at = (((size_t)b * gridDim.y + l) * P + p) * gs + g;
  cost[at] = cls + reg + (-ov) * prm.w_iou;   // IoU3DCost = -iou * weight
  iou[at] = ov;
}

// ------------------------------------------------------------------------------------------------ assignment
// linear_sum_assignment of the P x G cost (hungarian_assigner.py:137-141; scipy's shortest augmenting path, Crouse
// 2016).  The smaller side is assigned row by row; columns live one per thread (up to kLsaMax / kThreads each).  One
// Dijkstra step = every thread relaxes its columns, then a block argmin (lowest reduced cost, then an unassigned
// column, then the lowest index).
__global__ __launch_bounds__(kThreads) void assign_kernel(const float* __restrict__ cost, const float* __restrict__ iou,
                                                         int gs, const int64_t* __restrict__ labels, Offsets offs,
                                                         int P, int L, int ld, int32_t* __restrict__ assigned,
                                                         int64_t* __restrict__ assigned_labels,
                                                         float* __restrict__ max_overlaps) {
  __shared__ double v[kLsaMax], spc[kLsaMax], u[kLsaMax];
  __shared__ int path[kLsaMax], row4col[kLsaMax], col4row[kLsaMax];
  __shared__ unsigned char sc[kLsaMax], sr[kLsaMax];
  __shared__ double red_v[kThreads / 64];
  __shared__ int red_k[kThreads / 64];
  const int b = blockIdx.y, l = blockIdx.x, tid = threadIdx.x;
  const int G = offs.off[b + 1] - offs.off[b];
  const float* cm = cost + ((size_t)b * L + l) * P * gs;
  const float* im = iou + ((size_t)b * L + l) * P * gs;
  for (int p = tid; p < P; p += kThreads) {
    assigned[(size_t)b * ld + l * P + p] = 0;
    assigned_labels[(size_t)b * ld + l * P + p] = -1;
    max_overlaps[(size_t)b * ld + l * P + p] = 0.f;
  }
  if (G == 0 || P == 0) return;
  const bool tr = P > G;                    // rows = the smaller side
  const int n = tr ? G : P, m = tr ? P : G;
  for (int j = tid; j < m; j += kThreads) { v[j] = 0.0; row4col[j] = -1; }
  for (int i = tid; i < n; i += kThreads) { u[i] = 0.0; col4row[i] = -1; }
  __syncthreads();
  const double inf = __builtin_huge_val();
  for (int cur = 0; cur < n; ++cur) {
    for (int j = tid; j < m; j += kThreads) { spc[j] = inf; path[j] = -1; sc[j] = 0; }
    for (int i = tid; i < n; i += kThreads) sr[i] = 0;
    __syncthreads();
    double min_val = 0.0;
    int i = cur, sink = -1;
    for (int step = 0; step < m && sink < 0; ++step) {
      if (tid == 0) sr[i] = 1;
      const double ui = u[i];
      double best = inf;
      int key = 0x7fffffff;
      for (int j = tid; j < m; j += kThreads) {
        if (sc[j]) continue;
        const double c = (double)(tr ? cm[(size_t)j * gs + i] : cm[(size_t)i * gs + j]);
        const double r = min_val + c - ui - v[j];
        if (r < spc[j]) { spc[j] = r; path[j] = i; }
        const int k = (row4col[j] >= 0 ? (1 << 20) : 0) + j;
        if (spc[j] < best || (spc[j] == best && k < key)) { best = spc[j]; key = k; }
      }
      for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int ok = __shfl_xor(key, o);
        if (ob < best || (ob == best && ok < key)) { best = ob; key = ok; }
      }
      __syncthreads();
      if ((tid & 63) == 0) { red_v[tid >> 6] = best; red_k[tid >> 6] = key; }
      __syncthreads();
      best = red_v[0];
      key = red_k[0];
      for (int w = 1; w < kThreads / 64; ++w)
        if (red_v[w] < best || (red_v[w] == best && red_k[w] < key)) { best = red_v[w]; key = red_k[w]; }
      if (key == 0x7fffffff) break;         // no finite reduced cost (non-finite input): leave this row unassigned
      const int j = key & ((1 << 20) - 1);
      min_val = best;
      if (row4col[j] < 0) sink = j; else i = row4col[j];
      __syncthreads();                       // every thread has read sc / row4col / red_* of this step
      if (tid == 0) sc[j] = 1;
      __syncthreads();
    }
    if (sink < 0) { __syncthreads(); continue; }
    // dual update (scipy: u[cur] += minVal; u[i] += minVal - spc[col4row[i]] on SR rows; v[j] -= minVal - spc[j] on SC)
    for (int r = tid; r < n; r += kThreads) {
      if (r == cur) u[r] += min_val;
      else if (sr[r]) u[r] += min_val - spc[col4row[r]];
    }
    for (int j = tid; j < m; j += kThreads)
      if (sc[j]) v[j] -= min_val - spc[j];
    __syncthreads();
    if (tid == 0) {                          // augment along the path (at most n hops)
      int j = sink;
      for (int hop = 0; hop <= n; ++hop) {
        const int r = path[j];
        row4col[j] = r;
        const int t = col4row[r];
        col4row[r] = j;
        j = t;
        if (r == cur) break;
      }
    }
    __syncthreads();
  }
  // hungarian_assigner.py:143-156: gt index + 1, the GT's label and the pair's IoU on matched proposals
  for (int r = tid; r < n; r += kThreads) {
    const int c = col4row[r];
    if (c < 0) continue;
    const int p = tr ? c : r, g = tr ? r : c;
    const size_t at = (size_t)b * ld + l * P + p;
    assigned[at] = g + 1;
    assigned_labels[at] = labels[offs.off[b] + g];
    max_overlaps[at] = im[(size_t)p * gs + g];
  }
}

// ------------------------------------------------------------------------------------------------ target assembly
struct EncodeParams {
  float cell_x, cell_y, org_x, org_y, pos_weight;
  int code_size;
};

__global__ __launch_bounds__(kThreads) void assemble_targets_kernel(
    const int32_t* __restrict__ assigned, const float* __restrict__ max_overlaps, const float* __restrict__ gt,
    int box_ld, const int64_t* __restrict__ labels, Offsets offs, int B, int ld, int C, EncodeParams prm,
    int64_t* __restrict__ out_labels, float* __restrict__ label_weights, float* __restrict__ bbox_targets,
    float* __restrict__ bbox_weights, float* __restrict__ ious, int32_t* __restrict__ num_pos,
    float* __restrict__ stats) {
  __shared__ double red[kThreads / 64];
  const int code = prm.code_size;
  int total = 0;
  double miou = 0.0;
  for (int b = 0; b < B; ++b) {
    double cnt = 0.0, isum = 0.0;
    for (int p = threadIdx.x; p < ld; p += kThreads) {
      const size_t at = (size_t)b * ld + p;
      const int a = assigned[at];
      const float io = fminf(fmaxf(max_overlaps[at], 0.f), 1.f);
      ious[at] = io;
      float* bt = bbox_targets + at * code;
      float* bw = bbox_weights + at * code;
      if (a > 0) {
        // TransFusionBBoxCoder.encode (core/bbox/coders/transfusion_bbox_coder.py:24-40) of the bottom-centre GT box
        const int k = offs.off[b] + a - 1;
        const float* g = gt + (size_t)k * box_ld;
        out_labels[at] = labels[k];
        label_weights[at] = prm.pos_weight <= 0.f ? 1.f : prm.pos_weight;
        bt[0] = (g[0] - prm.org_x) / prm.cell_x;
        bt[1] = (g[1] - prm.org_y) / prm.cell_y;
        bt[3] = logf(g[3]);
        bt[4] = logf(g[4]);
        bt[5] = logf(g[5]);
        bt[2] = g[2] + g[5] * 0.5f;
        bt[6] = sinf(g[6]);
        bt[7] = cosf(g[6]);
        if (code == 10) { bt[8] = g[7]; bt[9] = g[8]; }
        for (int q = 0; q < code; ++q) bw[q] = 1.f;
        cnt += 1.0;
        isum += io;
      } else {
        out_labels[at] = C;                  // background = num_classes
        label_weights[at] = 1.f;
        for (int q = 0; q < code; ++q) { bt[q] = 0.f; bw[q] = 0.f; }
      }
    }
    const int n = (int)block_sum(cnt, red);
    const double s = block_sum(isum, red);
    total += n;
    miou += (double)(float)(s / (double)max(n, 1));   // per sample float(mean_iou) (:1130), then np.mean (:948)
  }
  if (threadIdx.x == 0) {
    num_pos[0] = total;
    stats[0] = (float)total;
    stats[1] = (float)(miou / (double)max(B, 1));
  }
}

// ------------------------------------------------------------------------------------------------ losses
__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float softplusf(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// GaussianFocalLoss (alpha 2, gamma 4; mmdet/models/losses/gaussian_focal_loss.py) on clip_sigmoid(logits)
// (mmdet3d/models/utils/clip_sigmoid.py: clamp(sigmoid(x), 1e-4, 1 - 1e-4)); grad = d loss_e / d logit
__global__ __launch_bounds__(kThreads) void gaussian_focal_stage1(const float* __restrict__ logits,
                                                                 const float* __restrict__ target, size_t n,
                                                                 float* __restrict__ grad, double* __restrict__ part) {
  __shared__ double red[kThreads / 64];
  double acc = 0.0, cnt = 0.0;
  const size_t stride = (size_t)gridDim.x * kThreads;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += stride) {
    const float x = logits[e], t = target[e];
    const float s = sigmoidf(x);
    const float p = fminf(fmaxf(s, 1e-4f), 1.f - 1e-4f);
    const float eps = 1e-12f;
    const float omt = 1.f - t, negw = (omt * omt) * (omt * omt);
    const float lp = logf(p + eps), ln = logf(1.f - p + eps);
    float loss = -ln * (p * p) * negw, dldp = negw * (p * p / (1.f - p + eps) - 2.f * p * ln);
    if (t == 1.f) {
      loss += -lp * ((1.f - p) * (1.f - p));
      dldp += -((1.f - p) * (1.f - p)) / (p + eps) + 2.f * (1.f - p) * lp;
      cnt += 1.0;
    }
    acc += loss;
    grad[e] = (s >= 1e-4f && s <= 1.f - 1e-4f) ? dldp * (s * (1.f - s)) : 0.f;
  }
  const double a = block_sum(acc, red);
  const double c = block_sum(cnt, red);
  if (threadIdx.x == 0) { part[blockIdx.x] = a; part[kPartials + blockIdx.x] = c; }
}

__global__ __launch_bounds__(kThreads) void gaussian_focal_stage2(const double* __restrict__ part, float loss_weight,
                                                                 float* __restrict__ loss, float* __restrict__ scale) {
  __shared__ double red[kThreads / 64];
  const double a = block_sum(part[threadIdx.x], red);
  const double c = block_sum(part[kPartials + threadIdx.x], red);
  if (threadIdx.x == 0) {
    const double avg = fmax(c, 1.0);        // max(heatmap.eq(1).sum(), 1) (:1174)
    loss[0] = (float)(a / avg * loss_weight);
    scale[0] = (float)(loss_weight / avg);
  }
}

// sigmoid FocalLoss (gamma, alpha; mmcv sigmoid_focal_loss as mmdet's FocalLoss calls it for label targets): label ==
// num_classes is all-negative; weight per proposal; reduction mean with avg_factor max(num_pos, 1)
__global__ __launch_bounds__(kThreads) void sigmoid_focal_kernel(
    const float* __restrict__ logits, int B, int C, int P, int ld, int off, const int64_t* __restrict__ labels,
    const float* __restrict__ weights, const int32_t* __restrict__ num_pos, float alpha, float gamma,
    float loss_weight, float* __restrict__ grad, float* __restrict__ loss, float* __restrict__ scale) {
  __shared__ double red[kThreads / 64];
  double acc = 0.0;
  const int n = B * P * C;
  for (int e = threadIdx.x; e < n; e += kThreads) {
    const int c = e % C, p = (e / C) % P, b = e / (C * P);
    const size_t xi = ((size_t)b * C + c) * ld + off + p;
    const float x = logits[xi];
    const float w = weights[(size_t)b * ld + off + p];
    const bool t = labels[(size_t)b * ld + off + p] == c;
    const float s = sigmoidf(x);
    float l, d;
    if (t) {   // -alpha (1-p)^g log p ;  d/dx = alpha (1-p)^g (g p log p - (1-p))
      const float lg = -softplusf(-x), q = powf(1.f - s, gamma);
      l = -alpha * q * lg;
      d = alpha * q * (gamma * s * lg - (1.f - s));
    } else {   // -(1-alpha) p^g log(1-p) ;  d/dx = (1-alpha) p^g (p - g (1-p) log(1-p))
      const float lg = -softplusf(x), q = powf(s, gamma);
      l = -(1.f - alpha) * q * lg;
      d = (1.f - alpha) * q * (s - gamma * (1.f - s) * lg);
    }
    acc += (double)(l * w);
    grad[xi] = d * w;
  }
  const double a = block_sum(acc, red);
  if (threadIdx.x == 0) {
    const double avg = (double)max(num_pos[0], 1);
    loss[0] = (float)(a / avg * loss_weight);
    scale[0] = (float)(loss_weight / avg);
  }
}

// L1Loss on [center, height, dim, rot, vel] vs bbox_targets, weight bbox_weights * code_weights, avg max(num_pos, 1);
// grad [B, code, ld] (the proposal slice [off, off + P) written), sign(pred - target) * weight
struct CodeWeights {
  float w[10];
};

__global__ __launch_bounds__(kThreads) void l1_kernel(const float* __restrict__ center, const float* __restrict__ height,
                                                      const float* __restrict__ dim, const float* __restrict__ rot,
                                                      const float* __restrict__ vel, int B, int P, int ld, int off,
                                                      int code, const float* __restrict__ targets,
                                                      const float* __restrict__ bweights, CodeWeights cw,
                                                      const int32_t* __restrict__ num_pos, float loss_weight,
                                                      float* __restrict__ grad, float* __restrict__ loss,
                                                      float* __restrict__ scale) {
  __shared__ double red[kThreads / 64];
  double acc = 0.0;
  const int n = B * P * code;
  for (int e = threadIdx.x; e < n; e += kThreads) {
    const int k = e % code, p = (e / code) % P, b = e / (code * P);
    const int col = off + p;
    float x;
    if (k < 2) x = center[((size_t)b * 2 + k) * ld + col];
    else if (k < 3) x = height[(size_t)b * ld + col];
    else if (k < 6) x = dim[((size_t)b * 3 + k - 3) * ld + col];
    else if (k < 8) x = rot[((size_t)b * 2 + k - 6) * ld + col];
    else x = vel[((size_t)b * 2 + k - 8) * ld + col];
    const size_t ti = ((size_t)b * ld + col) * code + k;
    const float w = bweights[ti] * cw.w[k];
    const float d = x - targets[ti];
    acc += (double)(fabsf(d) * w);
    grad[((size_t)b * code + k) * ld + col] = (d > 0.f ? w : d < 0.f ? -w : 0.f);
  }
  const double a = block_sum(acc, red);
  if (threadIdx.x == 0) {
    const double avg = (double)max(num_pos[0], 1);
    loss[0] = (float)(a / avg * loss_weight);
    scale[0] = (float)(loss_weight / avg);
  }
}

__global__ __launch_bounds__(kThreads) void grad_scale_kernel(const float* __restrict__ g, size_t n,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ grad_output,
                                                             float* __restrict__ out) {
  const float s = scale[0] * (grad_output ? grad_output[0] : 1.f);
  const size_t stride = (size_t)gridDim.x * kThreads;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += stride) out[e] = g[e] * s;
}

int read_offsets(const int* host, int B, Offsets* o, const char* what) {
  ISF_REQUIRE(B >= 1 && B <= kMaxBatch, ISF_ERR_ARG, "%s: batch size %d outside [1, %d]", what, B, kMaxBatch);
  ISF_REQUIRE(host != nullptr && host[0] == 0, ISF_ERR_ARG, "%s: gt_offsets must start at 0", what);
  for (int b = 0; b <= B; ++b) {
    ISF_REQUIRE(b == 0 || host[b] >= host[b - 1], ISF_ERR_ARG, "%s: gt_offsets not monotone at %d", what, b);
    o->off[b] = host[b];
  }
  return ISF_OK;
}

}  // namespace
}  // namespace isf

extern "C" {

int isf_head_heatmap_targets(const float* gt_boxes, int box_ld, const int64_t* gt_labels, const int* gt_offsets,
                             int batch_size, int num_classes, int height, int width, const float* params,
                             float* heatmap, isf_stream_t stream) {
  using namespace isf;
  Offsets offs;
  ISF_TRY(read_offsets(gt_offsets, batch_size, &offs, "head_heatmap_targets"));
  ISF_REQUIRE(num_classes > 0 && height > 0 && width > 0 && box_ld >= 7 && params && heatmap, ISF_ERR_ARG,
              "head_heatmap_targets: bad arguments (classes %d, %d x %d, box_ld %d)", num_classes, height, width,
              box_ld);
  ISF_REQUIRE(offs.off[batch_size] == 0 || (gt_boxes && gt_labels), ISF_ERR_ARG, "head_heatmap_targets: null GT");
  HeatmapParams prm{params[0], params[1], params[2], params[3], params[4], params[5], (int)params[6]};
  const int strips = ceil_div((long long)height * width, 4 * kThreads);
  hipLaunchKernelGGL(heatmap_targets_kernel, dim3(batch_size * num_classes * strips), dim3(kThreads), 0,
                     as_stream(stream), gt_boxes, box_ld, gt_labels, offs, num_classes, height, width, prm, heatmap);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_head_assign_cost(const float* heatmap, const float* center, const float* height, const float* dim,
                         const float* rot, const float* vel, int batch_size, int num_classes, int num_proposals,
                         int num_layers, const float* gt_boxes, int box_ld, const int64_t* gt_labels,
                         const int* gt_offsets, int gt_stride, const float* params, float* boxes, float* cost,
                         float* iou, isf_stream_t stream) {
  using namespace isf;
  Offsets offs;
  ISF_TRY(read_offsets(gt_offsets, batch_size, &offs, "head_assign_cost"));
  ISF_REQUIRE(num_classes > 0 && num_proposals > 0 && num_layers > 0 && box_ld >= 7 && params, ISF_ERR_ARG,
              "head_assign_cost: bad arguments");
  int gmax = 0;
  for (int b = 0; b < batch_size; ++b) gmax = max(gmax, offs.off[b + 1] - offs.off[b]);
  ISF_REQUIRE(gt_stride >= gmax, ISF_ERR_ARG, "head_assign_cost: gt_stride %d < max GT per sample %d", gt_stride, gmax);
  ISF_REQUIRE(heatmap && center && height && dim && rot && boxes && (gmax == 0 || (gt_boxes && gt_labels && cost && iou)),
              ISF_ERR_ARG, "head_assign_cost: null pointer");
  CostParams prm;
  prm.cell_x = params[0];
  prm.cell_y = params[1];
  prm.org_x = params[2];
  prm.org_y = params[3];
  for (int a = 0; a < 6; ++a) prm.pcr[a] = params[4 + a];
  prm.w_cls = params[10];
  prm.w_reg = params[11];
  prm.w_iou = params[12];
  prm.alpha = params[13];
  prm.gamma = params[14];
  const int ld = num_proposals * num_layers;
  const int blocks = ceil_div((long long)num_proposals * max(gmax, 1), kThreads);
  hipLaunchKernelGGL(assign_cost_kernel, dim3(blocks, num_layers, batch_size), dim3(kThreads), 0, as_stream(stream),
                     heatmap, center, height, dim, rot, vel, num_classes, num_proposals, ld, gt_boxes, box_ld,
                     gt_labels, offs, gt_stride, prm, boxes, cost, iou);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_head_assign(const float* cost, const float* iou, int gt_stride, const int64_t* gt_labels,
                    const int* gt_offsets, int batch_size, int num_proposals, int num_layers, int32_t* assigned_gt_inds,
                    int64_t* assigned_labels, float* max_overlaps, isf_stream_t stream) {
  using namespace isf;
  Offsets offs;
  ISF_TRY(read_offsets(gt_offsets, batch_size, &offs, "head_assign"));
  ISF_REQUIRE(num_proposals > 0 && num_proposals <= kLsaMax && num_layers > 0, ISF_ERR_ARG,
              "head_assign: num_proposals %d outside [1, %d]", num_proposals, kLsaMax);
  for (int b = 0; b < batch_size; ++b) {
    const int g = offs.off[b + 1] - offs.off[b];
    ISF_REQUIRE(g <= kLsaMax, ISF_ERR_UNSUPPORTED,
                "head_assign: sample %d has %d GT boxes; the on-device assignment handles at most %d per sample", b,
                g, kLsaMax);
    ISF_REQUIRE(g <= gt_stride, ISF_ERR_ARG, "head_assign: gt_stride %d < %d GT boxes", gt_stride, g);
  }
  ISF_REQUIRE(assigned_gt_inds && assigned_labels && max_overlaps, ISF_ERR_ARG, "head_assign: null output");
  hipLaunchKernelGGL(assign_kernel, dim3(num_layers, batch_size), dim3(kThreads), 0, as_stream(stream), cost, iou,
                     gt_stride, gt_labels, offs, num_proposals, num_layers, num_proposals * num_layers,
                     assigned_gt_inds, assigned_labels, max_overlaps);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_head_assemble_targets(const int32_t* assigned_gt_inds, const float* max_overlaps, const float* gt_boxes,
                              int box_ld, const int64_t* gt_labels, const int* gt_offsets, int batch_size,
                              int num_proposals_total, int num_classes, int code_size, const float* params,
                              int64_t* labels, float* label_weights, float* bbox_targets, float* bbox_weights,
                              float* ious, int32_t* num_pos, float* stats, isf_stream_t stream) {
  using namespace isf;
  Offsets offs;
  ISF_TRY(read_offsets(gt_offsets, batch_size, &offs, "head_assemble_targets"));
  ISF_REQUIRE(num_proposals_total > 0 && num_classes > 0 && (code_size == 8 || code_size == 10) && params,
              ISF_ERR_ARG, "head_assemble_targets: bad arguments (code_size %d)", code_size);
  ISF_REQUIRE(code_size == 8 || box_ld >= 9, ISF_ERR_ARG, "head_assemble_targets: code_size 10 needs velocities");
  EncodeParams prm{params[0], params[1], params[2], params[3], params[4], code_size};
  hipLaunchKernelGGL(assemble_targets_kernel, dim3(1), dim3(kThreads), 0, as_stream(stream), assigned_gt_inds,
                     max_overlaps, gt_boxes, box_ld, gt_labels, offs, batch_size, num_proposals_total, num_classes, prm,
                     labels, label_weights, bbox_targets, bbox_weights, ious, num_pos, stats);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_gaussian_focal_loss(const float* logits, const float* target, size_t n, float loss_weight, double* partials,
                            float* grad, float* loss, float* scale, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(logits && target && partials && grad && loss && scale && n > 0, ISF_ERR_ARG,
              "gaussian_focal_loss: bad arguments");
  hipLaunchKernelGGL(gaussian_focal_stage1, dim3(kPartials), dim3(kThreads), 0, as_stream(stream), logits, target, n,
                     grad, partials);
  ISF_LAUNCH_CHECK();
  hipLaunchKernelGGL(gaussian_focal_stage2, dim3(1), dim3(kThreads), 0, as_stream(stream), partials, loss_weight, loss,
                     scale);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_sigmoid_focal_loss(const float* logits, int batch_size, int num_classes, int num_proposals, int ld,
                           int offset, const int64_t* labels, const float* label_weights, const int32_t* num_pos,
                           float alpha, float gamma, float loss_weight, float* grad, float* loss, float* scale,
                           isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(batch_size > 0 && num_classes > 0 && num_proposals > 0 && offset >= 0 && offset + num_proposals <= ld,
              ISF_ERR_ARG, "sigmoid_focal_loss: bad sizes");
  ISF_REQUIRE(logits && labels && label_weights && num_pos && grad && loss && scale, ISF_ERR_ARG,
              "sigmoid_focal_loss: null pointer");
  hipLaunchKernelGGL(sigmoid_focal_kernel, dim3(1), dim3(kThreads), 0, as_stream(stream), logits, batch_size,
                     num_classes, num_proposals, ld, offset, labels, label_weights, num_pos, alpha, gamma, loss_weight,
                     grad, loss, scale);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_head_l1_loss(const float* center, const float* height, const float* dim, const float* rot, const float* vel,
                     int batch_size, int num_proposals, int ld, int offset, int code_size, const float* bbox_targets,
                     const float* bbox_weights, const float* code_weights, const int32_t* num_pos, float loss_weight,
                     float* grad, float* loss, float* scale, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(batch_size > 0 && num_proposals > 0 && offset >= 0 && offset + num_proposals <= ld &&
                  (code_size == 8 || (code_size == 10 && vel)),
              ISF_ERR_ARG, "head_l1_loss: bad sizes (code_size %d)", code_size);
  ISF_REQUIRE(center && height && dim && rot && bbox_targets && bbox_weights && code_weights && num_pos && grad &&
                  loss && scale,
              ISF_ERR_ARG, "head_l1_loss: null pointer");
  CodeWeights cw;
  for (int k = 0; k < 10; ++k) cw.w[k] = k < code_size ? code_weights[k] : 0.f;
  hipLaunchKernelGGL(l1_kernel, dim3(1), dim3(kThreads), 0, as_stream(stream), center, height, dim, rot, vel,
                     batch_size, num_proposals, ld, offset, code_size, bbox_targets, bbox_weights, cw, num_pos,
                     loss_weight, grad, loss, scale);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_head_loss_grad_scale(const float* grad, size_t n, const float* scale, const float* grad_output, float* out,
                             isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(grad && scale && out, ISF_ERR_ARG, "head_loss_grad_scale: null pointer");
  if (n == 0) return ISF_OK;
  const int blocks = (int)std::min<size_t>(1024, (n + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(grad_scale_kernel, dim3(blocks), dim3(kThreads), 0, as_stream(stream), grad, n, scale, grad_output,
                     out);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

}  // extern "C"
