// isf_eval.hip -- nuScenes detection evaluation (mAP / NDS) on the device, in four stages on the caller's stream:
//   match   one workgroup per sample: score order in LDS, one wave per distance threshold walks it greedily
//   order   stable LSD radix sort of all rows by (class, descending score); the index is the payload
//   curves  per (class, threshold): scan of the TP flags, 101-point interpolation; per class the TP error curves
//   scalars AP, TP means, nanmeans, NDS into one small fp64 block
// All arithmetic is fp64 on the fp32 inputs, written as the numpy expressions of the protocol (no contraction into FMAs,
// so the discrete decisions are those of a float64 host restatement).
#include "isf_common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace isf {

constexpr int kEvThreads = 256;
constexpr int kEvWaves = kEvThreads / 64;
constexpr int kEvPredLds = 512;            // >= ISF_EVAL_MAX_PRED
constexpr int kEvGtPerLane = ISF_EVAL_MAX_GT / 64;

struct EvalCfg {
  float range[ISF_EVAL_MAX_CLASSES];
  int half_period[ISF_EVAL_MAX_CLASSES];   // 1: yaw period pi (barrier)
  int nan_mask[ISF_EVAL_MAX_CLASSES];      // bit m: TP metric m of the class is NaN by definition
  double ths[ISF_EVAL_MAX_THS];
  int C, T, tp_index;
};

struct AttrTable {
  int moving[ISF_EVAL_MAX_CLASSES];
  int still[ISF_EVAL_MAX_CLASSES];
};

// ascending unsigned order of the result = DESCENDING score; negative scores map below the positive ones
__device__ __forceinline__ uint32_t ev_score_key(float s) {
  const uint32_t u = __float_as_uint(s);
  const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}

// ----------------------------------------------------------------------------- predicted attributes
__global__ void ev_attr_kernel(const int32_t* __restrict__ labels, const float* __restrict__ boxes, int box_ld, long long rows,
                               int C, AttrTable tab, int32_t* __restrict__ attrs) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  const int c = labels[i];
  int a = -1;
  if (c >= 0 && c < C) {
    const float vx = boxes[(size_t)i * box_ld + 7], vy = boxes[(size_t)i * box_ld + 8];
    const double sp = sqrt((double)vx * (double)vx + (double)vy * (double)vy);
    a = sp > 0.2 ? tab.moving[c] : tab.still[c];
  }
  attrs[i] = a;
}

// ----------------------------------------------------------------------------- stage 1: match
// |(R c + t)_xy| of the box's gravity centre
__device__ __forceinline__ double ev_ego_radius(const float* __restrict__ b, const double* __restrict__ M) {
  const double x = (double)b[0], y = (double)b[1], z = (double)b[2] + (double)b[5] * 0.5;
  const double ex = M[0] * x + M[1] * y + M[2] * z + M[3];
  const double ey = M[4] * x + M[5] * y + M[6] * z + M[7];
  return sqrt(ex * ex + ey * ey);
}

__global__ __launch_bounds__(kEvThreads) void ev_match_kernel(
    const float* __restrict__ pboxes, const float* __restrict__ pscores, const int32_t* __restrict__ plabels,
    const uint8_t* __restrict__ pvalid, const int32_t* __restrict__ pattrs, const int32_t* __restrict__ poff,
    const float* __restrict__ gboxes, const int32_t* __restrict__ glabels, const int32_t* __restrict__ gattrs,
    const int32_t* __restrict__ gnpts, const int32_t* __restrict__ goff, const double* __restrict__ l2e, EvalCfg cfg,
    uint32_t* __restrict__ keys, int32_t* __restrict__ cls, uint8_t* __restrict__ tp_mask, uint8_t* __restrict__ tp_mask_rows,
    double* __restrict__ conf, double* __restrict__ errs, int32_t* __restrict__ counts) {
  __shared__ float sc_s[kEvPredLds], px_s[kEvPredLds], py_s[kEvPredLds];
  __shared__ int lab_s[kEvPredLds];
  __shared__ short ord_s[kEvPredLds];
  __shared__ unsigned tpm_s[kEvPredLds];
  __shared__ float gx_s[ISF_EVAL_MAX_GT], gy_s[ISF_EVAL_MAX_GT];
  __shared__ int glab_s[ISF_EVAL_MAX_GT];
  __shared__ int nvalid_s;
  __shared__ int hist_s[2 * 32];           // npos, then predictions, per class: one global atomic per class and workgroup
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p0 = poff[s], g0 = goff[s];
  int P = poff[s + 1] - p0, G = goff[s + 1] - g0;
  P = P < 0 ? 0 : (P > ISF_EVAL_MAX_PRED ? ISF_EVAL_MAX_PRED : P);     // the host refuses more; never index past the LDS
  G = G < 0 ? 0 : (G > ISF_EVAL_MAX_GT ? ISF_EVAL_MAX_GT : G);
  const double* M = l2e + (size_t)s * 16;
  if (tid == 0) nvalid_s = 0;
  if (tid < 2 * 32) hist_s[tid] = 0;
  __syncthreads();
  for (int i = tid; i < P; i += kEvThreads) {
    const size_t r = (size_t)p0 + i;
    const float* b = pboxes + r * 9;
    const int c = plabels[r];
    const float sc = pscores[r] + 0.f;                                  // -0 -> +0
    bool ok = pvalid[r] != 0 && c >= 0 && c < cfg.C && sc == sc;
    if (ok) ok = !(ev_ego_radius(b, M) > (double)cfg.range[c]);
    lab_s[i] = ok ? c : -1;
    sc_s[i] = sc;
    px_s[i] = b[0];
    py_s[i] = b[1];
    tpm_s[i] = 0u;
    tp_mask_rows[r] = 0;
  }
  for (int g = tid; g < G; g += kEvThreads) {
    const size_t r = (size_t)g0 + g;
    const float* b = gboxes + r * 9;
    const int c = glabels[r];
    bool ok = c >= 0 && c < cfg.C && (gnpts == nullptr || gnpts[r] > 0);
    if (ok) ok = !(ev_ego_radius(b, M) > (double)cfg.range[c]);
    glab_s[g] = ok ? c : -1;
    gx_s[g] = b[0];
    gy_s[g] = b[1];
    if (ok) atomicAdd(&hist_s[c], 1);                                   // npos
  }
  __syncthreads();
  // rank sort: descending score, equal scores by ascending row
  for (int i = tid; i < P; i += kEvThreads) {
    if (lab_s[i] < 0) continue;
    const float si = sc_s[i];
    int rank = 0;
    for (int j = 0; j < P; ++j) {
      const float sj = sc_s[j];
      rank += (lab_s[j] >= 0 && (sj > si || (sj == si && j < i))) ? 1 : 0;
    }
    ord_s[rank] = (short)i;
    atomicAdd(&nvalid_s, 1);
  }
  __syncthreads();
  const int nv = nvalid_s;
  for (int k = tid; k < P; k += kEvThreads) {
    const size_t q = (size_t)p0 + k;
    if (k < nv) {
      const int i = ord_s[k], c = lab_s[i];
      keys[q] = ev_score_key(sc_s[i]);
      cls[q] = c;
      conf[q] = (double)sc_s[i];
      atomicAdd(&hist_s[32 + c], 1);                                    // predictions of the class
    } else {
      keys[q] = 0xffffffffu;
      cls[q] = cfg.C;                                                   // sorts behind every class
      conf[q] = 0.0;
    }
  }
  // the greedy walk, one wave per threshold; lane l owns the boxes l, l + 64, ... and their taken bits
  if (wave < cfg.T) {
    const double th = cfg.ths[wave];
    unsigned taken = 0u;
    for (int k = 0; k < nv; ++k) {
      const int i = ord_s[k], c = lab_s[i];
      const double px = (double)px_s[i], py = (double)py_s[i];
      double best = INFINITY;
      int bg = 0x7fffffff;
#pragma unroll
      for (int j = 0; j < kEvGtPerLane; ++j) {
        const int g = lane + 64 * j;
        if (64 * j >= G) break;
        if (g < G && glab_s[g] == c && !((taken >> j) & 1u)) {
          const double dx = (double)gx_s[g] - px, dy = (double)gy_s[g] - py;
          const double d2 = dx * dx + dy * dy;
          if (d2 < best) { best = d2; bg = g; }
        }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int og = __shfl_xor(bg, o, 64);
        if (ob < best || (ob == best && og < bg)) { best = ob; bg = og; }
      }
      if (bg == 0x7fffffff) continue;
      const double dist = sqrt(best);
      if (!(dist < th)) continue;
      if (lane == (bg & 63)) taken |= 1u << (bg >> 6);
      if (lane == 0) {
        atomicOr(&tpm_s[k], 1u << wave);
        if (wave == cfg.tp_index) {
          const float* gb = gboxes + ((size_t)g0 + bg) * 9;
          const float* pb = pboxes + ((size_t)p0 + i) * 9;
          double* e = errs + ((size_t)p0 + k) * ISF_EVAL_NUM_ERRS;
          e[0] = dist;
          double inter = 1.0, vg = 1.0, vp = 1.0;
          for (int a = 3; a < 6; ++a) {
            const double sg = (double)gb[a], sp = (double)pb[a];
            inter *= sg < sp ? sg : sp;
            vg *= sg;
            vp *= sp;
          }
          e[1] = 1.0 - inter / (vg + vp - inter);
          const double pi = 3.141592653589793;
          const double T = cfg.half_period[c] ? pi : 2.0 * pi;
          double m = fmod((double)gb[6] - (double)pb[6] + T / 2.0, T);
          if (m != 0.0 && m < 0.0) m += T;                              // Python's non-negative mod
          double d = m - T / 2.0;
          if (d > pi) d -= 2.0 * pi;
          e[2] = fabs(d);
          const double dvx = (double)gb[7] - (double)pb[7], dvy = (double)gb[8] - (double)pb[8];
          e[3] = sqrt(dvx * dvx + dvy * dvy);
          const int ga = gattrs ? gattrs[(size_t)g0 + bg] : -1;
          e[4] = ga < 0 ? (double)NAN : (ga == pattrs[(size_t)p0 + i] ? 0.0 : 1.0);
        }
      }
    }
  }
  __syncthreads();
  for (int k = tid; k < P; k += kEvThreads) {
    const unsigned m = k < nv ? tpm_s[k] : 0u;
    tp_mask[(size_t)p0 + k] = (uint8_t)m;
    if (k < nv) tp_mask_rows[(size_t)p0 + ord_s[k]] = (uint8_t)m;
  }
  if (tid < 2 * 32 && (tid & 31) < cfg.C && hist_s[tid]) atomicAdd(&counts[(tid >> 5) * cfg.C + (tid & 31)], hist_s[tid]);
}

// ----------------------------------------------------------------------------- stage 2: order
// (no kernel of its own: two calls of the stable sort, isf_sort.hip -- isf_eval_order below)

// ----------------------------------------------------------------------------- stage 3: curves
// inclusive scan over the workgroup's kEvThreads values; *total = their sum.  ws: kEvWaves shared entries.
template <typename T>
__device__ __forceinline__ T ev_block_scan(T v, T* ws, T* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  __syncthreads();                       // the previous round's readers are done with ws
  if (lane == 63) ws[wave] = v;
  __syncthreads();
  T pre = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kEvWaves; ++w) {
    if (w < wave) pre += ws[w];
    all += ws[w];
  }
  *total = all;
  return v + pre;
}

// curves [C][2 * T + NUM_ERRS][101]: precision of threshold t at row t, confidence at T + t, TP curve m at 2 T + m
__global__ __launch_bounds__(kEvThreads) void ev_curves_kernel(
    const int32_t* __restrict__ idx, const uint8_t* __restrict__ tp_mask, const double* __restrict__ conf,
    const double* __restrict__ errs, const int32_t* __restrict__ counts, const double* __restrict__ points, int R, int C, int T,
    int tp_index, int32_t* __restrict__ cum_tp /* [T][R] */, double* __restrict__ mconf /* [R] */,
    double* __restrict__ cmean /* [NUM_ERRS][R] */, double* __restrict__ curves) {
  __shared__ int iws[kEvWaves];
  __shared__ double dws[kEvWaves];
  __shared__ double conf_s[ISF_EVAL_POINTS];
  const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  int b = 0;
  for (int k = 0; k < c; ++k) b += counts[C + k];
  int n = counts[C + c];
  if (b > R) b = R;
  if (n > R - b) n = R - b;                                            // never past the arrays, whatever the counters hold
  const int npos = counts[c];
  int32_t* cum = cum_tp + (size_t)t * R + b;
  const int32_t* ix = idx + b;
  const int rows = 2 * T + ISF_EVAL_NUM_ERRS;
  double* prec_o = curves + ((size_t)c * rows + t) * ISF_EVAL_POINTS;
  double* conf_o = curves + ((size_t)c * rows + T + t) * ISF_EVAL_POINTS;
  double* tp_o = curves + ((size_t)c * rows + 2 * T) * ISF_EVAL_POINTS;
  int carry = 0;
  for (int base = 0; base < n; base += kEvThreads) {
    const int j = base + tid;
    const int flag = j < n ? (tp_mask[ix[j]] >> t) & 1 : 0;
    int tot;
    const int inc = ev_block_scan<int>(flag, iws, &tot) + carry;
    if (j < n) cum[j] = inc;
    carry += tot;
  }
  const int ntp = carry;
  __threadfence_block();
  __syncthreads();
  const bool empty = npos == 0 || ntp == 0;
  if (tid < ISF_EVAL_POINTS) {
    double pr = 0.0, cf = 0.0;
    if (!empty) {
      const double x = points[tid], dn = (double)npos;
      if (x < (double)cum[0] / dn) {
        pr = (double)cum[0];                                            // tp / (tp + fp) at the first row
        cf = conf[ix[0]];
      } else if (x > (double)cum[n - 1] / dn) {
        pr = 0.0;
        cf = 0.0;                                                       // right = 0
      } else {
        int lo = 0, hi = n - 1;                                         // the last j with rec[j] <= x
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if ((double)cum[mid] / dn <= x) lo = mid; else hi = mid - 1;
        }
        const int j = lo;
        const double xj = (double)cum[j] / dn;
        const double pj = (double)cum[j] / (double)(j + 1), cj = conf[ix[j]];
        if (j == n - 1 || xj == x) {
          pr = pj;
          cf = cj;
        } else {
          const double x1 = (double)cum[j + 1] / dn;
          const double p1 = (double)cum[j + 1] / (double)(j + 2), c1 = conf[ix[j + 1]];
          pr = (p1 - pj) / (x1 - xj) * (x - xj) + pj;
          cf = (c1 - cj) / (x1 - xj) * (x - xj) + cj;
        }
      }
    }
    prec_o[tid] = pr;
    conf_o[tid] = cf;
    conf_s[tid] = cf;
  }
  if (t != tp_index) return;
  if (empty) {
    for (int i = tid; i < ISF_EVAL_NUM_ERRS * ISF_EVAL_POINTS; i += kEvThreads) tp_o[i] = 1.0;
    return;
  }
  // the matches in order: confidence and the five errors
  double* mc = mconf + b;
  for (int j = tid; j < n; j += kEvThreads) {
    const int q = ix[j];
    if ((tp_mask[q] >> t) & 1) {
      const int k = cum[j] - 1;
      mc[k] = conf[q];
      for (int m = 0; m < ISF_EVAL_NUM_ERRS; ++m) cmean[(size_t)m * R + b + k] = errs[(size_t)q * ISF_EVAL_NUM_ERRS + m];
    }
  }
  __threadfence_block();
  __syncthreads();
  // cumulative means (NaN adds nothing to sum or count; 0 where the count is 0; all ones if every entry is NaN)
  for (int m = 0; m < ISF_EVAL_NUM_ERRS; ++m) {
    double* e = cmean + (size_t)m * R + b;
    double dcarry = 0.0;
    int ccarry = 0;
    for (int base = 0; base < ntp; base += kEvThreads) {
      const int k = base + tid;
      const double v = k < ntp ? e[k] : (double)NAN;
      const bool ok = v == v;
      double dt;
      int ct;
      const double ds = ev_block_scan<double>(ok ? v : 0.0, dws, &dt) + dcarry;
      const int cs = ev_block_scan<int>(ok ? 1 : 0, iws, &ct) + ccarry;
      if (k < ntp) e[k] = cs > 0 ? ds / (double)cs : 0.0;
      dcarry += dt;
      ccarry += ct;
    }
    __threadfence_block();
    __syncthreads();
    if (tid < ISF_EVAL_POINTS) {
      double r = 1.0;
      if (ccarry > 0) {
        // np.interp(confidence[::-1], match_conf[::-1], cm[::-1])[::-1]: k0 = the first match with conf <= x
        const double x = conf_s[tid];
        if (mc[ntp - 1] > x) {
          r = e[ntp - 1];                                               // below xp[0]
        } else {
          int lo = 0, hi = ntp - 1;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (mc[mid] <= x) hi = mid; else lo = mid + 1;
          }
          const int k0 = lo;
          if (k0 == 0 || mc[k0] == x) r = e[k0];
          else r = (e[k0 - 1] - e[k0]) / (mc[k0 - 1] - mc[k0]) * (x - mc[k0]) + e[k0];
        }
      }
      tp_o[m * ISF_EVAL_POINTS + tid] = r;
    }
    __syncthreads();
  }
}

// ----------------------------------------------------------------------------- stage 4: scalars
// result: ap [C][T], tp [C][NUM_ERRS], mean_dist_aps [C], max_recall_ind [C], tp_errors [5], tp_scores [5], mean_ap, nd_score
__global__ __launch_bounds__(kEvThreads) void ev_scalars_kernel(const double* __restrict__ curves, EvalCfg cfg, double min_recall,
                                                                double min_precision, double ap_weight,
                                                                double* __restrict__ result) {
  const int C = cfg.C, T = cfg.T, tid = threadIdx.x;
  const int rows = 2 * T + ISF_EVAL_NUM_ERRS;
  double* ap = result;
  double* tp = ap + C * T;
  double* mda = tp + C * ISF_EVAL_NUM_ERRS;
  double* mri = mda + C;
  double* tpe = mri + C;
  double* tps = tpe + ISF_EVAL_NUM_ERRS;
  double* tail = tps + ISF_EVAL_NUM_ERRS;
  const int first = (int)rint(100.0 * min_recall) + 1;
  for (int i = tid; i < C * T; i += kEvThreads) {
    const double* pr = curves + ((size_t)(i / T) * rows + (i % T)) * ISF_EVAL_POINTS;
    double sum = 0.0;
    for (int p = first; p < ISF_EVAL_POINTS; ++p) {
      const double v = pr[p] - min_precision;
      sum += v < 0.0 ? 0.0 : v;
    }
    ap[i] = sum / (double)(ISF_EVAL_POINTS - first) / (1.0 - min_precision);
  }
  for (int i = tid; i < C * ISF_EVAL_NUM_ERRS; i += kEvThreads) {
    const int c = i / ISF_EVAL_NUM_ERRS, m = i % ISF_EVAL_NUM_ERRS;
    const double* cf = curves + ((size_t)c * rows + T + cfg.tp_index) * ISF_EVAL_POINTS;
    const double* cu = curves + ((size_t)c * rows + 2 * T + m) * ISF_EVAL_POINTS;
    int last = 0;
    for (int p = 0; p < ISF_EVAL_POINTS; ++p)
      if (cf[p] != 0.0) last = p;
    double v = 1.0;
    if (last >= first) {
      double sum = 0.0;
      for (int p = first; p <= last; ++p) sum += cu[p];
      v = sum / (double)(last - first + 1);
    }
    if ((cfg.nan_mask[c] >> m) & 1) v = (double)NAN;
    tp[i] = v;
    if (m == 0) mri[c] = (double)last;
  }
  __threadfence_block();
  __syncthreads();
  if (tid == 0) {
    double map = 0.0;
    for (int c = 0; c < C; ++c) {
      double s = 0.0;
      for (int t = 0; t < T; ++t) s += ap[c * T + t];
      mda[c] = s / (double)T;
      map += mda[c];
    }
    map /= (double)C;
    double score_sum = 0.0;
    for (int m = 0; m < ISF_EVAL_NUM_ERRS; ++m) {
      double s = 0.0;
      int cnt = 0;
      for (int c = 0; c < C; ++c) {
        const double v = tp[c * ISF_EVAL_NUM_ERRS + m];
        if (v == v) { s += v; ++cnt; }
      }
      const double e = cnt ? s / (double)cnt : (double)NAN;
      tpe[m] = e;
      const double sc = 1.0 - e;
      tps[m] = sc < 0.0 ? 0.0 : sc;                                     // max(1 - err, 0); NaN stays NaN
      score_sum += tps[m];
    }
    tail[0] = map;
    tail[1] = (ap_weight * map + score_sum) / (ap_weight + (double)ISF_EVAL_NUM_ERRS);
  }
}

static int ev_fill_cfg(const char* who, EvalCfg* cfg, int C, const float* class_range, const int* half_period, const int* nan_mask,
                       const double* dist_ths, int T, int tp_index) {
  ISF_REQUIRE(C >= 1 && C <= ISF_EVAL_MAX_CLASSES && T >= 1 && T <= ISF_EVAL_MAX_THS && tp_index >= 0 && tp_index < T,
              ISF_ERR_ARG, "%s: %d classes (<= %d), %d thresholds (<= %d), tp index %d", who, C, ISF_EVAL_MAX_CLASSES, T,
              ISF_EVAL_MAX_THS, tp_index);
  memset(cfg, 0, sizeof(*cfg));
  cfg->C = C;
  cfg->T = T;
  cfg->tp_index = tp_index;
  for (int c = 0; c < C; ++c) {
    cfg->range[c] = class_range ? class_range[c] : 0.f;
    cfg->half_period[c] = half_period ? half_period[c] : 0;
    cfg->nan_mask[c] = nan_mask ? nan_mask[c] : 0;
  }
  for (int t = 0; t < T; ++t) cfg->ths[t] = dist_ths ? dist_ths[t] : 0.0;
  return ISF_OK;
}

}  // namespace isf

using namespace isf;

extern "C" {

int isf_eval_attributes(const int32_t* labels, const float* boxes, int box_ld, long long rows, int num_classes,
                        const int* moving_attr, const int* still_attr, int32_t* attrs, isf_stream_t stream) {
  ISF_REQUIRE(rows >= 0 && box_ld >= 9 && num_classes >= 1 && num_classes <= ISF_EVAL_MAX_CLASSES && moving_attr && still_attr,
              ISF_ERR_ARG, "isf_eval_attributes: bad arguments");
  if (rows == 0) return ISF_OK;
  ISF_REQUIRE(labels && boxes && attrs, ISF_ERR_ARG, "isf_eval_attributes: null pointer");
  AttrTable tab;
  memset(&tab, 0, sizeof(tab));
  for (int c = 0; c < num_classes; ++c) {
    tab.moving[c] = moving_attr[c];
    tab.still[c] = still_attr[c];
  }
  hipLaunchKernelGGL(ev_attr_kernel, dim3(ceil_div(rows, 256)), dim3(256), 0, as_stream(stream), labels, boxes, box_ld, rows,
                     num_classes, tab, attrs);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_eval_match(const float* pred_boxes, const float* pred_scores, const int32_t* pred_labels, const uint8_t* pred_valid,
                   const int32_t* pred_attrs, const int32_t* pred_off, int max_pred, const float* gt_boxes,
                   const int32_t* gt_labels, const int32_t* gt_attrs, const int32_t* gt_num_pts, const int32_t* gt_off,
                   int max_gt, const double* lidar2ego, int num_samples, int num_classes, const float* class_range,
                   const int* half_period, const double* dist_ths, int num_ths, int tp_index, uint32_t* keys, int32_t* cls,
                   uint8_t* tp_mask, uint8_t* tp_mask_rows, double* conf, double* errs, int32_t* counts, isf_stream_t stream) {
  EvalCfg cfg;
  ISF_TRY(ev_fill_cfg("isf_eval_match", &cfg, num_classes, class_range, half_period, nullptr, dist_ths, num_ths, tp_index));
  ISF_REQUIRE(num_samples >= 0 && class_range && half_period && dist_ths && counts, ISF_ERR_ARG, "isf_eval_match: bad arguments");
  ISF_REQUIRE(max_pred >= 0 && max_pred <= ISF_EVAL_MAX_PRED, ISF_ERR_UNSUPPORTED,
              "isf_eval_match: %d predictions in one sample; the kernel takes at most %d", max_pred, ISF_EVAL_MAX_PRED);
  ISF_REQUIRE(max_gt >= 0 && max_gt <= ISF_EVAL_MAX_GT, ISF_ERR_UNSUPPORTED,
              "isf_eval_match: %d ground-truth boxes in one sample; the kernel takes at most %d", max_gt, ISF_EVAL_MAX_GT);
  hipStream_t st = as_stream(stream);
  ISF_HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int32_t) * 2 * num_classes, st));
  if (num_samples == 0) return ISF_OK;
  ISF_REQUIRE(pred_off && gt_off && lidar2ego && keys && cls && tp_mask && tp_mask_rows && conf && errs, ISF_ERR_ARG,
              "isf_eval_match: null pointer");
  ISF_REQUIRE((max_pred == 0 || (pred_boxes && pred_scores && pred_labels && pred_valid && pred_attrs)) &&
                  (max_gt == 0 || (gt_boxes && gt_labels)),
              ISF_ERR_ARG, "isf_eval_match: null rows");
  hipLaunchKernelGGL(ev_match_kernel, dim3(num_samples), dim3(kEvThreads), 0, st, pred_boxes, pred_scores, pred_labels,
                     pred_valid, pred_attrs, pred_off, gt_boxes, gt_labels, gt_attrs, gt_num_pts, gt_off, lidar2ego, cfg, keys,
                     cls, tp_mask, tp_mask_rows, conf, errs, counts);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_eval_order(const uint32_t* keys, const int32_t* cls, int rows, int num_classes, int32_t* order, isf_stream_t stream) {
  ISF_REQUIRE(rows >= 0 && num_classes >= 1 && num_classes <= ISF_EVAL_MAX_CLASSES, ISF_ERR_ARG, "isf_eval_order: bad arguments");
  if (rows == 0) return ISF_OK;
  ISF_REQUIRE(keys && cls && order, ISF_ERR_ARG, "isf_eval_order: null pointer");
  hipStream_t st = as_stream(stream);
  Arena& a = arena_for_stream(st);
  ISF_TRY(a.reset());
  int* by_score = nullptr;
  ISF_TRY(a.alloc_n(&by_score, (size_t)rows));
  // LSD: the score digits first, the class (5 bits: num_classes = "dropped row") after them; both sorts stable
  ISF_TRY(stable_sort_u32_impl(a, keys, rows, 32, by_score, st));
  return stable_sort_u32_impl(a, reinterpret_cast<const uint32_t*>(cls), rows, 5, order, st, nullptr, by_score);
}

int isf_eval_curves(const int32_t* order, const uint8_t* tp_mask, const double* conf, const double* errs, const int32_t* counts,
                    const double* recall_points, int rows, int num_classes, int num_ths, int tp_index, double* curves,
                    isf_stream_t stream) {
  ISF_REQUIRE(rows >= 0 && num_classes >= 1 && num_classes <= ISF_EVAL_MAX_CLASSES && num_ths >= 1 && num_ths <= ISF_EVAL_MAX_THS &&
                  tp_index >= 0 && tp_index < num_ths && counts && recall_points && curves,
              ISF_ERR_ARG, "isf_eval_curves: bad arguments");
  ISF_REQUIRE(rows == 0 || (order && tp_mask && conf && errs), ISF_ERR_ARG, "isf_eval_curves: null pointer");
  hipStream_t st = as_stream(stream);
  Arena& a = arena_for_stream(st);
  ISF_TRY(a.reset());
  int32_t* cum = nullptr;
  double *mconf = nullptr, *cmean = nullptr;
  const size_t r = (size_t)(rows > 0 ? rows : 1);
  ISF_TRY(a.alloc_n(&cum, r * num_ths));
  ISF_TRY(a.alloc_n(&mconf, r));
  ISF_TRY(a.alloc_n(&cmean, r * ISF_EVAL_NUM_ERRS));
  hipLaunchKernelGGL(ev_curves_kernel, dim3(num_classes, num_ths), dim3(kEvThreads), 0, st, order, tp_mask, conf, errs, counts,
                     recall_points, rows, num_classes, num_ths, tp_index, cum, mconf, cmean, curves);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_eval_scalars(const double* curves, int num_classes, int num_ths, int tp_index, const int* nan_mask, double min_recall,
                     double min_precision, double mean_ap_weight, double* result, isf_stream_t stream) {
  EvalCfg cfg;
  ISF_TRY(ev_fill_cfg("isf_eval_scalars", &cfg, num_classes, nullptr, nullptr, nan_mask, nullptr, num_ths, tp_index));
  ISF_REQUIRE(curves && result && nan_mask && min_recall >= 0.0 && min_recall < 1.0 && min_precision >= 0.0 && min_precision < 1.0,
              ISF_ERR_ARG, "isf_eval_scalars: bad arguments");
  hipLaunchKernelGGL(ev_scalars_kernel, dim3(1), dim3(kEvThreads), 0, as_stream(stream), curves, cfg, min_recall, min_precision,
                     mean_ap_weight, result);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

}  // extern "C"
