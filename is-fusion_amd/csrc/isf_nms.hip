// isf_nms.hip -- BEV NMS of the detection head's post-processing and of the test-time-augmentation merge:
// rotated / axis-aligned / circle NMS over many independent segments in one launch, the M x N rotated BEV IoU, and the
// flip / scale map-back of augmented boxes.
//
// The reference runs these on the host or with host round trips: circle_nms is a numba loop over a .cpu().numpy() copy
// (core/post_processing/box3d_nms.py:183-218), nms_gpu / nms_normal_gpu sort on the device but copy the keep list back
// (ops/iou3d/iou3d_utils.py:26-77), and the callers loop over tasks / classes in Python with boolean-mask indexing
// (dense_heads/transfusion_head_v2.py:1344-1403, core/post_processing/merge_augs.py:8-101).  Here:
//
//   segmented NMS   one workgroup per segment = (group, task).  A group is a block of `group_stride` rows of which the
//                   first counts[g] (a DEVICE count, e.g. isf_decode_boxes's) are valid; a row belongs to task
//                   task_of_class[label].  The workgroup gathers its rows in input order, ranks them by score (ties:
//                   lower input index first), applies pre_maxsize, builds the suppression mask (64-bit words, one wave
//                   ballot per word, as the reference's nms_kernel), and one wave sweeps it greedily; then post_max_size.
//                   No host sync, no allocation: the mask lives in a caller-supplied scratch buffer.
//   boxes_iou_bev   one thread per pair, fp64 overlap (isf_bev.h)
//   map-back        one thread per row: LiDARInstance3DBoxes.flip + BaseInstance3DBoxes.scale per view
#include "isf_common.h"
#include "isf_bev.h"

// the fp32 comparisons below restate the reference's float32 arithmetic: keep every product and sum separately rounded
#pragma clang fp contract(off)

namespace isf {
namespace {

constexpr int kSeg = ISF_NMS_MAX_SEGMENT;   // rows of one segment (and of one group)
constexpr int kWords = kSeg / 64;           // mask words per row
constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;

struct NmsTasks {
  int num_classes, num_tasks;
  int task_of_class[ISF_NMS_MAX_CLASSES];
  int mode[ISF_NMS_MAX_TASKS];
  float thr[ISF_NMS_MAX_TASKS];
};

__device__ __forceinline__ int task_of(const NmsTasks& t, const int32_t* labels, size_t row) {
  if (!labels) return 0;
  const int c = labels[row];
  return (c >= 0 && c < t.num_classes) ? t.task_of_class[c] : -1;
}

// iou_normal (iou3d_kernel.cu:335-343) in float32
__device__ __forceinline__ float iou_normal(const float* a, const float* b) {
  const float left = fmaxf(a[0], b[0]), right = fminf(a[2], b[2]);
  const float top = fmaxf(a[1], b[1]), bottom = fminf(a[3], b[3]);
  const float width = fmaxf(right - left, 0.f), height = fmaxf(bottom - top, 0.f);
  const float inter = width * height;
  const float sa = (a[2] - a[0]) * (a[3] - a[1]);
  const float sb = (b[2] - b[0]) * (b[3] - b[1]);
  return inter / fmaxf(sa + sb - inter, 1e-8f);
}

// iou_bev (iou3d_kernel.cu:243-251): areas from the xyxy corners in float32, the overlap in fp64
__device__ __forceinline__ double iou_rotated(double overlap, float area_a, float area_b) {
  return overlap / fmax((double)area_a + (double)area_b - overlap, 1e-8);
}

__device__ __forceinline__ void load_xyxyr(const float* box, int box_format, float r[5]) {
  if (box_format == ISF_NMS_BOX_LIDAR) {
    bev_xyxyr(box, r);
  } else {
    for (int k = 0; k < 5; ++k) r[k] = box[k];
  }
}

__global__ __launch_bounds__(kThreads) void nms_segmented_kernel(
    const float* __restrict__ boxes, int box_ld, int box_format, const float* __restrict__ scores,
    const int32_t* __restrict__ labels, const int32_t* __restrict__ counts, int group_stride, NmsTasks tasks,
    int pre_maxsize, int post_max_size, int mask_rows, unsigned long long* __restrict__ mask,
    uint8_t* __restrict__ keep, int32_t* __restrict__ keep_index, int32_t* __restrict__ keep_count) {
  __shared__ int s_row[kSeg];        // members, in input order (row inside the group)
  __shared__ float s_score[kSeg];
  __shared__ int s_sorted[kSeg];     // sorted position -> member
  __shared__ double s_geo[kSeg * 8]; // per sorted position: rotate = 4 corners; normal = xyxy (float); circle = xy
  __shared__ float s_area[kSeg];     // rotate: area from the xyxy corners
  __shared__ float s_circ[kSeg * 3]; // rotate: centre and bounding radius (the exact-zero overlap test)
  __shared__ int s_kept[kSeg];       // sorted positions kept, in kept order
  __shared__ uint8_t s_flag[kSeg];
  __shared__ int s_wave[kWaves];
  __shared__ int s_nkept;

  const int T = tasks.num_tasks;
  const int seg = blockIdx.x, g = seg / T, t = seg % T;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mode = tasks.mode[t];
  const float thr = tasks.thr[t];
  const size_t base = (size_t)g * group_stride;
  int count = counts ? counts[g] : group_stride;
  count = count < 0 ? 0 : (count > group_stride ? group_stride : count);

  // rows of this group that no task owns (and the rows past the count) are written by the task-0 workgroup only
  if (t == 0) {
    for (int r = tid; r < group_stride; r += kThreads)
      if (r >= count || task_of(tasks, labels, base + r) < 0) keep[base + r] = 0;
  }

  // 1. gather the segment's rows in input order
  int n = 0;
  for (int r0 = 0; r0 < count; r0 += kThreads) {
    const int r = r0 + tid;
    const bool mine = r < count && task_of(tasks, labels, base + r) == t;
    const unsigned long long bal = __ballot(mine);
    if (lane == 0) s_wave[wave] = __popcll(bal);
    __syncthreads();
    int at = n;
    for (int w = 0; w < wave; ++w) at += s_wave[w];
    int total = 0;
    for (int w = 0; w < kWaves; ++w) total += s_wave[w];
    if (mine) {
      at += __popcll(bal & ((1ull << lane) - 1ull));
      s_row[at] = r;
      s_score[at] = scores[base + r];
    }
    n += total;
    __syncthreads();
  }
  int32_t* out_idx = keep_index + (size_t)seg * group_stride;

  if (mode == ISF_NMS_KEEP) {   // a task without NMS (radius <= 0): every row, in input order
    for (int k = tid; k < n; k += kThreads) {
      out_idx[k] = (int32_t)(base + s_row[k]);
      keep[base + s_row[k]] = 1;
    }
    if (tid == 0) keep_count[seg] = n;
    return;
  }

  // 2. rank by score, descending; equal scores keep their input order.  (The reference's torch.sort / np.argsort are
  // not stable, so its order among equal scores is undefined; this is one fixed choice.)
  for (int i = tid; i < n; i += kThreads) s_score[i] = isnan(s_score[i]) ? -INFINITY : s_score[i];  // a total order
  __syncthreads();
  for (int i = tid; i < n; i += kThreads) {
    const float si = s_score[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const float sj = s_score[j];
      rank += (sj > si) || (sj == si && j < i);
    }
    s_sorted[rank] = i;
  }
  __syncthreads();
  const int m = pre_maxsize >= 0 && pre_maxsize < n ? pre_maxsize : n;

  // 3. geometry of the m candidates, in sorted order
  float* geo_f = reinterpret_cast<float*>(s_geo);
  for (int p = tid; p < m; p += kThreads) {
    const float* box = boxes + (base + s_row[s_sorted[p]]) * box_ld;
    if (mode == ISF_NMS_CIRCLE) {
      geo_f[2 * p] = box[0];
      geo_f[2 * p + 1] = box[1];
    } else {
      float r[5];
      load_xyxyr(box, box_format, r);
      if (mode == ISF_NMS_NORMAL) {
        for (int k = 0; k < 4; ++k) geo_f[4 * p + k] = r[k];
      } else {
        bev_corners_xyxyr(r, s_geo + 8 * p, s_geo + 8 * p + 4);
        s_area[p] = (r[2] - r[0]) * (r[3] - r[1]);
        const float w = r[2] - r[0], h = r[3] - r[1];
        s_circ[3 * p] = 0.5f * (r[0] + r[2]);
        s_circ[3 * p + 1] = 0.5f * (r[1] + r[3]);
        s_circ[3 * p + 2] = 0.5f * sqrtf(w * w + h * h);
      }
    }
  }
  __syncthreads();

  // 4. suppression mask: row i, word w = bit (j - 64 w) set when sorted box j > i is suppressed by box i.  One wave per
  // (row, word), one lane per j, the word from a ballot.
  const int W = (m + 63) >> 6;
  unsigned long long* seg_mask = mask + (size_t)seg * mask_rows * kWords;
  for (int task = wave; task < m * W; task += kWaves) {
    const int i = task / W, w = task % W;
    const int j = w * 64 + lane;
    bool sup = false;
    if (j > i && j < m) {
      if (mode == ISF_NMS_CIRCLE) {
        // circle_nms: suppressed when the SQUARED centre distance is <= thr.  The reference passes the radius as thr
        // (transfusion_head_v2.py:1365-1370), so a radius of 0.175 m acts as a distance of sqrt(0.175); kept as is.
        const float dx = geo_f[2 * i] - geo_f[2 * j], dy = geo_f[2 * i + 1] - geo_f[2 * j + 1];
        sup = dx * dx + dy * dy <= thr;
      } else if (mode == ISF_NMS_NORMAL) {
        sup = iou_normal(geo_f + 4 * i, geo_f + 4 * j) > thr;
      } else {
        // bounding circles apart by more than rounding: the overlap is 0, so is the IoU, and 0 > thr is false
        const float dx = s_circ[3 * i] - s_circ[3 * j], dy = s_circ[3 * i + 1] - s_circ[3 * j + 1];
        const double rr = (double)s_circ[3 * i + 2] + s_circ[3 * j + 2] + 1e-3;   // 1 mm >> the float rounding
        const bool apart = thr >= 0.f && (double)dx * dx + (double)dy * dy > rr * rr;
        if (!apart) {
          const double ov = bev_overlap_corners(s_geo + 8 * i, s_geo + 8 * i + 4, s_geo + 8 * j, s_geo + 8 * j + 4);
          sup = iou_rotated(ov, s_area[i], s_area[j]) > (double)thr;
        }
      }
    }
    const unsigned long long word = __ballot(sup);
    if (lane == 0) seg_mask[(size_t)i * kWords + w] = word;
  }
  __syncthreads();   // the mask words are global: the barrier's fence makes them visible to wave 0

  // 5. greedy sweep (one wave): block of 64 sorted positions at a time, lane l holding row blk*64+l's words
  if (wave == 0) {
    const int cap = post_max_size >= 0 ? post_max_size : m;
    unsigned long long removed[kWords];
#pragma unroll
    for (int w = 0; w < kWords; ++w) removed[w] = 0ull;
    int nk = 0;
    for (int blk = 0; blk < W && nk < cap; ++blk) {
      const int i_l = blk * 64 + lane;
      unsigned long long rw[kWords];
#pragma unroll
      for (int w = 0; w < kWords; ++w)
        rw[w] = (w < W && w >= blk && i_l < m) ? seg_mask[(size_t)i_l * kWords + w] : 0ull;
      unsigned long long cur = 0ull;
#pragma unroll
      for (int w = 0; w < kWords; ++w)
        if (w == blk) cur = removed[w];
      const int kend = min(64, m - blk * 64);
      for (int k = 0; k < kend && nk < cap; ++k) {
        if ((cur >> k) & 1ull) continue;
        if (lane == 0) s_kept[nk] = blk * 64 + k;
        ++nk;
#pragma unroll
        for (int w = 0; w < kWords; ++w) {
          if (w < W && w >= blk) {
            const unsigned long long v = __shfl(rw[w], k);
            removed[w] |= v;
            if (w == blk) cur |= v;
          }
        }
      }
    }
    if (lane == 0) s_nkept = nk;
  }
  for (int k = tid; k < n; k += kThreads) s_flag[k] = 0;
  __syncthreads();

  // 6. outputs: kept rows in kept order, the keep flags of every member, the count
  const int nk = s_nkept;
  for (int q = tid; q < nk; q += kThreads) {
    const int member = s_sorted[s_kept[q]];
    out_idx[q] = (int32_t)(base + s_row[member]);
    s_flag[member] = 1;
  }
  __syncthreads();
  for (int k = tid; k < n; k += kThreads) keep[base + s_row[k]] = s_flag[k];
  if (tid == 0) keep_count[seg] = nk;
}

__global__ void boxes_iou_bev_kernel(const float* __restrict__ a, int M, const float* __restrict__ b, int N,
                                     float* __restrict__ out) {
  const int j = blockIdx.x * 16 + threadIdx.x, i = blockIdx.y * 16 + threadIdx.y;
  if (i >= M || j >= N) return;
  const float* ra = a + (size_t)i * 5;
  const float* rb = b + (size_t)j * 5;
  double ax[4], ay[4], bx[4], by[4];
  bev_corners_xyxyr(ra, ax, ay);
  bev_corners_xyxyr(rb, bx, by);
  const double ov = bev_overlap_corners(ax, ay, bx, by);
  const float sa = (ra[2] - ra[0]) * (ra[3] - ra[1]), sb = (rb[2] - rb[0]) * (rb[3] - rb[1]);
  out[(size_t)i * N + j] = (float)iou_rotated(ov, sa, sb);
}

struct ViewFlags {
  int horizontal[ISF_NMS_MAX_VIEWS], vertical[ISF_NMS_MAX_VIEWS];
  float inv_scale[ISF_NMS_MAX_VIEWS];
};

// bbox3d_mapping_back (core/bbox/transforms.py:5-24) of rows [v * view_stride, v * view_stride + counts[v]):
// LiDARInstance3DBoxes.flip (lidar_box3d.py:185-192) -- horizontal: columns 1::7 negated (y, vy), yaw -> pi - yaw;
// vertical: columns 0::7 negated (x, vx), yaw -> -yaw -- then BaseInstance3DBoxes.scale(1 / factor) (base_box3d.py:
// 216-223): columns 0-5 and 7+ multiplied, yaw untouched.  1 / factor is rounded to float32 on the host, as torch's
// in-place multiply of a float32 tensor by a Python float does.
__global__ void mapping_back_kernel(float* __restrict__ boxes, int box_ld, int num_views, int view_stride,
                                    const int32_t* __restrict__ counts, ViewFlags f) {
  const int v = blockIdx.y, r = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= num_views || r >= view_stride) return;
  if (counts && r >= counts[v]) return;
  float* box = boxes + ((size_t)v * view_stride + r) * box_ld;
  const float kPi = 3.14159265358979323846f;
  if (f.horizontal[v]) {
    for (int c = 1; c < box_ld; c += 7) box[c] = -box[c];
    box[6] = -box[6] + kPi;
  }
  if (f.vertical[v]) {
    for (int c = 0; c < box_ld; c += 7) box[c] = -box[c];
    box[6] = -box[6];
  }
  const float s = f.inv_scale[v];
  for (int c = 0; c < box_ld; ++c)
    if (c != 6) box[c] = box[c] * s;
}

}  // namespace
}  // namespace isf

extern "C" {

size_t isf_nms_workspace_size(int num_groups, int group_stride, int num_tasks, int pre_maxsize) {
  if (num_groups <= 0 || group_stride <= 0 || num_tasks <= 0) return 0;
  const int rows = pre_maxsize >= 0 && pre_maxsize < group_stride ? pre_maxsize : group_stride;
  return (size_t)num_groups * num_tasks * (rows > 0 ? rows : 1) * ISF_NMS_MAX_SEGMENT / 64 * sizeof(unsigned long long);
}

int isf_nms_segmented(const float* boxes, int box_ld, int box_format, const float* scores, const int32_t* labels,
                      const int32_t* counts, int num_groups, int group_stride, int num_classes,
                      const int* task_of_class, int num_tasks, const int* task_mode, const float* task_thr,
                      int pre_maxsize, int post_max_size, void* workspace, size_t workspace_bytes, uint8_t* keep,
                      int32_t* keep_index, int32_t* keep_count, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num_groups >= 0 && group_stride >= 0, ISF_ERR_ARG, "nms_segmented: bad sizes (groups %d, stride %d)",
              num_groups, group_stride);
  ISF_REQUIRE(group_stride <= ISF_NMS_MAX_SEGMENT, ISF_ERR_UNSUPPORTED,
              "nms_segmented: %d rows per group, at most %d are supported", group_stride, ISF_NMS_MAX_SEGMENT);
  ISF_REQUIRE(num_tasks >= 1 && num_tasks <= ISF_NMS_MAX_TASKS && task_mode && task_thr, ISF_ERR_ARG,
              "nms_segmented: %d tasks (1..%d) with mode / threshold arrays", num_tasks, ISF_NMS_MAX_TASKS);
  ISF_REQUIRE(!labels || (num_classes >= 1 && num_classes <= ISF_NMS_MAX_CLASSES && task_of_class), ISF_ERR_ARG,
              "nms_segmented: %d classes (1..%d) with a task table", num_classes, ISF_NMS_MAX_CLASSES);
  ISF_REQUIRE(box_format == ISF_NMS_BOX_XYXYR || box_format == ISF_NMS_BOX_LIDAR, ISF_ERR_ARG,
              "nms_segmented: box format %d", box_format);
  ISF_REQUIRE(box_ld >= (box_format == ISF_NMS_BOX_LIDAR ? 7 : 5) ||
                  (box_ld >= 2 && num_tasks == 1 && task_mode[0] == ISF_NMS_CIRCLE),
              ISF_ERR_ARG, "nms_segmented: %d box columns", box_ld);
  if (num_groups == 0 || group_stride == 0) return ISF_OK;
  ISF_REQUIRE(boxes && scores && keep && keep_index && keep_count, ISF_ERR_ARG, "nms_segmented: null pointer");
  NmsTasks t;
  memset(&t, 0, sizeof(t));
  t.num_tasks = num_tasks;
  t.num_classes = labels ? num_classes : 0;
  for (int c = 0; c < t.num_classes; ++c) {
    ISF_REQUIRE(task_of_class[c] >= -1 && task_of_class[c] < num_tasks, ISF_ERR_ARG,
                "nms_segmented: class %d -> task %d", c, task_of_class[c]);
    t.task_of_class[c] = task_of_class[c];
  }
  bool any_nms = false;
  for (int k = 0; k < num_tasks; ++k) {
    ISF_REQUIRE(task_mode[k] >= ISF_NMS_KEEP && task_mode[k] <= ISF_NMS_CIRCLE, ISF_ERR_ARG,
                "nms_segmented: task %d mode %d", k, task_mode[k]);
    t.mode[k] = task_mode[k];
    t.thr[k] = task_thr[k];
    any_nms = any_nms || task_mode[k] != ISF_NMS_KEEP;
  }
  const int rows = pre_maxsize >= 0 && pre_maxsize < group_stride ? pre_maxsize : group_stride;
  const size_t need = isf_nms_workspace_size(num_groups, group_stride, num_tasks, pre_maxsize);
  ISF_REQUIRE(!any_nms || (workspace && workspace_bytes >= need), ISF_ERR_ARG,
              "nms_segmented: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  const unsigned grid = (unsigned)num_groups * (unsigned)num_tasks;
  hipLaunchKernelGGL(nms_segmented_kernel, dim3(grid), dim3(kThreads), 0, as_stream(stream), boxes, box_ld,
                     box_format, scores, labels, counts, group_stride, t, pre_maxsize, post_max_size,
                     rows > 0 ? rows : 1, static_cast<unsigned long long*>(workspace), keep, keep_index, keep_count);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_boxes_iou_bev(const float* boxes_a, int num_a, const float* boxes_b, int num_b, float* iou,
                      isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num_a >= 0 && num_b >= 0, ISF_ERR_ARG, "boxes_iou_bev: bad sizes (%d, %d)", num_a, num_b);
  if (num_a == 0 || num_b == 0) return ISF_OK;
  ISF_REQUIRE(boxes_a && boxes_b && iou, ISF_ERR_ARG, "boxes_iou_bev: null pointer");
  hipLaunchKernelGGL(boxes_iou_bev_kernel, dim3((num_b + 15) / 16, (num_a + 15) / 16), dim3(16, 16), 0,
                     as_stream(stream), boxes_a, num_a, boxes_b, num_b, iou);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_bbox_mapping_back(float* boxes, int box_ld, int num_views, int view_stride, const int32_t* counts,
                          const int* horizontal, const int* vertical, const float* scale_factor, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num_views >= 0 && num_views <= ISF_NMS_MAX_VIEWS && view_stride >= 0 && box_ld >= 7, ISF_ERR_ARG,
              "bbox_mapping_back: bad sizes (views %d of at most %d, stride %d, %d columns)", num_views,
              ISF_NMS_MAX_VIEWS, view_stride, box_ld);
  if (num_views == 0 || view_stride == 0) return ISF_OK;
  ISF_REQUIRE(boxes && horizontal && vertical && scale_factor, ISF_ERR_ARG, "bbox_mapping_back: null pointer");
  ViewFlags f;
  memset(&f, 0, sizeof(f));
  for (int v = 0; v < num_views; ++v) {
    ISF_REQUIRE(scale_factor[v] != 0.f, ISF_ERR_ARG, "bbox_mapping_back: scale factor 0");
    f.horizontal[v] = horizontal[v] != 0;
    f.vertical[v] = vertical[v] != 0;
    f.inv_scale[v] = (float)(1.0 / (double)scale_factor[v]);
  }
  hipLaunchKernelGGL(mapping_back_kernel, dim3((view_stride + 255) / 256, num_views), dim3(256), 0, as_stream(stream),
                     boxes, box_ld, num_views, view_stride, counts, f);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

}  // extern "C"
