// isf_bev.h -- rotated bird's-eye-view overlap of two boxes, shared by the training-time IoU cost (isf_head_loss.hip)
// and the rotated NMS / boxes_iou_bev (isf_nms.hip): one formula in one place.
//
// Semantics of boxes_overlap_bev_gpu / iou_bev (mmdet3d/ops/iou3d/src/iou3d_kernel.cu) on xyxyr boxes: corner
// (x1,y1)..(x1,y2) of the axis-aligned box, each turned about the centre by (dx cos a + dy sin a, -dx sin a + dy cos a).
// Computed here as a convex clip (Sutherland-Hodgman) in fp64.  Every function body turns FMA contraction off itself, so
// both translation units get bit-identical results whatever their own setting.
#pragma once
#include <hip/hip_runtime.h>

namespace isf {

struct Poly {
  double x[16], y[16];
  int n;
};

// xywhr2xyxyr (core/bbox/structures/utils.py:66-84) of a LiDAR box row (x, y, z, dx, dy, dz, yaw, ...) in float32
__device__ inline void bev_xyxyr(const float* box, float r[5]) {
#pragma clang fp contract(off)
  const float hw = box[3] / 2.f, hl = box[4] / 2.f;
  r[0] = box[0] - hw;
  r[1] = box[1] - hl;
  r[2] = box[0] + hw;
  r[3] = box[1] + hl;
  r[4] = box[6];
}

// the four corners of an xyxyr box, turned about its centre as the reference's kernel does
__device__ inline void bev_corners_xyxyr(const float* r, double* px, double* py) {
#pragma clang fp contract(off)
  const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
  const double cx = ((double)x1 + x2) / 2.0, cy = ((double)y1 + y2) / 2.0;
  const double ca = cos((double)r[4]), sa = sin((double)r[4]);
  const double xs[4] = {x1, x2, x2, x1}, ys[4] = {y1, y1, y2, y2};
  for (int k = 0; k < 4; ++k) {
    const double dx = xs[k] - cx, dy = ys[k] - cy;
    px[k] = dx * ca + dy * sa + cx;
    py[k] = -dx * sa + dy * ca + cy;
  }
}

__device__ inline void bev_corners(const float* box, double* px, double* py) {
  float r[5];
  bev_xyxyr(box, r);
  bev_corners_xyxyr(r, px, py);
}

// overlap area of two convex quadrilaterals given by their corners
__device__ inline double bev_overlap_corners(const double* ax, const double* ay, const double* bx, const double* by) {
#pragma clang fp contract(off)
  // orientation of the clipping polygon (a mirror image only flips the sign)
  double sb = 0.0;
  for (int k = 0; k < 4; ++k) sb += bx[k] * by[(k + 1) & 3] - bx[(k + 1) & 3] * by[k];
  if (!(fabs(sb) > 0.0)) return 0.0;
  const double orient = sb > 0.0 ? 1.0 : -1.0;
  Poly cur, nxt;
  cur.n = 4;
  for (int k = 0; k < 4; ++k) { cur.x[k] = ax[k]; cur.y[k] = ay[k]; }
  for (int e = 0; e < 4 && cur.n > 0; ++e) {
    const double ex0 = bx[e], ey0 = by[e], ex1 = bx[(e + 1) & 3], ey1 = by[(e + 1) & 3];
    const double ux = ex1 - ex0, uy = ey1 - ey0;
    nxt.n = 0;
    for (int k = 0; k < cur.n; ++k) {
      const int k1 = (k + 1) % cur.n;
      const double s0 = orient * (ux * (cur.y[k] - ey0) - uy * (cur.x[k] - ex0));
      const double s1 = orient * (ux * (cur.y[k1] - ey0) - uy * (cur.x[k1] - ex0));
      if (s0 >= 0.0 && nxt.n < 16) { nxt.x[nxt.n] = cur.x[k]; nxt.y[nxt.n] = cur.y[k]; ++nxt.n; }
      if ((s0 >= 0.0) != (s1 >= 0.0) && nxt.n < 16) {
        const double t = s0 / (s0 - s1);
        nxt.x[nxt.n] = cur.x[k] + t * (cur.x[k1] - cur.x[k]);
        nxt.y[nxt.n] = cur.y[k] + t * (cur.y[k1] - cur.y[k]);
        ++nxt.n;
      }
    }
    cur = nxt;
  }
  double area = 0.0;
  for (int k = 0; k < cur.n; ++k) {
    const int k1 = (k + 1) % cur.n;
    area += cur.x[k] * cur.y[k1] - cur.x[k1] * cur.y[k];
  }
  return fabs(area) / 2.0;
}

// overlap of two LiDAR box rows (x, y, z, dx, dy, dz, yaw, ...)
__device__ inline double bev_overlap(const float* a, const float* b) {
  double ax[4], ay[4], bx[4], by[4];
  bev_corners(a, ax, ay);
  bev_corners(b, bx, by);
  return bev_overlap_corners(ax, ay, bx, by);
}

}  // namespace isf
