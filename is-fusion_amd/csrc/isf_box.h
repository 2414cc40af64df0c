// isf_box.h -- TransFusionBBoxCoder.decode of one proposal (core/bbox/coders/transfusion_bbox_coder.py:63-74), shared by
// the inference decode (isf_decode.hip) and the training-time assignment cost (isf_head_loss.hip): one formula in one
// place.  The two translation units compile it under different floating-point contraction settings (isf_head_loss.hip
// turns FMA contraction off), so the boxes they decode can differ in the last bit of x / y.  Inputs are the head's
// [B, k, ld] outputs of one sample; box = x, y, z_bottom, dx, dy, dz, yaw (, vx, vy).
#pragma once
#include <hip/hip_runtime.h>

namespace isf {

__device__ __forceinline__ void decode_box(const float* __restrict__ center, const float* __restrict__ height,
                                           const float* __restrict__ dim, const float* __restrict__ rot,
                                           const float* __restrict__ vel, int ld, int p, float cell_x, float cell_y,
                                           float org_x, float org_y, float box[9]) {
  box[0] = center[p] * cell_x + org_x;
  box[1] = center[ld + p] * cell_y + org_y;
  box[3] = expf(dim[p]);
  box[4] = expf(dim[ld + p]);
  box[5] = expf(dim[2 * ld + p]);
  box[2] = height[p] - box[5] * 0.5f;   // gravity centre -> bottom centre
  box[6] = atan2f(rot[p], rot[ld + p]);
  if (vel) {
    box[7] = vel[p];
    box[8] = vel[ld + p];
  }
}

}  // namespace isf
