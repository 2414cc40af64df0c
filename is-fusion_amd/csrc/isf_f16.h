// isf_f16.h -- what the f16 inference mode of the camera backbone shares between its units (isf_swin.hip,
// isf_swin_f16.hip): the f16 vector types and the saturating store conversion.
#pragma once

namespace isf {

typedef _Float16 fh4 __attribute__((ext_vector_type(4)));
typedef _Float16 fh8 __attribute__((ext_vector_type(8)));

// fp32 -> f16 for every value that is STORED as f16 (activation rows, packed weights, the padded cells' bias): round
// to nearest, saturating at +-65504 instead of producing inf.  NaN stays NaN (both comparisons are false).
__device__ __forceinline__ _Float16 sat_f16(float z) {
  z = z > 65504.f ? 65504.f : (z < -65504.f ? -65504.f : z);
  return (_Float16)z;
}

}  // namespace isf
