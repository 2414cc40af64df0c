// isf_fixed.hip -- the passes around a fixed-point accumulation (isf_fixed.h): bound, exponent, conversion back.
#include <math.h>

#include "isf_fixed.h"

namespace isf {

// integer max on the bit pattern of |x|: order-free, and a NaN (pattern above inf's) wins instead of being dropped
__global__ __launch_bounds__(256) void fixed_absmax_kernel(const float* __restrict__ x, size_t n, unsigned* __restrict__ out) {
  unsigned m = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    m = max(m, __float_as_uint(x[i]) & 0x7fffffffu);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, d, 64));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

__global__ void fixed_ctl_kernel(const unsigned* __restrict__ bits, int nfac, unsigned clamp_mask, int extra_ex, int log2n,
                                 FixedCtl* __restrict__ ctl) {
  if (threadIdx.x || blockIdx.x) return;
  int ex = extra_ex, bad = 0;
  for (int f = 0; f < nfac; ++f) {
    const unsigned b = bits[f];
    if (b >= 0x7f800000u) { bad = 1; continue; }
    int k = 0;
    frexpf(__uint_as_float(b), &k);          // |x| < 2^k (0 -> k = 0)
    if ((clamp_mask >> f) & 1) k = max(k, 0);
    ex += k;
  }
  ctl->e = 62 - log2n - ex;
  ctl->nonfinite = bad;
}

__global__ __launch_bounds__(256) void fixed_finish_kernel(const unsigned long long* __restrict__ acc,
                                                           const FixedCtl* __restrict__ ctl, size_t n, float* __restrict__ out,
                                                           int accumulate, const int32_t* __restrict__ count, int C) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float v;
  if (ctl->nonfinite) {
    v = __uint_as_float(0x7fc00000u);
  } else {
    v = (float)ldexp((double)(long long)acc[i], -ctl->e);
    if (count) v = __fdiv_rn(v, (float)count[i / C]);
    if (accumulate) v = out[i] + v;
  }
  out[i] = v;
}

__global__ __launch_bounds__(256) void fixed_poison_kernel(float* __restrict__ p, size_t n, const FixedCtl* __restrict__ ctl) {
  if (!ctl->nonfinite) return;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = __uint_as_float(0x7fc00000u);
}

int fixed_ctl_begin(Arena& a, unsigned** bits, FixedCtl** ctl, int num_ctl, hipStream_t st) {
  ISF_TRY(a.alloc_n(bits, 64));
  ISF_TRY(a.alloc_n(ctl, (size_t)num_ctl));
  ISF_HIP_TRY(hipMemsetAsync(*bits, 0, 4 * sizeof(unsigned), st));
  return ISF_OK;
}

int fixed_absmax(const float* x, size_t n, unsigned* bits_slot, hipStream_t st) {
  if (n == 0) return ISF_OK;
  const int nb = (int)std::min<size_t>(512, (n + 1023) / 1024);
  hipLaunchKernelGGL(fixed_absmax_kernel, dim3(nb), dim3(256), 0, st, x, n, bits_slot);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int fixed_ctl(const unsigned* bits, int nfac, unsigned clamp_mask, int extra_ex, int log2n, FixedCtl* ctl, hipStream_t st) {
  hipLaunchKernelGGL(fixed_ctl_kernel, dim3(1), dim3(64), 0, st, bits, nfac, clamp_mask, extra_ex, log2n, ctl);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int fixed_finish(const unsigned long long* acc, const FixedCtl* ctl, size_t n, float* out, bool accumulate,
                 const int32_t* count, int C, hipStream_t st) {
  if (n == 0) return ISF_OK;
  hipLaunchKernelGGL(fixed_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, acc, ctl, n, out,
                     accumulate ? 1 : 0, count, C);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int fixed_poison(float* p, size_t n, const FixedCtl* ctl, hipStream_t st) {
  if (n == 0) return ISF_OK;
  hipLaunchKernelGGL(fixed_poison_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, n, ctl);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

}  // namespace isf
