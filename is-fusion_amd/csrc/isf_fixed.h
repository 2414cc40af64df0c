// isf_fixed.h -- the accumulators of the kernels that scatter with atomics: the default's fp32 atomicAdd, and the
// deterministic entries' (isf_*_det) exact sum in 64-bit fixed point.
//
// A float atomicAdd rounds after every add, so its result depends on the order the contributions arrive in.  An integer
// add does not round: the sum of q_i = llrint(c_i * 2^e) is the same in every order, so the *_det entries give the same
// bits run to run and under any permutation of the contributions.  Per call:
//   A   an upper bound of |c_i|, from an absmax pass over the call's inputs (integer max on the bit pattern: order-free);
//       A < 2^ex with ex = frexp's exponent (a product of factors: the sum of their exponents)
//   N   a static bound of the contributions one destination receives, from the call's sizes
//   e = 62 - ceil(log2 N) - ex, formed ON THE DEVICE (fixed_ctl) and read by the accumulating kernel from device memory:
//       no host sync.  |q_i| <= 2^(62 - ceil(log2 N)), so |sum| <= 2^62: one bit of head room for the half units of the
//       roundings, no overflow.  The scaling by 2^e is exact (done in double); the resolution of a contribution is
//       2^-(62 - ceil(log2 N)) of 2^ex, i.e. finer than 2^-(61 - ceil(log2 N)) of A.
//   a second pass (fixed_finish) writes float(ldexp(double(S), -e)).
// A == 0: every q is 0, the output is zeros.  A non-finite (an inf or NaN among the inputs the bound is taken from): the
// finish pass writes NaN to EVERY element of the accumulated output (and fixed_poison to the call's other float outputs).
#pragma once
#include "isf_common.h"

namespace isf {

// ctl[0] = e, ctl[1] = 1 when the bound is not finite
struct FixedCtl {
  int e;
  int nonfinite;
};

struct AccF32 {    // the default entries: hardware fp32 atomics
  float* p;
  __device__ __forceinline__ void add(size_t i, float c) const { atomicAdd(p + i, c); }
};

struct AccFixed {  // the *_det entries
  unsigned long long* p;
  const FixedCtl* ctl;
  __device__ __forceinline__ void add(size_t i, float c) const {
    const long long q = llrint(ldexp((double)c, ctl->e));
    atomicAdd(p + i, (unsigned long long)q);   // two's complement: the unsigned add is the signed sum
  }
};

static inline int ceil_log2(long long n) {
  int l = 0;
  while ((1ll << l) < n) ++l;
  return l;
}

// isf_fixed.hip
// bits[slot] = max(bits[slot], max_i bit pattern of |x_i|); bits zeroed by fixed_ctl_begin
int fixed_ctl_begin(Arena& a, unsigned** bits, FixedCtl** ctl, int num_ctl, hipStream_t st);   // bits [4] zeroed, ctl [num_ctl]
int fixed_absmax(const float* x, size_t n, unsigned* bits_slot, hipStream_t st);
// ex = sum over the `nfac` factors bits[0..nfac) of their exponents (factor f with bit f of clamp_mask set: max(ex_f, 0),
// a factor that only matters where it exceeds 1) + extra_ex;  ctl = {62 - log2n - ex, any factor non-finite}
int fixed_ctl(const unsigned* bits, int nfac, unsigned clamp_mask, int extra_ex, int log2n, FixedCtl* ctl, hipStream_t st);
// out[i] = float(ldexp(double(S_i), -e)) (+ the old out[i] with accumulate; / count[i / C] with count), NaN when non-finite
int fixed_finish(const unsigned long long* acc, const FixedCtl* ctl, size_t n, float* out, bool accumulate,
                 const int32_t* count, int C, hipStream_t st);
int fixed_poison(float* p, size_t n, const FixedCtl* ctl, hipStream_t st);   // p[:] = NaN when non-finite

}  // namespace isf
