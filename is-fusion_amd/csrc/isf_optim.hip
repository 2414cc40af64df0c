// isf_optim.hip -- multi-tensor optimizer step: global L2 norm of every gradient, gradient clipping and AdamW in two
// launches for any number of tensors (include/isf_hip.h, "Fused AdamW").
//
// Work is cut into chunks of ISF_OPTIM_CHUNK elements of one tensor (chunk table: tensor id, chunk index); one workgroup
// owns one chunk in both kernels.  isf_optim_grad_sumsq writes one fp64 sum of squares per chunk; isf_optim_adamw has every
// workgroup reduce those partials in the same fixed order (no atomics: the norm, the clip coefficient and therefore the
// whole update are bit-identical from run to run), then update its chunk.  Gradients may sit at any 4-byte offset (DDP's
// gradient_as_bucket_view buckets): float4 loads where the address allows, a scalar head and tail around them.
#include <math.h>

#include "isf_common.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = ISF_OPTIM_CHUNK;

struct HpArgs {                 // the per-step hyperparameter tuples, passed by value while they fit
  isf_adamw_hp v[ISF_OPTIM_MAX_HP_ARGS];
};

struct Chunk {
  const int64_t* e;             // tensor entry: p, g, m, v (addresses), numel, hp index
  int64_t start;
  int len;
};

__device__ __forceinline__ Chunk chunk_of(const int64_t* tensors, const int32_t* chunks, int c) {
  const int t = chunks[2 * c], k = chunks[2 * c + 1];
  Chunk r;
  r.e = tensors + 6 * (int64_t)t;
  r.start = (int64_t)k * kChunk;
  const int64_t rest = r.e[4] - r.start;
  r.len = rest < kChunk ? (int)rest : kChunk;
  return r;
}

// fixed-order block sum: wave shuffles, then wave 0 adds the kWaves wave sums in order; every thread gets the result
__device__ __forceinline__ double block_sum(double x, double* lds) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                                    // lds may still be read by a previous call
  if (lane == 0) lds[wave] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < kWaves; ++w) s += lds[w];
    lds[kWaves] = s;
  }
  __syncthreads();
  return lds[kWaves];
}

// elements before the first 16-byte aligned address, at most len
__device__ __forceinline__ int head_of(const void* p, int len) {
  const int h = (int)(((16u - ((uintptr_t)p & 15u)) & 15u) >> 2);
  return h < len ? h : len;
}

__global__ __launch_bounds__(kThreads) void sumsq_kernel(const int64_t* __restrict__ tensors,
                                                        const int32_t* __restrict__ chunks,
                                                        double* __restrict__ partials) {
  __shared__ double lds[kWaves + 1];
  const Chunk ck = chunk_of(tensors, chunks, blockIdx.x);
  const float* x = reinterpret_cast<const float*>(ck.e[1]) + ck.start;
  const int head = head_of(x, ck.len);
  const int nv = (ck.len - head) >> 2;
  double acc = 0.0;
  if ((int)threadIdx.x < head) {
    const double a = x[threadIdx.x];
    acc += a * a;
  }
  const float4* xv = reinterpret_cast<const float4*>(x + head);
  for (int i = threadIdx.x; i < nv; i += kThreads) {
    const float4 q = xv[i];
    acc += (double)q.x * q.x + (double)q.y * q.y + (double)q.z * q.z + (double)q.w * q.w;
  }
  for (int i = head + 4 * nv + threadIdx.x; i < ck.len; i += kThreads) {
    const double a = x[i];
    acc += a * a;
  }
  const double s = block_sum(acc, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

struct Hp {
  float decay, w1, b2, w2, eps, neg_step, bc2_sqrt;
};

// torch 2.x AdamW (_single_tensor_adam, decoupled weight decay), fp32 arithmetic in the same order
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, const Hp& h) {
  p *= h.decay;
  m = h.w1 < 0.5f ? m + h.w1 * (g - m) : g - (g - m) * (1.0f - h.w1);      // lerp(m, g, 1 - b1)
  v = v * h.b2 + h.w2 * g * g;
  const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
  p = p + h.neg_step * (m / denom);
}

__global__ __launch_bounds__(kThreads) void adamw_kernel(const int64_t* __restrict__ tensors,
                                                        const int32_t* __restrict__ chunks, int num_chunks, HpArgs hpa,
                                                        int num_hp, const isf_adamw_hp* __restrict__ hp_dev,
                                                        const double* __restrict__ partials, float max_norm,
                                                        float* __restrict__ norm_out, int mode) {
  __shared__ double lds[kWaves + 1];
  float coef = 1.0f;
  if (mode != ISF_OPTIM_NO_CLIP) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < num_chunks; i += kThreads) acc += partials[i];
    const double norm = sqrt(block_sum(acc, lds));
    coef = (float)fmin(1.0, (double)max_norm / (norm + 1e-6));               // clip_grad_norm_: clamp(max / (n + 1e-6), max=1)
    if (blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = (float)norm;
  }
  if ((int)blockIdx.x >= num_chunks) return;                                  // grid is >= 1 so the norm is always written
  const Chunk ck = chunk_of(tensors, chunks, blockIdx.x);
  float* g = reinterpret_cast<float*>(ck.e[1]) + ck.start;
  if (mode == ISF_OPTIM_SCALE_GRADS) {
    if (coef == 1.0f) return;                                                 // g * 1 == g
    const int head = head_of(g, ck.len);
    const int nv = (ck.len - head) >> 2;
    if ((int)threadIdx.x < head) g[threadIdx.x] *= coef;
    float4* gv = reinterpret_cast<float4*>(g + head);
    for (int i = threadIdx.x; i < nv; i += kThreads) {
      float4 q = gv[i];
      q.x *= coef; q.y *= coef; q.z *= coef; q.w *= coef;
      gv[i] = q;
    }
    for (int i = head + 4 * nv + threadIdx.x; i < ck.len; i += kThreads) g[i] *= coef;
    return;
  }
  float* p = reinterpret_cast<float*>(ck.e[0]) + ck.start;
  float* m = reinterpret_cast<float*>(ck.e[2]) + ck.start;
  float* v = reinterpret_cast<float*>(ck.e[3]) + ck.start;
  const int hi = (int)ck.e[5];
  const isf_adamw_hp t = num_hp <= ISF_OPTIM_MAX_HP_ARGS ? hpa.v[hi] : hp_dev[hi];
  const Hp h{t.decay, t.w1, t.b2, t.w2, t.eps, t.neg_step_size, t.bc2_sqrt};
  const uintptr_t mis = (uintptr_t)p & 15u;
  int head = ck.len, nv = 0;                                                  // all scalar unless the four agree mod 16
  if (((uintptr_t)g & 15u) == mis && ((uintptr_t)m & 15u) == mis && ((uintptr_t)v & 15u) == mis) {
    head = head_of(p, ck.len);
    nv = (ck.len - head) >> 2;
  }
  for (int i = threadIdx.x; i < head; i += kThreads) adamw_elem(p[i], g[i] * coef, m[i], v[i], h);
  float4* pv = reinterpret_cast<float4*>(p + head);
  const float4* gv = reinterpret_cast<const float4*>(g + head);
  float4* mv = reinterpret_cast<float4*>(m + head);
  float4* vv = reinterpret_cast<float4*>(v + head);
  for (int i = threadIdx.x; i < nv; i += kThreads) {
    float4 a = pv[i], b = mv[i], c = vv[i];
    const float4 q = gv[i];
    adamw_elem(a.x, q.x * coef, b.x, c.x, h);
    adamw_elem(a.y, q.y * coef, b.y, c.y, h);
    adamw_elem(a.z, q.z * coef, b.z, c.z, h);
    adamw_elem(a.w, q.w * coef, b.w, c.w, h);
    pv[i] = a;
    mv[i] = b;
    vv[i] = c;
  }
  for (int i = head + 4 * nv + threadIdx.x; i < ck.len; i += kThreads) adamw_elem(p[i], g[i] * coef, m[i], v[i], h);
}

}  // namespace

extern "C" {

int isf_optim_grad_sumsq(const int64_t* tensors, const int32_t* chunks, int num_chunks, double* partials,
                         isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num_chunks >= 0, ISF_ERR_ARG, "optim_grad_sumsq: num_chunks %d", num_chunks);
  if (num_chunks == 0) return ISF_OK;
  ISF_REQUIRE(tensors && chunks && partials, ISF_ERR_ARG, "optim_grad_sumsq: null pointer");
  hipLaunchKernelGGL(sumsq_kernel, dim3(num_chunks), dim3(kThreads), 0, as_stream(stream), tensors, chunks, partials);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_optim_adamw(const int64_t* tensors, const int32_t* chunks, int num_chunks, const isf_adamw_hp* hp, int num_hp,
                    const isf_adamw_hp* hp_device, const double* partials, float max_norm, float* norm_out, int mode,
                    isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num_chunks >= 0, ISF_ERR_ARG, "optim_adamw: num_chunks %d", num_chunks);
  ISF_REQUIRE(mode == ISF_OPTIM_NO_CLIP || mode == ISF_OPTIM_CLIP || mode == ISF_OPTIM_SCALE_GRADS, ISF_ERR_ARG,
              "optim_adamw: mode %d", mode);
  const bool clip = mode != ISF_OPTIM_NO_CLIP;
  if (num_chunks == 0 && !clip) return ISF_OK;
  ISF_REQUIRE(!clip || (partials && norm_out), ISF_ERR_ARG, "optim_adamw: clipping needs partials and norm_out");
  ISF_REQUIRE(num_chunks == 0 || (tensors && chunks), ISF_ERR_ARG, "optim_adamw: null table");
  HpArgs hpa;
  memset(&hpa, 0, sizeof(hpa));
  if (mode != ISF_OPTIM_SCALE_GRADS) {
    ISF_REQUIRE(num_hp >= 1, ISF_ERR_ARG, "optim_adamw: %d hyperparameter tuples", num_hp);
    if (num_hp <= ISF_OPTIM_MAX_HP_ARGS) {
      ISF_REQUIRE(hp, ISF_ERR_ARG, "optim_adamw: null host hyperparameters");
      memcpy(hpa.v, hp, sizeof(isf_adamw_hp) * num_hp);
    } else {
      ISF_REQUIRE(hp_device, ISF_ERR_ARG, "optim_adamw: %d tuples need hp_device", num_hp);
    }
  }
  hipLaunchKernelGGL(adamw_kernel, dim3(num_chunks > 0 ? num_chunks : 1), dim3(kThreads), 0, as_stream(stream), tensors,
                     chunks, num_chunks, hpa, num_hp, hp_device, partials, max_norm, norm_out, mode);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

}  // extern "C"
