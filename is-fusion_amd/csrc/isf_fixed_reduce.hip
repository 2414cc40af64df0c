// isf_fixed_reduce.hip -- the fixed-point sum of isf_fixed.h carried ACROSS RANKS (include/isf_hip.h, "Exact cross-rank
// sums"): the passes on either side of an integer collective, for any number of tensors in one launch each.
//
//   isf_fixed_absmax_tensors   bits[t] = largest bit pattern of |x| in tensor t      (then: integer MAX over the ranks)
//   isf_fixed_pack_tensors     q = llrint(g * 2^e), e = 62 - log2_world - ex(bits)   (then: int64 SUM over the ranks)
//   isf_fixed_finish_tensors   g = float(S * 2^-e / divisor), NaN where the bound is not finite
//   isf_fixed_sum_rows         all three for W gathered rows of one short vector (the sync-BN statistics)
//
// Work is cut as in isf_optim.hip: a tensor table, a chunk table (tensor, chunk index), one workgroup per chunk of
// ISF_OPTIM_CHUNK elements; tensors at any 4-byte offset (DDP bucket views): float4 where the address allows, a scalar head
// and tail.  The only atomic is the integer max of the bound; every 64-bit value leaves in ordinary vector stores.
#include <math.h>

#include "isf_fixed.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = ISF_OPTIM_CHUNK;
constexpr unsigned kInfBits = 0x7f800000u;
constexpr unsigned kNanBits = 0x7fc00000u;

struct Chunk {
  float* x;                     // first element of the chunk
  long long* q;                 // its fixed-point image (null table entry: unused)
  int len, t;
};

// tensor entry: address, numel, offset of the tensor's first element in q
__device__ __forceinline__ Chunk chunk_of(const int64_t* tensors, const int32_t* chunks, long long* q, int c) {
  const int t = chunks[2 * c], k = chunks[2 * c + 1];
  const int64_t* e = tensors + 3 * (int64_t)t;
  const int64_t start = (int64_t)k * kChunk, rest = e[1] - start;
  Chunk r;
  r.x = reinterpret_cast<float*>(e[0]) + start;
  r.q = q + e[2] + start;
  r.len = rest < kChunk ? (int)rest : kChunk;
  r.t = t;
  return r;
}

// elements before the first 16-byte aligned address, at most len
__device__ __forceinline__ int head_of(const void* p, int len) {
  const int h = (int)(((16u - ((uintptr_t)p & 15u)) & 15u) >> 2);
  return h < len ? h : len;
}

// e of isf_fixed.h for the bound `b` (a bit pattern of |x|) and N = 2^log2n contributions; false: the bound is not finite
__device__ __forceinline__ bool fixed_exponent(unsigned b, int log2n, int* e) {
  if (b >= kInfBits) return false;
  int ex = 0;
  frexpf(__uint_as_float(b), &ex);              // |x| < 2^ex (0 -> ex = 0: every q is 0)
  *e = 62 - log2n - ex;
  return true;
}

__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

__global__ __launch_bounds__(kThreads) void absmax_kernel(const int64_t* __restrict__ tensors,
                                                         const int32_t* __restrict__ chunks, unsigned* __restrict__ bits) {
  __shared__ unsigned lds[kWaves];
  const Chunk ck = chunk_of(tensors, chunks, nullptr, blockIdx.x);
  const float* x = ck.x;
  const int head = head_of(x, ck.len);
  const int nv = (ck.len - head) >> 2;
  unsigned m = 0;
  if ((int)threadIdx.x < head) m = abs_bits(x[threadIdx.x]);
  const float4* xv = reinterpret_cast<const float4*>(x + head);
  for (int i = threadIdx.x; i < nv; i += kThreads) {
    const float4 v = xv[i];
    m = max(max(m, abs_bits(v.x)), max(max(abs_bits(v.y), abs_bits(v.z)), abs_bits(v.w)));
  }
  for (int i = head + 4 * nv + threadIdx.x; i < ck.len; i += kThreads) m = max(m, abs_bits(x[i]));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, d, 64));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) m = max(m, lds[w]);
    if (m) atomicMax(bits + ck.t, m);           // integer max: order-free, and a NaN pattern (above inf's) wins
  }
}

__global__ __launch_bounds__(kThreads) void pack_kernel(const int64_t* __restrict__ tensors,
                                                       const int32_t* __restrict__ chunks,
                                                       const unsigned* __restrict__ bits, int log2_world,
                                                       long long* __restrict__ q) {
  const Chunk ck = chunk_of(tensors, chunks, q, blockIdx.x);
  int e = 0;
  const bool finite = fixed_exponent(bits[ck.t], log2_world, &e);
  auto fixed = [&](float g) -> long long { return finite ? llrint(ldexp((double)g, e)) : 0ll; };
  const float* x = ck.x;
  const int head = head_of(x, ck.len);
  const int nv = (ck.len - head) >> 2;
  if ((int)threadIdx.x < head) ck.q[threadIdx.x] = fixed(x[threadIdx.x]);
  const float4* xv = reinterpret_cast<const float4*>(x + head);
  long long* qv = ck.q + head;
  const bool pairs = ((uintptr_t)qv & 15u) == 0;      // 16-byte stores where q's address allows, 8-byte ones otherwise
  for (int i = threadIdx.x; i < nv; i += kThreads) {
    const float4 v = xv[i];
    const long long a = fixed(v.x), b = fixed(v.y), c = fixed(v.z), d = fixed(v.w);
    if (pairs) {
      longlong2* o = reinterpret_cast<longlong2*>(qv + 4 * i);
      o[0] = make_longlong2(a, b);
      o[1] = make_longlong2(c, d);
    } else {
      qv[4 * i] = a; qv[4 * i + 1] = b; qv[4 * i + 2] = c; qv[4 * i + 3] = d;
    }
  }
  for (int i = head + 4 * nv + threadIdx.x; i < ck.len; i += kThreads) ck.q[i] = fixed(x[i]);
}

__global__ __launch_bounds__(kThreads) void finish_kernel(const int64_t* __restrict__ tensors,
                                                         const int32_t* __restrict__ chunks,
                                                         const unsigned* __restrict__ bits, int log2_world,
                                                         long long* __restrict__ q, double divisor) {
  const Chunk ck = chunk_of(tensors, chunks, q, blockIdx.x);
  int e = 0;
  const bool finite = fixed_exponent(bits[ck.t], log2_world, &e);
  auto value = [&](long long s) -> float {
    return finite ? (float)(ldexp((double)s, -e) / divisor) : __uint_as_float(kNanBits);
  };
  float* x = ck.x;
  const int head = head_of(x, ck.len);
  const int nv = (ck.len - head) >> 2;
  if ((int)threadIdx.x < head) x[threadIdx.x] = value(ck.q[threadIdx.x]);
  float4* xv = reinterpret_cast<float4*>(x + head);
  const long long* qv = ck.q + head;
  const bool pairs = ((uintptr_t)qv & 15u) == 0;
  for (int i = threadIdx.x; i < nv; i += kThreads) {
    long long a, b, c, d;
    if (pairs) {
      const longlong2* s = reinterpret_cast<const longlong2*>(qv + 4 * i);
      const longlong2 lo = s[0], hi = s[1];
      a = lo.x; b = lo.y; c = hi.x; d = hi.y;
    } else {
      a = qv[4 * i]; b = qv[4 * i + 1]; c = qv[4 * i + 2]; d = qv[4 * i + 3];
    }
    xv[i] = make_float4(value(a), value(b), value(c), value(d));
  }
  for (int i = head + 4 * nv + threadIdx.x; i < ck.len; i += kThreads) x[i] = value(ck.q[i]);
}

// one thread per column: bound, integer sum and finish over the W rows; neighbouring threads read neighbouring columns
__global__ __launch_bounds__(256) void sum_rows_kernel(const float* __restrict__ rows, int W, int n, int log2w,
                                                       double divisor, float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  unsigned m = 0;
  for (int r = 0; r < W; ++r) m = max(m, abs_bits(rows[(size_t)r * n + c]));
  int e = 0;
  float v = __uint_as_float(kNanBits);
  if (fixed_exponent(m, log2w, &e)) {
    long long s = 0;
    for (int r = 0; r < W; ++r) s += llrint(ldexp((double)rows[(size_t)r * n + c], e));
    v = (float)(ldexp((double)s, -e) / divisor);
  }
  out[c] = v;
}

int check_tables(const char* entry, const int64_t* tensors, const int32_t* chunks, int num_chunks, const void* bits,
                 int log2_world) {
  using namespace isf;
  ISF_REQUIRE(num_chunks >= 0, ISF_ERR_ARG, "%s: num_chunks %d", entry, num_chunks);
  ISF_REQUIRE(log2_world >= 0 && log2_world <= 10, ISF_ERR_ARG, "%s: log2_world %d outside [0, 10]", entry, log2_world);
  ISF_REQUIRE(num_chunks == 0 || (tensors && chunks && bits), ISF_ERR_ARG, "%s: null pointer", entry);
  return ISF_OK;
}

}  // namespace

extern "C" {

int isf_fixed_absmax_tensors(const int64_t* tensors, const int32_t* chunks, int num_chunks, int num_tensors, uint32_t* bits,
                             isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num_tensors >= 0, ISF_ERR_ARG, "fixed_absmax_tensors: num_tensors %d", num_tensors);
  ISF_REQUIRE(num_tensors == 0 || bits, ISF_ERR_ARG, "fixed_absmax_tensors: null bits");
  ISF_TRY(check_tables("fixed_absmax_tensors", tensors, chunks, num_chunks, bits, 0));
  if (num_tensors) ISF_HIP_TRY(hipMemsetAsync(bits, 0, sizeof(uint32_t) * (size_t)num_tensors, as_stream(stream)));
  if (num_chunks == 0) return ISF_OK;
  hipLaunchKernelGGL(absmax_kernel, dim3(num_chunks), dim3(kThreads), 0, as_stream(stream), tensors, chunks, bits);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_fixed_pack_tensors(const int64_t* tensors, const int32_t* chunks, int num_chunks, const uint32_t* bits,
                           int log2_world, int64_t* q, isf_stream_t stream) {
  using namespace isf;
  ISF_TRY(check_tables("fixed_pack_tensors", tensors, chunks, num_chunks, bits, log2_world));
  if (num_chunks == 0) return ISF_OK;
  ISF_REQUIRE(q && ((uintptr_t)q & 7u) == 0, ISF_ERR_ARG, "fixed_pack_tensors: q must be a non-null 8-byte aligned address");
  hipLaunchKernelGGL(pack_kernel, dim3(num_chunks), dim3(kThreads), 0, as_stream(stream), tensors, chunks, bits, log2_world,
                     reinterpret_cast<long long*>(q));
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_fixed_finish_tensors(const int64_t* tensors, const int32_t* chunks, int num_chunks, const uint32_t* bits,
                             int log2_world, const int64_t* q, double divisor, isf_stream_t stream) {
  using namespace isf;
  ISF_TRY(check_tables("fixed_finish_tensors", tensors, chunks, num_chunks, bits, log2_world));
  ISF_REQUIRE(divisor >= 1.0 && divisor <= 1024.0, ISF_ERR_ARG, "fixed_finish_tensors: divisor %g outside [1, 1024]", divisor);
  if (num_chunks == 0) return ISF_OK;
  ISF_REQUIRE(q && ((uintptr_t)q & 7u) == 0, ISF_ERR_ARG, "fixed_finish_tensors: q must be a non-null 8-byte aligned address");
  hipLaunchKernelGGL(finish_kernel, dim3(num_chunks), dim3(kThreads), 0, as_stream(stream), tensors, chunks, bits,
                     log2_world, const_cast<long long*>(reinterpret_cast<const long long*>(q)), divisor);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_fixed_sum_rows(const float* rows, int W, int n, double divisor, float* out, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(W >= 1 && W <= ISF_FIXED_MAX_ROWS, ISF_ERR_ARG, "fixed_sum_rows: %d rows outside [1, %d]", W,
              ISF_FIXED_MAX_ROWS);
  ISF_REQUIRE(n >= 0, ISF_ERR_ARG, "fixed_sum_rows: n %d", n);
  ISF_REQUIRE(divisor >= 1.0 && divisor <= 1024.0, ISF_ERR_ARG, "fixed_sum_rows: divisor %g outside [1, 1024]", divisor);
  if (n == 0) return ISF_OK;
  ISF_REQUIRE(rows && out, ISF_ERR_ARG, "fixed_sum_rows: null pointer");
  hipLaunchKernelGGL(sum_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), rows, W, n, ceil_log2(W),
                     divisor, out);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

}  // extern "C"
