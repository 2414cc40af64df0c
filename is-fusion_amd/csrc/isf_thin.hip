// isf_thin.hip -- a linear layer with a THIN input (1 <= K <= 8 input features), forward and backward, in training mode:
// the first layer of the reference's PositionEmbeddingLearned (fusion_encoder.py:173-189: Conv1d(2 -> E, k = 1) on
// [B, 2, N] positions = a linear layer over B * N rows of two coordinates).
//
// The fused linear kernel (isf_linear.hip) tiles K in steps of 32 on the matrix cores; K = 2 there would mean coordinates
// padded to 32 columns and split into f16 halves -- 16 x the traffic, and a rounding of positions that go up to 180.  A
// library GEMM promises no summation order.  These kernels are plain fp32 FMA on the vector ALU with every sum in a fixed
// order, so the results are bit-identical run to run (deterministic mode needs nothing from them):
//
//   forward   y [M, N] = x w^T + b.  Write-bound (M * N * 4 bytes against M * K * 4 read): a lane owns four adjacent output
//             columns with their w rows and b in registers, reads its row of x by broadcast (every lane of a row the same
//             address) and stores 16 bytes.
//   backward  grad_w / grad_b: pass 1, one workgroup per chunk of kThinChunk rows, the lane of column n keeps K + 1 sums
//             over the chunk's rows in ascending order (coalesced reads of grad_y rows) and writes them to
//             parts [chunk][K + 1][N]; pass 2 adds the chunks in ascending order.  No atomics; the chunking depends on M only.
//             grad_x [M, K] = grad_y w, only when asked for: a wave per row, a lane's four columns in ascending order (16-byte
//             loads), then an xor butterfly over the 64 lanes (the same tree for every row).
//
// At the sizes of the model (at most 64 800 rows x 128 columns) all of them are launch-bound.
#include <algorithm>

#include "isf_common.h"

namespace isf {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThinThreads = 256;
constexpr int kThinChunk = 128;      // rows per chunk of the backward's first pass (isf_thin_linear_parts)
constexpr int kThinMaxK = 8;
constexpr int kThinMaxN = 256;

static bool thin_shape_ok(int n, int k) { return k >= 1 && k <= kThinMaxK && n >= 16 && n <= kThinMaxN && n % 16 == 0; }

// lanes_per_row = N / 4 lanes cover a row; a block covers kThinThreads / lanes_per_row rows per step (the lanes left over
// when N / 4 does not divide the block idle)
template <int K>
__global__ __launch_bounds__(kThinThreads) void thin_forward_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                    const float* __restrict__ b, float* __restrict__ y,
                                                                    int m, int n) {
  const int lanes_per_row = n >> 2;
  const int rows_per_step = kThinThreads / lanes_per_row;
  const int q = threadIdx.x % lanes_per_row, r0 = threadIdx.x / lanes_per_row;
  if (r0 >= rows_per_step) return;
  float wr[4][K];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < K; ++k) wr[j][k] = w[(size_t)(4 * q + j) * K + k];
  f32x4 bias = f32x4{0.f, 0.f, 0.f, 0.f};
  if (b) bias = *reinterpret_cast<const f32x4*>(b + 4 * q);
  for (long long r = (long long)blockIdx.x * rows_per_step + r0; r < m; r += (long long)gridDim.x * rows_per_step) {
    float xr[K];
#pragma unroll
    for (int k = 0; k < K; ++k) xr[k] = x[r * K + k];
    f32x4 acc = bias;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      acc.x = fmaf(xr[k], wr[0][k], acc.x);
      acc.y = fmaf(xr[k], wr[1][k], acc.y);
      acc.z = fmaf(xr[k], wr[2][k], acc.z);
      acc.w = fmaf(xr[k], wr[3][k], acc.w);
    }
    *reinterpret_cast<f32x4*>(y + r * n + 4 * q) = acc;
  }
}

// pass 1: block = chunk, thread = column; parts [chunk][K + 1][n], entry K = the column sum (grad_b)
template <int K>
__global__ __launch_bounds__(kThinMaxN) void thin_backward_partial_kernel(const float* __restrict__ g,
                                                                          const float* __restrict__ x, int m, int n,
                                                                          float* __restrict__ parts) {
  const int col = threadIdx.x;
  if (col >= n) return;
  const long long first = (long long)blockIdx.x * kThinChunk;
  const long long last = first + kThinChunk < m ? first + kThinChunk : m;
  float s[K + 1];
#pragma unroll
  for (int k = 0; k <= K; ++k) s[k] = 0.f;
  for (long long r = first; r < last; ++r) {
    const float gv = g[r * n + col];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = fmaf(gv, x[r * K + k], s[k]);
    s[K] += gv;
  }
  float* out = parts + (size_t)blockIdx.x * (K + 1) * n;
#pragma unroll
  for (int k = 0; k <= K; ++k) out[(size_t)k * n + col] = s[k];
}

// pass 2: thread = one of the (K + 1) * n sums, the chunks added in ascending order
__global__ __launch_bounds__(kThinThreads) void thin_backward_final_kernel(const float* __restrict__ parts, int num_parts,
                                                                           int n, int k_in, float* __restrict__ grad_w,
                                                                           float* __restrict__ grad_b) {
  const int i = blockIdx.x * kThinThreads + threadIdx.x;      // = k * n + col
  const int total = (k_in + 1) * n;
  if (i >= total) return;
  float s = 0.f;
  for (int p = 0; p < num_parts; ++p) s += parts[(size_t)p * total + i];
  const int k = i / n, col = i - k * n;
  if (k < k_in)
    grad_w[(size_t)col * k_in + k] = s;
  else if (grad_b)
    grad_b[col] = s;
}

// grad_x: wave = row; lane l holds columns 4l .. 4l + 3 (lanes past n / 4 hold zeros)
template <int K>
__global__ __launch_bounds__(kThinThreads) void thin_backward_input_kernel(const float* __restrict__ g,
                                                                           const float* __restrict__ w, int m, int n,
                                                                           float* __restrict__ grad_x) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool live = 4 * lane < n;
  float wr[4][K];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < K; ++k) wr[j][k] = live ? w[(size_t)(4 * lane + j) * K + k] : 0.f;
  constexpr int kWaves = kThinThreads / 64;
  for (long long r = (long long)blockIdx.x * kWaves + wave; r < m; r += (long long)gridDim.x * kWaves) {
    f32x4 gv = f32x4{0.f, 0.f, 0.f, 0.f};
    if (live) gv = *reinterpret_cast<const f32x4*>(g + r * n + 4 * lane);
    float s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float a = gv.x * wr[0][k];
      a = fmaf(gv.y, wr[1][k], a);
      a = fmaf(gv.z, wr[2][k], a);
      a = fmaf(gv.w, wr[3][k], a);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
      s[k] = a;
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) grad_x[r * K + k] = s[k];
    }
  }
}

template <int K>
static void thin_launch_forward(const float* x, const float* w, const float* b, float* y, int m, int n, hipStream_t st) {
  const int rows_per_step = kThinThreads / (n / 4);
  const int blocks = std::max(1, std::min(2048, ceil_div(m, rows_per_step)));
  hipLaunchKernelGGL(thin_forward_kernel<K>, dim3(blocks), dim3(kThinThreads), 0, st, x, w, b, y, m, n);
}

template <int K>
static void thin_launch_backward(const float* g, const float* x, const float* w, float* parts, float* grad_w, float* grad_b,
                                 float* grad_x, int m, int n, hipStream_t st) {
  if (grad_w) {
    const int num_parts = ceil_div(m, kThinChunk);
    hipLaunchKernelGGL(thin_backward_partial_kernel<K>, dim3(num_parts), dim3(kThinMaxN), 0, st, g, x, m, n, parts);
    hipLaunchKernelGGL(thin_backward_final_kernel, dim3(ceil_div((K + 1) * n, kThinThreads)), dim3(kThinThreads), 0, st,
                       parts, num_parts, n, K, grad_w, grad_b);
  }
  if (grad_x) {
    const int blocks = std::max(1, std::min(2048, ceil_div(m, kThinThreads / 64)));
    hipLaunchKernelGGL(thin_backward_input_kernel<K>, dim3(blocks), dim3(kThinThreads), 0, st, g, w, m, n, grad_x);
  }
}

#define ISF_THIN_DISPATCH(k, call) \
  switch (k) {                     \
    case 1: call(1); break;        \
    case 2: call(2); break;        \
    case 3: call(3); break;        \
    case 4: call(4); break;        \
    case 5: call(5); break;        \
    case 6: call(6); break;        \
    case 7: call(7); break;        \
    default: call(8); break;       \
  }

}  // namespace isf

extern "C" {

int isf_thin_linear_parts(int num_rows) { return num_rows > 0 ? isf::ceil_div(num_rows, isf::kThinChunk) : 0; }

int isf_thin_linear_forward(const float* x, const float* w, const float* b, float* y, int num_rows, int out_features,
                            int in_features, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(x && w && y && num_rows > 0, ISF_ERR_ARG, "thin_linear_forward: bad arguments");
  ISF_REQUIRE(thin_shape_ok(out_features, in_features), ISF_ERR_UNSUPPORTED,
              "thin_linear_forward: %d -> %d features (1 <= in <= 8, out a multiple of 16 up to 256)", in_features, out_features);
#define ISF_THIN_FWD(K) thin_launch_forward<K>(x, w, b, y, num_rows, out_features, as_stream(stream))
  ISF_THIN_DISPATCH(in_features, ISF_THIN_FWD)
#undef ISF_THIN_FWD
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_thin_linear_backward(const float* grad_y, const float* x, const float* w, float* parts, float* grad_w,
                             float* grad_b, float* grad_x, int num_rows, int out_features, int in_features,
                             isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(grad_y && x && w && num_rows > 0 && (grad_w || !grad_b) && (parts || !grad_w), ISF_ERR_ARG,
              "thin_linear_backward: bad arguments");
  ISF_REQUIRE(thin_shape_ok(out_features, in_features), ISF_ERR_UNSUPPORTED,
              "thin_linear_backward: %d -> %d features (1 <= in <= 8, out a multiple of 16 up to 256)", in_features, out_features);
#define ISF_THIN_BWD(K) \
  thin_launch_backward<K>(grad_y, x, w, parts, grad_w, grad_b, grad_x, num_rows, out_features, as_stream(stream))
  ISF_THIN_DISPATCH(in_features, ISF_THIN_BWD)
#undef ISF_THIN_BWD
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

}  // extern "C"
