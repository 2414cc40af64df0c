// isf_image.hip -- the camera side of the input pipeline as a GPU pre-pass.  Replaces, for every view of a batch in ONE
// launch, what the reference's dataloader workers do per image in Pillow / torchvision on the CPU:
//   ImageAug3D.img_transform   datasets/pipelines/transforms_3d.py:82-112  (img.resize -> img.crop -> FLIP_LEFT_RIGHT ->
//                                                                          img.rotate)
//   ImageNormalize             transforms_3d.py:25-43                      (ToTensor + Normalize, HWC uint8 -> CHW float32)
// The decoded images (uint8 HWC RGB, any size per view) are uploaded untouched; img [V, 3, fH, fW] float32 comes out.
//
// Bit-exact against Pillow: every step before the normalise table is integer arithmetic.
//   resize   separable antialiased bicubic in Pillow's 8-bit path: per output index a window [xmin, xmin + n) of the
//            input and n coefficients with 22 fractional bits (host tables, float64 as Pillow computes them);
//            acc = 2^21 + sum u8 * k in int32, result = clip(acc >> 22, 0, 255).  The HORIZONTAL pass runs first and is
//            rounded to uint8 before the vertical pass.  A pass that keeps the size is the table (n = 1, k = 2^22), which
//            reproduces the byte: (2^21 + v * 2^22) >> 22 = v.
//   crop     a shift; pixels outside the resized image are 0.
//   rotate   nearest neighbour in 16.16 fixed point: (x, y) reads ((a2 + y a1 + x a0) >> 16, (a5 + y a4 + x a3) >> 16) of
//            the (flipped) cropped image, 0 outside.
//   normalise  a 3 x 256 float32 table built on the host with the float32 ops torchvision uses.
//
// Memory-bound byte work, so one workgroup owns a 32 x 64 output tile of one view and recomputes its halo:
//   1. bounding box of the tile's source pixels in the resized image (rotation corners -> flip -> crop origin -> clamp);
//   2. horizontal pass global uint8 -> LDS uint8 over the source rows the box's vertical windows need, in chunks of
//      rows that fit the LDS buffer;
//   3. vertical pass LDS -> LDS uint8: the tile's piece of the resized image;
//   4. every output pixel picks its (rotated, flipped, cropped) source from that piece or 0, looks up the normalise
//      table and is stored: a wave writes one 256-byte run of one channel plane per store.
// No float arithmetic on the device, no atomics, no host data: the call is one asynchronous launch.
//
// isf_image_paste runs before it, in place on the same uploaded bytes: the image side of the multi-modal GT-paste
//   MMDataBaseSamplerV2.sample_all   datasets/pipelines/dbsampler.py:779-831  (far-to-near loop: real-GT mix-back, :814)
//   MMDataBaseSamplerV2.paste_obj_v2 dbsampler.py:902-928                     (patch with a 5 % soft margin)
// A thread owns one pixel of one view and applies, in plan order, every operation whose rectangle holds it: overlapping
// rectangles need no ordering between threads.  float64 / float32 products and sums are written with the _rn
// intrinsics, so nothing is contracted and every byte is what numpy stores.
#include <limits.h>

#include "isf_common.h"

namespace isf {

constexpr int kImgTileH = 32, kImgTileW = 64, kImgThreads = 256;
// side of the largest source box of a tile: a rotation maps the 64 x 32 tile into a box of at most
// 64 |cos| + 32 |sin| + 2 <= 74 pixels a side, whatever the angle
constexpr int kImgRegion = 76;
constexpr int kImgHBytes = 20 * 1024;     // horizontal-pass rows held in LDS: 37 KB with the box piece, four workgroups a CU;
                                          // the shipped draws need <= 16 KB (0.57, +-5.4 deg: 77 rows x 68 px), more is chunked
constexpr int kImgPrecBits = 22;

__device__ __forceinline__ uint8_t clip8(int acc) { return (uint8_t)min(max(acc >> kImgPrecBits, 0), 255); }

__global__ __launch_bounds__(kImgThreads) void image_prepass_kernel(const uint8_t* __restrict__ raw,
                                                                    const isf_image_view_t* __restrict__ views,
                                                                    const int32_t* __restrict__ tables,
                                                                    const float* __restrict__ lut, int out_h, int out_w,
                                                                    float* __restrict__ out) {
  __shared__ uint8_t hbuf[kImgHBytes];
  __shared__ uint8_t piece[kImgRegion * kImgRegion * 3];
  const int tid = threadIdx.x, view = blockIdx.z;
  const isf_image_view_t& vw = views[view];          // uniform: scalar loads
  const int ox0 = blockIdx.x * kImgTileW, oy0 = blockIdx.y * kImgTileH;
  const int ox1 = min(ox0 + kImgTileW, out_w) - 1, oy1 = min(oy0 + kImgTileH, out_h) - 1;
  const int a0 = vw.rot[0], a1 = vw.rot[1], a2 = vw.rot[2], a3 = vw.rot[3], a4 = vw.rot[4], a5 = vw.rot[5];

  // 1. source box.  The fixed-point map is monotone in x and in y, so the corners bound the tile.
  int xlo = ox0, xhi = ox1, ylo = oy0, yhi = oy1;
  if (vw.rotate) {
    xlo = ylo = INT_MAX;
    xhi = yhi = INT_MIN;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int x = (c & 1) ? ox1 : ox0, y = (c & 2) ? oy1 : oy0;
      const int xi = (a2 + y * a1 + x * a0) >> 16, yi = (a5 + y * a4 + x * a3) >> 16;
      xlo = min(xlo, xi); xhi = max(xhi, xi);
      ylo = min(ylo, yi); yhi = max(yhi, yi);
    }
  }
  xlo = max(xlo, 0); xhi = min(xhi, out_w - 1);
  ylo = max(ylo, 0); yhi = min(yhi, out_h - 1);
  if (vw.flip) {
    const int t = xlo;
    xlo = out_w - 1 - xhi;
    xhi = out_w - 1 - t;
  }
  const int rx0 = max(xlo + vw.crop_x, 0), rx1 = min(xhi + vw.crop_x, vw.resize_w - 1);
  const int ry0 = max(ylo + vw.crop_y, 0), ry1 = min(yhi + vw.crop_y, vw.resize_h - 1);
  const bool empty = rx0 > rx1 || ry0 > ry1;
  const int rw = rx1 - rx0 + 1, rh = ry1 - ry0 + 1, pitch = rw * 3;
  // outside what the tile buffers hold (rotation integers that are no rotation, a vertical window longer than the LDS
  // rows): the tile is written as NaN, never silently wrong
  bool bad = !empty && (rw > kImgRegion || rh > kImgRegion);

  if (!empty && !bad) {
    const int32_t* __restrict__ bh = tables + vw.h_bounds;
    const int32_t* __restrict__ kh = tables + vw.h_coeffs;
    const int32_t* __restrict__ bv = tables + vw.v_bounds;
    const int32_t* __restrict__ kv = tables + vw.v_coeffs;
    const uint8_t* __restrict__ src = raw + vw.src_offset;
    const int cap_rows = kImgHBytes / pitch;
    int ra = ry0;
    while (ra <= ry1) {
      // rows ra..rb of the box whose vertical windows fit the LDS rows together (uniform over the workgroup)
      int s0 = bv[2 * ra], s1 = s0 + bv[2 * ra + 1];
      if (s1 - s0 > cap_rows) {
        bad = true;
        break;
      }
      int rb = ra;
      while (rb < ry1) {
        const int lo = min(s0, bv[2 * rb + 2]), hi = max(s1, bv[2 * rb + 2] + bv[2 * rb + 3]);
        if (hi - lo > cap_rows) break;
        s0 = lo;
        s1 = hi;
        ++rb;
      }
      // 2. horizontal pass: source rows s0..s1-1, columns rx0..rx1 of the resized image
      const int srows = s1 - s0;
      for (int e = tid; e < srows * rw; e += kImgThreads) {
        const int r = e / rw, cx = e - r * rw, rx = rx0 + cx;
        const int xmin = bh[2 * rx], n = bh[2 * rx + 1];
        const int32_t* __restrict__ k = kh + (size_t)rx * vw.h_ksize;
        const uint8_t* __restrict__ p = src + ((size_t)(s0 + r) * vw.src_w + xmin) * 3;
        int c0 = 1 << (kImgPrecBits - 1), c1 = c0, c2 = c0;
        for (int j = 0; j < n; ++j) {
          const int kk = k[j];
          c0 += (int)p[3 * j] * kk;
          c1 += (int)p[3 * j + 1] * kk;
          c2 += (int)p[3 * j + 2] * kk;
        }
        uint8_t* q = hbuf + r * pitch + cx * 3;
        q[0] = clip8(c0);
        q[1] = clip8(c1);
        q[2] = clip8(c2);
      }
      __syncthreads();
      // 3. vertical pass: rows ra..rb of the box
      for (int e = tid; e < (rb - ra + 1) * rw; e += kImgThreads) {
        const int r = e / rw, cx = e - r * rw, ry = ra + r;
        const int ymin = bv[2 * ry] - s0, n = bv[2 * ry + 1];
        const int32_t* __restrict__ k = kv + (size_t)ry * vw.v_ksize;
        const uint8_t* p = hbuf + ymin * pitch + cx * 3;
        int c0 = 1 << (kImgPrecBits - 1), c1 = c0, c2 = c0;
        for (int j = 0; j < n; ++j) {
          const int kk = k[j];
          c0 += (int)p[j * pitch] * kk;
          c1 += (int)p[j * pitch + 1] * kk;
          c2 += (int)p[j * pitch + 2] * kk;
        }
        uint8_t* q = piece + (ry - ry0) * pitch + cx * 3;
        q[0] = clip8(c0);
        q[1] = clip8(c1);
        q[2] = clip8(c2);
      }
      __syncthreads();      // piece written; hbuf free for the next chunk
      ra = rb + 1;
    }
  }

  // 4. rotate + flip + crop + normalise; lanes run along x, one wave per output row
  const size_t plane = (size_t)out_h * out_w;
  float* __restrict__ o = out + (size_t)view * 3 * plane;
  const int lx = tid & (kImgTileW - 1), ly0 = tid / kImgTileW;
  const int ox = ox0 + lx;
  if (ox > ox1) return;
  for (int oy = oy0 + ly0; oy <= oy1; oy += kImgThreads / kImgTileW) {
    int v0 = 0, v1 = 0, v2 = 0;
    int xi = ox, yi = oy;
    if (vw.rotate) {
      xi = (a2 + oy * a1 + ox * a0) >> 16;
      yi = (a5 + oy * a4 + ox * a3) >> 16;
    }
    if (xi >= 0 && xi < out_w && yi >= 0 && yi < out_h) {
      if (vw.flip) xi = out_w - 1 - xi;
      const int X = xi + vw.crop_x, Y = yi + vw.crop_y;
      // inside the resized image <=> inside the box (step 1 bounds every pixel of the tile)
      if (X >= rx0 && X <= rx1 && Y >= ry0 && Y <= ry1 && !empty) {
        const uint8_t* p = piece + (Y - ry0) * pitch + (X - rx0) * 3;
        v0 = p[0];
        v1 = p[1];
        v2 = p[2];
      }
    }
    const size_t at = (size_t)oy * out_w + ox;
    if (bad) {
      const float nan = __int_as_float(0x7fc00000);
      o[at] = nan;
      o[at + plane] = nan;
      o[at + 2 * plane] = nan;
    } else {
      o[at] = lut[v0];
      o[at + plane] = lut[256 + v1];
      o[at + 2 * plane] = lut[512 + v2];
    }
  }
}

constexpr int kPasteTileW = 64, kPasteTileH = 4;

__global__ __launch_bounds__(kPasteTileW * kPasteTileH) void image_paste_kernel(
    uint8_t* __restrict__ raw, const isf_paste_view_t* __restrict__ views, const isf_paste_op_t* __restrict__ ops,
    double mixup, double one_minus_mixup, float mixup_f32) {
  const isf_paste_view_t& vw = views[blockIdx.z];      // uniform: scalar loads
  const int x = vw.box_x0 + blockIdx.x * kPasteTileW + threadIdx.x;
  const int y = vw.box_y0 + blockIdx.y * kPasteTileH + threadIdx.y;
  if (x >= vw.box_x1 || y >= vw.box_y1 || x >= vw.width || y >= vw.height) return;
  uint8_t* px = raw + vw.src_offset + ((size_t)y * vw.width + x) * 3;
  uint8_t orig[3], v[3];
  bool loaded = false;
  for (int i = vw.op_begin; i < vw.op_end; ++i) {
    const isf_paste_op_t& op = ops[i];                 // uniform index: scalar loads
    if (x < op.x0 || x >= op.x1 || y < op.y0 || y >= op.y1) continue;
    if (!loaded) {
#pragma unroll
      for (int c = 0; c < 3; ++c) orig[c] = v[c] = px[c];
      loaded = true;
    }
    if (op.kind == ISF_PASTE_MIX) {
      // img[rows, cols] = mixup * origin_img[rows, cols] + (1 - mixup) * img[rows, cols]: float64, stored as uint8
#pragma unroll
      for (int c = 0; c < 3; ++c)
        v[c] = (uint8_t)(int)__dadd_rn(__dmul_rn(mixup, (double)orig[c]), __dmul_rn(one_minus_mixup, (double)v[c]));
    } else {
      const bool inner = x >= op.mask_x0 && x < op.mask_x1 && y >= op.mask_y0 && y < op.mask_y1;
      const double paste_mask = inner ? one_minus_mixup : 1.0, mask = inner ? 1.0 : 0.0;
      const uint8_t* pp = raw + op.patch_offset + ((size_t)(y - op.y0) * op.patch_pitch + (x - op.x0)) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint8_t kept = (uint8_t)(int)__dmul_rn((double)(float)v[c], paste_mask);
        const uint8_t add = (uint8_t)(int)__dmul_rn((double)__fmul_rn(mixup_f32, (float)pp[c]), mask);
        v[c] = (uint8_t)(kept + add);                  // uint8 += wraps
      }
    }
  }
  if (loaded) {
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = v[c];
  }
}

}  // namespace isf

extern "C" {

int isf_image_paste(uint8_t* raw, const isf_paste_view_t* views, int num_views, const isf_paste_op_t* ops,
                    int max_ops_per_view, int max_box_w, int max_box_h, double mixup, double one_minus_mixup,
                    float mixup_f32, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num_views >= 0 && num_views <= 65535 && max_ops_per_view >= 0 && max_box_w >= 0 && max_box_h >= 0,
              ISF_ERR_ARG, "image_paste: bad sizes");
  ISF_REQUIRE(max_ops_per_view <= ISF_PASTE_MAX_OPS, ISF_ERR_UNSUPPORTED,
              "image_paste: %d operations on one view, at most %d are walked", max_ops_per_view, ISF_PASTE_MAX_OPS);
  if (num_views == 0 || max_ops_per_view == 0 || max_box_w == 0 || max_box_h == 0) return ISF_OK;
  ISF_REQUIRE(raw && views && ops, ISF_ERR_ARG, "image_paste: null pointer");
  const dim3 grid(ceil_div(max_box_w, kPasteTileW), ceil_div(max_box_h, kPasteTileH), num_views);
  ISF_REQUIRE(grid.y <= 65535, ISF_ERR_ARG, "image_paste: region too tall");
  hipLaunchKernelGGL(image_paste_kernel, grid, dim3(kPasteTileW, kPasteTileH), 0, as_stream(stream), raw, views, ops,
                     mixup, one_minus_mixup, mixup_f32);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

int isf_image_prepass(const uint8_t* raw, const isf_image_view_t* views, int num_views, const int32_t* tables,
                      const float* norm_lut, int out_h, int out_w, float* img_out, isf_stream_t stream) {
  using namespace isf;
  ISF_REQUIRE(num_views >= 0 && num_views <= 65535 && out_h > 0 && out_w > 0, ISF_ERR_ARG, "image_prepass: bad sizes");
  if (num_views == 0) return ISF_OK;
  ISF_REQUIRE(raw && views && tables && norm_lut && img_out, ISF_ERR_ARG, "image_prepass: null pointer");
  const dim3 grid(ceil_div(out_w, kImgTileW), ceil_div(out_h, kImgTileH), num_views);
  ISF_REQUIRE(grid.y <= 65535, ISF_ERR_ARG, "image_prepass: output too tall");
  hipLaunchKernelGGL(image_prepass_kernel, grid, dim3(kImgThreads), 0, as_stream(stream), raw, views, tables, norm_lut,
                     out_h, out_w, img_out);
  ISF_LAUNCH_CHECK();
  return ISF_OK;
}

}  // extern "C"
