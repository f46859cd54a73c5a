// preprocess_kernels.hpp -- keyframe preprocessing producers for gfx950: brightness,
// bilateral depth filter + cutoff, pixel normals, point radii + isolated-pixel removal, min / max depth; before them
// the input conditioning of the raw frame (depth median + densify, depth / rgb pyramid level).
// Replaces BS/cuda_image_processing.cu:165-194 and BS/cuda_depth_processing.cu:42-465.  These define the
// u16 / half / uchar4 image formats the bundle-adjustment kernels read.  All outputs are
// integers (u8 / u16 / half bits): they are compared bit for bit with the oracle.
#pragma once

#include <hip/hip_fp16.h>

#include "device_math.hpp"

namespace bslam {

struct Img {   // pitched 2-D image
  uint8_t* base; uint32_t pitch; int width, height;
  template <class T> __device__ __forceinline__ T& at(int y, int x) const { return *((T*)(base + (size_t)y * pitch) + x); }
};

// ------------------------------------------------------------------------------------------------
// Input conditioning of BadSlam::PreprocessFrame (BS/bad_slam.cc:645-685), which the reference runs on the host with a
// sort per pixel: 3x3 median + densify, median downscale of the raw depth, half-size steps of the rgb image.
// ------------------------------------------------------------------------------------------------

// The median of the non-zero values of v[0..N) (0 = no measurement); *count = how many there are.  An odd count gives
// the middle value.  An even count gives the lower middle value if it is strictly nearer to the fp32 mean than the upper
// one, else the upper one (BS/preprocessing.cc:66-76, LV/image.h:1033-1047): the sum (<= 64 * 65535) is exact in fp32,
// the division is correctly rounded and the differences are fp32 subtractions.  The middle value is found by a binary
// search on its 16 bits, counting the values below each candidate, so v is only ever indexed by unrolled loops and
// stays in registers for N = 4 ... 64 alike.  Undefined for a count of 0.
template <int N>
__device__ __forceinline__ uint32_t nonzero_median(const uint32_t (&v)[N], uint32_t* count) {
  constexpr uint32_t kAbsent = 0x10000u;   // above every u16: never below a candidate
  uint32_t key[N], n = 0, sum = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    n += (v[i] != 0) ? 1u : 0u;
    sum += v[i];
    key[i] = v[i] ? v[i] : kAbsent;
  }
  *count = n;
  const uint32_t k = (n - 1) >> 1;   // 0-based rank of the (lower) middle value
  uint32_t low = 0;                  // the largest x with #{key < x} <= k
  for (int bit = 15; bit >= 0; --bit) {
    const uint32_t candidate = low | (1u << bit);
    uint32_t below = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) below += (key[i] < candidate) ? 1u : 0u;
    if (below <= k) low = candidate;
  }
  if (n & 1u) return low;
  uint32_t at_most = 0, next = kAbsent;   // the upper middle value: `low` again if it occurs often enough, else the next larger value
#pragma unroll
  for (int i = 0; i < N; ++i) {
    at_most += (key[i] <= low) ? 1u : 0u;
    next = min(next, (key[i] > low) ? key[i] : kAbsent);
  }
  const uint32_t high = (at_most > (n >> 1)) ? low : next;
  const float average = (float)sum / (float)n;
  return (fabsf((float)low - average) < fabsf((float)high - average)) ? low : high;
}

// R consecutive u16 of one row -> v[0..R); wide: one R * 2 byte load (p must be aligned to it)
template <int R>
__device__ __forceinline__ void load_depth_run(const uint16_t* p, bool wide, uint32_t* v) {
  struct alignas(2 * R) Packed { uint32_t d[R / 2]; };
  if (wide) {
    const Packed packed = *(const Packed*)p;
#pragma unroll
    for (int i = 0; i < R / 2; ++i) { v[2 * i] = packed.d[i] & 0xffffu; v[2 * i + 1] = packed.d[i] >> 16; }
  } else {
#pragma unroll
    for (int i = 0; i < R; ++i) v[i] = p[i];
  }
}

// MedianFilterAndDensifyDepthMap BS/preprocessing.cc:40-85, one iteration.  A thread makes 4 adjacent pixels from the
// 3 x 6 values around them.  Clipping the window at the border = padding with 0, because zeros are not collected.
// rows_aligned: every row of both images starts on an 8 byte boundary.
__global__ __launch_bounds__(256) void median_densify_kernel(Img in, Img out, int quads_per_row, bool rows_aligned) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = q / quads_per_row, x0 = 4 * (q - y * quads_per_row);
  if (y >= in.height) return;
  const bool wide = rows_aligned && x0 + 3 < in.width;
  uint32_t v[3][6];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int i = 0; i < 6; ++i) v[r][i] = 0;
    const int sy = y + r - 1;
    if (sy < 0 || sy >= in.height) continue;
    const uint16_t* row = (const uint16_t*)(in.base + (size_t)sy * in.pitch);
    if (wide) {
      load_depth_run<4>(row + x0, true, &v[r][1]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (x0 + i < in.width) v[r][1 + i] = row[x0 + i];
    }
    if (x0 > 0) v[r][0] = row[x0 - 1];
    if (x0 + 4 < in.width) v[r][5] = row[x0 + 4];
  }
  uint32_t result[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const uint32_t window[9] = {v[0][p], v[0][p + 1], v[0][p + 2], v[1][p], v[1][p + 1], v[1][p + 2], v[2][p], v[2][p + 1], v[2][p + 2]};
    uint32_t count;
    const uint32_t median = nonzero_median<9>(window, &count);
    result[p] = (count >= 2) ? median : v[1][p + 1];   // kMinNeighbors = 2: otherwise the pixel stays what it is
  }
  uint16_t* out_row = (uint16_t*)(out.base + (size_t)y * out.pitch);
  if (wide) {
    *(uint2*)(out_row + x0) = make_uint2(result[0] | (result[1] << 16), result[2] | (result[3] << 16));
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p)
      if (x0 + p < out.width) out_row[x0 + p] = (uint16_t)result[p];
  }
}

// Image<u16>::DownscaleUsingMedianWhileExcluding(0, ...) LV/image.h:1003-1053 for in = out * 2^L: one output pixel per
// thread from its 2^L x 2^L block.  rows_aligned: every input row starts on a 2 * 2^L byte boundary.
template <int L>
__global__ __launch_bounds__(256) void downscale_depth_median_kernel(Img in, Img out, bool rows_aligned) {
  constexpr int S = 1 << L;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = q / out.width, x = q - y * out.width;
  if (y >= out.height) return;
  uint32_t v[S * S];
#pragma unroll
  for (int i = 0; i < S; ++i)
    load_depth_run<S>((const uint16_t*)(in.base + (size_t)(y * S + i) * in.pitch) + (size_t)x * S, rows_aligned, &v[i * S]);
  uint32_t count;
  const uint32_t median = nonzero_median<S * S>(v, &count);
  out.at<uint16_t>(y, x) = (uint16_t)(count ? median : 0u);
}

// L times Image<Vec3u8>::DownscaleToHalfSize (LV/image.h:929-948, LV/image_cache.h:212-231) in one pass: one output
// byte (pixel, channel) per thread from its 2^L x 2^L block.  One step is a / 4 + b / 4 + c / 4 + d / 4 with each
// quotient truncated, so the steps do not collapse into one box mean.
template <int L>
__global__ __launch_bounds__(256) void downscale_rgb_kernel(Img in, Img out) {
  constexpr int S = 1 << L;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int row_bytes = 3 * out.width;
  const int y = q / row_bytes, b = q - y * row_bytes;
  if (y >= out.height) return;
  const int x = b / 3, channel = b - 3 * x;
  const uint8_t* block = in.base + (size_t)(y * S) * in.pitch + 3 * (size_t)(x * S) + channel;
  uint32_t v[S][S];
#pragma unroll
  for (int i = 0; i < S; ++i)
#pragma unroll
    for (int j = 0; j < S; ++j) v[i][j] = block[(size_t)i * in.pitch + 3 * j];
  // in place: step l leaves its (S >> l + 1)^2 results in the top left corner; v[i][j] is written after its last read
#pragma unroll
  for (int l = 0; l < L; ++l)
#pragma unroll
    for (int i = 0; i < S / 2; ++i)
#pragma unroll
      for (int j = 0; j < S / 2; ++j)
        if (i < (S >> (l + 1)) && j < (S >> (l + 1))) v[i][j] = v[2 * i][2 * j] / 4 + v[2 * i][2 * j + 1] / 4 + v[2 * i + 1][2 * j] / 4 + v[2 * i + 1][2 * j + 1] / 4;
  out.base[(size_t)y * out.pitch + b] = (uint8_t)v[0][0];
}

// ComputeBrightnessKernel BS/cuda_image_processing.cu:165-176: rgb (3 B / pixel) -> rgb + luma
__global__ __launch_bounds__(256) void brightness_kernel(Img rgb, Img color) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= color.width || y >= color.height) return;
  const uint8_t* p = rgb.base + (size_t)y * rgb.pitch + 3 * (size_t)x;
  const uint32_t r = p[0], g = p[1], b = p[2];
  const uint32_t intensity = (uint32_t)f2i((0.299f * (float)r + 0.587f * (float)g + 0.114f * (float)b) + 0.5f) & 0xffu;
  color.at<uint32_t>(y, x) = r | (g << 8) | (b << 16) | (intensity << 24);
}

// BilateralFilteringAndDepthCutoffCUDAKernel BS/cuda_depth_processing.cu:42-100
__global__ __launch_bounds__(256) void bilateral_kernel(float denom_xy, float denom_value, int radius, int radius_squared, uint32_t max_depth,
                                                       float raw_to_float_depth, Img in, Img out) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= out.width || y >= out.height) return;
  const uint32_t center_value = in.at<uint16_t>(y, x);
  if (center_value == 0 || center_value > max_depth) { out.at<uint16_t>(y, x) = BSLAM_UNKNOWN_DEPTH; return; }
  const float inv_center_value = 1.0f / (raw_to_float_depth * (float)center_value);
  float sum = 0, weight = 0;
  const int min_y = max(0, y - radius), max_y = min(out.height - 1, y + radius);
  const int min_x = max(0, x - radius), max_x = min(out.width - 1, x + radius);
  for (int sy = min_y; sy <= max_y; ++sy) {
    const int dy = sy - y;
    for (int sx = min_x; sx <= max_x; ++sx) {
      const int dx = sx - x;
      const int grid_distance_squared = dx * dx + dy * dy;
      if (grid_distance_squared > radius_squared) continue;
      const uint32_t sample = in.at<uint16_t>(sy, sx);
      if (sample == 0) continue;
      const float inv_sample = 1.0f / (raw_to_float_depth * (float)sample);
      float value_distance_squared = inv_center_value - inv_sample;
      value_distance_squared *= value_distance_squared;
      const float w = det_expf((float)(-grid_distance_squared) / denom_xy + -value_distance_squared / denom_value);
      sum += w * inv_sample;
      weight += w;
    }
  }
  if (weight == 0) { out.at<uint16_t>(y, x) = BSLAM_UNKNOWN_DEPTH; return; }
  const float v = 1.0f / (raw_to_float_depth * sum / weight);
  out.at<uint16_t>(y, x) = (uint16_t)min(65535, max(0, f2i(v)));   // cvt.rzi.u16.f32 saturates
}

__device__ __forceinline__ uint32_t small_float_to_s8(float value) {   // BS/util.cuh:105-107
  return (uint32_t)f2i(value * 127 + ((value > 0) ? 0.5f : -0.5f)) & 0xffu;
}
__device__ __forceinline__ uint32_t image_space_normal_to_u16(float x, float y) { return small_float_to_s8(x) | (small_float_to_s8(y) << 8); }

// ComputeNormalsCUDAKernel BS/cuda_depth_processing.cu:134-255
__global__ __launch_bounds__(256) void normals_kernel(CamConsts c, Img in, Img out_depth, Img out_normals) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= in.width || y >= in.height) return;
  const uint32_t zero_normal = image_space_normal_to_u16(0, 0);
  constexpr int kBorder = 1;
  bool ok = !(x < kBorder || y < kBorder || x >= in.width - kBorder || y >= in.height - kBorder);
  uint32_t cc = 0, rr = 0, ll = 0, bb = 0, tt = 0;
  if (ok) {
    cc = in.at<uint16_t>(y, x);
    ok = !(cc & BSLAM_INVALID_DEPTH_BIT);
  }
  if (ok) {
    rr = in.at<uint16_t>(y, x + 1); ll = in.at<uint16_t>(y, x - 1); bb = in.at<uint16_t>(y + 1, x); tt = in.at<uint16_t>(y - 1, x);
    ok = !((rr | ll | bb | tt) & BSLAM_INVALID_DEPTH_BIT);
  }
  if (!ok) { out_depth.at<uint16_t>(y, x) = BSLAM_UNKNOWN_DEPTH; out_normals.at<uint16_t>(y, x) = (uint16_t)zero_normal; return; }
  auto cf = [&](int yy, int xx) { return *(const float*)((const uint8_t*)c.cfactor + (size_t)(yy / c.cell) * c.cfactor_pitch + 4 * (size_t)(xx / c.cell)); };
  const float center_depth = raw_to_calibrated_depth(c.a, cf(y, x), c.raw_to_float_depth, cc);
  const float left_depth = raw_to_calibrated_depth(c.a, cf(y, x - 1), c.raw_to_float_depth, ll);
  const float top_depth = raw_to_calibrated_depth(c.a, cf(y - 1, x), c.raw_to_float_depth, tt);
  const float right_depth = raw_to_calibrated_depth(c.a, cf(y, x + 1), c.raw_to_float_depth, rr);
  const float bottom_depth = raw_to_calibrated_depth(c.a, cf(y + 1, x), c.raw_to_float_depth, bb);
  const f3 left_point = unproject(c, x - 1, y, left_depth);
  const f3 top_point = unproject(c, x, y - 1, top_depth);
  const f3 right_point = unproject(c, x + 1, y, right_depth);
  const f3 bottom_point = unproject(c, x, y + 1, bottom_depth);
  const f3 center_point = unproject(c, x, y, center_depth);
  constexpr float kRatioThresholdSquared = 2.f * 2.f;
  const float left_dist_squared = sqlen(sub3(left_point, center_point));
  const float right_dist_squared = sqlen(sub3(right_point, center_point));
  const float left_right_ratio = left_dist_squared / right_dist_squared;
  f3 left_to_right;
  if (left_right_ratio < kRatioThresholdSquared && left_right_ratio > 1.f / kRatioThresholdSquared) left_to_right = sub3(right_point, left_point);
  else if (left_dist_squared < right_dist_squared) left_to_right = sub3(center_point, left_point);
  else left_to_right = sub3(right_point, center_point);
  const float bottom_dist_squared = sqlen(sub3(bottom_point, center_point));
  const float top_dist_squared = sqlen(sub3(top_point, center_point));
  const float bottom_top_ratio = bottom_dist_squared / top_dist_squared;
  f3 bottom_to_top;
  if (bottom_top_ratio < kRatioThresholdSquared && bottom_top_ratio > 1.f / kRatioThresholdSquared) bottom_to_top = sub3(top_point, bottom_point);
  else if (bottom_dist_squared < top_dist_squared) bottom_to_top = sub3(center_point, bottom_point);
  else bottom_to_top = sub3(top_point, center_point);
  f3 normal = cross(left_to_right, bottom_to_top);
  const float length = norm3(normal);
  if (!(length > 1e-6f)) {
    normal = mk3(0, 0, -1);
  } else {
    const float inv_length = ((c.fy_inv < 0) ? -1.0f : 1.0f) / length;
    normal.x *= inv_length;
    normal.y *= inv_length;
  }
  out_normals.at<uint16_t>(y, x) = (uint16_t)image_space_normal_to_u16(normal.x, normal.y);
  out_depth.at<uint16_t>(y, x) = (uint16_t)cc;
}

// ComputePointRadiiAndRemoveIsolatedPixelsCUDAKernel<4> BS/cuda_depth_processing.cu:286-357
__global__ __launch_bounds__(256) void radii_kernel(CamConsts c, float raw_to_float_depth, Img in, Img out_radius, Img out_depth) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= in.width || y >= in.height) return;
  const uint32_t d16 = in.at<uint16_t>(y, x);
  if (d16 & BSLAM_INVALID_DEPTH_BIT) {
    out_depth.at<uint16_t>(y, x) = BSLAM_UNKNOWN_DEPTH;
    out_radius.at<uint16_t>(y, x) = 0;   // the reference leaves it unwritten
    return;
  }
  const float depth = raw_to_float_depth * (float)d16;
  const f3 local = mk3(depth * (c.fx_inv * x + c.cx_inv), depth * (c.fy_inv * y + c.cy_inv), depth);
  int neighbor_count = 0;
  float min_sq = __uint_as_float(0x7f800000u);
  for (int dy = y - 1; dy < y + 2; ++dy) {
    for (int dx = x - 1; dx < x + 2; ++dx) {
      if ((dx != x && dy != y) || (dx == x && dy == y)) continue;
      if (dx < 0 || dy < 0 || dx >= in.width || dy >= in.height) continue;
      const uint32_t dd = in.at<uint16_t>(dy, dx);
      if (dd & BSLAM_INVALID_DEPTH_BIT) continue;
      ++neighbor_count;
      const float ddepth = raw_to_float_depth * (float)dd;
      const f3 other = mk3(ddepth * (c.fx_inv * dx + c.cx_inv), ddepth * (c.fy_inv * dy + c.cy_inv), ddepth);
      const float dsq = sqlen(sub3(other, local));
      if (dsq < min_sq) min_sq = dsq;
    }
  }
  const bool valid = neighbor_count >= 4;
  out_radius.at<uint16_t>(y, x) = __half_as_ushort(__float2half_rn(valid ? min_sq : 0.f));
  out_depth.at<uint16_t>(y, x) = valid ? (uint16_t)d16 : (uint16_t)BSLAM_UNKNOWN_DEPTH;
}

// ComputeMinMaxDepthCUDAKernel BS/cuda_depth_processing.cu:391-428: positive floats order like their bit patterns
__global__ __launch_bounds__(256) void min_max_depth_kernel(float raw_to_float_depth, Img depth, uint32_t* __restrict__ result /* [2] */) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  float mn = __uint_as_float(0x7f800000u), mx = 0.f;
  if (x < depth.width && y < depth.height) {
    const uint32_t d16 = depth.at<uint16_t>(y, x);
    if (!(d16 & BSLAM_INVALID_DEPTH_BIT)) mn = mx = raw_to_float_depth * (float)d16;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, off, 64));
    mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&result[0], __float_as_uint(mn));
    atomicMax(&result[1], __float_as_uint(mx));
  }
}

}  // namespace bslam
