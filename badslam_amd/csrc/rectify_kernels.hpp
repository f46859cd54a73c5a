// rectify_kernels.hpp -- sensor rectification of the raw frame for gfx950: undistortion map, colour undistortion,
// depth-mesh reprojection.  Replaces host code of the reference: BS/undistortion.cc:122-156 and
// BS/input_structure.cc:196-298 (there a CPU mesh build + an OpenGL render + a download).  All arithmetic is fp32,
// nothing is contracted; the expression order of every kernel is written out so that a NumPy float32 restatement can
// follow it operation by operation.
#pragma once

#include "preprocess_kernels.hpp"

namespace bslam {

struct MapEntry { float x, y; };   // 8 bytes per pixel; rows 4 byte aligned (checked by the entry points)

// ------------------------------------------------------------------------------------------------
// Undistortion map.  One thread per target pixel (x, y); target camera pixel-corner, source camera pixel-centre.
//   nx   = ((float(x) + 0.5f) - t.cx) / t.fx                       ny alike
//   mx2  = nx * nx;  my2 = ny * ny;  mxy = nx * ny;  rho2 = mx2 + my2
//   rad  = (k1 * rho2 + (k2 * rho2) * rho2) + ((k3 * rho2) * rho2) * rho2
//   dx   = ((nx + nx * rad) + (2 * p1) * mxy) + p2 * (rho2 + 2 * mx2)
//   dy   = ((ny + ny * rad) + (2 * p2) * mxy) + p1 * (rho2 + 2 * my2)
//   px   = min(max(s.fx * dx + s.cx, 0), float(s.width - 1) - FLT_EPSILON)      py alike
// (RadtanDistortion5::Project LV/camera.h:615-631, clamp BS/undistortion.cc:132-135.)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void undistortion_map_kernel(bslam_radtan_camera s, bslam_camera4f t, Img map) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= map.width || y >= map.height) return;
  const float nx = (((float)x + 0.5f) - t.cx) / t.fx, ny = (((float)y + 0.5f) - t.cy) / t.fy;
  const float mx2 = nx * nx, my2 = ny * ny, mxy = nx * ny, rho2 = mx2 + my2;
  const float rad = (s.k1 * rho2 + (s.k2 * rho2) * rho2) + ((s.k3 * rho2) * rho2) * rho2;
  const float dx = ((nx + nx * rad) + (2.0f * s.p1) * mxy) + s.p2 * (rho2 + 2.0f * mx2);
  const float dy = ((ny + ny * rad) + (2.0f * s.p2) * mxy) + s.p1 * (rho2 + 2.0f * my2);
  const float px = fminf(fmaxf(s.fx * dx + s.cx, 0.0f), (float)(s.width - 1) - 1.1920929e-07f);
  const float py = fminf(fmaxf(s.fy * dy + s.cy, 0.0f), (float)(s.height - 1) - 1.1920929e-07f);
  map.at<MapEntry>(y, x) = MapEntry{px, py};
}

// ------------------------------------------------------------------------------------------------
// Colour undistortion.  One thread per output pixel: one 8 byte map load, four texels of 3 adjacent bytes.
//   ix = min(int(mx), width - 2);  fx = mx - float(ix)              iy, fy alike (mx, my >= 0 by the map's clamp)
//   w00 = (1 - fx) * (1 - fy);  w10 = fx * (1 - fy);  w01 = (1 - fx) * fy;  w11 = fx * fy
//   v   = ((w00 * a + w10 * b) + w01 * c) + w11 * d     a = (iy, ix), b = (iy, ix + 1), c = (iy + 1, ix), d = (iy + 1, ix + 1)
//   out = u8(v + 0.5f)
// The index limit keeps ix + 1 / iy + 1 inside the image for a position on the last column / row (there fx = 1).
// Map entries outside [0, width - 1] x [0, height - 1] (not produced by undistortion_map_kernel) are clamped first.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void undistort_rgb_kernel(Img in, Img map, Img out) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= out.width || y >= out.height) return;
  const MapEntry m = map.at<MapEntry>(y, x);
  const float mx = fminf(fmaxf(m.x, 0.0f), (float)(in.width - 1)), my = fminf(fmaxf(m.y, 0.0f), (float)(in.height - 1));   // NaN -> 0
  const int ix = min((int)mx, in.width - 2), iy = min((int)my, in.height - 2);
  const float fx = mx - (float)ix, fy = my - (float)iy;
  const float w00 = (1.0f - fx) * (1.0f - fy), w10 = fx * (1.0f - fy), w01 = (1.0f - fx) * fy, w11 = fx * fy;
  const uint8_t* top = in.base + (size_t)iy * in.pitch + 3 * (size_t)ix;
  const uint8_t* bottom = top + in.pitch;
  uint8_t* o = out.base + (size_t)y * out.pitch + 3 * (size_t)x;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float a = (float)top[ch], b = (float)top[3 + ch], c = (float)bottom[ch], d = (float)bottom[3 + ch];
    const float v = ((w00 * a + w10 * b) + w01 * c) + w11 * d;
    o[ch] = (uint8_t)(v + 0.5f);
  }
}

// ------------------------------------------------------------------------------------------------
// Depth reprojection: clear, rasterise, resolve.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kZEmpty = 0xFFFFFFFFu;
constexpr int kRasterTile = 16;                  // raw 2 x 2 blocks per tile side
constexpr int kRasterVerts = kRasterTile + 1;    // vertices per tile side

__global__ __launch_bounds__(256) void zbuffer_clear_kernel(uint32_t* zbuffer, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) zbuffer[i] = kZEmpty;
}

struct RasterVertex { float px, py, z; };

// edge function of p against the line a -> b:  (b.px - a.px) * (py - a.py) - (b.py - a.py) * (px - a.px)
__device__ __forceinline__ float edge_function(const RasterVertex& a, const RasterVertex& b, float px, float py) {
  return (b.px - a.px) * (py - a.py) - (b.py - a.py) * (px - a.px);
}

// One triangle (v0, v1, v2) into the z-buffer.  Every edge is evaluated from its endpoint with the lower mesh index to
// the one with the higher (the callers pass v0 < v1 < v2 in that order), and the same two vertices in the same order
// give bit-identical values in both triangles that share the edge: a pixel centre can not fall between them.
//   w0 = edge(v1 -> v2), w1 = -edge(v0 -> v2), w2 = edge(v0 -> v1), each at the centre (i + 0.5, j + 0.5)
//   covered: w0, w1, w2 all >= 0 or all <= 0;  s = (w0 + w1) + w2, skipped when 0
//   z = 1 / ((w0 / s) / v0.z + (w1 / s) / v1.z + (w2 / s) / v2.z), summed left to right
// The bounding box is [ceil(min - 0.5), floor(max - 0.5)] per axis, clipped to the image in fp32 before the conversion.
__device__ __forceinline__ void rasterize_triangle(const RasterVertex& v0, const RasterVertex& v1, const RasterVertex& v2, uint32_t* zbuffer, int width,
                                                   int height) {
  if (edge_function(v0, v1, v2.px, v2.py) == 0.0f) return;   // zero area
  const float min_x = fminf(fminf(v0.px, v1.px), v2.px), max_x = fmaxf(fmaxf(v0.px, v1.px), v2.px);
  const float min_y = fminf(fminf(v0.py, v1.py), v2.py), max_y = fmaxf(fmaxf(v0.py, v1.py), v2.py);
  const int i0 = (int)fminf(fmaxf(ceilf(min_x - 0.5f), 0.0f), (float)width), i1 = (int)fmaxf(fminf(floorf(max_x - 0.5f), (float)(width - 1)), -1.0f);
  const int j0 = (int)fminf(fmaxf(ceilf(min_y - 0.5f), 0.0f), (float)height), j1 = (int)fmaxf(fminf(floorf(max_y - 0.5f), (float)(height - 1)), -1.0f);
  for (int j = j0; j <= j1; ++j) {
    const float cy = (float)j + 0.5f;
    for (int i = i0; i <= i1; ++i) {
      const float cx = (float)i + 0.5f;
      const float w0 = edge_function(v1, v2, cx, cy), w1 = -edge_function(v0, v2, cx, cy), w2 = edge_function(v0, v1, cx, cy);
      if (!((w0 >= 0.0f && w1 >= 0.0f && w2 >= 0.0f) || (w0 <= 0.0f && w1 <= 0.0f && w2 <= 0.0f))) continue;
      const float s = (w0 + w1) + w2;
      if (s == 0.0f) continue;
      const float z = 1.0f / (((w0 / s) / v0.z + (w1 / s) / v1.z) + (w2 / s) / v2.z);
      if (z > 0.0f) atomicMin(&zbuffer[(size_t)j * width + i], __float_as_uint(z));   // positive floats order like their bits
    }
  }
}

// A block takes a 16 x 16 tile of raw 2 x 2 pixel blocks: its 17 x 17 vertices are projected once into LDS (px, py, z
// and the raw depth in metres, 0 = no vertex: 4.6 KB), then each thread draws the two triangles of its pixel block.
//   d  = float(raw) * input_depth_to_metres;  X = d * ux;  Y = d * uy;  Z = d
//   tx = ((m0 * X + m1 * Y) + m2 * Z) + m3    ty, tz alike with rows 1, 2 of target_T_depth
//   px = t.fx * (tx / tz) + t.cx;  py = t.fy * (ty / tz) + t.cy;  z = tz
// Pixel block (x, y): vertices 0 = (x, y), 1 = (x + 1, y), 2 = (x, y + 1), 3 = (x + 1, y + 1); triangles (0, 1, 2) and
// (1, 2, 3) (BS/input_structure.cc:235-245, the second reordered by index).  Both are dropped unless all four depths
// are non-zero, the largest of the six |d_a - d_b| is < threshold, and every z lies in [0.05, 50].
__global__ __launch_bounds__(256) void reproject_depth_kernel(Img depth, float input_depth_to_metres, Img unprojection, bslam_mat3x4 T, bslam_camera4f t,
                                                              float threshold, uint32_t* zbuffer) {
  __shared__ RasterVertex vertex[kRasterVerts * kRasterVerts];
  __shared__ float metres[kRasterVerts * kRasterVerts];
  const int tile_x = blockIdx.x * kRasterTile, tile_y = blockIdx.y * kRasterTile;
  for (int i = threadIdx.x; i < kRasterVerts * kRasterVerts; i += 256) {
    const int vy = i / kRasterVerts, vx = i - vy * kRasterVerts;
    const int x = tile_x + vx, y = tile_y + vy;
    float d = 0.0f;
    RasterVertex v = {0.0f, 0.0f, 0.0f};
    if (x < depth.width && y < depth.height) {
      d = (float)depth.at<uint16_t>(y, x) * input_depth_to_metres;
      const MapEntry u = unprojection.at<MapEntry>(y, x);
      const float X = d * u.x, Y = d * u.y, Z = d;
      const float tx = ((T.m[0] * X + T.m[1] * Y) + T.m[2] * Z) + T.m[3];
      const float ty = ((T.m[4] * X + T.m[5] * Y) + T.m[6] * Z) + T.m[7];
      const float tz = ((T.m[8] * X + T.m[9] * Y) + T.m[10] * Z) + T.m[11];
      v.px = t.fx * (tx / tz) + t.cx;
      v.py = t.fy * (ty / tz) + t.cy;
      v.z = tz;
    }
    vertex[i] = v;
    metres[i] = d;
  }
  __syncthreads();
  const int qy = threadIdx.x / kRasterTile, qx = threadIdx.x - qy * kRasterTile;
  if (tile_x + qx + 1 >= depth.width || tile_y + qy + 1 >= depth.height) return;
  const int i00 = qy * kRasterVerts + qx;
  const float d0 = metres[i00], d1 = metres[i00 + 1], d2 = metres[i00 + kRasterVerts], d3 = metres[i00 + kRasterVerts + 1];
  if (!(d0 > 0.0f && d1 > 0.0f && d2 > 0.0f && d3 > 0.0f)) return;
  const float max_diff = fmaxf(fmaxf(fmaxf(fabsf(d0 - d1), fabsf(d0 - d2)), fmaxf(fabsf(d0 - d3), fabsf(d1 - d2))), fmaxf(fabsf(d1 - d3), fabsf(d2 - d3)));
  if (!(max_diff < threshold)) return;
  const RasterVertex v0 = vertex[i00], v1 = vertex[i00 + 1], v2 = vertex[i00 + kRasterVerts], v3 = vertex[i00 + kRasterVerts + 1];
  const float z_min = fminf(fminf(v0.z, v1.z), fminf(v2.z, v3.z)), z_max = fmaxf(fmaxf(v0.z, v1.z), fmaxf(v2.z, v3.z));
  if (!(z_min >= 0.05f && z_max <= 50.0f)) return;   // dropped, not clipped (BS/input_structure.cc:282 clips at these planes)
  rasterize_triangle(v0, v1, v2, zbuffer, t.width, t.height);
  rasterize_triangle(v1, v2, v3, zbuffer, t.width, t.height);
}

// r = output_metres_to_depth * z + 0.5f;  out = r < 65536 ? u16(r) : 0;  empty -> 0
__global__ __launch_bounds__(256) void zbuffer_resolve_kernel(const uint32_t* zbuffer, float output_metres_to_depth, Img out) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= out.width || y >= out.height) return;
  const uint32_t bits = zbuffer[(size_t)y * out.width + x];
  uint16_t value = 0;
  if (bits != kZEmpty) {
    const float r = output_metres_to_depth * __uint_as_float(bits) + 0.5f;
    if (r < 65536.0f) value = (uint16_t)r;
  }
  out.at<uint16_t>(y, x) = value;
}

}  // namespace bslam
