// render_kernels.hpp -- views of the surfel model for gfx950: every surfel is an oriented disc, drawn into a z-buffer of
// 64-bit keys that keeps the nearest surface per pixel, then resolved into depth / index / colour / normal images.
// Stands in for the reference's on-screen view of the model (BS/render_window.cc, BS/kernel_update_visualization.cu:
// screen-aligned splats of a fixed pixel size through OpenGL).  Like rectify_kernels.hpp: all arithmetic is fp32, nothing
// is contracted, / and sqrtf are correctly rounded, and the expression order is written out so that a NumPy float32
// restatement reproduces the depth, index and colour views bit for bit.
#pragma once

#include "rectify_kernels.hpp"

namespace bslam {

constexpr unsigned long long kKeyEmpty = ~0ull;
constexpr int kSplatSmallBox = 64;   // pixel centres a lane draws itself; larger boxes are drawn by the whole wave

__global__ __launch_bounds__(256) void render_clear_kernel(unsigned long long* keys, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) keys[i] = kKeyEmpty;
}

// What the pixel test needs of one surfel (wave-uniform in the cooperative path, where it is broadcast from its lane).
struct Splat {
  float Lx, Ly, Lz;   // centre in the camera frame
  float nx, ny, nz;   // normal in the camera frame, not normalised
  float r2, k;        // scaled squared radius;  k = n . L  (< 0: front-facing)
  uint32_t index;     // surfel column
  int i0, i1, j0, j1; // box of pixel centres to test, inside the image; empty when i1 < i0 or j1 < j0
};

// The surfel rows a view reads.
struct RenderRows {
  const float* x; const float* y; const float* z;
  const uint32_t* normal;
  const float* radius_squared;
  const uint32_t* color;
  uint32_t size;
};

// Prologue of surfel s; false: the surfel draws nothing.
//   x != x                                             -> skipped (merged / deleted)
//   L.x = ((m0 * x + m1 * y) + m2 * z) + m3            L.y, L.z alike with rows 1, 2 of camera_T_global
//   sx, sy, sz = the sign-extended 10-bit fields of the packed normal as floats (no 1 / 511, no normalisation: the
//                intersection below does not depend on the normal's length)
//   n.x = (m0 * sx + m1 * sy) + m2 * sz                n.y, n.z alike
//   r2  = radius_squared * (radius_scale * radius_scale);  skipped unless r2 > 0;  r = sqrtf(r2)
//   skipped unless L.z - r >= min_depth and L.z <= max_depth (dropped, not clipped)
//   k   = (n.x * L.x + n.y * L.y) + n.z * L.z;         skipped unless k < 0 (back faces, zero normals)
// Box: the disc lies in the ball (L, r) and L.z - r > 0, so X / Z of every point of it lies between the four quotients
// (L.x -/+ r) / (L.z -/+ r); pixel-corner positions fx * q + cx of the smallest and largest, turned into centre indices
// [ceil(min - 0.5), floor(max - 0.5)], widened by one pixel and clipped to the image in fp32 before the conversion to int
// (as rasterize_triangle does).  Non-finite intermediates give some box inside the image; such a surfel covers no pixel.
__device__ __forceinline__ bool splat_prologue(const RenderRows& rows, uint32_t s, const bslam_mat3x4& T, const bslam_camera4f& cam, float min_depth,
                                               float max_depth, float radius_scale, Splat* out) {
  const float x = rows.x[s];
  if (x != x) return false;
  const float y = rows.y[s], z = rows.z[s];
  const float Lx = ((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3];
  const float Ly = ((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7];
  const float Lz = ((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11];
  const uint32_t packed = rows.normal[s];
  const float sx = (float)(((int32_t)(packed << 22)) >> 22), sy = (float)(((int32_t)(packed << 12)) >> 22), sz = (float)(((int32_t)(packed << 2)) >> 22);
  const float nx = (T.m[0] * sx + T.m[1] * sy) + T.m[2] * sz;
  const float ny = (T.m[4] * sx + T.m[5] * sy) + T.m[6] * sz;
  const float nz = (T.m[8] * sx + T.m[9] * sy) + T.m[10] * sz;
  const float r2 = rows.radius_squared[s] * (radius_scale * radius_scale);
  if (!(r2 > 0.0f)) return false;
  const float r = sqrtf(r2);
  if (!(Lz - r >= min_depth && Lz <= max_depth)) return false;
  const float k = (nx * Lx + ny * Ly) + nz * Lz;
  if (!(k < 0.0f)) return false;
  const float z_near = Lz - r, z_far = Lz + r;
  const float xa = (Lx - r) / z_near, xb = (Lx - r) / z_far, xc = (Lx + r) / z_near, xd = (Lx + r) / z_far;
  const float ya = (Ly - r) / z_near, yb = (Ly - r) / z_far, yc = (Ly + r) / z_near, yd = (Ly + r) / z_far;
  const float min_px = cam.fx * fminf(fminf(xa, xb), fminf(xc, xd)) + cam.cx, max_px = cam.fx * fmaxf(fmaxf(xa, xb), fmaxf(xc, xd)) + cam.cx;
  const float min_py = cam.fy * fminf(fminf(ya, yb), fminf(yc, yd)) + cam.cy, max_py = cam.fy * fmaxf(fmaxf(ya, yb), fmaxf(yc, yd)) + cam.cy;
  const float w = (float)cam.width, h = (float)cam.height;
  const int i0 = (int)fminf(fmaxf(ceilf(min_px - 0.5f) - 1.0f, 0.0f), w), i1 = (int)fmaxf(fminf(floorf(max_px - 0.5f) + 1.0f, w - 1.0f), -1.0f);
  const int j0 = (int)fminf(fmaxf(ceilf(min_py - 0.5f) - 1.0f, 0.0f), h), j1 = (int)fmaxf(fminf(floorf(max_py - 0.5f) + 1.0f, h - 1.0f), -1.0f);
  out->Lx = Lx; out->Ly = Ly; out->Lz = Lz;
  out->nx = nx; out->ny = ny; out->nz = nz;
  out->r2 = r2; out->k = k;
  out->index = s;
  out->i0 = i0; out->j0 = j0;
  out->i1 = min(i1, cam.width - 1); out->j1 = min(j1, cam.height - 1);   // (float)(width - 1) may round up above 2^24
  return true;
}

// Pixel centre (i + 0.5, j + 0.5) against one surfel; (i, j) lies inside the image.
//   dx  = ((float(i) + 0.5f) - cx) / fx                dy alike
//   den = (n.x * dx + n.y * dy) + n.z;                 skipped unless den < 0
//   t   = k / den                                      (> 0: depth of the ray's intersection with the disc's plane)
//   hx  = t * dx - L.x;  hy = t * dy - L.y;  hz = t - L.z
//   covered iff (hx * hx + hy * hy) + hz * hz <= r2
//   key = (float_bits(t) << 32) | index;  the pixel keeps the smallest key: positive floats order like their bits, so that
//         is the nearest surface, and among equal depths the lower surfel index, whatever the order of arrival.
// Keys only decrease, so a plain load that already shows a key <= ours (even a stale one) means the atomic cannot win.
__device__ __forceinline__ void splat_pixel(const Splat& s, int i, int j, const bslam_camera4f& cam, unsigned long long* keys) {
  const float dx = (((float)i + 0.5f) - cam.cx) / cam.fx, dy = (((float)j + 0.5f) - cam.cy) / cam.fy;
  const float den = (s.nx * dx + s.ny * dy) + s.nz;
  if (!(den < 0.0f)) return;
  const float t = s.k / den;
  const float hx = t * dx - s.Lx, hy = t * dy - s.Ly, hz = t - s.Lz;
  if (!((hx * hx + hy * hy) + hz * hz <= s.r2)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(t) << 32) | s.index;
  unsigned long long* slot = keys + ((size_t)j * cam.width + i);
  if (*slot > key) atomicMin(slot, key);
}

// One thread per surfel.  A lane whose box holds at most kSplatSmallBox centres walks it itself, columns inner.  The other
// lanes of the wave are collected with a ballot, and all 64 lanes stride over each such box together in row-major order
// (a wave-instruction's atomics fall on runs of adjacent keys), with the surfel's constants broadcast from its lane: a
// surfel close to the camera does not hold a wave behind one lane.  A minimum does not care who issues it, so the result is
// that of testing every pixel against every surfel.  No thread leaves before the ballot; the loop over the ballot's bits is
// wave-uniform, and the strided loop inside it, whose trip count differs between lanes, holds no wave-wide operation.
__global__ __launch_bounds__(256) void render_splat_kernel(RenderRows rows, bslam_mat3x4 T, bslam_camera4f cam, float min_depth, float max_depth,
                                                           float radius_scale, unsigned long long* keys) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  Splat mine;
  mine.Lx = mine.Ly = mine.Lz = mine.nx = mine.ny = mine.nz = mine.r2 = mine.k = 0.0f;
  mine.index = s;
  mine.i0 = mine.j0 = 0;
  mine.i1 = mine.j1 = -1;
  bool live = s < rows.size && splat_prologue(rows, s, T, cam, min_depth, max_depth, radius_scale, &mine);
  live = live && mine.i1 >= mine.i0 && mine.j1 >= mine.j0;
  const uint32_t box_w = live ? (uint32_t)(mine.i1 - mine.i0 + 1) : 0u, box_h = live ? (uint32_t)(mine.j1 - mine.j0 + 1) : 0u;
  const bool large = box_w * box_h > (uint32_t)kSplatSmallBox;   // box_w * box_h <= width * height <= 2^31 - 1
  if (live && !large) {
    for (int j = mine.j0; j <= mine.j1; ++j)
      for (int i = mine.i0; i <= mine.i1; ++i) splat_pixel(mine, i, j, cam, keys);
  }
  unsigned long long todo = __ballot(large);
  const int lane = (int)(threadIdx.x & 63u);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    Splat b;
    b.Lx = __shfl(mine.Lx, src); b.Ly = __shfl(mine.Ly, src); b.Lz = __shfl(mine.Lz, src);
    b.nx = __shfl(mine.nx, src); b.ny = __shfl(mine.ny, src); b.nz = __shfl(mine.nz, src);
    b.r2 = __shfl(mine.r2, src); b.k = __shfl(mine.k, src);
    b.index = (uint32_t)__shfl((int)mine.index, src);
    b.i0 = __shfl(mine.i0, src); b.i1 = __shfl(mine.i1, src); b.j0 = __shfl(mine.j0, src); b.j1 = __shfl(mine.j1, src);
    // lane l takes the centres l, l + 64, ... of the box in row-major order: (i, j) advances by 64 = q * w + r centres
    const int w = b.i1 - b.i0 + 1, q = 64 / w, r = 64 - q * w;
    int j = b.j0 + lane / w, i = b.i0 + (lane - (lane / w) * w);
    while (j <= b.j1) {
      splat_pixel(b, i, j, cam, keys);
      i += r; j += q;
      if (i > b.i1) { i -= w; ++j; }
    }
  }
}

// One thread per pixel; a null output is not written.
//   depth  u16:     v = metres_to_depth * t + 0.5f;  v < 65536 ? u16(v) : 0;  empty -> 0
//   index  u32:     the surfel column;                                        empty -> 0xFFFFFFFF
//   color  uchar4:  the winner's colour row entry, bits unchanged;            empty -> 0
//   normal 3 x f32: unpack_normal of the winner, rotated: (m0 * n.x + m1 * n.y) + m2 * n.z, rows 1, 2 alike;  empty -> 0
__global__ __launch_bounds__(256) void render_resolve_kernel(const unsigned long long* keys, RenderRows rows, bslam_mat3x4 T, float metres_to_depth, int width,
                                                             int height, Img depth, Img index, Img color, Img normal) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= width || y >= height) return;
  const unsigned long long key = keys[(size_t)y * width + x];
  const bool empty = key == kKeyEmpty;
  const uint32_t s = (uint32_t)key;
  if (depth.base) {
    uint16_t value = 0;
    if (!empty) {
      const float v = metres_to_depth * __uint_as_float((uint32_t)(key >> 32)) + 0.5f;
      if (v < 65536.0f) value = (uint16_t)v;
    }
    depth.at<uint16_t>(y, x) = value;
  }
  if (index.base) index.at<uint32_t>(y, x) = empty ? 0xFFFFFFFFu : s;
  if (color.base) color.at<uint32_t>(y, x) = empty ? 0u : rows.color[s];
  if (normal.base) {
    f3 out = mk3(0.0f, 0.0f, 0.0f);
    if (!empty) {
      const f3 n = unpack_normal(rows.normal[s]);
      out.x = (T.m[0] * n.x + T.m[1] * n.y) + T.m[2] * n.z;
      out.y = (T.m[4] * n.x + T.m[5] * n.y) + T.m[6] * n.z;
      out.z = (T.m[8] * n.x + T.m[9] * n.y) + T.m[10] * n.z;
    }
    float* o = (float*)(normal.base + (size_t)y * normal.pitch) + 3 * (size_t)x;
    o[0] = out.x; o[1] = out.y; o[2] = out.z;
  }
}

}  // namespace bslam
