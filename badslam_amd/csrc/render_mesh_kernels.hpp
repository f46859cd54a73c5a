// render_mesh_kernels.hpp -- views of an indexed triangle mesh for gfx950: the edge-function rasteriser of rectify_kernels.hpp
// (rasterize_triangle, its watertight shared-edge rule) drawn into the 64-bit key z-buffer of render_kernels.hpp, then resolved
// into depth / index / colour / normal images with perspective-correct attributes.  Like those two files: all arithmetic is fp32,
// nothing is contracted, / and sqrtf are correctly rounded, and the expression order is written out so that a NumPy float32
// restatement reproduces the depth, index and colour views bit for bit (tests/render_mesh_util.py).
//
// Vertex stage, vertex v at (x, y, z):
//   L.x = ((m0 * x + m1 * y) + m2 * z) + m3            L.y, L.z alike with rows 1, 2 of camera_T_global (splat_prologue)
//   px  = fx * (L.x / L.z) + cx                        py = fy * (L.y / L.z) + cy          (reproject_depth_kernel)
//   vz  = L.z if L.x, L.y and L.z are all finite, else NaN
// Triangle t = (a, b, c) draws nothing when
//   one of a, b, c is >= vertex_count (never dereferenced; the error word is set);  two of a, b, c are equal;
//   one of its three vz is not in [min_depth, max_depth] (NaN is not: a vertex that is not finite; dropped, not clipped);
//   its pixel-space area in its own winding  A = (b.px - a.px) * (c.py - a.py) - (b.py - a.py) * (c.px - a.px)  is 0;
//   cull_backfaces is set and not A < 0.  A < 0 is front-facing: counter-clockwise seen from the camera in a frame with x right,
//   y down, z forward, the winding of bslam_extract_mesh.  The facing comes from this expression, not from the sign of s below.
// Coverage and depth: (v0, v1, v2) = the three vertices in ascending vertex id, so that every edge is evaluated from the lower id
// to the higher and two triangles that share an edge get bit-identical edge values.  At the centre (i + 0.5, j + 0.5):
//   w0 = edge(v1 -> v2), w1 = -edge(v0 -> v2), w2 = edge(v0 -> v1)        (edge_function of rectify_kernels.hpp)
//   covered iff w0, w1, w2 are all >= 0 or all <= 0, and s = (w0 + w1) + w2 is not 0
//   b_k = (w_k / s) / v_k.z;   z = 1 / ((b0 + b1) + b2);   drawn iff z > 0
// Box: [ceil(min - 0.5), floor(max - 0.5)] per axis over the three px / py, clipped to the image in fp32 before the conversion to
// int and capped once more as ints (splat_prologue).
// Key: (float_bits(z) << 32) | t; the pixel keeps the smallest, i.e. the nearest surface and among bit-equal depths the lower
// triangle id, whatever the order of arrival.
// Who draws a box (a lane, its wave, or eight workgroups), and whether the vertex stage is a pass of its own or runs where a
// vertex is needed, changes no bit: every path evaluates the expressions above (DESIGN.md 8 "Mesh views" has the measurements).
#pragma once

#include "mesh_kernels.hpp"
#include "render_kernels.hpp"

namespace bslam {

// The arrays a mesh view reads, laid out as bslam_extract_mesh writes them.
struct MeshView {
  const float* positions;          // float[3 V]
  const float* normals;            // float[3 V] or null
  const uint32_t* colors;          // uchar4[V] or null
  const uint32_t* indices;         // uint32[3 T]
  const RasterVertex* projected;   // RasterVertex[V], the vertex stage's output, or null: the reader runs the vertex stage itself
  uint32_t vertices, triangles;
};

__device__ __forceinline__ f3 mesh_camera_point(const float* positions, uint32_t v, const bslam_mat3x4& T) {
  const float x = positions[3 * (size_t)v], y = positions[3 * (size_t)v + 1], z = positions[3 * (size_t)v + 2];
  return mk3(((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3], ((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7],
             ((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11]);
}

__device__ __forceinline__ RasterVertex mesh_project(const f3& L, const bslam_camera4f& cam) {
  RasterVertex r;
  r.px = cam.fx * (L.x / L.z) + cam.cx;
  r.py = cam.fy * (L.y / L.z) + cam.cy;
  r.z = (isfinite(L.x) && isfinite(L.y) && isfinite(L.z)) ? L.z : __uint_as_float(0x7fc00000u);
  return r;
}

// The vertex stage's record of vertex v (< view.vertices): read back, or computed here by the same expressions.
__device__ __forceinline__ RasterVertex mesh_vertex(const MeshView& view, uint32_t v, const bslam_mat3x4& T, const bslam_camera4f& cam) {
  if (view.projected) return view.projected[v];
  return mesh_project(mesh_camera_point(view.positions, v, T), cam);
}

// One thread per vertex.
__global__ __launch_bounds__(256) void render_mesh_vertex_kernel(MeshView view, bslam_mat3x4 T, bslam_camera4f cam, RasterVertex* projected) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < view.vertices) projected[v] = mesh_project(mesh_camera_point(view.positions, v, T), cam);
}

// The winding's area of a triangle given in its own order (a, b, c): see the head of the file.
__device__ __forceinline__ float mesh_winding_area(const RasterVertex& a, const RasterVertex& b, const RasterVertex& c) {
  return (b.px - a.px) * (c.py - a.py) - (b.py - a.py) * (c.px - a.px);
}

// One compare-and-swap of the sort by vertex id: the ids and what travels with them.
template <class V>
__device__ __forceinline__ void mesh_order(uint32_t& ia, uint32_t& ib, V& va, V& vb) {
  if (ia > ib) {
    const uint32_t i = ia; ia = ib; ib = i;
    const V v = va; va = vb; vb = v;
  }
}

// Pixel centre (i + 0.5, j + 0.5) against the triangle (v0, v1, v2), given in ascending vertex id; false: not drawn.
__device__ __forceinline__ bool mesh_pixel(const RasterVertex& v0, const RasterVertex& v1, const RasterVertex& v2, int i, int j, float* b0, float* b1, float* b2,
                                           float* z) {
  const float cx = (float)i + 0.5f, cy = (float)j + 0.5f;
  const float w0 = edge_function(v1, v2, cx, cy), w1 = -edge_function(v0, v2, cx, cy), w2 = edge_function(v0, v1, cx, cy);
  if (!((w0 >= 0.0f && w1 >= 0.0f && w2 >= 0.0f) || (w0 <= 0.0f && w1 <= 0.0f && w2 <= 0.0f))) return false;
  const float s = (w0 + w1) + w2;
  if (s == 0.0f) return false;
  *b0 = (w0 / s) / v0.z; *b1 = (w1 / s) / v1.z; *b2 = (w2 / s) / v2.z;
  *z = 1.0f / ((*b0 + *b1) + *b2);
  return *z > 0.0f;
}

// What the pixel test needs of one triangle (wave-uniform in the cooperative path, where it is broadcast from its lane).
struct MeshTriangle {
  RasterVertex v0, v1, v2;   // in ascending vertex id
  uint32_t index;            // triangle id
  int i0, i1, j0, j1;        // box of pixel centres to test, inside the image; empty when i1 < i0 or j1 < j0
};

// Prologue of triangle t (< view.triangles); false: the triangle draws nothing.  *bad_index: it names a vertex >= view.vertices.
__device__ __forceinline__ bool mesh_triangle_prologue(const MeshView& view, uint32_t t, const bslam_mat3x4& T, const bslam_camera4f& cam, float min_depth,
                                                       float max_depth, int cull_backfaces, MeshTriangle* out, bool* bad_index) {
  const uint32_t a = view.indices[3 * (size_t)t], b = view.indices[3 * (size_t)t + 1], c = view.indices[3 * (size_t)t + 2];
  if (a >= view.vertices || b >= view.vertices || c >= view.vertices) { *bad_index = true; return false; }
  if (a == b || a == c || b == c) return false;
  RasterVertex v0 = mesh_vertex(view, a, T, cam), v1 = mesh_vertex(view, b, T, cam), v2 = mesh_vertex(view, c, T, cam);
  if (!(v0.z >= min_depth && v0.z <= max_depth && v1.z >= min_depth && v1.z <= max_depth && v2.z >= min_depth && v2.z <= max_depth)) return false;
  const float area = mesh_winding_area(v0, v1, v2);
  if (area == 0.0f) return false;
  if (cull_backfaces && !(area < 0.0f)) return false;
  uint32_t id0 = a, id1 = b, id2 = c;
  mesh_order(id0, id1, v0, v1); mesh_order(id1, id2, v1, v2); mesh_order(id0, id1, v0, v1);
  const float min_x = fminf(fminf(v0.px, v1.px), v2.px), max_x = fmaxf(fmaxf(v0.px, v1.px), v2.px);
  const float min_y = fminf(fminf(v0.py, v1.py), v2.py), max_y = fmaxf(fmaxf(v0.py, v1.py), v2.py);
  const float w = (float)cam.width, h = (float)cam.height;
  const int i0 = (int)fminf(fmaxf(ceilf(min_x - 0.5f), 0.0f), w), i1 = (int)fmaxf(fminf(floorf(max_x - 0.5f), w - 1.0f), -1.0f);
  const int j0 = (int)fminf(fmaxf(ceilf(min_y - 0.5f), 0.0f), h), j1 = (int)fmaxf(fminf(floorf(max_y - 0.5f), h - 1.0f), -1.0f);
  out->v0 = v0; out->v1 = v1; out->v2 = v2;
  out->index = t;
  out->i0 = i0; out->j0 = j0;
  out->i1 = min(i1, cam.width - 1); out->j1 = min(j1, cam.height - 1);   // (float)(width - 1) may round up above 2^24
  return true;
}

// Keys only decrease, so a plain load that already shows a key <= ours (even a stale one) means the atomic cannot win (splat_pixel).
__device__ __forceinline__ void mesh_draw_pixel(const MeshTriangle& t, int i, int j, int width, unsigned long long* keys) {
  float b0, b1, b2, z;
  if (!mesh_pixel(t.v0, t.v1, t.v2, i, j, &b0, &b1, &b2, &z)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | t.index;
  unsigned long long* slot = keys + ((size_t)j * width + i);
  if (*slot > key) atomicMin(slot, key);
}

// One thread per triangle, the scheme of render_splat_kernel.  A lane whose box holds at most small_box centres walks it itself,
// columns inner.  The other lanes of the wave are collected with a ballot, and all 64 lanes stride over each such box together
// in row-major order with the triangle's constants broadcast from its lane: a decimated wall a metre from the camera does not
// hold a wave behind one lane.  A minimum does not care who issues it, so the result is that of testing every pixel against
// every triangle.  No thread leaves before the ballot; the loop over the ballot's bits is wave-uniform, and the strided loop
// inside it, whose trip count differs between lanes, holds no wave-wide operation.
// A box of more than wave_box centres is not drawn here: a wave issues one dependent load-and-atomic after another, about a
// microsecond per 64 centres, so a triangle that spans thousands of pixels would still hold its wave, and the other large
// triangles of that wave behind it, for most of the call.  Its id goes to `queue` (words[kMeshQueued] counts them), and
// render_mesh_queue_kernel spreads every queued box over several workgroups.
constexpr int kMeshQueued = 1;          // word that counts the queued triangles (word 0: the error bits)
constexpr int kMeshQueueChunks = 8;     // workgroups that share one queued box
constexpr int kMeshQueueBlocks = 1024;  // grid of render_mesh_queue_kernel: 128 boxes in flight

__global__ __launch_bounds__(256) void render_mesh_draw_kernel(MeshView view, bslam_mat3x4 T, bslam_camera4f cam, float min_depth, float max_depth,
                                                               int cull_backfaces, int small_box, int wave_box, unsigned long long* keys, uint32_t* words,
                                                               uint32_t* queue) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  MeshTriangle mine;
  mine.v0 = mine.v1 = mine.v2 = RasterVertex{0.0f, 0.0f, 0.0f};
  mine.index = t;
  mine.i0 = mine.j0 = 0;
  mine.i1 = mine.j1 = -1;
  bool bad_index = false;
  bool live = t < view.triangles && mesh_triangle_prologue(view, t, T, cam, min_depth, max_depth, cull_backfaces, &mine, &bad_index);
  if (bad_index) atomicOr(&words[0], kMeshBadIndex);
  live = live && mine.i1 >= mine.i0 && mine.j1 >= mine.j0;
  const uint32_t box_w = live ? (uint32_t)(mine.i1 - mine.i0 + 1) : 0u, box_h = live ? (uint32_t)(mine.j1 - mine.j0 + 1) : 0u;
  const uint32_t box = box_w * box_h;                        // <= width * height <= 2^31 - 1
  const bool small = box <= (uint32_t)small_box, queued = !small && box > (uint32_t)wave_box, large = !small && !queued;
  if (queued) queue[atomicAdd(&words[kMeshQueued], 1u)] = t;   // at most one entry per triangle: the queue has room for all
  if (live && small) {
    for (int j = mine.j0; j <= mine.j1; ++j)
      for (int i = mine.i0; i <= mine.i1; ++i) mesh_draw_pixel(mine, i, j, cam.width, keys);
  }
  unsigned long long todo = __ballot(large);
  const int lane = (int)(threadIdx.x & 63u);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    MeshTriangle b;
    b.v0.px = __shfl(mine.v0.px, src); b.v0.py = __shfl(mine.v0.py, src); b.v0.z = __shfl(mine.v0.z, src);
    b.v1.px = __shfl(mine.v1.px, src); b.v1.py = __shfl(mine.v1.py, src); b.v1.z = __shfl(mine.v1.z, src);
    b.v2.px = __shfl(mine.v2.px, src); b.v2.py = __shfl(mine.v2.py, src); b.v2.z = __shfl(mine.v2.z, src);
    b.index = (uint32_t)__shfl((int)mine.index, src);
    b.i0 = __shfl(mine.i0, src); b.i1 = __shfl(mine.i1, src); b.j0 = __shfl(mine.j0, src); b.j1 = __shfl(mine.j1, src);
    // lane l takes the centres l, l + 64, ... of the box in row-major order: (i, j) advances by 64 = q * w + r centres
    const int w = b.i1 - b.i0 + 1, q = 64 / w, r = 64 - q * w;
    int j = b.j0 + lane / w, i = b.i0 + (lane - (lane / w) * w);
    while (j <= b.j1) {
      mesh_draw_pixel(b, i, j, cam.width, keys);
      i += r; j += q;
      if (i > b.i1) { i -= w; ++j; }
    }
  }
}

// The queued triangles, in whatever order they arrived: kMeshQueueChunks workgroups share a box, workgroup c of them takes the
// centres 256 c + thread, + 256 kMeshQueueChunks, ... of the box in row-major order.  Every thread runs the prologue again -- the
// same expressions on the same inputs, so the triangle passes as it did and has the same box.
__global__ __launch_bounds__(256) void render_mesh_queue_kernel(MeshView view, bslam_mat3x4 T, bslam_camera4f cam, float min_depth, float max_depth,
                                                                int cull_backfaces, unsigned long long* keys, const uint32_t* words, const uint32_t* queue) {
  const uint32_t count = words[kMeshQueued], chunk = blockIdx.x % kMeshQueueChunks;
  for (uint32_t e = blockIdx.x / kMeshQueueChunks; e < count; e += gridDim.x / kMeshQueueChunks) {
    MeshTriangle tri;
    bool bad_index = false;
    if (!mesh_triangle_prologue(view, queue[e], T, cam, min_depth, max_depth, cull_backfaces, &tri, &bad_index)) continue;
    const uint32_t w = (uint32_t)(tri.i1 - tri.i0 + 1), area = w * (uint32_t)(tri.j1 - tri.j0 + 1);
    for (uint32_t p = chunk * 256u + threadIdx.x; p < area; p += 256u * kMeshQueueChunks) {
      const uint32_t row = p / w;
      mesh_draw_pixel(tri, tri.i0 + (int)(p - row * w), tri.j0 + (int)row, cam.width, keys);
    }
  }
}

// One thread per pixel; a null output is not written.  The winner's w, s, b and z are recomputed at this pixel by the
// expressions of mesh_pixel, so they carry the bits the draw pass saw (z is the key's upper half).  c_k, n_k: the attribute of
// vertex v_k, in ascending vertex id.
//   depth  u16:     v = metres_to_depth * z + 0.5f;  v < 65536 ? u16(v) : 0;                                      empty -> 0
//   index  u32:     the triangle id;                                                                              empty -> 0xFFFFFFFF
//   color  uchar4:  per channel u8(fminf(z * ((b0 * c0 + b1 * c1) + b2 * c2) + 0.5f, 255.0f)), alpha 255;        empty -> 0
//   normal 3 x f32, with vertex normals:  n = z * ((b0 * n0 + b1 * n1) + b2 * n2) per component, rotated:
//                   r.x = (m0 * n.x + m1 * n.y) + m2 * n.z, rows 1, 2 alike;  len = sqrtf((r.x * r.x + r.y * r.y) + r.z * r.z);
//                   r / len per component where len > 0, else 0
//                   without:  the face normal.  e = L_b - L_a, f = L_c - L_a in the triangle's own winding (camera frame);
//                   g = (e.y * f.z - e.z * f.y, e.z * f.x - e.x * f.z, e.x * f.y - e.y * f.x);  len as above;  g / len where
//                   len > 0, else 0;  negated where it points away from the camera: (g.x * L_a.x + g.y * L_a.y) + g.z * L_a.z > 0
//                                                                                                                 empty -> 0
__global__ __launch_bounds__(256) void render_mesh_resolve_kernel(const unsigned long long* keys, MeshView view, bslam_mat3x4 T, bslam_camera4f cam,
                                                                  float metres_to_depth, Img depth, Img index, Img color, Img normal) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= cam.width || y >= cam.height) return;
  const unsigned long long key = keys[(size_t)y * cam.width + x];
  const bool empty = key == kKeyEmpty;
  const uint32_t t = (uint32_t)key;
  if (depth.base) {
    uint16_t value = 0;
    if (!empty) {
      const float v = metres_to_depth * __uint_as_float((uint32_t)(key >> 32)) + 0.5f;
      if (v < 65536.0f) value = (uint16_t)v;
    }
    depth.at<uint16_t>(y, x) = value;
  }
  if (index.base) index.at<uint32_t>(y, x) = empty ? 0xFFFFFFFFu : t;
  if (!color.base && !normal.base) return;
  uint32_t rgba = 0u;
  f3 out = mk3(0.0f, 0.0f, 0.0f);
  if (!empty) {   // a winner passed the prologue: its indices are below view.vertices
    const uint32_t a = view.indices[3 * (size_t)t], b = view.indices[3 * (size_t)t + 1], c = view.indices[3 * (size_t)t + 2];
    uint32_t i0 = a, i1 = b, i2 = c;
    int nothing = 0;
    mesh_order(i0, i1, nothing, nothing); mesh_order(i1, i2, nothing, nothing); mesh_order(i0, i1, nothing, nothing);
    float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, z = 0.0f;
    mesh_pixel(mesh_vertex(view, i0, T, cam), mesh_vertex(view, i1, T, cam), mesh_vertex(view, i2, T, cam), x, y, &b0, &b1, &b2, &z);
    if (color.base) {
      const uint32_t c0 = view.colors[i0], c1 = view.colors[i1], c2 = view.colors[i2];
      rgba = 0xFF000000u;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float f0 = (float)((c0 >> (8 * ch)) & 0xffu), f1 = (float)((c1 >> (8 * ch)) & 0xffu), f2 = (float)((c2 >> (8 * ch)) & 0xffu);
        rgba |= (uint32_t)(uint8_t)fminf(z * ((b0 * f0 + b1 * f1) + b2 * f2) + 0.5f, 255.0f) << (8 * ch);
      }
    }
    if (normal.base) {
      if (view.normals) {
        const float* n0 = view.normals + 3 * (size_t)i0;
        const float* n1 = view.normals + 3 * (size_t)i1;
        const float* n2 = view.normals + 3 * (size_t)i2;
        const float nx = z * ((b0 * n0[0] + b1 * n1[0]) + b2 * n2[0]), ny = z * ((b0 * n0[1] + b1 * n1[1]) + b2 * n2[1]),
                    nz = z * ((b0 * n0[2] + b1 * n1[2]) + b2 * n2[2]);
        out.x = (T.m[0] * nx + T.m[1] * ny) + T.m[2] * nz;
        out.y = (T.m[4] * nx + T.m[5] * ny) + T.m[6] * nz;
        out.z = (T.m[8] * nx + T.m[9] * ny) + T.m[10] * nz;
      } else {
        const f3 La = mesh_camera_point(view.positions, a, T), Lb = mesh_camera_point(view.positions, b, T), Lc = mesh_camera_point(view.positions, c, T);
        const float ex = Lb.x - La.x, ey = Lb.y - La.y, ez = Lb.z - La.z, fx = Lc.x - La.x, fy = Lc.y - La.y, fz = Lc.z - La.z;
        out.x = ey * fz - ez * fy;
        out.y = ez * fx - ex * fz;
        out.z = ex * fy - ey * fx;
        if ((out.x * La.x + out.y * La.y) + out.z * La.z > 0.0f) { out.x = -out.x; out.y = -out.y; out.z = -out.z; }
      }
      const float len = sqrtf((out.x * out.x + out.y * out.y) + out.z * out.z);
      if (len > 0.0f) { out.x = out.x / len; out.y = out.y / len; out.z = out.z / len; }
      else out = mk3(0.0f, 0.0f, 0.0f);
    }
  }
  if (color.base) color.at<uint32_t>(y, x) = rgba;
  if (normal.base) {
    float* o = (float*)(normal.base + (size_t)y * normal.pitch) + 3 * (size_t)x;
    o[0] = out.x; o[1] = out.y; o[2] = out.z;
  }
}

}  // namespace bslam
