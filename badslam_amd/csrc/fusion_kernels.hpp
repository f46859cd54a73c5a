// fusion_kernels.hpp -- volumetric fusion of the keyframes and surface extraction for gfx950.  The reference ends at a point
// cloud of surfel centres (BS/io.cc:694 SavePointCloudAsPLY) and sends its users to an external mesher; here every keyframe's
// calibrated depth is averaged into a truncated signed distance volume, from scratch, at the poses and with the depth
// calibration the bundle adjustment left behind, and naive surface nets turn the volume into a triangle mesh.  Like
// render_kernels.hpp: all arithmetic is fp32 (colours: integers), nothing is contracted, / and sqrtf are correctly rounded, and
// the expression order is written out so that a NumPy float32 restatement reproduces every output bit for bit.
#pragma once

#include "lifecycle_kernels.hpp"
#include "preprocess_kernels.hpp"

namespace bslam {

// bslam_volume on the device.  Sample (x, y, z) lies at  origin + (float(i) + 0.5f) * voxel  per axis (a multiply, then an add)
// and is element x of row z * ny + y of every volume buffer.
struct VolumeDev { float ox, oy, oz, voxel; int nx, ny, nz; };

__device__ __forceinline__ float voxel_centre(float origin, int i, float voxel) { return origin + ((float)i + 0.5f) * voxel; }

// A workgroup owns a brick of 8 x 8 x 4 voxels, one voxel per thread, x fastest: a wave is one 8 x 8 slab of constant z, whose
// 64 centres project onto a compact patch of every keyframe.
constexpr int kBrickX = 8, kBrickY = 8, kBrickZ = 4;

// ---------------------------------------------------------------------------------------------
// Integration.  Per voxel, keyframes in list order (activation is not looked at, as in assign_colors_kernel):
//   p      = the voxel's centre
//   project_to_pixel(p) false                        -> no observation        (the projection of a surfel, device_math.hpp)
//   d      = calibrated depth of the pixel's derived record (load_record);  d == 0 -> no observation
//   sdf    = d - local.z;   sdf < -truncation        -> no observation        (occluded)
//   S     += fminf(sdf, truncation);  n += 1
//   colour (only when a colour volume is given and sdf <= truncation):
//     cp   = project(colour fx, fy, cx, cy, local);  pixel (f2i(cp.x), f2i(cp.y));  outside the colour image -> no sample
//     r, g, b of that uchar4 pixel are added to three integer sums;  nc += 1
// After the last keyframe:  tsdf = n ? S / float(n) : truncation  (metres, not normalised);  count = n;
//   colour = nc ? {(sum_r + nc / 2) / nc, (sum_g + nc / 2) / nc, (sum_b + nc / 2) / nc, 255} : {0, 0, 0, 0}.
// One launch for the whole list; the sums live in registers and every output element is written once.
//
// Culling: before it walks 64 keyframes, a wave tests one keyframe per lane against the bounding box of the brick's voxel
// centres (box_outside_frustum, the test of the surfel kernels' work slots) and walks only those that some point of the box
// can project into.  The centres are monotone in the index, so the box of the first and last centre holds them all; the test
// is exactly conservative, so every output is the same bits with it on and off.  Threads of a brick that lie outside the
// volume stay in the loop (the ballot needs whole waves) and write nothing.
// stats: {(brick, keyframe) pairs, pairs walked} of bslam_debug_cull_stats, or nullptr.
// ---------------------------------------------------------------------------------------------
template <bool kColor>
__global__ __launch_bounds__(256) void fuse_keyframes_kernel(CamConsts c, const KfDev* __restrict__ kfs, int kf_count, VolumeDev vol, float truncation, int culling,
                                                             uint32_t bricks_x, uint32_t bricks_y, Img tsdf, Img count, Img color,
                                                             unsigned long long* __restrict__ stats) {
  const uint32_t brick = blockIdx.x;
  const uint32_t bz = brick / (bricks_x * bricks_y), rest = brick - bz * (bricks_x * bricks_y);
  const uint32_t by = rest / bricks_x, bx = rest - by * bricks_x;
  const int x0 = (int)bx * kBrickX, y0 = (int)by * kBrickY, z0 = (int)bz * kBrickZ;
  const int x = x0 + (int)(threadIdx.x & 7u), y = y0 + (int)((threadIdx.x >> 3) & 7u), z = z0 + (int)(threadIdx.x >> 6);
  const bool inside = x < vol.nx && y < vol.ny && z < vol.nz;
  const f3 gp = mk3(voxel_centre(vol.ox, x, vol.voxel), voxel_centre(vol.oy, y, vol.voxel), voxel_centre(vol.oz, z, vol.voxel));

  SlotBox box;
  {
    const f3 lo = mk3(voxel_centre(vol.ox, x0, vol.voxel), voxel_centre(vol.oy, y0, vol.voxel), voxel_centre(vol.oz, z0, vol.voxel));
    const f3 hi = mk3(voxel_centre(vol.ox, min(x0 + kBrickX, vol.nx) - 1, vol.voxel), voxel_centre(vol.oy, min(y0 + kBrickY, vol.ny) - 1, vol.voxel),
                      voxel_centre(vol.oz, min(z0 + kBrickZ, vol.nz) - 1, vol.voxel));
    box.c = mk3(0.5f * (lo.x + hi.x), 0.5f * (lo.y + hi.y), 0.5f * (lo.z + hi.z));
    box.e = mk3(0.5f * (hi.x - lo.x), 0.5f * (hi.y - lo.y), 0.5f * (hi.z - lo.z));
  }

  float S = 0.0f;
  uint32_t n = 0, nc = 0, sum_r = 0, sum_g = 0, sum_b = 0, walked = 0;
  const int lane = (int)(threadIdx.x & 63u);
  for (int k0 = 0; k0 < kf_count; k0 += 64) {
    bool visit = k0 + lane < kf_count;
    if (visit && culling) {
      float T[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) T[i] = kfs[k0 + lane].frame_T_global.m[i];
      visit = !box_outside_frustum(c, T, box);
    }
    unsigned long long todo = __ballot(visit);
    walked += (uint32_t)__popcll(todo);
    for (; todo != 0; todo &= todo - 1) {
      const KfDev& kf = kfs[k0 + __builtin_ctzll(todo)];   // wave-uniform: scalar loads
      Proj p;
      if (!project_to_pixel(c, kf, gp, &p)) continue;
      const float d = load_record(c, kf, p).depth;
      if (d == 0.0f) continue;
      const float sdf = d - p.local.z;
      if (sdf < -truncation) continue;
      S += fminf(sdf, truncation);
      n += 1;
      if (kColor && sdf <= truncation) {
        const f2 cp = project(c.cfx, c.cfy, c.ccx, c.ccy, p.local);
        const int ix = f2i(cp.x), iy = f2i(cp.y);
        if (cp.x < 0 || cp.y < 0 || ix >= c.color_width || iy >= c.color_height) continue;
        const uint32_t rgba = gload((const uint32_t*)(kf.color + (size_t)iy * kf.color_pitch) + ix);
        sum_r += rgba & 0xffu; sum_g += (rgba >> 8) & 0xffu; sum_b += (rgba >> 16) & 0xffu;
        nc += 1;
      }
    }
  }
  if (stats != nullptr && threadIdx.x == 0) { atomicAdd(&stats[0], (unsigned long long)kf_count); atomicAdd(&stats[1], (unsigned long long)walked); }
  if (!inside) return;
  const int row = z * vol.ny + y;
  tsdf.at<float>(row, x) = n ? S / (float)n : truncation;
  count.at<uint32_t>(row, x) = n;
  if (kColor) {
    uint32_t packed = 0;
    if (nc) packed = ((sum_r + nc / 2) / nc) | (((sum_g + nc / 2) / nc) << 8) | (((sum_b + nc / 2) / nc) << 16) | 0xff000000u;
    color.at<uint32_t>(row, x) = packed;
  }
}

// ---------------------------------------------------------------------------------------------
// Extraction: naive surface nets.  A sample is observed iff count >= min_count and inside iff tsdf < 0.  Cell (x, y, z),
// 0 <= x < nx - 1 and alike, has the samples (x + dx, y + dy, z + dz) as corners, is active iff all eight are observed and not
// all on one side, and has the linear index (z * (ny - 1) + y) * (nx - 1) + x.  Every active cell carries one vertex, whose id
// is the cell's rank among the active cells (exclusive scan of the flags), and owns the three grid edges that leave its minimum
// corner; a sign change along such an edge whose four surrounding cells are all active gives a quad of their vertices.
// Faces are ordered by (cell, axis) through a second scan, over the quads per cell.
// ---------------------------------------------------------------------------------------------
struct MeshVolume {
  VolumeDev vol;
  Img tsdf, count, color;   // color.base == nullptr: no colours
  uint32_t min_count;
  uint32_t cells;           // (nx - 1) (ny - 1) (nz - 1)
};

__device__ __forceinline__ void cell_xyz(const MeshVolume& m, uint32_t cell, int* x, int* y, int* z) {
  const uint32_t cx = (uint32_t)(m.vol.nx - 1), cy = (uint32_t)(m.vol.ny - 1);
  const uint32_t zy = cell / cx;
  *x = (int)(cell - zy * cx);
  *z = (int)(zy / cy);
  *y = (int)(zy - (uint32_t)*z * cy);
}
__device__ __forceinline__ uint32_t cell_index(const MeshVolume& m, int x, int y, int z) {
  return ((uint32_t)z * (uint32_t)(m.vol.ny - 1) + (uint32_t)y) * (uint32_t)(m.vol.nx - 1) + (uint32_t)x;
}
__device__ __forceinline__ float sample_tsdf(const MeshVolume& m, int x, int y, int z) { return m.tsdf.at<float>(z * m.vol.ny + y, x); }

__global__ __launch_bounds__(256) void mesh_flag_cells_kernel(MeshVolume m, uint8_t* __restrict__ active) {
  const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= m.cells) return;
  int x, y, z;
  cell_xyz(m, cell, &x, &y, &z);
  bool observed = true;
  int inside = 0;
#pragma unroll
  for (int corner = 0; corner < 8; ++corner) {
    const int sx = x + (corner & 1), sy = y + ((corner >> 1) & 1), sz = z + (corner >> 2);
    observed &= m.count.at<uint32_t>(sz * m.vol.ny + sy, sx) >= m.min_count;
    inside += sample_tsdf(m, sx, sy, sz) < 0.0f ? 1 : 0;
  }
  active[cell] = (observed && inside != 0 && inside != 8) ? 1 : 0;
}

// Bit A of the result: the edge from the minimum corner of active cell (x, y, z) along axis A (0: x, 1: y, 2: z) yields a quad.
// *a_inside: the side of the minimum corner.
__device__ __forceinline__ uint32_t cell_quad_mask(const MeshVolume& m, const uint8_t* __restrict__ active, int x, int y, int z, bool* a_inside) {
  const bool a = sample_tsdf(m, x, y, z) < 0.0f;
  *a_inside = a;
  uint32_t mask = 0;
  if (y >= 1 && z >= 1 && (sample_tsdf(m, x + 1, y, z) < 0.0f) != a &&
      active[cell_index(m, x, y - 1, z - 1)] && active[cell_index(m, x, y, z - 1)] && active[cell_index(m, x, y - 1, z)]) mask |= 1u;
  if (z >= 1 && x >= 1 && (sample_tsdf(m, x, y + 1, z) < 0.0f) != a &&
      active[cell_index(m, x - 1, y, z - 1)] && active[cell_index(m, x - 1, y, z)] && active[cell_index(m, x, y, z - 1)]) mask |= 2u;
  if (x >= 1 && y >= 1 && (sample_tsdf(m, x, y, z + 1) < 0.0f) != a &&
      active[cell_index(m, x - 1, y - 1, z)] && active[cell_index(m, x, y - 1, z)] && active[cell_index(m, x - 1, y, z)]) mask |= 4u;
  return mask;
}

__global__ __launch_bounds__(256) void mesh_count_quads_kernel(MeshVolume m, const uint8_t* __restrict__ active, uint8_t* __restrict__ quads) {
  const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= m.cells) return;
  uint32_t count = 0;
  if (active[cell]) {
    int x, y, z;
    cell_xyz(m, cell, &x, &y, &z);
    bool a;
    count = (uint32_t)__popc(cell_quad_mask(m, active, x, y, z, &a));
  }
  quads[cell] = (uint8_t)count;
}

// Vertex of an active cell, with D[dz][dy][dx] its corner samples.  The 12 edges are walked in the order: the four x-edges at
// (dy, dz) = (0,0), (1,0), (0,1), (1,1), then the four y-edges at (dx, dz) in the same pattern, then the four z-edges at (dx, dy).
//   edge a -> b = a + axis whose sides differ:  t = Da / (Da - Db);  s += (a.dx, a.dy, a.dz) with t in place of the axis
//                                               component;  edges += 1
//   mean     = s / float(edges)                                     per component
//   position = origin + ((float(x) + 0.5f) + mean.x) * voxel        per component
//   g.axis   = sum over the four edges of that axis, in the order above, of (Db - Da)
//   normal   = g / sqrtf((g.x * g.x + g.y * g.y) + g.z * g.z), or 0 where that root is 0: towards free space
//   colour   = {(sum + k / 2) / k per channel, 255} over the k corners whose colour sample has alpha 255; all 0 for k = 0
// Faces: for the +x edge the cells q0 .. q3 = (x, y-1, z-1), (x, y, z-1), (x, y, z), (x, y-1, z); +y and +z permute cyclically
// ((z, x) and (x, y) take the places of (y, z)).  Triangles (q0, q1, q2), (q0, q2, q3) when the minimum corner is inside, else
// the reversed quad (q3, q2, q1, q0) cut the same way: counter-clockwise seen from free space.
__global__ __launch_bounds__(256) void mesh_emit_kernel(MeshVolume m, const uint8_t* __restrict__ active, const uint32_t* __restrict__ vertex_id,
                                                        const uint32_t* __restrict__ quad_offset, float* __restrict__ positions, float* __restrict__ normals,
                                                        uint32_t* __restrict__ colors, uint32_t* __restrict__ indices) {
  const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= m.cells || !active[cell]) return;
  int x, y, z;
  cell_xyz(m, cell, &x, &y, &z);
  float D[2][2][2];
#pragma unroll
  for (int corner = 0; corner < 8; ++corner) D[corner >> 2][(corner >> 1) & 1][corner & 1] = sample_tsdf(m, x + (corner & 1), y + ((corner >> 1) & 1), z + (corner >> 2));
  float sx = 0.0f, sy = 0.0f, sz = 0.0f, gx = 0.0f, gy = 0.0f, gz = 0.0f;
  int edges = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {   // x-edges at (dy, dz)
    const int u = e & 1, v = e >> 1;
    const float Da = D[v][u][0], Db = D[v][u][1];
    if ((Da < 0.0f) != (Db < 0.0f)) { sx += Da / (Da - Db); sy += (float)u; sz += (float)v; edges += 1; }
    gx += Db - Da;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {   // y-edges at (dx, dz)
    const int u = e & 1, v = e >> 1;
    const float Da = D[v][0][u], Db = D[v][1][u];
    if ((Da < 0.0f) != (Db < 0.0f)) { sx += (float)u; sy += Da / (Da - Db); sz += (float)v; edges += 1; }
    gy += Db - Da;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {   // z-edges at (dx, dy)
    const int u = e & 1, v = e >> 1;
    const float Da = D[0][v][u], Db = D[1][v][u];
    if ((Da < 0.0f) != (Db < 0.0f)) { sx += (float)u; sy += (float)v; sz += Da / (Da - Db); edges += 1; }
    gz += Db - Da;
  }
  const uint32_t id = vertex_id[cell];
  const float count = (float)edges;
  positions[3 * (size_t)id + 0] = m.vol.ox + (((float)x + 0.5f) + sx / count) * m.vol.voxel;
  positions[3 * (size_t)id + 1] = m.vol.oy + (((float)y + 0.5f) + sy / count) * m.vol.voxel;
  positions[3 * (size_t)id + 2] = m.vol.oz + (((float)z + 0.5f) + sz / count) * m.vol.voxel;
  if (normals != nullptr) {
    const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
    const bool zero = len == 0.0f;
    normals[3 * (size_t)id + 0] = zero ? 0.0f : gx / len;
    normals[3 * (size_t)id + 1] = zero ? 0.0f : gy / len;
    normals[3 * (size_t)id + 2] = zero ? 0.0f : gz / len;
  }
  if (colors != nullptr) {
    uint32_t k = 0, r = 0, g = 0, b = 0;
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
      const uint32_t rgba = m.color.at<uint32_t>((z + (corner >> 2)) * m.vol.ny + y + ((corner >> 1) & 1), x + (corner & 1));
      if ((rgba >> 24) == 255u) { r += rgba & 0xffu; g += (rgba >> 8) & 0xffu; b += (rgba >> 16) & 0xffu; k += 1; }
    }
    colors[id] = k ? (((r + k / 2) / k) | (((g + k / 2) / k) << 8) | (((b + k / 2) / k) << 16) | 0xff000000u) : 0u;
  }
  bool a_inside;
  const uint32_t mask = cell_quad_mask(m, active, x, y, z, &a_inside);
  uint32_t* out = indices + 6 * (size_t)quad_offset[cell];
#pragma unroll
  for (int axis = 0; axis < 3; ++axis) {
    if (!(mask & (1u << axis))) continue;
    // the two other axes in cyclic order: (y, z), (z, x), (x, y)
    const int ux = axis == 2, uy = axis == 0, uz = axis == 1;
    const int vx = axis == 1, vy = axis == 2, vz = axis == 0;
    uint32_t q[4];
    q[0] = vertex_id[cell_index(m, x - ux - vx, y - uy - vy, z - uz - vz)];
    q[1] = vertex_id[cell_index(m, x - vx, y - vy, z - vz)];
    q[2] = id;
    q[3] = vertex_id[cell_index(m, x - ux, y - uy, z - uz)];
    if (!a_inside) { const uint32_t t0 = q[0], t1 = q[1]; q[0] = q[3]; q[1] = q[2]; q[2] = t1; q[3] = t0; }
    out[0] = q[0]; out[1] = q[1]; out[2] = q[2];
    out[3] = q[0]; out[4] = q[2]; out[5] = q[3];
    out += 6;
  }
}

}  // namespace bslam
