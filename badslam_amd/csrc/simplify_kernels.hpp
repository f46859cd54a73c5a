// simplify_kernels.hpp -- vertex clustering of an indexed triangle mesh on a uniform grid, for gfx950: a key pass with one vertex per
// lane, a stable radix sort of (key, vertex id) (rocPRIM, mesh_sort.hip), head flags of the sorted keys and their scan
// (lifecycle_kernels.hpp), a cluster pass that walks each segment from its head, and the triangle remap of mesh_kernels.hpp.
// The reference has no mesh; every mesher its users know ships this step.  With no triangles it is voxel-grid down-sampling.
//
// The rule (include/badslam_hip.h "Mesh simplification", DESIGN.md 8 "Mesh simplification"): the cell is fp32 in the form of
// pmd_cell, the sums of a cluster run over its members in ascending vertex id in double and in 64-bit integers, so a brute-force
// restatement reproduces every bit.  Atomics touch the error word alone.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "distance_kernels.hpp"
#include "mesh_kernels.hpp"

namespace bslam {

constexpr uint32_t kSimplifyBadVertex = 4u;   // a bit of the mesh error word: a vertex is not finite or lies outside the grid
constexpr int kSimplifyCellBits = 21;         // per axis: 0 <= c < 2^21
constexpr float kSimplifyCells = 2097152.f;
constexpr unsigned long long kSimplifyInvalidKey = ~0ull;   // no cell has it: a valid key uses 63 bits

// Words of the small device block of a call (u32 units).
constexpr int kSimplifyError = 0, kSimplifyClusters = 2, kSimplifyTriangles = 3, kSimplifyWords = 16;

// Key pass: key[v] = c_x | c_y << 21 | c_z << 42, so that ascending keys are ascending (c_z, c_y, c_x); id[v] = v.  An invalid
// vertex raises the error bit and gets the invalid key, which sorts behind every cell and which the cluster pass does not gather.
__global__ __launch_bounds__(256) void simplify_key_kernel(uint32_t vertices, const float* __restrict__ positions, f3 origin, float inv_cell,
                                                           unsigned long long* __restrict__ keys, uint32_t* __restrict__ ids, uint32_t* __restrict__ words) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= vertices) return;
  const float x = positions[3 * (size_t)v], y = positions[3 * (size_t)v + 1], z = positions[3 * (size_t)v + 2];
  const float cx = pmd_cell(x, origin.x, inv_cell), cy = pmd_cell(y, origin.y, inv_cell), cz = pmd_cell(z, origin.z, inv_cell);
  // a NaN cell fails every comparison
  const bool valid = pmd_finite(x) && pmd_finite(y) && pmd_finite(z) && cx >= 0.f && cx < kSimplifyCells && cy >= 0.f && cy < kSimplifyCells && cz >= 0.f &&
                     cz < kSimplifyCells;
  unsigned long long key = kSimplifyInvalidKey;
  if (valid) {
    key = (unsigned long long)(uint32_t)cx | ((unsigned long long)(uint32_t)cy << kSimplifyCellBits) | ((unsigned long long)(uint32_t)cz << (2 * kSimplifyCellBits));
  } else {
    atomicOr(&words[kSimplifyError], kSimplifyBadVertex);
  }
  keys[v] = key;
  ids[v] = v;
}

// head[i] = 1 iff sorted position i starts a segment of equal keys.
__global__ __launch_bounds__(256) void simplify_heads_kernel(uint32_t vertices, const unsigned long long* __restrict__ sorted_keys, uint8_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= vertices) return;
  head[i] = (i == 0 || sorted_keys[i] != sorted_keys[i - 1]) ? 1 : 0;
}

struct SimplifyClusters {
  uint32_t vertices;
  const unsigned long long* sorted_keys; const uint32_t* sorted_ids;   // by (key, id): the sort is stable
  const uint8_t* head; const uint32_t* rank;                           // rank: the inclusive scan of head, so the cluster of position i is rank[i] - 1
  const float* positions; const float* normals; const uint32_t* colors;   // normals, colors: may be null
  float* out_positions; float* out_normals; uint32_t* out_colors;
  uint32_t* vertex_cluster;
};

// Cluster pass, one lane per sorted position: every lane writes its member's cluster; the lane of a segment's head walks the
// segment in order -- ascending vertex id -- and writes the representative.  The sums start from -0.0, which leaves the first
// member's bits alone, so a cluster of one keeps them.  A segment of n members is n dependent gathers on one lane.
__global__ __launch_bounds__(256) void simplify_cluster_kernel(SimplifyClusters m) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m.vertices) return;
  const uint32_t cluster = m.rank[i] - 1u;
  m.vertex_cluster[m.sorted_ids[i]] = cluster;
  if (!m.head[i] || m.sorted_keys[i] == kSimplifyInvalidKey) return;
  double px = -0.0, py = -0.0, pz = -0.0, nx = -0.0, ny = -0.0, nz = -0.0;
  unsigned long long c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  bool normals_finite = true;
  uint32_t n = 0;
  for (uint32_t j = i; j < m.vertices && (j == i || !m.head[j]); ++j) {
    const size_t at = 3 * (size_t)m.sorted_ids[j];
    px += (double)m.positions[at]; py += (double)m.positions[at + 1]; pz += (double)m.positions[at + 2];
    if (m.normals != nullptr) {
      const float a = m.normals[at], b = m.normals[at + 1], c = m.normals[at + 2];
      normals_finite = normals_finite && pmd_finite(a) && pmd_finite(b) && pmd_finite(c);
      nx += (double)a; ny += (double)b; nz += (double)c;
    }
    if (m.colors != nullptr) {
      const uint32_t rgba = m.colors[at / 3];
      c0 += rgba & 0xffu; c1 += (rgba >> 8) & 0xffu; c2 += (rgba >> 16) & 0xffu; c3 += rgba >> 24;
    }
    ++n;
  }
  const size_t to = 3 * (size_t)cluster;
  const double count = (double)n;
  m.out_positions[to] = (float)(px / count); m.out_positions[to + 1] = (float)(py / count); m.out_positions[to + 2] = (float)(pz / count);
  if (m.normals != nullptr) {
    const double ss = (nx * nx + ny * ny) + nz * nz;
    float ox = 0.f, oy = 0.f, oz = 0.f;
    if (normals_finite && ss > 0.0) {
      const double len = sqrt(ss);
      ox = (float)(nx / len); oy = (float)(ny / len); oz = (float)(nz / len);
    }
    m.out_normals[to] = ox; m.out_normals[to + 1] = oy; m.out_normals[to + 2] = oz;
  }
  if (m.colors != nullptr) {
    const unsigned long long half = n / 2u;
    m.out_colors[cluster] = (uint32_t)((c0 + half) / n) | ((uint32_t)((c1 + half) / n) << 8) | ((uint32_t)((c2 + half) / n) << 16) | ((uint32_t)((c3 + half) / n) << 24);
  }
}

}  // namespace bslam
