// smooth_kernels.hpp -- Taubin lambda|mu smoothing of an indexed triangle mesh and vertex normals from its geometry, for gfx950.
// Once per call: the six directed pairs v << bits | u and the three (vertex, slot) keys of every live triangle, two stable radix
// sorts (rocPRIM, mesh_sort.hip), head flags of the sorted pairs and their scan (lifecycle_kernels.hpp), and a pass that
// turns the runs into a CSR neighbour list per vertex -- ascending in u by construction, with the run length 1 as the rim flag --
// and the fans.  Per step: one lane per vertex walks its list over the previous positions and writes the other buffer.  The
// reference has no mesh.
//
// The rule (include/badslam_hip.h "Mesh smoothing", DESIGN.md 8 "Mesh smoothing"): everything that decides a bit is float64 in
// separate operations in a stated order, every ordered sum is a walk in that order, and the only atomic is the integer OR of the
// error word.  So a restatement with sets and dictionaries reproduces every position bit.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "distance_kernels.hpp"
#include "mesh_kernels.hpp"

namespace bslam {

// Words of the small device block of a call (u32 units).
constexpr int kSmoothError = 0, kSmoothPairs = 1, kSmoothWords = 16;

// What the kernels of a call share.  P = 6 * triangles directed pairs, C = 3 * triangles corners.
struct SmoothState {
  uint32_t vertices, triangles, pairs, corners, bits;   // bits: of a vertex id
  const uint32_t* tri;                                  // [3 triangles] the caller's indices
  unsigned long long *pair_keys, *sorted_pairs;         // [P] v << bits | u, or the dead key of an ignored triangle
  uint32_t *ids, *pair_slots;                           // [P] 0 .. P - 1 and their order by (pair, slot)
  unsigned long long *fan_keys, *sorted_fans;           // [C] the corner's vertex, or 1 << bits for an ignored triangle; null when no normals are asked for
  uint32_t* fan;                                        // [C] the slots 3 t + k by (vertex, slot): ascending t within a vertex
  uint8_t* head;                                        // [P] by sorted position: the first use of a live pair
  uint32_t* rank;                                       // [P] inclusive scan of head: the pair of sorted position i is rank[i] - 1
  uint32_t* neighbour;                                  // [P] by pair: u
  uint8_t* single;                                      // [P] by pair: c(v, u) = 1
  uint32_t *list_start, *list_end;                      // [V] N(v) is neighbour[list_start[v] .. list_end[v]); 0, 0 without a live triangle
  uint32_t *fan_start, *fan_end;                        // [V] the fan of v is fan[fan_start[v] .. fan_end[v]); 0, 0 without one
  uint8_t* boundary;                                    // [V]
  uint32_t* words;
};

__device__ __forceinline__ unsigned long long smooth_dead_pair(uint32_t bits) { return ~0ull >> (64u - 2u * bits); }   // v == u == 2^bits - 1: no live pair

// The keys of the two sorts, one triangle per lane.  A triangle with an index >= V raises the error bit and, like one that repeats
// an index, gets the keys that sort last, so that nothing behind this launch dereferences it.
__global__ __launch_bounds__(256) void smooth_keys_kernel(SmoothState s) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= s.triangles) return;
  const uint32_t i[3] = {s.tri[3 * (size_t)t], s.tri[3 * (size_t)t + 1], s.tri[3 * (size_t)t + 2]};
  const bool bad = i[0] >= s.vertices || i[1] >= s.vertices || i[2] >= s.vertices;
  if (bad) atomicOr(&s.words[kSmoothError], kMeshBadIndex);
  const bool live = !bad && i[0] != i[1] && i[0] != i[2] && i[1] != i[2];
  for (int k = 0; k < 3; ++k) {
    const size_t pair = 6 * (size_t)t + 2 * k, corner = 3 * (size_t)t + k;
    const unsigned long long v = (unsigned long long)i[k] << s.bits;
    s.pair_keys[pair] = live ? (v | i[(k + 1) % 3]) : smooth_dead_pair(s.bits);
    s.pair_keys[pair + 1] = live ? (v | i[(k + 2) % 3]) : smooth_dead_pair(s.bits);
    s.ids[pair] = (uint32_t)pair;
    s.ids[pair + 1] = (uint32_t)pair + 1u;
    if (s.fan_keys != nullptr) s.fan_keys[corner] = live ? (unsigned long long)i[k] : (1ull << s.bits);
  }
}

// head[i] = sorted position i is the first use of a live pair.
__global__ __launch_bounds__(256) void smooth_heads_kernel(SmoothState s) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.pairs) return;
  const unsigned long long key = s.sorted_pairs[i];
  s.head[i] = (key != smooth_dead_pair(s.bits) && (i == 0 || s.sorted_pairs[i - 1] != key)) ? 1 : 0;
}

// By sorted position: the head of a run writes u and whether the run has length 1, which also marks v as boundary; the first run
// and the last of a vertex write the ends of its list.  list_start, list_end and boundary are zero before.
__global__ __launch_bounds__(256) void smooth_lists_kernel(SmoothState s) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.pairs) return;
  const unsigned long long dead = smooth_dead_pair(s.bits), key = s.sorted_pairs[i];
  if (key == dead) return;
  const uint32_t v = (uint32_t)(key >> s.bits), u = (uint32_t)(key & ((1ull << s.bits) - 1ull)), pair = s.rank[i] - 1u;
  const bool first = i == 0, end = i + 1 == s.pairs;
  const unsigned long long before = first ? 0ull : s.sorted_pairs[i - 1], after = end ? dead : s.sorted_pairs[i + 1];
  const bool head = first || before != key, last = end || after != key;
  if (head) {
    s.neighbour[pair] = u;
    s.single[pair] = last ? 1 : 0;
    if (last) s.boundary[v] = 1;   // every writer writes 1
    if (first || (uint32_t)(before >> s.bits) != v) s.list_start[v] = pair;
  }
  if (last && (after == dead || (uint32_t)(after >> s.bits) != v)) s.list_end[v] = pair + 1u;
}

// The ends of every vertex's fan in the sorted corners.  fan_start and fan_end are zero before.
__global__ __launch_bounds__(256) void smooth_fans_kernel(SmoothState s) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.corners) return;
  const unsigned long long v = s.sorted_fans[i];
  if (v >= s.vertices) return;   // an ignored triangle
  if (i == 0 || s.sorted_fans[i - 1] != v) s.fan_start[v] = i;
  if (i + 1 == s.corners || s.sorted_fans[i + 1] != v) s.fan_end[v] = i + 1;
}

// One Jacobi step with factor f, one vertex per lane: the mean of the stencil in ascending id from the first member, then
// p' = (float)(p + f * (m - p)) per axis.  An empty stencil keeps the position's bits.  mode: 0 fixed, 1 rim, 2 free.
__global__ __launch_bounds__(256) void smooth_step_kernel(SmoothState s, const float* __restrict__ in, float* __restrict__ out, double f, uint32_t mode) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= s.vertices) return;
  const uint32_t begin = s.list_start[v], end = s.list_end[v];
  const bool boundary = s.boundary[v] != 0, rim = mode == 1u && boundary;
  dec3 sum = {0.0, 0.0, 0.0};
  uint32_t members = 0;
  if (!(mode == 0u && boundary)) {
    for (uint32_t j = begin; j < end; ++j) {
      if (rim && !s.single[j]) continue;
      const dec3 q = dec_load(in, s.neighbour[j]);
      sum = members == 0 ? q : dec3{sum.x + q.x, sum.y + q.y, sum.z + q.z};
      ++members;
    }
  }
  const size_t at = 3 * (size_t)v;
  if (members == 0) {
    out[at] = in[at]; out[at + 1] = in[at + 1]; out[at + 2] = in[at + 2];
    return;
  }
  const dec3 p = dec_load(in, v);
  const double n = (double)members, mx = sum.x / n, my = sum.y / n, mz = sum.z / n;
  out[at] = (float)(p.x + f * (mx - p.x));
  out[at + 1] = (float)(p.y + f * (my - p.y));
  out[at + 2] = (float)(p.z + f * (mz - p.z));
}

// The normal of every vertex from `positions`: the sum of cross(b - a, c - a) over its fan in ascending t from +0.0, normalised;
// the input normal, or zero without one, where the vertex has no live triangle or the sum has no length.  with_fans == 0: no
// vertex has a fan (a mesh without triangles) and the fan arrays are not read.
__global__ __launch_bounds__(256) void smooth_normals_kernel(SmoothState s, const float* __restrict__ positions, const float* __restrict__ normals,
                                                             float* __restrict__ out_normals, int with_fans) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= s.vertices) return;
  const uint32_t begin = with_fans ? s.fan_start[v] : 0u, end = with_fans ? s.fan_end[v] : 0u;
  dec3 g = {0.0, 0.0, 0.0};
  for (uint32_t j = begin; j < end; ++j) {
    const uint32_t t = s.fan[j] / 3u;
    const dec3 a = dec_load(positions, s.tri[3 * (size_t)t]), b = dec_load(positions, s.tri[3 * (size_t)t + 1]), c = dec_load(positions, s.tri[3 * (size_t)t + 2]);
    const dec3 n = dec_normal(a, b, c);
    g = dec3{g.x + n.x, g.y + n.y, g.z + n.z};
  }
  const double ss = (g.x * g.x + g.y * g.y) + g.z * g.z;
  const size_t at = 3 * (size_t)v;
  float x = 0.f, y = 0.f, z = 0.f;
  if (end > begin && ss > 0.0) {
    const double len = sqrt(ss);
    x = (float)(g.x / len); y = (float)(g.y / len); z = (float)(g.z / len);
  } else if (normals != nullptr) {
    x = normals[at]; y = normals[at + 1]; z = normals[at + 2];
  }
  out_normals[at] = x; out_normals[at + 1] = y; out_normals[at + 2] = z;
}

}  // namespace bslam
