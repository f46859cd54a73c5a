// decimate_kernels.hpp -- quadric-error edge collapse of an indexed triangle mesh in data-parallel rounds, for gfx950.  Per round: the
// three edge keys and the three (vertex, slot) keys of every live triangle, two stable radix sorts (rocPRIM, mesh_sort.hip),
// head flags of the sorted edges and their scan (lifecycle_kernels.hpp), an evaluation pass with one lane per unique edge that walks
// the triangle fans of its two ends, a minimum per vertex and per vertex neighbourhood that selects collapses with pairwise
// non-adjacent ends, the collapses, and the triangle remap of mesh_kernels.hpp through the parents.  The reference has no mesh.
//
// The rule (include/badslam_hip.h "Mesh decimation", DESIGN.md 8 "Mesh decimation"): every decision is float64 in separate
// operations in a stated order, every ordered sum is a walk in that order, and the only atomics are integer: the 64-bit minimum of
// the selection keys -- which does not depend on the order -- the two counters of a round and the error word.  So a brute-force
// restatement reproduces every bit.  A slot is 3 t + k: corner k of live triangle t, and the edge from corner k to corner k + 1.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "distance_kernels.hpp"
#include "mesh_kernels.hpp"

namespace bslam {

constexpr unsigned long long kDecimateNoKey = ~0ull;   // no candidate has it: the bits of a finite cost32 stay below 0x7f800000
constexpr uint32_t kDecimateGolden = 0x9E3779B1u;

// Words of the small device block of a call (u32 units).
constexpr int kDecimateError = 0, kDecimateSelected = 1, kDecimateRemoved = 2, kDecimateTriangles = 3, kDecimateVertices = 4, kDecimateEdges = 5,
              kDecimateCut = 6, kDecimateWords = 16;

__device__ __forceinline__ double dec_dot(dec3 a, dec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// The ten products (xx, xy, xz, xd, yy, yz, yd, zz, zd, dd) of the plane (n, d = -n . a).
__device__ __forceinline__ void dec_plane_quadric(dec3 n, dec3 a, double* k) {
  const double d = -dec_dot(n, a);
  k[0] = n.x * n.x; k[1] = n.x * n.y; k[2] = n.x * n.z; k[3] = n.x * d; k[4] = n.y * n.y; k[5] = n.y * n.z; k[6] = n.y * d; k[7] = n.z * n.z; k[8] = n.z * d; k[9] = d * d;
}

__device__ __forceinline__ double dec_cost(const double* q, dec3 p) {
  const double sq = ((q[0] * p.x) * p.x + (q[4] * p.y) * p.y) + (q[7] * p.z) * p.z;
  const double cr = ((q[1] * p.x) * p.y + (q[2] * p.x) * p.z) + (q[5] * p.y) * p.z;
  const double li = (q[3] * p.x + q[6] * p.y) + q[8] * p.z;
  return (sq + 2.0 * cr) + (2.0 * li + q[9]);
}

__device__ __forceinline__ bool dec_has(const uint32_t* __restrict__ tri, uint32_t t, uint32_t x) {
  return tri[3 * (size_t)t] == x || tri[3 * (size_t)t + 1] == x || tri[3 * (size_t)t + 2] == x;
}

// The midpoint of two fp32 coordinates: the double sum, halved, rounded once.
__device__ __forceinline__ float dec_mid(float a, float b) { return (float)(((double)a + (double)b) * 0.5); }

// What the kernels of a call share.  E = 3 * triangles slots; the sorted arrays have E entries.
struct DecimateState {
  uint32_t vertices, triangles, edges, bits;        // live triangles of the round; bits: of a vertex id
  const uint32_t* tri;                              // [3 triangles] the live triangles, current vertex ids
  float* positions; float* normals; uint32_t* colors;   // working copies [V]; normals, colors: may be null
  double* quadrics;                                 // [10 V]
  uint32_t* parent;                                 // [V] v while live, else the vertex it was merged into
  unsigned long long *edge_keys, *vertex_keys;      // [E] unsorted: lo << bits | hi;  the corner's vertex
  uint32_t* ids;                                    // [E] the slots 0 .. E - 1
  unsigned long long *sorted_edges, *sorted_vertices;
  uint32_t *edge_slots, *fan;                       // [E] the slots by (edge, slot) and by (vertex, slot): the sorts are stable
  uint8_t *head, *first, *single;                   // head: by sorted position; first, single: by slot (the edge's first use; its only use)
  uint32_t* rank;                                   // [E] inclusive scan of head: the edge of sorted position i is rank[i] - 1
  uint32_t *fan_start, *fan_end;                    // [V] the fan of v is fan[fan_start[v] .. fan_end[v]); 0, 0 without a triangle
  uint8_t* boundary;                                // [V]
  unsigned long long *m1, *m2;                      // [V]
  unsigned long long* key;                          // [E] by sorted position: the candidate's key or kDecimateNoKey
  uint8_t *choice, *selected;                       // [E] by sorted position
  uint32_t* words;
};

// Copies the attributes into the working arrays, parent[v] = v, and raises the error bit for a position that is not finite.
__global__ __launch_bounds__(256) void decimate_init_kernel(DecimateState s, const float* __restrict__ positions, const float* __restrict__ normals,
                                                            const uint32_t* __restrict__ colors) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= s.vertices) return;
  bool finite = true;
  for (int a = 0; a < 3; ++a) {
    const float x = positions[3 * (size_t)v + a];
    finite = finite && pmd_finite(x);
    s.positions[3 * (size_t)v + a] = x;
    if (normals != nullptr) s.normals[3 * (size_t)v + a] = normals[3 * (size_t)v + a];
  }
  if (colors != nullptr) s.colors[v] = colors[v];
  s.parent[v] = v;
  if (!finite) atomicOr(&s.words[kDecimateError], kMeshBadPosition);
}

// The keys of the two sorts of a round, one triangle per lane.
__global__ __launch_bounds__(256) void decimate_keys_kernel(DecimateState s) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= s.triangles) return;
  const uint32_t i[3] = {s.tri[3 * (size_t)t], s.tri[3 * (size_t)t + 1], s.tri[3 * (size_t)t + 2]};
  for (int k = 0; k < 3; ++k) {
    const size_t slot = 3 * (size_t)t + k;
    s.edge_keys[slot] = mesh_edge_key(i[k], i[(k + 1) % 3], s.bits);
    s.vertex_keys[slot] = i[k];
    s.ids[slot] = (uint32_t)slot;
  }
}

// By sorted position: the head flag of an edge, the first-use and only-use flags of its slots, the boundary flags of its ends, and
// the ends of every vertex's fan.  fan_start, fan_end and boundary are zero before.
__global__ __launch_bounds__(256) void decimate_heads_kernel(DecimateState s) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.edges) return;
  const unsigned long long e = s.sorted_edges[i];
  const bool head = i == 0 || s.sorted_edges[i - 1] != e, last = i + 1 == s.edges || s.sorted_edges[i + 1] != e;
  s.head[i] = head ? 1 : 0;
  const uint32_t slot = s.edge_slots[i];
  s.first[slot] = head ? 1 : 0;
  s.single[slot] = head && last ? 1 : 0;
  if (head && last) {
    s.boundary[mesh_edge_lo(e, s.bits)] = 1;   // every writer writes 1
    s.boundary[mesh_edge_hi(e, s.bits)] = 1;
  }
  const unsigned long long v = s.sorted_vertices[i];
  if (i == 0 || s.sorted_vertices[i - 1] != v) s.fan_start[v] = i;
  if (i + 1 == s.edges || s.sorted_vertices[i + 1] != v) s.fan_end[v] = i + 1;
}

// Q[v], once, one vertex per lane: the quadrics of its triangles in ascending triangle id -- its fan -- then the boundary quadrics of
// its boundary edges by (triangle, edge).
__global__ __launch_bounds__(256) void decimate_quadrics_kernel(DecimateState s, double boundary_weight) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= s.vertices) return;
  double q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, k[10];
  const uint32_t begin = s.fan_start[v], end = s.fan_end[v];
  for (uint32_t j = begin; j < end; ++j) {
    const uint32_t t = s.fan[j] / 3u;
    const dec3 a = dec_load(s.positions, s.tri[3 * (size_t)t]), b = dec_load(s.positions, s.tri[3 * (size_t)t + 1]), c = dec_load(s.positions, s.tri[3 * (size_t)t + 2]);
    dec_plane_quadric(dec_normal(a, b, c), a, k);
    for (int n = 0; n < 10; ++n) q[n] = q[n] + k[n];
  }
  for (uint32_t j = begin; j < end; ++j) {
    const uint32_t slot = s.fan[j], t = slot / 3u, corner = slot - 3u * t, before = (corner + 2u) % 3u;
    const uint32_t e1 = corner < before ? corner : before, e2 = corner < before ? before : corner;   // the two edges at v, in edge order
    for (int side = 0; side < 2; ++side) {
      const uint32_t e = side == 0 ? e1 : e2;
      if (!s.single[3 * (size_t)t + e]) continue;
      const dec3 a = dec_load(s.positions, s.tri[3 * (size_t)t]), b = dec_load(s.positions, s.tri[3 * (size_t)t + 1]), c = dec_load(s.positions, s.tri[3 * (size_t)t + 2]);
      const dec3 from = e == 0 ? a : (e == 1 ? b : c), to = e == 0 ? b : (e == 1 ? c : a);
      const dec3 ev = dec_sub(to, from);
      const double ee = (ev.x * ev.x + ev.y * ev.y) + ev.z * ev.z;
      if (!(ee > 0.0)) continue;
      dec_plane_quadric(dec_cross(ev, dec_normal(a, b, c)), from, k);
      for (int n = 0; n < 10; ++n) q[n] = q[n] + (k[n] * boundary_weight) / ee;
    }
  }
  for (int n = 0; n < 10; ++n) s.quadrics[10 * (size_t)v + n] = q[n];
}

// Evaluation, one lane per sorted position; the lane of an edge's head decides whether the edge is a candidate, and with which
// position and key.  m1 is kDecimateNoKey before.
__global__ __launch_bounds__(256) void decimate_eval_kernel(DecimateState s, float max_cost) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.edges) return;
  unsigned long long key = kDecimateNoKey;
  uint32_t choice = 0;
  if (s.head[i]) {
    const unsigned long long e = s.sorted_edges[i];
    const uint32_t lo = mesh_edge_lo(e, s.bits), hi = mesh_edge_hi(e, s.bits);
    const uint32_t c = 1u + ((i + 1 < s.edges && s.sorted_edges[i + 1] == e) ? 1u : 0u) + ((i + 2 < s.edges && s.sorted_edges[i + 2] == e) ? 1u : 0u);   // 3: more than two
    const uint32_t lo_begin = s.fan_start[lo], lo_end = s.fan_end[lo], hi_begin = s.fan_start[hi], hi_end = s.fan_end[hi];
    bool ok = c <= 2u;
    if (ok) {
      // the link condition and the valence of the common neighbours: every neighbour x of lo once, at the first use of the edge (lo, x)
      uint32_t common = 0;
      for (uint32_t j = lo_begin; j < lo_end; ++j) {
        const uint32_t slot = s.fan[j], t = slot / 3u, corner = slot - 3u * t, after = (corner + 1u) % 3u, before = (corner + 2u) % 3u;
        for (int side = 0; side < 2; ++side) {
          if (!s.first[3 * (size_t)t + (side == 0 ? corner : before)]) continue;
          const uint32_t x = s.tri[3 * (size_t)t + (side == 0 ? after : before)];
          if (x == hi) continue;
          bool shared = false;
          for (uint32_t m = hi_begin; m < hi_end && !shared; ++m) shared = dec_has(s.tri, s.fan[m] / 3u, x);
          if (!shared) continue;
          ++common;
          if (!s.boundary[x] && s.fan_end[x] - s.fan_start[x] == 3u) ok = false;
        }
      }
      const uint32_t both = (s.boundary[lo] && s.boundary[hi]) ? 1u : 0u;
      ok = ok && common + both == c + (c == 1u ? 1u : 0u);
    }
    if (ok) {
      double q[10];
      for (int n = 0; n < 10; ++n) q[n] = s.quadrics[10 * (size_t)lo + n] + s.quadrics[10 * (size_t)hi + n];
      const float* pl = s.positions + 3 * (size_t)lo;
      const float* ph = s.positions + 3 * (size_t)hi;
      const dec3 p0 = dec_load(s.positions, lo), p1 = dec_load(s.positions, hi);
      const dec3 p2 = dec3{(double)dec_mid(pl[0], ph[0]), (double)dec_mid(pl[1], ph[1]), (double)dec_mid(pl[2], ph[2])};
      const double c0 = dec_cost(q, p0), c1 = dec_cost(q, p1), c2 = dec_cost(q, p2);
      double cost = c0;
      dec3 p = p0;
      if (c1 < cost) { cost = c1; p = p1; choice = 1; }
      if (c2 < cost) { cost = c2; p = p2; choice = 2; }
      const float cost32 = (float)(cost > 0.0 ? cost : 0.0);
      ok = cost == cost && cost32 < __builtin_huge_valf() && cost32 <= max_cost;
      // the flip test over the triangles at one end only
      for (int end = 0; end < 2 && ok; ++end) {
        const uint32_t other = end == 0 ? hi : lo;
        for (uint32_t j = end == 0 ? lo_begin : hi_begin; j < (end == 0 ? lo_end : hi_end); ++j) {
          const uint32_t slot = s.fan[j], t = slot / 3u, corner = slot - 3u * t;
          if (dec_has(s.tri, t, other)) continue;
          const dec3 a = dec_load(s.positions, s.tri[3 * (size_t)t]), b = dec_load(s.positions, s.tri[3 * (size_t)t + 1]), d = dec_load(s.positions, s.tri[3 * (size_t)t + 2]);
          const dec3 moved = dec_normal(corner == 0 ? p : a, corner == 1 ? p : b, corner == 2 ? p : d);
          if (!(dec_dot(dec_normal(a, b, d), moved) > 0.0)) ok = false;
        }
      }
      if (ok) {
        key = ((unsigned long long)__float_as_uint(cost32) << 32) | (unsigned long long)((s.rank[i] - 1u) * kDecimateGolden);
        atomicMin(&s.m1[lo], key);
        atomicMin(&s.m1[hi], key);
      }
    }
  }
  s.key[i] = key;
  s.choice[i] = (uint8_t)choice;
}

// m2[v] = the minimum of m1 over v and its neighbours: a walk over the corners of v's fan.
__global__ __launch_bounds__(256) void decimate_neighbourhood_kernel(DecimateState s) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= s.vertices) return;
  unsigned long long m = s.m1[v];
  for (uint32_t j = s.fan_start[v]; j < s.fan_end[v]; ++j) {
    const uint32_t t = s.fan[j] / 3u;
    for (int k = 0; k < 3; ++k) {
      const unsigned long long other = s.m1[s.tri[3 * (size_t)t + k]];
      m = other < m ? other : m;
    }
  }
  s.m2[v] = m;
}

// selected[i] = the candidate's key is the minimum of both neighbourhoods; counts the selected edges and the triangles on them.
__global__ __launch_bounds__(256) void decimate_select_kernel(DecimateState s) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.edges) return;
  const unsigned long long key = s.key[i];
  bool selected = false;
  if (key != kDecimateNoKey) {
    const unsigned long long e = s.sorted_edges[i];
    const uint32_t lo = mesh_edge_lo(e, s.bits), hi = mesh_edge_hi(e, s.bits);
    selected = key == s.m2[lo] && key == s.m2[hi];
    if (selected) {
      atomicAdd(&s.words[kDecimateSelected], 1u);
      atomicAdd(&s.words[kDecimateRemoved], (i + 1 < s.edges && s.sorted_edges[i + 1] == e) ? 2u : 1u);
    }
  }
  s.selected[i] = selected ? 1 : 0;
}

// The cut to the room left: the keys of the selected edges to their ranks among them ...
__global__ __launch_bounds__(256) void decimate_cut_gather_kernel(DecimateState s, const uint32_t* __restrict__ selected_rank, unsigned long long* __restrict__ keys) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.edges || !s.selected[i]) return;
  keys[selected_rank[i]] = s.key[i];
}

// ... and, those keys sorted, an edge stays selected iff its key is among the first `room`.
__global__ __launch_bounds__(256) void decimate_cut_kernel(DecimateState s, const unsigned long long* __restrict__ sorted_keys, uint32_t room) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.edges || !s.selected[i]) return;
  if (s.key[i] > sorted_keys[room - 1u]) s.selected[i] = 0;
}

// The collapses, one selected edge per lane; their ends are pairwise non-adjacent, so no lane reads what another writes.
__global__ __launch_bounds__(256) void decimate_apply_kernel(DecimateState s) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.edges || !s.selected[i]) return;
  const unsigned long long e = s.sorted_edges[i];
  const uint32_t lo = mesh_edge_lo(e, s.bits), hi = mesh_edge_hi(e, s.bits), choice = s.choice[i];
  for (int n = 0; n < 10; ++n) s.quadrics[10 * (size_t)lo + n] = s.quadrics[10 * (size_t)lo + n] + s.quadrics[10 * (size_t)hi + n];
  float* pl = s.positions + 3 * (size_t)lo;
  const float* ph = s.positions + 3 * (size_t)hi;
  if (choice == 1u) {
    for (int a = 0; a < 3; ++a) pl[a] = ph[a];
    if (s.normals != nullptr)
      for (int a = 0; a < 3; ++a) s.normals[3 * (size_t)lo + a] = s.normals[3 * (size_t)hi + a];
    if (s.colors != nullptr) s.colors[lo] = s.colors[hi];
  } else if (choice == 2u) {
    for (int a = 0; a < 3; ++a) pl[a] = dec_mid(pl[a], ph[a]);
    if (s.normals != nullptr) {
      float* nl = s.normals + 3 * (size_t)lo;
      const float* nh = s.normals + 3 * (size_t)hi;
      const bool finite = pmd_finite(nl[0]) && pmd_finite(nl[1]) && pmd_finite(nl[2]) && pmd_finite(nh[0]) && pmd_finite(nh[1]) && pmd_finite(nh[2]);
      const double x = (double)nl[0] + (double)nh[0], y = (double)nl[1] + (double)nh[1], z = (double)nl[2] + (double)nh[2];
      const double ss = (x * x + y * y) + z * z;
      float ox = 0.f, oy = 0.f, oz = 0.f;
      if (finite && ss > 0.0) {
        const double len = sqrt(ss);
        ox = (float)(x / len); oy = (float)(y / len); oz = (float)(z / len);
      }
      nl[0] = ox; nl[1] = oy; nl[2] = oz;
    }
    if (s.colors != nullptr) {
      const uint32_t a = s.colors[lo], b = s.colors[hi];
      uint32_t out = 0;
      for (int k = 0; k < 32; k += 8) out |= ((((a >> k) & 0xffu) + ((b >> k) & 0xffu) + 1u) / 2u) << k;
      s.colors[lo] = out;
    }
  }
  s.parent[hi] = lo;
}

// Output: live[v] = v was never merged away ...
__global__ __launch_bounds__(256) void decimate_live_kernel(uint32_t vertices, const uint32_t* __restrict__ parent, uint8_t* __restrict__ live) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < vertices) live[v] = parent[v] == v ? 1 : 0;
}

// ... a survivor goes to its rank among the survivors, and every vertex follows its merges to the end (one step per round at most).
__global__ __launch_bounds__(256) void decimate_vertices_kernel(DecimateState s, const uint32_t* __restrict__ live_rank, float* __restrict__ out_positions,
                                                                float* __restrict__ out_normals, uint32_t* __restrict__ out_colors, uint32_t* __restrict__ vertex_map) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= s.vertices) return;
  uint32_t root = v;
  for (uint32_t step = 0; step < s.vertices && s.parent[root] != root; ++step) root = s.parent[root];
  if (vertex_map != nullptr) vertex_map[v] = live_rank[root];
  if (root != v) return;
  const size_t to = 3 * (size_t)live_rank[v], from = 3 * (size_t)v;
  for (int a = 0; a < 3; ++a) {
    out_positions[to + a] = s.positions[from + a];
    if (out_normals != nullptr) out_normals[to + a] = s.normals[from + a];
  }
  if (out_colors != nullptr) out_colors[to / 3] = s.colors[v];
}

// The live triangles in their order with the new vertex ids; their number is words[kDecimateTriangles] <= bound.
__global__ __launch_bounds__(256) void decimate_indices_kernel(uint32_t bound, const uint32_t* __restrict__ tri, const uint32_t* __restrict__ live_rank,
                                                               const uint32_t* __restrict__ words, uint32_t* __restrict__ out_indices) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= bound || t >= words[kDecimateTriangles]) return;
  for (int k = 0; k < 3; ++k) out_indices[3 * (size_t)t + k] = live_rank[tri[3 * (size_t)t + k]];
}

}  // namespace bslam
