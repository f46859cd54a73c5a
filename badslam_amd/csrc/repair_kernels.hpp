// repair_kernels.hpp -- repair of an indexed triangle mesh, for gfx950: welding of bit-equal vertices, removal of degenerate and
// duplicate triangles and of unreferenced vertices; the census of the undirected edges and the boundary loops; and the closing of
// small loops with a centroid fan.  One lane handles one vertex, triangle, slot or loop.  The sorts are the stable radix sort of
// mesh_sort.hip, the scans those of lifecycle_kernels.hpp.  The reference has no mesh.
//
// The rule (include/badslam_hip.h "Mesh repair", DESIGN.md 8 "Mesh repair"): everything is integer but the centroid of a hole, which
// is a float64 sum in the order of the walk along its loop.  The only atomics are atomicOr of the error word and of flags, atomicAdd
// of counts and atomicMin of slots: none depends on the order of execution, so a brute-force restatement reproduces every bit.
// A slot is 3 t + k: corner k of triangle t, and the directed half-edge from corner k to corner (k + 1) % 3.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "distance_kernels.hpp"
#include "mesh_kernels.hpp"

namespace bslam {


// Words of the small device block of a call (u32 units).
constexpr int kRepairError = 0, kRepairUnique = 1, kRepairVertices = 2, kRepairTriangles = 3, kRepairDegenerates = 4, kRepairDuplicates = 5,
              kRepairReferenced = 8, kRepairEdges = 9, kRepairBoundary = 10, kRepairInterior = 11, kRepairNonManifold = 12, kRepairInconsistent = 13,
              kRepairBlocked = 14, kRepairBoundarySlots = 15, kRepairLoops = 16, kRepairLongest = 17, kRepairLoopEdges = 18, kRepairOpenSlots = 19,
              kRepairFilled = 20, kRepairFanTriangles = 21, kRepairWords = 32;

// The bits of a coordinate as the weld compares them: -0.0f is +0.0f.
__device__ __forceinline__ uint32_t repair_bits(float x) {
  const uint32_t b = __float_as_uint(x);
  return b == 0x80000000u ? 0u : b;
}

// ---------------------------------------------------------------------------------------------
// Clean.  rep[v] is the representative of v: the smallest vertex id with the same three coordinates, or v without welding.
// ---------------------------------------------------------------------------------------------

// One vertex per lane: the error bit of a position that is not finite; with `weld` the keys of the two sorts -- z, then y << 32 | x --
// and id[v] = v; without it rep[v] = v.
__global__ __launch_bounds__(256) void repair_vertex_kernel(uint32_t vertices, const float* __restrict__ positions, int weld, unsigned long long* __restrict__ key_z,
                                                            unsigned long long* __restrict__ key_yx, uint32_t* __restrict__ ids, uint32_t* __restrict__ rep,
                                                            uint32_t* __restrict__ words) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= vertices) return;
  const float x = positions[3 * (size_t)v], y = positions[3 * (size_t)v + 1], z = positions[3 * (size_t)v + 2];
  if (!(pmd_finite(x) && pmd_finite(y) && pmd_finite(z))) atomicOr(&words[kRepairError], kMeshBadPosition);
  if (weld) {
    key_z[v] = repair_bits(z);
    key_yx[v] = ((unsigned long long)repair_bits(y) << 32) | repair_bits(x);
    ids[v] = v;
  } else {
    rep[v] = v;
  }
}

// first[r] = the element at the head of run r (rank: the inclusive scan of head).  Both sorts are stable, so it is the run's smallest id.
__global__ __launch_bounds__(256) void repair_run_first_kernel(uint32_t count, const uint8_t* __restrict__ head, const uint32_t* __restrict__ rank,
                                                               const uint32_t* __restrict__ ids, uint32_t* __restrict__ first) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count && head[i]) first[rank[i] - 1u] = ids[i];
}

__global__ __launch_bounds__(256) void repair_representative_kernel(uint32_t count, const uint32_t* __restrict__ rank, const uint32_t* __restrict__ ids,
                                                                    const uint32_t* __restrict__ first, uint32_t* __restrict__ rep) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) rep[ids[i]] = first[rank[i] - 1u];
}

// One triangle per lane: its corners through rep; keep[t] = 1 iff they are pairwise distinct.  A triangle with an index >= V raises
// the error bit, is not kept and is not looked at again.  With `duplicates` the keys of the two sorts over the sorted triple
// (lo, mid, hi) -- hi, then lo << bits | mid -- and id[t] = t; a degenerate triple equals no other kind of triple.
__global__ __launch_bounds__(256) void repair_triangle_kernel(uint32_t vertices, uint32_t triangles, const uint32_t* __restrict__ indices, const uint32_t* __restrict__ rep,
                                                              int duplicates, unsigned bits, uint8_t* __restrict__ keep, unsigned long long* __restrict__ key_hi,
                                                              unsigned long long* __restrict__ key_lomid, uint32_t* __restrict__ ids, uint32_t* __restrict__ words) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= triangles) return;
  const uint32_t i0 = indices[3 * (size_t)t], i1 = indices[3 * (size_t)t + 1], i2 = indices[3 * (size_t)t + 2];
  const bool valid = i0 < vertices && i1 < vertices && i2 < vertices;
  uint32_t a = 0, b = 0, c = 0;
  if (valid) { a = rep[i0]; b = rep[i1]; c = rep[i2]; }
  else atomicOr(&words[kRepairError], kMeshBadIndex);
  const bool distinct = valid && a != b && a != c && b != c;
  keep[t] = distinct ? 1 : 0;
  mesh_wave_count(&words[kRepairDegenerates], valid && !distinct);
  if (!duplicates) return;
  const uint32_t lo = min(a, min(b, c)), hi = max(a, max(b, c)), mid = (a ^ b ^ c) ^ lo ^ hi;   // two equal corners cancel: mid is the third
  key_hi[t] = hi;
  key_lomid[t] = ((unsigned long long)lo << bits) | mid;
  ids[t] = t;
}

// By sorted position: a kept triangle that does not start its run repeats the run's head, the smallest triangle id of the triple.
__global__ __launch_bounds__(256) void repair_duplicate_kernel(uint32_t triangles, const uint8_t* __restrict__ head, const uint32_t* __restrict__ ids,
                                                               uint8_t* __restrict__ keep, uint32_t* __restrict__ words) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool duplicate = false;
  if (i < triangles && !head[i]) {
    const uint32_t t = ids[i];
    duplicate = keep[t] != 0;
    if (duplicate) keep[t] = 0;
  }
  mesh_wave_count(&words[kRepairDuplicates], duplicate);
}

// referenced[rep[corner]] = 1 for the corners of the kept triangles (zero before; every writer writes 1).
__global__ __launch_bounds__(256) void repair_reference_kernel(uint32_t triangles, const uint32_t* __restrict__ indices, const uint32_t* __restrict__ rep,
                                                               const uint8_t* __restrict__ keep, uint8_t* __restrict__ referenced) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= triangles || !keep[t]) return;
  for (int k = 0; k < 3; ++k) referenced[rep[indices[3 * (size_t)t + k]]] = 1;
}

// keep_vertex[v] = 1 iff v is a representative and, unless `all`, a kept triangle names it.
__global__ __launch_bounds__(256) void repair_keep_vertex_kernel(uint32_t vertices, const uint32_t* __restrict__ rep, const uint8_t* __restrict__ referenced, int all,
                                                                 uint8_t* __restrict__ keep_vertex) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < vertices) keep_vertex[v] = (rep[v] == v && (all || referenced[v])) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// Topology, over the edge runs of mesh_kernels.hpp.  A boundary slot is the one slot of a run of one; they are numbered in ascending
// slot (boundary_id, the exclusive scan of their flags), and the loop arrays are indexed by that number.
// ---------------------------------------------------------------------------------------------
struct RepairTopology {
  EdgeRuns runs;                              // vertices, triangles, slots, indices; referenced[V] is given
  uint32_t *starts, *ends, *start_slot;       // [V] boundary slots that start / end at v; the smallest that starts there
  uint8_t* boundary; uint32_t* boundary_id;   // [E] by slot
  uint32_t* loop_slot;                        // [B] the slot of a boundary slot's number
  uint32_t *next[2], *label[2]; uint8_t* open[2];   // [B] double buffered
  uint32_t* loop_length;                      // [B] by the number of the loop's smallest slot
  uint32_t* edge_uses; uint32_t* loop_of_slot;      // the caller's, may be null
  uint32_t* words;                            // runs.error = &words[kRepairError]
};

__device__ __forceinline__ uint32_t repair_slot_end(const uint32_t* __restrict__ indices, uint32_t slot) {
  const uint32_t t = slot / 3u, k = slot - 3u * t;
  return indices[3 * (size_t)t + (k + 1u) % 3u];
}

// By sorted position: the uses of the slot's edge; at the head of a run the class of the edge, the orientation test of an interior
// edge -- its two slots start at the same end iff they run the same way -- and for a boundary edge the flag of its slot, the counts
// at its two ends and the smallest slot that starts at its origin.
__global__ __launch_bounds__(256) void topology_census_kernel(RepairTopology s) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < s.runs.slots;
  uint32_t uses = 0, slot = 0;
  bool head = false;
  if (live) {
    const uint32_t r = s.runs.rank[i] - 1u;
    uses = s.runs.start_of[r + 1] - s.runs.start_of[r];
    slot = s.runs.sorted_slots[i];
    head = s.runs.head[i] != 0;
    if (s.edge_uses != nullptr) s.edge_uses[slot] = uses;
    s.boundary[slot] = uses == 1 ? 1 : 0;
  }
  mesh_wave_count(&s.words[kRepairBoundary], head && uses == 1);
  mesh_wave_count(&s.words[kRepairInterior], head && uses == 2);
  mesh_wave_count(&s.words[kRepairNonManifold], head && uses >= 3);
  bool same_way = false;
  if (head && uses == 2) same_way = s.runs.indices[slot] == s.runs.indices[s.runs.sorted_slots[i + 1]];
  mesh_wave_count(&s.words[kRepairInconsistent], same_way);
  if (head && uses == 1) {
    const uint32_t from = s.runs.indices[slot], to = repair_slot_end(s.runs.indices, slot);
    atomicAdd(&s.starts[from], 1u);
    atomicAdd(&s.ends[to], 1u);
    atomicMin(&s.start_slot[from], slot);
  }
}

// One vertex per lane: the referenced vertices, and the blocked ones -- touched by a boundary slot, but not by exactly one that starts
// and one that ends there.
__global__ __launch_bounds__(256) void topology_vertex_kernel(RepairTopology s) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = v < s.runs.vertices;
  mesh_wave_count(&s.words[kRepairReferenced], live && s.runs.referenced[v]);
  mesh_wave_count(&s.words[kRepairBlocked], live && s.starts[v] + s.ends[v] != 0 && !(s.starts[v] == 1 && s.ends[v] == 1));
}

// One slot per lane, boundary slots only: next = the number of the boundary slot that starts where this one ends if that vertex is
// passable; else the walk ends here: next = itself and the slot is open.  label = the slot.
__global__ __launch_bounds__(256) void topology_loop_init_kernel(RepairTopology s) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= s.runs.slots || !s.boundary[slot]) return;
  const uint32_t j = s.boundary_id[slot], to = repair_slot_end(s.runs.indices, slot);
  const bool passable = s.starts[to] == 1 && s.ends[to] == 1;
  s.loop_slot[j] = slot;
  s.next[0][j] = passable ? s.boundary_id[s.start_slot[to]] : j;
  s.label[0][j] = slot;
  s.open[0][j] = passable ? 0 : 1;
}

// One round of pointer jumping from buffer `from` into the other one: after k rounds next is 2^k steps ahead, label the smallest
// slot and open the disjunction over those steps.
__global__ __launch_bounds__(256) void topology_jump_kernel(RepairTopology s, uint32_t count, int from) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  const uint32_t n = s.next[from][j], l = s.label[from][j], ln = s.label[from][n];
  s.label[from ^ 1][j] = l < ln ? l : ln;
  s.open[from ^ 1][j] = s.open[from][j] | s.open[from][n];
  s.next[from ^ 1][j] = s.next[from][n];
}

// One boundary slot per lane, from buffer `at`: a slot that is not open lies on the loop of its label and adds one to that loop's length.
__global__ __launch_bounds__(256) void topology_loop_label_kernel(RepairTopology s, uint32_t count, int at) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = j < count, open = live && s.open[at][j] != 0;
  mesh_wave_count(&s.words[kRepairOpenSlots], open);
  if (!live || open) return;
  const uint32_t label = s.label[at][j];
  if (s.loop_of_slot != nullptr) s.loop_of_slot[s.loop_slot[j]] = label;
  atomicAdd(&s.loop_length[s.boundary_id[label]], 1u);
}

// One boundary slot per lane: the smallest slot of a loop reports it.  The longest loop is kept as the minimum of the complements.  A
// loop of at most max_hole_edges edges (0: none) is to be filled: fill_flag, and fan[j] = its length, else 0.
__global__ __launch_bounds__(256) void topology_loop_stats_kernel(RepairTopology s, uint32_t count, int at, uint32_t max_hole_edges, uint8_t* __restrict__ fill_flag,
                                                                  uint32_t* __restrict__ fan) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  const bool first = j < count && !s.open[at][j] && s.label[at][j] == s.loop_slot[j];
  const uint32_t length = first ? s.loop_length[j] : 0u;
  mesh_wave_count(&s.words[kRepairLoops], first);
  if (first) {
    atomicAdd(&s.words[kRepairLoopEdges], length);
    atomicMin(&s.words[kRepairLongest], ~length);
  }
  if (j < count && fill_flag != nullptr) {
    const bool fill = first && length <= max_hole_edges;
    fill_flag[j] = fill ? 1 : 0;
    fan[j] = fill ? length : 0u;
  }
}

// ---------------------------------------------------------------------------------------------
// Hole filling.  One lane per loop to be filled walks it from its smallest slot: the new vertex is the centroid of the origins of
// the slots in that order, slot (a -> b) gives the triangle (b, a, centroid).
// ---------------------------------------------------------------------------------------------
struct RepairFill {
  uint32_t vertices, triangles;                                           // of the input
  const float* positions; const float* normals; const uint32_t* colors;   // of the input; normals, colors: may be null
  const uint8_t* fill_flag; const uint32_t* fan; const uint32_t* ordinal; const uint32_t* fan_offset;   // [B]; the exclusive scans of fill_flag and fan
  float* out_positions; float* out_normals; uint32_t* out_colors; uint32_t* out_indices;
  uint32_t* hole_of_triangle;                                             // may be null
};

__global__ __launch_bounds__(256) void repair_fill_kernel(RepairTopology s, RepairFill f, uint32_t count) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count || !f.fill_flag[j]) return;
  const uint32_t n = f.fan[j], hole = f.ordinal[j], centre = f.vertices + hole;
  const size_t first = (size_t)f.triangles + f.fan_offset[j];
  double px = 0.0, py = 0.0, pz = 0.0, nx = 0.0, ny = 0.0, nz = 0.0;
  uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;   // n <= 4096: 4096 * 255 fits
  uint32_t slot = s.loop_slot[j];
  for (uint32_t k = 0; k < n && slot < s.runs.slots; ++k) {
    const uint32_t a = s.runs.indices[slot], b = repair_slot_end(s.runs.indices, slot);
    px = px + (double)f.positions[3 * (size_t)a]; py = py + (double)f.positions[3 * (size_t)a + 1]; pz = pz + (double)f.positions[3 * (size_t)a + 2];
    if (f.normals != nullptr) {
      nx = nx + (double)f.normals[3 * (size_t)a]; ny = ny + (double)f.normals[3 * (size_t)a + 1]; nz = nz + (double)f.normals[3 * (size_t)a + 2];
    }
    if (f.colors != nullptr) {
      const uint32_t rgba = f.colors[a];
      c0 += rgba & 0xffu; c1 += (rgba >> 8) & 0xffu; c2 += (rgba >> 16) & 0xffu; c3 += rgba >> 24;
    }
    const size_t to = 3 * (first + k);
    f.out_indices[to] = b; f.out_indices[to + 1] = a; f.out_indices[to + 2] = centre;
    if (f.hole_of_triangle != nullptr) f.hole_of_triangle[first - f.triangles + k] = hole;
    slot = s.start_slot[b];
  }
  const double count_d = (double)n;
  const size_t to = 3 * (size_t)centre;
  f.out_positions[to] = (float)(px / count_d); f.out_positions[to + 1] = (float)(py / count_d); f.out_positions[to + 2] = (float)(pz / count_d);
  if (f.normals != nullptr) {
    const double ss = (nx * nx + ny * ny) + nz * nz;
    float ox = 0.f, oy = 0.f, oz = 0.f;
    if (ss > 0.0 && ss < __builtin_inf()) {
      const double len = sqrt(ss);
      ox = (float)(nx / len); oy = (float)(ny / len); oz = (float)(nz / len);
    }
    f.out_normals[to] = ox; f.out_normals[to + 1] = oy; f.out_normals[to + 2] = oz;
  }
  if (f.colors != nullptr) {
    const uint32_t half = n / 2u;
    f.out_colors[centre] = ((c0 + half) / n) | (((c1 + half) / n) << 8) | (((c2 + half) / n) << 16) | (((c3 + half) / n) << 24);
  }
}

}  // namespace bslam
