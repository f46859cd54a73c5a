// mesh_kernels.hpp -- an indexed triangle mesh as a graph, for gfx950: connected components by a data-parallel union-find and
// the compaction that drops the components below a vertex count.  The reference has no mesh at all (fusion_kernels.hpp); every
// mesher its users know ships this step.  Everything is integer, so the outputs do not depend on the order of execution and a
// sequential restatement reproduces every bit.
//
// The rule (include/badslam_hip.h, DESIGN.md 8 "Mesh components"): vertices a and b are joined iff a triangle contains both; a
// component is a class of the transitive closure; label[v] = the smallest vertex id of v's component, size[v] = its vertex count.
//
// Behind them, what the mesh operators built on this file share (simplify_, decimate_, smooth_kernels.hpp): the triangle remap --
// keep flag and scatter of the triangles through a vertex map -- and the float64 vector helpers of their ordered sums.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace bslam {

// Bits of the device error word of every mesh call: words[0] of its small device block.
constexpr uint32_t kMeshBadIndex = 1u;      // a triangle names a vertex >= V: never dereferenced
constexpr uint32_t kMeshOverrun = 2u;       // a find or a retry loop ran into its cap: cannot happen while parent[v] <= v holds
constexpr uint32_t kMeshBadPosition = 8u;   // a position is not finite (4 is simplification's own, kSimplifyBadVertex)

// ---------------------------------------------------------------------------------------------
// Union-find over parent[V] with the invariant parent[v] <= v at all times: a find walks strictly downwards, so it ends after at
// most V steps whatever other threads do, and the root of a finished component is its smallest id whatever the schedule.
//
// The eight XCDs have separate L2s and a CU's L1 is never refreshed by another CU's stores, so inside the union kernel every
// access to parent[] is a relaxed atomic at agent scope (loads and stores that bypass the L1 and write through the L2; the hook
// is a compare-and-swap, which the memory side serialises).  Nothing is ordered and nothing needs to be: a stale parent[v] is a
// value parent[v] held earlier, parents only ever move to ancestors, so an old pointer still leads into the same tree and
// towards its root.  Only the hook has to be exact, and it is: it succeeds only if the entry still holds the root itself.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t parent_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void parent_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of v with path halving: every second node on the way is pointed at its grandparent, an ancestor below it.  A node that
// is rewritten was seen with a parent other than itself, so it is no root and never becomes one again: the store cannot undo a
// hook.  At most `cap` steps; *overrun is set beyond.
__device__ __forceinline__ uint32_t mesh_find(uint32_t* parent, uint32_t v, uint32_t cap, bool* overrun) {
  uint32_t p = parent_load(parent + v);
  for (uint32_t steps = 0; p != v; ++steps) {
    if (steps >= cap) { *overrun = true; return v; }
    const uint32_t g = parent_load(parent + p);
    if (g != p) parent_store(parent + v, g);
    v = p;
    p = g;
  }
  return v;
}

// Joins the trees of a and b for every lane of a wave whose `active` is set; all 64 lanes call it together.  Per round a lane
// finds its two roots and, if they differ, wants to hook the larger one, hi, under the smaller one by a compare-and-swap on hi's
// entry that expects hi itself.  Neighbouring triangles mostly want the same hook, and same-address atomics are serialised by
// the memory side, so of the lanes that hold the same hi only the lowest one swaps in a round; the others find again in the
// next round and as a rule see the hook done.  A failed swap means the entry no longer holds the root -- another thread hooked
// it, or the find ended on a stale value -- and returns what it holds now: that lane goes on from this parent, strictly below
// the failed root.  Termination needs no other wave: whenever a lane swaps, succeeds or fails, the larger of its two nodes
// decreases or it is done; a lane that does not swap waits for at most the 63 lanes below it that hold the same hi, each of
// which leaves that value for good in the round it swaps.  So 64 (V + 64) rounds are more than the loop can take.
// tries / fails: swaps attempted and failed (profiling).
__device__ __forceinline__ void mesh_unite_wave(uint32_t* parent, bool active, uint32_t a, uint32_t b, uint32_t vertices, bool* overrun, uint32_t* tries,
                                                uint32_t* fails) {
  const uint32_t cap = vertices + 64u;
  const int lane = (int)(threadIdx.x & 63u);
  for (unsigned long long round = 0; __ballot(active) != 0; ++round) {   // wave-uniform
    uint32_t hi = 0, lo = 0;
    if (active) {
      a = mesh_find(parent, a, cap, overrun);
      b = mesh_find(parent, b, cap, overrun);
      if (a == b || *overrun) active = false;
      hi = a > b ? a : b;
      lo = a > b ? b : a;
    }
    bool swaps = false;
    for (unsigned long long pending = __ballot(active); pending != 0;) {   // wave-uniform: one pass per distinct hi
      const int first = __builtin_ctzll(pending);
      const uint32_t h = __shfl(hi, first, 64);
      if (lane == first) swaps = true;
      pending &= ~__ballot(active && hi == h);
    }
    if (swaps) {
      uint32_t expected = hi;
      *tries += 1;
      if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        active = false;
      } else {
        *fails += 1;
        a = expected;   // the parent the entry holds now, < hi
        b = lo;
      }
    }
    if (active && round >= 64ull * cap) { *overrun = true; active = false; }
  }
}

// parent[v] = v, size_of_root[v] = 0; thread 0 clears words[0 .. 1] = {error bits, component count}.
__global__ __launch_bounds__(256) void mesh_init_kernel(uint32_t vertices, uint32_t* __restrict__ parent, uint32_t* __restrict__ size_of_root,
                                                        uint32_t* __restrict__ words) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v == 0) { words[0] = 0; words[1] = 0; }
  if (v >= vertices) return;
  parent[v] = v;
  size_of_root[v] = 0;
}

// A head start for the union launch, one thread per triangle and no retries: behind mesh_init_kernel every vertex is a root, and
// parent[hi] = min(parent[hi], lo) for the three vertex pairs of a triangle leaves parent[v] = the smallest of v and its
// neighbours.  Every link is an edge of the mesh, so the forest joins nothing the rule does not join, and parent[v] <= v holds.
// What it buys: the atomics are spread over all entries (a handful per address), while hooks contend for the few roots every
// tree is being merged into -- same-address atomics that the memory side serialises.  Behind this launch the only roots left are
// the vertices smaller than all their neighbours, and the union launch finds most pairs joined already.  A triangle with an
// index >= V raises the error bit here and is skipped.
__global__ __launch_bounds__(256) void mesh_seed_kernel(uint32_t vertices, uint32_t triangles, const uint32_t* __restrict__ indices, uint32_t* __restrict__ parent,
                                                        uint32_t* __restrict__ words) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= triangles) return;
  const uint32_t i0 = indices[3 * (size_t)t], i1 = indices[3 * (size_t)t + 1], i2 = indices[3 * (size_t)t + 2];
  if (i0 >= vertices || i1 >= vertices || i2 >= vertices) { atomicOr(&words[0], kMeshBadIndex); return; }
  if (i0 != i1) atomicMin(&parent[i0 > i1 ? i0 : i1], i0 > i1 ? i1 : i0);
  if (i0 != i2) atomicMin(&parent[i0 > i2 ? i0 : i2], i0 > i2 ? i2 : i0);
  if (i1 != i2) atomicMin(&parent[i1 > i2 ? i1 : i2], i1 > i2 ? i2 : i1);
}

// Root of v by plain loads, for the launches in which no hook runs: the entries other threads rewrite meanwhile (compress) only
// move to ancestors, and an aligned word is read whole.  At most V + 64 steps; *overrun is set beyond.
__device__ __forceinline__ uint32_t mesh_root(const uint32_t* parent, uint32_t v, uint32_t vertices, bool* overrun) {
  uint32_t p = parent[v];
  for (uint32_t steps = 0; p != v; ++steps) {
    if (steps >= vertices + 64u) { *overrun = true; break; }
    v = p;
    p = parent[v];
  }
  return v;
}

// Behind the seeding, the trees are chains as deep as the mesh is long in vertex order (about one link per slab of the volume).
// One thread per vertex points its entry at its root, so that the finds of the union launch start two loads from a root
// instead of walking and halving those chains with write-through stores, all of them at once.
__global__ __launch_bounds__(256) void mesh_compress_kernel(uint32_t vertices, uint32_t* parent, uint32_t* __restrict__ words) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= vertices) return;
  bool overrun = false;
  const uint32_t first = parent[v];
  const uint32_t root = mesh_root(parent, first, vertices, &overrun);
  if (overrun) { atomicOr(&words[0], kMeshOverrun); return; }
  if (root != first) parent[v] = root;
}

// One thread per triangle: joins (i0, i1) and (i0, i2).  One launch whatever the graph's diameter.
// stats: {swaps attempted, swaps that succeeded} while profiling is on (bslam_debug_cull_stats), else nullptr.
__global__ __launch_bounds__(256) void mesh_union_kernel(uint32_t vertices, uint32_t triangles, const uint32_t* __restrict__ indices, uint32_t* parent,
                                                         uint32_t* __restrict__ words, unsigned long long* __restrict__ stats) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t i0 = 0, i1 = 0, i2 = 0;
  bool valid = t < triangles;   // lanes beyond the last triangle stay: the wave votes as a whole
  if (valid) {
    i0 = indices[3 * (size_t)t]; i1 = indices[3 * (size_t)t + 1]; i2 = indices[3 * (size_t)t + 2];
    if (i0 >= vertices || i1 >= vertices || i2 >= vertices) { atomicOr(&words[0], kMeshBadIndex); valid = false; }
  }
  bool overrun = false;
  uint32_t tries = 0, fails = 0;
  mesh_unite_wave(parent, valid && i1 != i0, i0, i1, vertices, &overrun, &tries, &fails);
  mesh_unite_wave(parent, valid && i2 != i0 && i2 != i1, i0, i2, vertices, &overrun, &tries, &fails);
  if (overrun) atomicOr(&words[0], kMeshOverrun);
  if (stats != nullptr && tries) { atomicAdd(&stats[0], (unsigned long long)tries); atomicAdd(&stats[1], (unsigned long long)(tries - fails)); }
}

// Flatten and count, a launch of its own behind the union (plain loads: the kernel boundary made every hook visible):
// label[v] = the root of v;  size_of_root[label[v]] += 1;  words[1] += 1 for every root.  The lanes of a wave that share a label
// add once: on a mesh that is mostly one surface that is one atomic per wave in place of 64 on one address.  After four
// distinct labels the lanes that are left add for themselves (a wave of singletons would otherwise take 64 rounds).
__global__ __launch_bounds__(256) void mesh_flatten_kernel(uint32_t vertices, const uint32_t* __restrict__ parent, uint32_t* __restrict__ labels,
                                                           uint32_t* __restrict__ size_of_root, uint32_t* __restrict__ words) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = v < vertices;
  uint32_t root = 0;
  bool overrun = false;
  if (live) {
    root = mesh_root(parent, v, vertices, &overrun);
    labels[v] = root;
  }
  if (overrun) atomicOr(&words[0], kMeshOverrun);
  const int lane = (int)(threadIdx.x & 63u);
  unsigned long long todo = __ballot(live && !overrun);
  const unsigned long long roots = __ballot(live && !overrun && root == v);
  if (lane == 0 && roots) atomicAdd(&words[1], (uint32_t)__popcll(roots));
  for (int round = 0; round < 4 && todo != 0; ++round) {
    const int leader = __builtin_ctzll(todo);
    const uint32_t l = __shfl(root, leader, 64);
    const unsigned long long same = __ballot(((todo >> lane) & 1ull) && root == l);
    if (lane == leader) atomicAdd(&size_of_root[l], (uint32_t)__popcll(same));
    todo &= ~same;
  }
  if ((todo >> lane) & 1ull) atomicAdd(&size_of_root[root], 1u);
}

// size[v] = size_of_root[label[v]], behind the launch that finished the sums.
__global__ __launch_bounds__(256) void mesh_sizes_kernel(uint32_t vertices, const uint32_t* __restrict__ labels, const uint32_t* __restrict__ size_of_root,
                                                         uint32_t* __restrict__ sizes) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < vertices) sizes[v] = size_of_root[labels[v]];
}

// ---------------------------------------------------------------------------------------------
// Filter.  Vertex v is kept iff size[v] >= min_vertices, a triangle iff its first vertex is; exclusive scans of the two flag
// arrays (device_scan) give the new ids; one launch scatters both.  The launches cover the vertices first and the triangles
// behind them: blocks [0, vertex_blocks) take a vertex per thread, the others a triangle.
// ---------------------------------------------------------------------------------------------
struct MeshFilter {
  uint32_t vertices, triangles, vertex_blocks, min_vertices;
  const float* positions; const float* normals; const uint32_t* colors;   // normals, colors: may be null
  const uint32_t* indices; const uint32_t* sizes;
  float* out_positions; float* out_normals; uint32_t* out_colors; uint32_t* out_indices;
};

// keep_vertex[v], keep_triangle[t] as u8.  A triangle with an index >= V raises the error bit and is not kept, so that nothing
// behind this launch dereferences it.
__global__ __launch_bounds__(256) void mesh_keep_flags_kernel(MeshFilter m, uint8_t* __restrict__ keep_vertex, uint8_t* __restrict__ keep_triangle,
                                                              uint32_t* __restrict__ words) {
  if (blockIdx.x < m.vertex_blocks) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < m.vertices) keep_vertex[v] = m.sizes[v] >= m.min_vertices ? 1 : 0;
    return;
  }
  const uint32_t t = (blockIdx.x - m.vertex_blocks) * blockDim.x + threadIdx.x;
  if (t >= m.triangles) return;
  const uint32_t i0 = m.indices[3 * (size_t)t], i1 = m.indices[3 * (size_t)t + 1], i2 = m.indices[3 * (size_t)t + 2];
  if (i0 >= m.vertices || i1 >= m.vertices || i2 >= m.vertices) {
    atomicOr(&words[0], kMeshBadIndex);
    keep_triangle[t] = 0;
    return;
  }
  keep_triangle[t] = m.sizes[i0] >= m.min_vertices ? 1 : 0;
}

// Kept vertices and triangles go to their rank among the kept ones, attributes with their bits unchanged, indices through the
// vertices' ranks.  Nothing at or beyond the kept counts is written.
__global__ __launch_bounds__(256) void mesh_scatter_kernel(MeshFilter m, const uint8_t* __restrict__ keep_vertex, const uint8_t* __restrict__ keep_triangle,
                                                           const uint32_t* __restrict__ vertex_rank, const uint32_t* __restrict__ triangle_rank) {
  if (blockIdx.x < m.vertex_blocks) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= m.vertices || !keep_vertex[v]) return;
    const size_t from = 3 * (size_t)v, to = 3 * (size_t)vertex_rank[v];
    // as words: a copy must not canonicalise a NaN's payload
    const uint32_t* pos = (const uint32_t*)m.positions;
    uint32_t* out_pos = (uint32_t*)m.out_positions;
    out_pos[to] = pos[from]; out_pos[to + 1] = pos[from + 1]; out_pos[to + 2] = pos[from + 2];
    if (m.normals != nullptr) {
      const uint32_t* nrm = (const uint32_t*)m.normals;
      uint32_t* out_nrm = (uint32_t*)m.out_normals;
      out_nrm[to] = nrm[from]; out_nrm[to + 1] = nrm[from + 1]; out_nrm[to + 2] = nrm[from + 2];
    }
    if (m.colors != nullptr) m.out_colors[vertex_rank[v]] = m.colors[v];
    return;
  }
  const uint32_t t = (blockIdx.x - m.vertex_blocks) * blockDim.x + threadIdx.x;
  if (t >= m.triangles || !keep_triangle[t]) return;
  const size_t from = 3 * (size_t)t, to = 3 * (size_t)triangle_rank[t];
  m.out_indices[to] = vertex_rank[m.indices[from]];
  m.out_indices[to + 1] = vertex_rank[m.indices[from + 1]];
  m.out_indices[to + 2] = vertex_rank[m.indices[from + 2]];
}

// ---------------------------------------------------------------------------------------------
// Triangle remap.  map[v] is what vertex v became (its cluster; the vertex it was merged into, or itself).  A triangle is kept iff
// its three mapped corners are pairwise distinct; an exclusive scan of the flags (device_scan) gives the new ids; a kept triangle
// goes to its rank with its corners mapped, in their order.
// ---------------------------------------------------------------------------------------------

// keep[t] as u8.  A triangle with an index >= V raises the error bit and is not kept, so that nothing behind this launch
// dereferences it.
__global__ __launch_bounds__(256) void mesh_remap_keep_kernel(uint32_t vertices, uint32_t triangles, const uint32_t* __restrict__ indices, const uint32_t* __restrict__ map,
                                                              uint8_t* __restrict__ keep, uint32_t* __restrict__ words) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= triangles) return;
  const uint32_t i0 = indices[3 * (size_t)t], i1 = indices[3 * (size_t)t + 1], i2 = indices[3 * (size_t)t + 2];
  if (i0 >= vertices || i1 >= vertices || i2 >= vertices) {
    atomicOr(&words[0], kMeshBadIndex);
    keep[t] = 0;
    return;
  }
  const uint32_t a = map[i0], b = map[i1], c = map[i2];
  keep[t] = (a != b && a != c && b != c) ? 1 : 0;
}

__global__ __launch_bounds__(256) void mesh_remap_scatter_kernel(uint32_t triangles, const uint32_t* __restrict__ indices, const uint32_t* __restrict__ map,
                                                                 const uint8_t* __restrict__ keep, const uint32_t* __restrict__ rank, uint32_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= triangles || !keep[t]) return;
  const size_t from = 3 * (size_t)t, to = 3 * (size_t)rank[t];
  out[to] = map[indices[from]];
  out[to + 1] = map[indices[from + 1]];
  out[to + 2] = map[indices[from + 2]];
}

// ---------------------------------------------------------------------------------------------
// float64 vectors of the ordered sums of decimation and smoothing: separate operations in the stated order (the library is built
// without contraction).
// ---------------------------------------------------------------------------------------------
struct dec3 { double x, y, z; };
__device__ __forceinline__ dec3 dec_sub(dec3 a, dec3 b) { return dec3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ dec3 dec_cross(dec3 u, dec3 v) { return dec3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; }
__device__ __forceinline__ dec3 dec_load(const float* __restrict__ p, uint32_t v) { return dec3{(double)p[3 * (size_t)v], (double)p[3 * (size_t)v + 1], (double)p[3 * (size_t)v + 2]}; }
__device__ __forceinline__ dec3 dec_normal(dec3 a, dec3 b, dec3 c) { return dec_cross(dec_sub(b, a), dec_sub(c, a)); }

}  // namespace bslam
