// mesh_kernels.hpp -- an indexed triangle mesh as a graph, for gfx950: connected components by a data-parallel union-find and
// the compaction that drops the components below a vertex count.  The reference has no mesh at all (fusion_kernels.hpp); every
// mesher its users know ships this step.  Everything is integer, so the outputs do not depend on the order of execution and a
// sequential restatement reproduces every bit.
//
// The rule (include/badslam_hip.h, DESIGN.md 8 "Mesh components"): vertices a and b are joined iff a triangle contains both; a
// component is a class of the transitive closure; label[v] = the smallest vertex id of v's component, size[v] = its vertex count.
//
// Behind them, what the mesh operators built on this file share (simplify_, decimate_, smooth_, repair_, orient_kernels.hpp): the
// position check, the wave-aggregated count, the compaction of an attributed mesh, the triangle remap -- keep flag and scatter of the
// triangles through a vertex map --, the runs of a stable sort and the edge runs, and the float64 vector helpers of the ordered sums.
// The union-find is a template: plain here, with a parity bit for the orientation.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace bslam {

// Bits of the device error word of every mesh call: words[0] of its small device block.
constexpr uint32_t kMeshBadIndex = 1u;      // a triangle names a vertex >= V: never dereferenced
constexpr uint32_t kMeshOverrun = 2u;       // a find or a retry loop ran into its cap: cannot happen while parent[v] <= v holds
constexpr uint32_t kMeshBadPosition = 8u;   // a position is not finite (4 is simplification's own, kSimplifyBadVertex)
constexpr uint32_t kMeshDegenerate = 16u;   // a triangle given to the edge runs repeats an index

// Neither an infinity nor a NaN (named for its first user, distance_kernels.hpp, which includes this file).
__device__ __forceinline__ bool pmd_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// One vertex per lane: raises the error bit for a position that is not finite.
__global__ __launch_bounds__(256) void mesh_check_positions_kernel(uint32_t vertices, const float* __restrict__ positions, uint32_t* __restrict__ error) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= vertices) return;
  if (!(pmd_finite(positions[3 * (size_t)v]) && pmd_finite(positions[3 * (size_t)v + 1]) && pmd_finite(positions[3 * (size_t)v + 2]))) atomicOr(error, kMeshBadPosition);
}

// *word += the number of lanes of the wave that arrive with `flag` set: one atomic per wave.
__device__ __forceinline__ void mesh_wave_count(uint32_t* word, bool flag) {
  const unsigned long long votes = __ballot(flag);
  if (flag && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(votes)) atomicAdd(word, (uint32_t)__popcll(votes));
}

// ---------------------------------------------------------------------------------------------
// Union-find over entry[N], plain (kParity = false: entry[v] = parent) or with a parity bit (kParity = true: entry[v] =
// parent << 1 | parity, where parity is f[v] ^ f[parent] of every assignment f that satisfies the relations joined so far;
// orient_kernels.hpp).  The invariant, at all times: parent <= v, and every word holds a true (ancestor, parity to that ancestor)
// pair.  So a find walks strictly downwards and ends after at most N steps whatever other threads do, and the root of a finished
// component is its smallest id whatever the schedule.  A hook writes the parity that the relation demands between the two roots,
// and path halving replaces (parent, p1) by (grandparent, p1 ^ p2) in one 32-bit store.  Links are only ever added, so the parity
// between two connected nodes never changes.
//
// The eight XCDs have separate L2s and a CU's L1 is never refreshed by another CU's stores, so inside the union kernels every
// access to entry[] is a relaxed atomic at agent scope (loads and stores that bypass the L1 and write through the L2; the hook
// is a compare-and-swap, which the memory side serialises).  Nothing is ordered and nothing needs to be: a stale word is a
// word the entry held earlier, parents only ever move to ancestors, so an old pointer still leads into the same tree and
// towards its root, with the right parity.  Only the hook has to be exact, and it is: it succeeds only if the entry still holds
// the root itself.
//
// Termination of mesh_unite_wave needs no other wave: whenever a lane swaps, succeeds or fails, the larger of its two nodes
// decreases or it is done; a lane that does not swap waits for at most the 63 lanes below it that hold the same larger root,
// each of which leaves that value for good in the round it swaps.  So 64 (N + 64) rounds are more than the loop can take.
//
// In the plain instantiation the parity arguments are dead: `parity` may be null and `rel` is ignored.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t parent_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void parent_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of v with path halving: every second node on the way is pointed at its grandparent, an ancestor below it; *parity ^= the
// parity from v to the root.  A node that is rewritten was seen with a parent other than itself, so it is no root and never
// becomes one again: the store cannot undo a hook.  At most `cap` steps; *overrun is set beyond.
template <bool kParity>
__device__ __forceinline__ uint32_t mesh_find(uint32_t* entry, uint32_t v, uint32_t* parity, uint32_t cap, bool* overrun) {
  uint32_t w = parent_load(entry + v);
  for (uint32_t steps = 0; (w >> kParity) != v; ++steps) {
    if (steps >= cap) { *overrun = true; return v; }
    const uint32_t p = w >> kParity, wp = parent_load(entry + p);
    if ((wp >> kParity) != p) parent_store(entry + v, kParity ? (wp & ~1u) | ((w ^ wp) & 1u) : wp);
    if constexpr (kParity) *parity ^= w & 1u;
    v = p;
    w = wp;
  }
  return v;
}

// Joins the trees of a and b, which must differ by `rel` (f[a] ^ f[b]), for every lane of a wave whose `active` is set; all 64
// lanes call it together.  Per round a lane finds its two roots, folding their parities into rel, which then is what the two
// roots must differ by; if they differ, it wants to hook the larger one, hi, under the smaller one with that parity by a
// compare-and-swap on hi's entry that expects hi itself.  Neighbours mostly want the same hook, and same-address atomics are
// serialised by the memory side, so of the lanes that hold the same hi only the lowest one swaps in a round; the others find
// again in the next round and as a rule see the hook done.  A failed swap means the entry no longer holds the root -- another
// thread hooked it, or the find ended on a stale value -- and returns the word it holds now, a true (ancestor, parity) pair of
// the failed root: that lane goes on from this ancestor, strictly below the failed root, with the parity folded in.  Two nodes
// found under one root are left alone, whatever rel says.  tries / fails: swaps attempted and failed (profiling).
template <bool kParity>
__device__ __forceinline__ void mesh_unite_wave(uint32_t* entry, bool active, uint32_t a, uint32_t b, uint32_t rel, uint32_t count, bool* overrun,
                                                uint32_t* tries, uint32_t* fails) {
  const uint32_t cap = count + 64u;
  const int lane = (int)(threadIdx.x & 63u);
  for (unsigned long long round = 0; __ballot(active) != 0; ++round) {   // wave-uniform
    uint32_t hi = 0, lo = 0;
    if (active) {
      a = mesh_find<kParity>(entry, a, &rel, cap, overrun);
      b = mesh_find<kParity>(entry, b, &rel, cap, overrun);
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
      uint32_t expected = hi << kParity;
      *tries += 1;
      if (__hip_atomic_compare_exchange_strong(entry + hi, &expected, kParity ? (lo << 1) | rel : lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT)) {
        active = false;
      } else {
        *fails += 1;
        a = expected >> kParity;   // the parent the entry holds now, < hi
        if constexpr (kParity) rel ^= expected & 1u;
        b = lo;
      }
    }
    if (active && round >= 64ull * cap) { *overrun = true; active = false; }
  }
}

// Root of v by plain loads, for the launches in which no hook runs: the entries other threads rewrite meanwhile (compress) only
// move to ancestors, and an aligned word is read whole.  *parity = the parity from v to the root.  At most N + 64 steps; *overrun
// is set beyond.
template <bool kParity>
__device__ __forceinline__ uint32_t mesh_root(const uint32_t* entry, uint32_t v, uint32_t count, uint32_t* parity, bool* overrun) {
  uint32_t w = entry[v], p = 0;
  for (uint32_t steps = 0; (w >> kParity) != v; ++steps) {
    if (steps >= count + 64u) { *overrun = true; break; }
    p ^= w & 1u;
    v = w >> kParity;
    w = entry[v];
  }
  if constexpr (kParity) *parity = p;
  return v;
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

// Behind the seeding, the trees are chains as deep as the mesh is long in vertex order (about one link per slab of the volume).
// One thread per vertex points its entry at its root, so that the finds of the union launch start two loads from a root
// instead of walking and halving those chains with write-through stores, all of them at once.
__global__ __launch_bounds__(256) void mesh_compress_kernel(uint32_t vertices, uint32_t* parent, uint32_t* __restrict__ words) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= vertices) return;
  bool overrun = false;
  const uint32_t first = parent[v];
  const uint32_t root = mesh_root<false>(parent, first, vertices, nullptr, &overrun);
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
  mesh_unite_wave<false>(parent, valid && i1 != i0, i0, i1, 0, vertices, &overrun, &tries, &fails);
  mesh_unite_wave<false>(parent, valid && i2 != i0 && i2 != i1, i0, i2, 0, vertices, &overrun, &tries, &fails);
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
    root = mesh_root<false>(parent, v, vertices, nullptr, &overrun);
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
// arrays (device_scan) give the new ids; mesh_compact_kernel scatters both.  The launches cover the vertices first and the
// triangles behind them: blocks [0, vertex_blocks) take a vertex per thread, the others a triangle.
// ---------------------------------------------------------------------------------------------
struct MeshFilter {
  uint32_t vertices, triangles, vertex_blocks, min_vertices;
  const uint32_t* indices; const uint32_t* sizes;
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

// ---------------------------------------------------------------------------------------------
// Compaction of an attributed mesh (bslam_filter_mesh, bslam_clean_mesh).  The ranks are the exclusive scans of the keep flags.
// ---------------------------------------------------------------------------------------------
struct MeshCompact {
  uint32_t vertices, triangles, vertex_blocks;
  const float* positions; const float* normals; const uint32_t* colors;   // normals, colors: may be null
  const uint32_t* indices;
  const uint8_t* keep_vertex; const uint8_t* keep_triangle; const uint32_t* vertex_rank; const uint32_t* triangle_rank;
  const uint32_t* rep;                                                    // the representative of a vertex; null: itself
  float* out_positions; float* out_normals; uint32_t* out_colors; uint32_t* out_indices;
  uint32_t* vertex_map; uint32_t* triangle_map;                           // may be null
};

// out[to .. to + 2] = in[from .. from + 2] as words: a copy must not canonicalise a NaN's payload.
__device__ __forceinline__ void mesh_copy3(const float* in, size_t from, float* out, size_t to) {
  const uint32_t* src = (const uint32_t*)in;
  uint32_t* dst = (uint32_t*)out;
  dst[to] = src[from]; dst[to + 1] = src[from + 1]; dst[to + 2] = src[from + 2];
}

// Blocks [0, vertex_blocks) take a vertex per lane, the others a triangle.  A kept vertex goes to its rank with the bits of its
// attributes, a kept triangle to its rank with its corners through rep and the ranks, in their order; the maps get the new ids or
// 0xffffffff.  Nothing at or beyond the kept counts is written.  The null tests are uniform over the launch.
__global__ __launch_bounds__(256) void mesh_compact_kernel(MeshCompact m) {
  if (blockIdx.x < m.vertex_blocks) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= m.vertices) return;
    if (m.vertex_map != nullptr) {
      const uint32_t r = m.rep != nullptr ? m.rep[v] : v;
      m.vertex_map[v] = m.keep_vertex[r] ? m.vertex_rank[r] : 0xffffffffu;
    }
    if (!m.keep_vertex[v]) return;
    const size_t from = 3 * (size_t)v, to = 3 * (size_t)m.vertex_rank[v];
    mesh_copy3(m.positions, from, m.out_positions, to);
    if (m.normals != nullptr) mesh_copy3(m.normals, from, m.out_normals, to);
    if (m.colors != nullptr) m.out_colors[m.vertex_rank[v]] = m.colors[v];
    return;
  }
  const uint32_t t = (blockIdx.x - m.vertex_blocks) * blockDim.x + threadIdx.x;
  if (t >= m.triangles) return;
  if (m.triangle_map != nullptr) m.triangle_map[t] = m.keep_triangle[t] ? m.triangle_rank[t] : 0xffffffffu;
  if (!m.keep_triangle[t]) return;
  const size_t from = 3 * (size_t)t, to = 3 * (size_t)m.triangle_rank[t];
  for (int k = 0; k < 3; ++k) {
    const uint32_t corner = m.indices[from + k];
    m.out_indices[to + k] = m.vertex_rank[m.rep != nullptr ? m.rep[corner] : corner];
  }
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
// Runs of equal keys behind a stable sort (mesh_sort), and the edge runs: the sorted incidence table "which slots use which
// undirected edge" of the census and of the orientation (repair_kernels.hpp, orient_kernels.hpp).  A slot is 3 t + k: corner k of
// triangle t, and the directed half-edge from corner k to corner (k + 1) % 3.  E = 3 T slots.  By sorted position i the edges lie
// in runs, each in ascending slot; run r starts at start_of[r] and start_of[U] = E.
// ---------------------------------------------------------------------------------------------

// The key of the undirected edge {a, b} for vertex ids of `bits` bits, lo << bits | hi, and its two ends.
__device__ __forceinline__ unsigned long long mesh_edge_key(uint32_t a, uint32_t b, uint32_t bits) {
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
  return ((unsigned long long)lo << bits) | hi;
}
__device__ __forceinline__ uint32_t mesh_edge_lo(unsigned long long e, uint32_t bits) { return (uint32_t)(e >> bits); }
__device__ __forceinline__ uint32_t mesh_edge_hi(unsigned long long e, uint32_t bits) { return (uint32_t)(e & ((1ull << bits) - 1ull)); }

// The keys of the second of two stable sorts, in the order the first one left: out[i] = key[ids[i]].
__global__ __launch_bounds__(256) void mesh_gather_kernel(uint32_t count, const unsigned long long* __restrict__ key, const uint32_t* __restrict__ ids,
                                                          unsigned long long* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) out[i] = key[ids[i]];
}

// head[i] = 1 iff sorted position i starts a run of equal keys: the sorted key of the last sort and, where an earlier sort took part
// of the key, that part of the element itself (first_key, by id; may be null).
__global__ __launch_bounds__(256) void mesh_heads_kernel(uint32_t count, const unsigned long long* __restrict__ sorted_keys, const uint32_t* __restrict__ ids,
                                                         const unsigned long long* __restrict__ first_key, uint8_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  bool h = i == 0 || sorted_keys[i] != sorted_keys[i - 1];
  if (!h && first_key != nullptr) h = first_key[ids[i]] != first_key[ids[i - 1]];
  head[i] = h ? 1 : 0;
}

struct EdgeRuns {
  uint32_t vertices, triangles, slots, bits;   // bits: of a vertex id
  const uint32_t* indices;
  unsigned long long *keys, *sorted_keys;      // [E] mesh_edge_key
  uint32_t *ids, *sorted_slots;                // [E]
  uint8_t* head; uint32_t* rank;               // [E] by sorted position; rank: the inclusive scan of head
  uint32_t* start_of;                          // [E + 1]
  uint8_t* referenced;                         // [V] a triangle names the vertex; zero before; may be null
  uint32_t* error;                             // the error word of the call
};

// One triangle per lane: the three edge keys, id[slot] = slot, referenced[corner] = 1.  An index >= V and a repeated index raise
// their error bits; the call reads the word back before anything is decoded from a key.
__global__ __launch_bounds__(256) void edge_keys_kernel(EdgeRuns s) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= s.triangles) return;
  const uint32_t i[3] = {s.indices[3 * (size_t)t], s.indices[3 * (size_t)t + 1], s.indices[3 * (size_t)t + 2]};
  const bool valid = i[0] < s.vertices && i[1] < s.vertices && i[2] < s.vertices;
  if (!valid) atomicOr(s.error, kMeshBadIndex);
  else if (i[0] == i[1] || i[0] == i[2] || i[1] == i[2]) atomicOr(s.error, kMeshDegenerate);
  for (int k = 0; k < 3; ++k) {
    const size_t slot = 3 * (size_t)t + k;
    s.keys[slot] = valid ? mesh_edge_key(i[k], i[(k + 1) % 3], s.bits) : ~0ull;
    s.ids[slot] = (uint32_t)slot;
    if (valid && s.referenced != nullptr) s.referenced[i[k]] = 1;
  }
}

// start_of[r] = the sorted position at which run r starts, and start_of[U] = E.
__global__ __launch_bounds__(256) void edge_starts_kernel(EdgeRuns s) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.slots) return;
  if (s.head[i]) s.start_of[s.rank[i] - 1u] = i;
  if (i + 1 == s.slots) s.start_of[s.rank[i]] = s.slots;
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
