// orient_kernels.hpp -- consistent winding of an indexed triangle mesh, for gfx950: a union-find over the triangles that carries a
// parity bit (the kParity = true instantiation of mesh_kernels.hpp: link[t] = parent << 1 | parity, where parity is f[t] ^ f[parent]
// of every assignment f that satisfies the seams joined so far), a conflict pass that finds the pieces that cannot be oriented, the
// per-patch votes for which side is out, and the pass that writes the flipped triangles.  The edge runs are those of mesh_kernels.hpp
// (EdgeRuns; build_edge_runs of mesh_abi.inc).  The reference has no mesh.
//
// The rule (include/badslam_hip.h "Mesh orientation", DESIGN.md 8 "Mesh orientation"): a seam is an edge with exactly two uses; it
// disagrees iff its two slots start at the same vertex.  Triangles that share a seam are joined; a patch is a class of the transitive
// closure and its id its smallest triangle.  flip0[t] is the parity of t relative to that triangle over any path of seams, which is
// well defined iff the patch is orientable.  Everything is integer but the two votes, which are float64 expressions of one triangle
// each, summed as integers: nothing depends on the order of execution, and a breadth-first restatement reproduces every bit.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mesh_kernels.hpp"

namespace bslam {

constexpr int kOrientMajority = 0, kOrientNormals = 1, kOrientVolume = 2;

// Words of the call's second device block (u32 units): the report, then the bounds of the positions as ordered keys.
constexpr int kOrientSeams = 0, kOrientDisagreeBefore = 1, kOrientDisagreeAfter = 2, kOrientPatches = 3, kOrientOrientable = 4, kOrientNonOrientable = 5,
              kOrientClosed = 6, kOrientFlipped = 7, kOrientInverted = 8, kOrientFallback = 9, kOrientMin = 16, kOrientMax = 19, kOrientWords = 32;

// Bits of state[root].
constexpr uint32_t kOrientConflict = 1u, kOrientOpen = 2u;

struct OrientMesh {
  EdgeRuns runs;                                       // triangles, slots, indices, the runs; runs.error: the error word of the call
  int mode;
  int size_bits;                                       // the bit length of T
  const float* positions; const float* normals;        // normals: null unless mode 1
  uint32_t* link;                                      // [T] parent << 1 | parity to the parent; parent <= t
  uint8_t* seam;                                       // [E] by sorted position: 0, or 1 | disagrees << 1 at the head of a run of two
  uint8_t* open;                                       // [T] a slot of t lies on an edge with other than two uses
  uint32_t* patch; uint8_t* flip0;                     // [T]
  uint32_t *state, *size, *ones, *positive, *negative; // [T] at the root
  long long* volume;                                   // [T] at the root
  uint8_t* invert;                                     // [T] at the root
  uint32_t* out_indices; uint8_t* flipped; uint32_t* patch_of_triangle;   // the caller's; the last two may be null
  uint32_t* counts;                                    // kOrientWords
};

// A float as a key whose unsigned order is the order of the floats (-0.0f below +0.0f), and back.
__device__ __forceinline__ uint32_t orient_key(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float orient_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? k & 0x7fffffffu : ~k); }

// One vertex per lane: the componentwise minimum and maximum of the positions.  The lanes are reduced over the wave, the four waves
// through LDS, and one lane per axis adds for the block.  The six words only ever move one way, so a block that cannot move the
// value it reads skips its atomic: few of them queue up on the same six addresses.  counts[kOrientMin ..] is all ones and
// counts[kOrientMax ..] zero before.
__global__ __launch_bounds__(256) void orient_bounds_kernel(uint32_t vertices, const float* __restrict__ positions, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wave_lo[4][3], wave_hi[4][3];
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < vertices)
    for (int a = 0; a < 3; ++a) lo[a] = hi[a] = orient_key(positions[3 * (size_t)v + a]);
  for (int o = 32; o > 0; o >>= 1)
    for (int a = 0; a < 3; ++a) {
      lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], o, 64));
      hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], o, 64));
    }
  if ((threadIdx.x & 63u) == 0)
    for (int a = 0; a < 3; ++a) { wave_lo[threadIdx.x >> 6][a] = lo[a]; wave_hi[threadIdx.x >> 6][a] = hi[a]; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int a = (int)threadIdx.x;
    const uint32_t l = min(min(wave_lo[0][a], wave_lo[1][a]), min(wave_lo[2][a], wave_lo[3][a]));
    const uint32_t h = max(max(wave_hi[0][a], wave_hi[1][a]), max(wave_hi[2][a], wave_hi[3][a]));
    if (l < parent_load(&counts[kOrientMin + a])) atomicMin(&counts[kOrientMin + a], l);
    if (h > parent_load(&counts[kOrientMax + a])) atomicMax(&counts[kOrientMax + a], h);
  }
}

// link[t] = t << 1: every triangle a root with parity 0; the per-triangle and per-root sums are cleared.
__global__ __launch_bounds__(256) void orient_init_kernel(OrientMesh m) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m.runs.triangles) return;
  m.link[t] = t << 1;
  m.open[t] = 0;
  m.state[t] = 0; m.size[t] = 0; m.ones[t] = 0; m.positive[t] = 0; m.negative[t] = 0;
  m.volume[t] = 0;
  m.invert[t] = 0;
}

// By sorted position, one launch whatever the diameter: the triangles of a slot on an edge with other than two uses are open; the head
// of a run of two is a seam, counted, kept in seam[] with its disagreement for the launches behind, and its two triangles are joined
// with that disagreement as their relation.  Two triangles already under one root are left alone, whatever the seam says: the
// conflict pass looks at every seam again.
__global__ __launch_bounds__(256) void orient_union_kernel(OrientMesh m) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool is_seam = false;
  uint32_t a = 0, b = 0, d = 0;
  if (i < m.runs.slots) {   // lanes beyond the last slot stay: the wave votes as a whole
    const uint32_t r = m.runs.rank[i] - 1u, uses = m.runs.start_of[r + 1] - m.runs.start_of[r], slot = m.runs.sorted_slots[i];
    if (uses != 2) m.open[slot / 3u] = 1;
    is_seam = uses == 2 && m.runs.head[i] != 0;
    if (is_seam) {
      const uint32_t other = m.runs.sorted_slots[i + 1];   // a run of two: i + 1 < E
      a = slot / 3u;
      b = other / 3u;
      d = m.runs.indices[slot] == m.runs.indices[other] ? 1u : 0u;
    }
    m.seam[i] = is_seam ? (uint8_t)(1u | (d << 1)) : (uint8_t)0;
  }
  mesh_wave_count(&m.counts[kOrientSeams], is_seam);
  mesh_wave_count(&m.counts[kOrientDisagreeBefore], is_seam && d != 0);
  bool overrun = false;
  uint32_t tries = 0, fails = 0;   // not reported
  mesh_unite_wave<true>(m.link, is_seam, a, b, d, m.runs.triangles, &overrun, &tries, &fails);
  if (overrun) atomicOr(m.runs.error, kMeshOverrun);
}

// By sorted position, behind the union: the two triangles of a seam have one root, and the patch cannot be oriented iff for one of
// its seams their parities to it differ by other than the seam's disagreement -- whichever spanning forest the hooks built.
__global__ __launch_bounds__(256) void orient_conflict_kernel(OrientMesh m) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m.runs.slots) return;
  const uint32_t code = m.seam[i];
  if (code == 0) return;
  bool overrun = false;
  uint32_t pa = 0, pb = 0;
  const uint32_t ra = mesh_root<true>(m.link, m.runs.sorted_slots[i] / 3u, m.runs.triangles, &pa, &overrun);
  const uint32_t rb = mesh_root<true>(m.link, m.runs.sorted_slots[i + 1] / 3u, m.runs.triangles, &pb, &overrun);
  if (overrun || ra != rb) { atomicOr(m.runs.error, kMeshOverrun); return; }
  if ((pa ^ pb) != (code >> 1) && !(m.state[ra] & kOrientConflict)) atomicOr(&m.state[ra], kOrientConflict);
}

struct orient3 { double x, y, z; };
__device__ __forceinline__ orient3 orient_load(const float* __restrict__ p, uint32_t v) {
  return orient3{(double)p[3 * (size_t)v], (double)p[3 * (size_t)v + 1], (double)p[3 * (size_t)v + 2]};
}
__device__ __forceinline__ orient3 orient_sub(orient3 a, orient3 b) { return orient3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ orient3 orient_cross(orient3 u, orient3 v) { return orient3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; }
__device__ __forceinline__ double orient_dot(orient3 a, orient3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// One triangle per lane: patch[t], flip0[t], and the sums of its patch at the root: triangles, those with flip0 = 1, the open flag and
// the vote of the mode, evaluated on the triangle as flip0 leaves it -- corners 1 and 2 exchanged where it is 1.  The lanes of a wave
// that share a root add once; after four distinct roots the lanes that are left add for themselves (mesh_flatten_kernel).
__global__ __launch_bounds__(256) void orient_flatten_kernel(OrientMesh m) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  bool live = t < m.runs.triangles, overrun = false;
  uint32_t root = 0, par = 0;
  bool open = false, plus = false, minus = false;
  long long q = 0;
  if (live) {
    root = mesh_root<true>(m.link, t, m.runs.triangles, &par, &overrun);
    if (overrun) { atomicOr(m.runs.error, kMeshOverrun); live = false; }
  }
  if (live) {
    m.patch[t] = root;
    m.flip0[t] = (uint8_t)par;
    open = m.open[t] != 0;
    const uint32_t i0 = m.runs.indices[3 * (size_t)t], i1 = m.runs.indices[3 * (size_t)t + 1 + par], i2 = m.runs.indices[3 * (size_t)t + 2 - par];
    if (m.mode == kOrientNormals) {
      const orient3 p0 = orient_load(m.positions, i0), p1 = orient_load(m.positions, i1), p2 = orient_load(m.positions, i2);
      const orient3 n0 = orient_load(m.normals, i0), n1 = orient_load(m.normals, i1), n2 = orient_load(m.normals, i2);
      const orient3 n = {(n0.x + n1.x) + n2.x, (n0.y + n1.y) + n2.y, (n0.z + n1.z) + n2.z};
      const double vote = orient_dot(orient_cross(orient_sub(p1, p0), orient_sub(p2, p0)), n);
      plus = vote > 0.0;
      minus = vote < 0.0;
    } else if (m.mode == kOrientVolume) {
      const orient3 c = {(double)orient_unkey(m.counts[kOrientMin]), (double)orient_unkey(m.counts[kOrientMin + 1]), (double)orient_unkey(m.counts[kOrientMin + 2])};
      const orient3 e = {(double)orient_unkey(m.counts[kOrientMax]) - c.x, (double)orient_unkey(m.counts[kOrientMax + 1]) - c.y,
                         (double)orient_unkey(m.counts[kOrientMax + 2]) - c.z};
      const double extent = fmax(e.x, fmax(e.y, e.z));
      if (extent > 0.0) {
        int exponent = 0;
        (void)frexp(extent, &exponent);
        const orient3 a = orient_sub(orient_load(m.positions, i0), c), b = orient_sub(orient_load(m.positions, i1), c), d = orient_sub(orient_load(m.positions, i2), c);
        q = __double2ll_rn(ldexp(orient_dot(a, orient_cross(b, d)), 58 - 3 * exponent - m.size_bits));
      }
    }
  }
  const int lane = (int)(threadIdx.x & 63u);
  unsigned long long todo = __ballot(live);
  for (int round = 0; round < 4 && todo != 0; ++round) {   // wave-uniform
    const int leader = __builtin_ctzll(todo);
    const uint32_t l = __shfl(root, leader, 64);
    const bool mine = ((todo >> lane) & 1ull) && root == l;
    const unsigned long long same = __ballot(mine), ones = __ballot(mine && par), opens = __ballot(mine && open), pluses = __ballot(mine && plus),
                             minuses = __ballot(mine && minus);
    long long sum = mine ? q : 0;
    if (m.mode == kOrientVolume)
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == leader) {
      atomicAdd(&m.size[l], (uint32_t)__popcll(same));
      if (ones) atomicAdd(&m.ones[l], (uint32_t)__popcll(ones));
      if (opens) atomicOr(&m.state[l], kOrientOpen);
      if (pluses) atomicAdd(&m.positive[l], (uint32_t)__popcll(pluses));
      if (minuses) atomicAdd(&m.negative[l], (uint32_t)__popcll(minuses));
      if (sum != 0) atomicAdd((unsigned long long*)&m.volume[l], (unsigned long long)sum);
    }
    todo &= ~same;
  }
  if ((todo >> lane) & 1ull) {
    atomicAdd(&m.size[root], 1u);
    if (par) atomicAdd(&m.ones[root], 1u);
    if (open) atomicOr(&m.state[root], kOrientOpen);
    if (plus) atomicAdd(&m.positive[root], 1u);
    if (minus) atomicAdd(&m.negative[root], 1u);
    if (q != 0) atomicAdd((unsigned long long*)&m.volume[root], (unsigned long long)q);
  }
}

// One triangle per lane, the roots alone: the patch counts of the report and invert[root] by the rule of the mode; a patch whose
// vote does not decide falls back to the majority.  With an extent of zero no volume was added, so every sum is zero.
__global__ __launch_bounds__(256) void orient_decide_kernel(OrientMesh m) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool root = t < m.runs.triangles && m.patch[t] == t;
  bool orientable = false, closed = false, fallback = false, invert = false;
  if (root) {
    const uint32_t state = m.state[t], size = m.size[t], ones = m.ones[t];
    orientable = !(state & kOrientConflict);
    closed = !(state & kOrientOpen);
    if (orientable) {
      const bool majority = ones > size - ones;
      if (m.mode == kOrientNormals) {
        fallback = m.positive[t] == m.negative[t];
        invert = fallback ? majority : m.negative[t] > m.positive[t];
      } else if (m.mode == kOrientVolume) {
        const long long volume = m.volume[t];
        fallback = !closed || volume == 0;
        invert = fallback ? majority : volume < 0;
      } else {
        invert = majority;
      }
      m.invert[t] = invert ? 1 : 0;
    }
  }
  mesh_wave_count(&m.counts[kOrientPatches], root);
  mesh_wave_count(&m.counts[kOrientOrientable], root && orientable);
  mesh_wave_count(&m.counts[kOrientNonOrientable], root && !orientable);
  mesh_wave_count(&m.counts[kOrientClosed], root && closed);
  mesh_wave_count(&m.counts[kOrientFallback], fallback);
  mesh_wave_count(&m.counts[kOrientInverted], invert);
}

// Blocks [0, triangle_blocks) take a triangle per lane: flipped = flip0 ^ invert of its patch, or 0 where the patch cannot be oriented;
// (a, b, c) is written as (a, c, b) where it is set.  The other blocks take a sorted position per lane and count the seams that
// disagree in the output: those of the patches that were left alone.
__global__ __launch_bounds__(256) void orient_write_kernel(OrientMesh m, uint32_t triangle_blocks) {
  if (blockIdx.x < triangle_blocks) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    bool flip = false;
    if (t < m.runs.triangles) {
      const uint32_t root = m.patch[t];
      flip = !(m.state[root] & kOrientConflict) && (m.flip0[t] ^ m.invert[root]) != 0;
      const size_t at = 3 * (size_t)t;
      const uint32_t a = m.runs.indices[at], b = m.runs.indices[at + 1], c = m.runs.indices[at + 2];
      m.out_indices[at] = a; m.out_indices[at + 1] = flip ? c : b; m.out_indices[at + 2] = flip ? b : c;
      if (m.flipped != nullptr) m.flipped[t] = flip ? 1 : 0;
      if (m.patch_of_triangle != nullptr) m.patch_of_triangle[t] = root;
    }
    mesh_wave_count(&m.counts[kOrientFlipped], flip);
    return;
  }
  const uint32_t i = (blockIdx.x - triangle_blocks) * blockDim.x + threadIdx.x;
  bool disagrees = false;
  if (i < m.runs.slots && (m.seam[i] & 2u)) disagrees = (m.state[m.patch[m.runs.sorted_slots[i] / 3u]] & kOrientConflict) != 0;
  mesh_wave_count(&m.counts[kOrientDisagreeAfter], disagrees);
}

}  // namespace bslam
