// bvh_kernels.hpp -- the nearest triangle of an indexed mesh for each of N points, without a search radius, for gfx950: a linear
// bounding-volume hierarchy over the triangles (Morton codes of the box centres, one stable radix sort, the radix tree of Karras,
// "Maximizing Parallelism in the Construction of BVHs, Octrees, and k-d Trees", HPG 2012) and a stack traversal, one lane per point.
// The reference has neither a mesh nor a way to measure one.
//
// The rule (include/badslam_hip.h "Nearest triangle", DESIGN.md 8 "Nearest triangle") is the pair value of "Surface evaluation"
// clamped from below by the distance to the triangle's own box, b2.  b2 is monotone under inclusion of boxes AS FLOATS (fp32
// subtraction, max, the product of non-negatives and an fma with non-negative addends are monotone under round-to-nearest), so
// b2(p, box of a node) <= d2(p, t) for every triangle t below the node, and skipping a subtree iff b2 > min(best, fl(R * R)) loses
// no minimum and no tie: the result is a function of the rule alone, not of the tree's shape, the key width, the traversal order or
// the order in which atomics arrive.  A brute-force restatement over all N x T pairs reproduces every bit.
//
// No kernel here waits on another thread: every loop is bounded by the height bound or by log2 of the leaf count, and data passes
// between workgroups only from one launch to the next or through atomics on the word itself.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_math.hpp"
#include "distance_kernels.hpp"
#include "mesh_kernels.hpp"

namespace bslam {

// Words of the small device block of a call (u32 units).
constexpr int kBvhError = 0;     // kMeshBadIndex
constexpr int kBvhValid = 1;     // triangles with nine finite coordinates: the leaves
constexpr int kBvhMinKey = 2;    // [3]: order-preserving keys of the minimum of the box centres
constexpr int kBvhMaxKey = 5;    // [3]: ... of the maximum
constexpr int kBvhHeight = 8;    // edges from the root to the deepest leaf
constexpr int kBvhWords = 16;

// The Morton code: kBvhAxisBits per axis.  In the sorted order the augmented key of leaf j is (code << 32) | j, and delta(i, j) is
// the number of leading bits two augmented keys share: 64 - 32 - kBvhKeyBits <= delta <= 63.  delta grows strictly from a node to
// its child, so a path from the root holds at most kBvhKeyBits + 32 internal nodes: the height bound, and the most entries a
// traversal stack can hold (one deferred sibling per level).
constexpr int kBvhAxisBits = 10;
constexpr int kBvhKeyBits = 3 * kBvhAxisBits;
constexpr int kBvhMaxHeight = kBvhKeyBits + 32;
constexpr int kBvhStack = 64;
constexpr int kBvhQueryBlock = 64;   // one wave: its stack is kBvhStack x 64 words of LDS, 16 KiB
static_assert(kBvhKeyBits <= 31, "the key of an invalid triangle, 1 << kBvhKeyBits, has to sort behind every code inside 32 bits");
static_assert(kBvhStack >= kBvhMaxHeight, "no input may overflow the traversal stack");
static_assert(kBvhStack * kBvhQueryBlock * sizeof(uint32_t) <= 64 * 1024, "the stack has to fit the LDS of a block");

constexpr uint32_t kBvhLeafBit = 0x80000000u;   // of a child reference: the rest is a position in the sorted order, else an internal node
constexpr uint32_t kBvhNoNode = 0xffffffffu;    // the root's parent
constexpr int kBvhNodeQuads = 4;                // float4 per packed node
constexpr int kBvhLeafQuads = 3;                // float4 per leaf record

// Quantisation of the box centres: cell = (c - origin) * scale on each axis, clamped to the code's range.
struct BvhQuantiser {
  float origin[3];
  float scale[3];   // 2^kBvhAxisBits / extent, or 0 where the extent is 0 or not finite: any key is a correct key
};

struct BvhTriangle {
  bool valid;
  f3 a, b, c, lo, hi;   // lo, hi: the component-wise fp32 minimum and maximum
};

__device__ __forceinline__ float bvh_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// Vertices and box of triangle t.  *bad is set for an index >= V, which is never dereferenced.
__device__ __forceinline__ BvhTriangle bvh_load_triangle(uint32_t t, uint32_t vertices, const float* __restrict__ positions, const uint32_t* __restrict__ indices, bool* bad) {
  BvhTriangle r;
  r.valid = false;
  const uint32_t i0 = indices[3 * (size_t)t], i1 = indices[3 * (size_t)t + 1], i2 = indices[3 * (size_t)t + 2];
  if (i0 >= vertices || i1 >= vertices || i2 >= vertices) { *bad = true; return r; }
  r.a = mk3(positions[3 * (size_t)i0], positions[3 * (size_t)i0 + 1], positions[3 * (size_t)i0 + 2]);
  r.b = mk3(positions[3 * (size_t)i1], positions[3 * (size_t)i1 + 1], positions[3 * (size_t)i1 + 2]);
  r.c = mk3(positions[3 * (size_t)i2], positions[3 * (size_t)i2 + 1], positions[3 * (size_t)i2 + 2]);
  r.valid = pmd_finite(r.a.x) && pmd_finite(r.a.y) && pmd_finite(r.a.z) && pmd_finite(r.b.x) && pmd_finite(r.b.y) && pmd_finite(r.b.z) &&
            pmd_finite(r.c.x) && pmd_finite(r.c.y) && pmd_finite(r.c.z);
  if (!r.valid) return r;
  r.lo = mk3(fminf(fminf(r.a.x, r.b.x), r.c.x), fminf(fminf(r.a.y, r.b.y), r.c.y), fminf(fminf(r.a.z, r.b.z), r.c.z));
  r.hi = mk3(fmaxf(fmaxf(r.a.x, r.b.x), r.c.x), fmaxf(fmaxf(r.a.y, r.b.y), r.c.y), fmaxf(fmaxf(r.a.z, r.b.z), r.c.z));
  return r;
}

// The centre of a box; halving first keeps it finite.  It places a triangle in the sorted order and decides nothing else.
__device__ __forceinline__ f3 bvh_centre(f3 lo, f3 hi) { return mk3(0.5f * lo.x + 0.5f * hi.x, 0.5f * lo.y + 0.5f * hi.y, 0.5f * lo.z + 0.5f * hi.z); }

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, off, 64));
  return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off, 64));
  return v;
}

// The census: the index check, the number of valid triangles and the bounds of their box centres, reduced per wave and then by
// integer atomics on order-preserving keys.  Every lane of a wave reaches the shuffles.
__global__ __launch_bounds__(256) void bvh_census_kernel(uint32_t vertices, uint32_t triangles, const float* __restrict__ positions, const uint32_t* __restrict__ indices,
                                                         uint32_t* __restrict__ words) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  BvhTriangle tri;
  tri.valid = false;
  if (t < triangles) tri = bvh_load_triangle(t, vertices, positions, indices, &bad);
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  if (tri.valid) {
    const f3 c = bvh_centre(tri.lo, tri.hi);
    lo[0] = hi[0] = pmd_key(c.x); lo[1] = hi[1] = pmd_key(c.y); lo[2] = hi[2] = pmd_key(c.z);
  }
  const unsigned long long any_bad = __ballot(bad), valid = __ballot(tri.valid);
#pragma unroll
  for (int a = 0; a < 3; ++a) { lo[a] = wave_min_u32(lo[a]); hi[a] = wave_max_u32(hi[a]); }
  if ((threadIdx.x & 63u) != 0) return;
  if (any_bad) atomicOr(&words[kBvhError], kMeshBadIndex);
  if (valid == 0) return;
  atomicAdd(&words[kBvhValid], (uint32_t)__popcll(valid));
#pragma unroll
  for (int a = 0; a < 3; ++a) { atomicMin(&words[kBvhMinKey + a], lo[a]); atomicMax(&words[kBvhMaxKey + a], hi[a]); }
}

// x with two zero bits in front of each of its low 10 bits.
__device__ __forceinline__ uint32_t bvh_spread(uint32_t x) {
  x &= 0x3ffu;
  x = (x | (x << 16)) & 0x030000ffu;
  x = (x | (x << 8)) & 0x0300f00fu;
  x = (x | (x << 4)) & 0x030c30c3u;
  x = (x | (x << 2)) & 0x09249249u;
  return x;
}
static_assert(kBvhAxisBits == 10, "bvh_spread interleaves 10 bits per axis");

__device__ __forceinline__ uint32_t bvh_cell(float c, float origin, float scale) {
  const float q = fmaxf((c - origin) * scale, 0.f);   // a NaN (inf * 0) becomes 0
  return q >= (float)((1 << kBvhAxisBits) - 1) ? (uint32_t)((1 << kBvhAxisBits) - 1) : (uint32_t)q;
}

// The sort keys: the Morton code of a valid triangle, 1 << kBvhKeyBits of every other one, which sorts them behind; ids[t] = t.
__global__ __launch_bounds__(256) void bvh_keys_kernel(BvhQuantiser qz, uint32_t vertices, uint32_t triangles, const float* __restrict__ positions,
                                                       const uint32_t* __restrict__ indices, unsigned long long* __restrict__ keys, uint32_t* __restrict__ ids) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= triangles) return;
  bool bad = false;
  const BvhTriangle tri = bvh_load_triangle(t, vertices, positions, indices, &bad);
  uint32_t key = 1u << kBvhKeyBits;
  if (tri.valid) {
    const f3 c = bvh_centre(tri.lo, tri.hi);
    key = bvh_spread(bvh_cell(c.x, qz.origin[0], qz.scale[0])) | (bvh_spread(bvh_cell(c.y, qz.origin[1], qz.scale[1])) << 1) |
          (bvh_spread(bvh_cell(c.z, qz.origin[2], qz.scale[2])) << 2);
  }
  keys[t] = key;
  ids[t] = t;
}

// The tree as the build holds it.  Internal nodes are 0 .. leaves - 2 and node 0 is the root; leaf j is position j of the sorted order.
struct BvhBuild {
  uint32_t leaves;
  const unsigned long long* sorted_keys;   // [leaves ...]: the Morton codes, ascending; equal codes in ascending triangle id
  const uint32_t* sorted_ids;              // the triangle of each leaf
  uint32_t* parent_internal;               // [leaves - 1]; kBvhNoNode for the root
  uint32_t* parent_leaf;                   // [leaves]
  uint32_t* children;                      // [2 (leaves - 1)]: child references
  uint32_t* box_min;                       // [3 (leaves - 1)]: order-preserving keys of the internal nodes' boxes, initialised to the empty box
  uint32_t* box_max;
  float* leaf_lo;                          // [3 leaves]
  float* leaf_hi;
  float4* nodes;                           // [kBvhNodeQuads (leaves - 1)]: the traversal layout (bvh_pack_kernel)
  float4* records;                         // [kBvhLeafQuads leaves]: a.xyz, bits of the triangle id | b.xyz, 0 | c.xyz, 0
};

// delta(i, j) of the augmented keys, -1 for j outside [0, leaves).
__device__ __forceinline__ int bvh_delta(const BvhBuild& b, uint32_t i, unsigned long long key_i, long long j) {
  if (j < 0 || j >= (long long)b.leaves) return -1;
  const unsigned long long key_j = ((unsigned long long)(uint32_t)b.sorted_keys[j] << 32) | (unsigned long long)j;
  return __clzll((long long)(key_i ^ key_j));   // i != j: the keys differ
}

// The radix tree, one thread per internal node (Karras 2012, section 3): the range of leaves the node covers from the deltas of
// its neighbours, its split by binary search, and the two children with their parent links.  Each thread reads the sorted keys of an
// earlier launch and writes words no other thread of this launch touches.  The searches halve or double a length below 2^33.
__global__ __launch_bounds__(256) void bvh_tree_kernel(BvhBuild b) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i + 1 >= b.leaves) return;
  const unsigned long long key_i = ((unsigned long long)(uint32_t)b.sorted_keys[i] << 32) | (unsigned long long)i;
  const long long d = bvh_delta(b, i, key_i, (long long)i + 1) > bvh_delta(b, i, key_i, (long long)i - 1) ? 1 : -1;
  const int delta_min = bvh_delta(b, i, key_i, (long long)i - d);
  long long l_max = 2;
  while (bvh_delta(b, i, key_i, (long long)i + l_max * d) > delta_min) l_max *= 2;   // ends outside the range at the latest: l_max <= 2^33
  long long l = 0;
  for (long long t = l_max / 2; t >= 1; t /= 2)
    if (bvh_delta(b, i, key_i, (long long)i + (l + t) * d) > delta_min) l += t;
  const long long j = (long long)i + l * d;
  const int delta_node = bvh_delta(b, i, key_i, j);
  long long s = 0;
  for (long long t = (l + 1) / 2;; t = (t + 1) / 2) {
    if (bvh_delta(b, i, key_i, (long long)i + (s + t) * d) > delta_node) s += t;
    if (t <= 1) break;
  }
  const long long gamma = (long long)i + s * d + (d < 0 ? -1 : 0);
  if (gamma < 0 || gamma + 1 >= (long long)b.leaves) return;   // never: the split lies inside the range
  const long long first = d > 0 ? (long long)i : j, last = d > 0 ? j : (long long)i;
  const bool left_leaf = first == gamma, right_leaf = last == gamma + 1;
  b.children[2 * (size_t)i] = (uint32_t)gamma | (left_leaf ? kBvhLeafBit : 0u);
  b.children[2 * (size_t)i + 1] = (uint32_t)(gamma + 1) | (right_leaf ? kBvhLeafBit : 0u);
  (left_leaf ? b.parent_leaf : b.parent_internal)[gamma] = i;
  (right_leaf ? b.parent_leaf : b.parent_internal)[gamma + 1] = i;
  if (i == 0) b.parent_internal[0] = kBvhNoNode;
}

// The boxes, one thread per leaf: the leaf's record and box, and the climb.  Every internal node's box is six order-preserving
// keys that start as the empty box.  A leaf folds ITS OWN box into its parent with six atomicMin / atomicMax, and goes on to the next
// ancestor only if one of the six values it got back shows that it changed the node; otherwise it stops.
//   Why every ancestor covers every leaf below it when the kernel ends: let leaf m stop at ancestor X.  Each of the six values it
//   found there was written by a leaf below X whose own bound it is and whose atomic changed X, so that leaf went on to X's parent.
//   By induction on the distance of the stopping node from the root (a leaf that reaches the root has folded into every ancestor),
//   all ancestors of X cover the boxes of those leaves, hence the six values, hence m's box.  Below X, m folded itself.
//   Nothing is read but what an atomic on the same word returns; min and max are exact, so the keys do not depend on the order of
//   arrival, and each equals the bound of some leaf below: the box IS the minimum and maximum over the leaves below.
// kHeight: the leaf also walks on to the root (parent links of an earlier launch) and the deepest depth goes to words[kBvhHeight].
template <bool kHeight>
__global__ __launch_bounds__(256) void bvh_boxes_kernel(BvhBuild b, uint32_t vertices, const float* __restrict__ positions, const uint32_t* __restrict__ indices,
                                                        uint32_t* __restrict__ words) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t depth = 0;
  if (j < b.leaves) {
    const uint32_t t = b.sorted_ids[j];
    bool bad = false;
    const BvhTriangle tri = bvh_load_triangle(t, vertices, positions, indices, &bad);   // valid: the census counted it
    b.records[kBvhLeafQuads * (size_t)j] = make_float4(tri.a.x, tri.a.y, tri.a.z, __uint_as_float(t));
    b.records[kBvhLeafQuads * (size_t)j + 1] = make_float4(tri.b.x, tri.b.y, tri.b.z, 0.f);
    b.records[kBvhLeafQuads * (size_t)j + 2] = make_float4(tri.c.x, tri.c.y, tri.c.z, 0.f);
    b.leaf_lo[3 * (size_t)j] = tri.lo.x; b.leaf_lo[3 * (size_t)j + 1] = tri.lo.y; b.leaf_lo[3 * (size_t)j + 2] = tri.lo.z;
    b.leaf_hi[3 * (size_t)j] = tri.hi.x; b.leaf_hi[3 * (size_t)j + 1] = tri.hi.y; b.leaf_hi[3 * (size_t)j + 2] = tri.hi.z;
    if (b.leaves > 1) {
      const uint32_t lo[3] = {pmd_key(tri.lo.x), pmd_key(tri.lo.y), pmd_key(tri.lo.z)}, hi[3] = {pmd_key(tri.hi.x), pmd_key(tri.hi.y), pmd_key(tri.hi.z)};
      uint32_t node = b.parent_leaf[j];
      bool climbing = true;
      for (int step = 0; step < kBvhMaxHeight && node < b.leaves - 1; ++step) {
        ++depth;
        if (climbing) {
          bool changed = false;
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            changed |= atomicMin(&b.box_min[3 * (size_t)node + a], lo[a]) > lo[a];
            changed |= atomicMax(&b.box_max[3 * (size_t)node + a], hi[a]) < hi[a];
          }
          climbing = changed;
        }
        if (!climbing && !kHeight) break;
        node = b.parent_internal[node];   // kBvhNoNode above the root ends the loop
      }
    }
  }
  if (kHeight) {
    depth = wave_max_u32(depth);
    if ((threadIdx.x & 63u) == 0 && depth) atomicMax(&words[kBvhHeight], depth);
  }
}

// The traversal layout, one thread per internal node: both children's boxes and references in 64 bytes, so that one fetch decides
// both children.  quad 0 = lo0.xyz, hi0.x   quad 1 = hi0.yz, lo1.xy   quad 2 = lo1.z, hi1.xyz   quad 3 = bits of the two references, 0, 0.
__global__ __launch_bounds__(256) void bvh_pack_kernel(BvhBuild b) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i + 1 >= b.leaves) return;
  f3 lo[2], hi[2];
  uint32_t ref[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    ref[c] = b.children[2 * (size_t)i + c];
    const bool is_leaf = (ref[c] & kBvhLeafBit) != 0;
    const size_t at = 3 * (size_t)min(ref[c] & ~kBvhLeafBit, is_leaf ? b.leaves - 1 : b.leaves - 2);   // the min changes nothing: no reference leaves the arrays
    if (is_leaf) {
      lo[c] = mk3(b.leaf_lo[at], b.leaf_lo[at + 1], b.leaf_lo[at + 2]);
      hi[c] = mk3(b.leaf_hi[at], b.leaf_hi[at + 1], b.leaf_hi[at + 2]);
    } else {
      lo[c] = mk3(bvh_unkey(b.box_min[at]), bvh_unkey(b.box_min[at + 1]), bvh_unkey(b.box_min[at + 2]));
      hi[c] = mk3(bvh_unkey(b.box_max[at]), bvh_unkey(b.box_max[at + 1]), bvh_unkey(b.box_max[at + 2]));
    }
  }
  float4* node = b.nodes + kBvhNodeQuads * (size_t)i;
  node[0] = make_float4(lo[0].x, lo[0].y, lo[0].z, hi[0].x);
  node[1] = make_float4(hi[0].y, hi[0].z, lo[1].x, lo[1].y);
  node[2] = make_float4(lo[1].z, hi[1].x, hi[1].y, hi[1].z);
  node[3] = make_float4(__uint_as_float(ref[0]), __uint_as_float(ref[1]), 0.f, 0.f);
}

// b2 of the rule: the squared distance from p to a box, all finite.  A difference may overflow to +inf, never to a NaN.
__device__ __forceinline__ float bvh_box_d2(f3 p, f3 lo, f3 hi) {
  const float ex = fmaxf(fmaxf(lo.x - p.x, p.x - hi.x), 0.f), ey = fmaxf(fmaxf(lo.y - p.y, p.y - hi.y), 0.f), ez = fmaxf(fmaxf(lo.z - p.z, p.z - hi.z), 0.f);
  return __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex));
}

// d2(p, t) of the rule: the pair value of "Surface evaluation" -- the expressions of pmd_records_kernel and pmd_query_kernel, formed
// here per pair -- clamped from below by b2 of the triangle's own box.
__device__ __forceinline__ float bvh_pair_d2(f3 p, f3 a, f3 b, f3 c) {
  const f3 eab = sub3(b, a), ebc = sub3(c, b), eca = sub3(a, c);
  const f3 wa = sub3(p, a), wb = sub3(p, b), wc = sub3(p, c);
  float d2 = __uint_as_float(0x7f800000u);
  const float s0 = pmd_segment(wa, make_float4(eab.x, eab.y, eab.z, dot(eab, eab)));
  const float s1 = pmd_segment(wb, make_float4(ebc.x, ebc.y, ebc.z, dot(ebc, ebc)));
  const float s2 = pmd_segment(wc, make_float4(eca.x, eca.y, eca.z, dot(eca, eca)));
  if (s0 < d2) d2 = s0;   // a NaN is no value
  if (s1 < d2) d2 = s1;
  if (s2 < d2) d2 = s2;
  const f3 n = cross(eab, sub3(c, a));
  const float nn = dot(n, n);
  if (nn > 0.f && dot(cross(eab, wa), n) >= 0.f && dot(cross(ebc, wb), n) >= 0.f && dot(cross(eca, wc), n) >= 0.f) {
    const float d = dot(wa, n) / sqrtf(nn);
    const float f = d * d;
    if (f < d2) d2 = f;
  }
  const f3 lo = mk3(fminf(fminf(a.x, b.x), c.x), fminf(fminf(a.y, b.y), c.y), fminf(fminf(a.z, b.z), c.z));
  const f3 hi = mk3(fmaxf(fmaxf(a.x, b.x), c.x), fmaxf(fmaxf(a.y, b.y), c.y), fmaxf(fmaxf(a.z, b.z), c.z));
  return fmaxf(d2, bvh_box_d2(p, lo, hi));   // neither is a NaN
}

struct BvhQuery {
  uint32_t points;
  uint32_t leaves;               // >= 1
  const float* xyz;
  const float4* nodes;
  const float4* records;
  float r_squared;               // fl(R * R), formed on the host; +inf without a radius
  float* out_distance;
  uint32_t* out_triangle;        // may be null
};

// The query, one point per lane.  (best, triangle) and the current node stay in registers; the deferred siblings go to a stack in
// LDS laid out [depth][lane], so that the lanes of a wave, whatever their depths, push and pop in distinct banks.  A node is one
// 64-byte fetch that decides both children: a leaf child that passes the test is evaluated at once (leaves are never pushed), an
// internal child that passes is entered, the nearer first, and the farther is pushed.  A popped node was tested when it was pushed,
// against a bound that can only have shrunk since; its children are tested against the current one.  A subtree is skipped iff
// b2 > min(best, r_squared) -- entered on equality, where a lower index may tie.  The stack holds at most one entry per level of
// the path, kBvhMaxHeight <= kBvhStack.  Each lane writes its own point once.  kStats: {nodes fetched, triangles evaluated}.
template <bool kStats>
__global__ __launch_bounds__(kBvhQueryBlock) void bvh_query_kernel(BvhQuery q, unsigned long long* __restrict__ stats) {
  __shared__ uint32_t stack[kBvhStack][kBvhQueryBlock];
  const int lane = (int)threadIdx.x;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < q.points;
  f3 p = mk3(0.f, 0.f, 0.f);
  if (live) p = mk3(q.xyz[3 * (size_t)i], q.xyz[3 * (size_t)i + 1], q.xyz[3 * (size_t)i + 2]);
  float best = __uint_as_float(0x7f800000u);
  uint32_t best_triangle = kPmdNoTriangle;
  uint32_t fetched = 0, evaluated = 0;
  auto leaf = [&](uint32_t j) {
    if (j >= q.leaves) return;   // never
    const float4 q0 = q.records[kBvhLeafQuads * (size_t)j], q1 = q.records[kBvhLeafQuads * (size_t)j + 1], q2 = q.records[kBvhLeafQuads * (size_t)j + 2];
    const float d2 = bvh_pair_d2(p, mk3(q0.x, q0.y, q0.z), mk3(q1.x, q1.y, q1.z), mk3(q2.x, q2.y, q2.z));
    const uint32_t t = __float_as_uint(q0.w);
    if (d2 < best || (d2 == best && t < best_triangle)) { best = d2; best_triangle = t; }
    if (kStats) ++evaluated;
  };
  if (live && pmd_finite(p.x) && pmd_finite(p.y) && pmd_finite(p.z)) {
    if (q.leaves == 1) {
      leaf(0);
    } else {
      uint32_t node = 0;
      int depth = 0;
      for (uint32_t pass = 1; pass < q.leaves; ++pass) {   // every pass fetches a node not fetched before on this lane: at most leaves - 1 passes
        if (node >= q.leaves - 1) break;   // never: no reference leaves the arrays
        const float4* nq = q.nodes + kBvhNodeQuads * (size_t)node;
        const float4 n0 = nq[0], n1 = nq[1], n2 = nq[2], n3 = nq[3];
        if (kStats) ++fetched;
        const float b0 = bvh_box_d2(p, mk3(n0.x, n0.y, n0.z), mk3(n0.w, n1.x, n1.y)), b1 = bvh_box_d2(p, mk3(n1.z, n1.w, n2.x), mk3(n2.y, n2.z, n2.w));
        const uint32_t r0 = __float_as_uint(n3.x), r1 = __float_as_uint(n3.y);
        const bool swap = b1 < b0;   // the nearer child first
        const float bn = swap ? b1 : b0, bf = swap ? b0 : b1;
        const uint32_t rn = swap ? r1 : r0, rf = swap ? r0 : r1;
        if ((rn & kBvhLeafBit) && !(bn > fminf(best, q.r_squared))) leaf(rn & ~kBvhLeafBit);
        if ((rf & kBvhLeafBit) && !(bf > fminf(best, q.r_squared))) leaf(rf & ~kBvhLeafBit);
        const float bound = fminf(best, q.r_squared);
        const bool enter_near = !(rn & kBvhLeafBit) && !(bn > bound), enter_far = !(rf & kBvhLeafBit) && !(bf > bound);
        if (enter_near) {
          node = rn;
          if (enter_far && depth < kBvhStack) stack[depth++][lane] = rf;   // always depth < kBvhStack: one entry per level of the path
        } else if (enter_far) {
          node = rf;
        } else {
          if (depth == 0) break;
          node = stack[--depth][lane];
        }
      }
    }
  }
  if (live) {
    const bool hit = pmd_finite(best) && best <= q.r_squared;
    q.out_distance[i] = hit ? sqrtf(best) : __uint_as_float(0x7f800000u);
    if (q.out_triangle != nullptr) q.out_triangle[i] = hit ? best_triangle : kPmdNoTriangle;
  }
  if (kStats) {
    unsigned long long a = fetched, b = evaluated;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
    if (lane == 0 && (a | b)) { atomicAdd(&stats[0], a); atomicAdd(&stats[1], b); }
  }
}

}  // namespace bslam
