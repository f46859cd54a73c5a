// ray_kernels.hpp -- rays against an indexed mesh, for gfx950: closest hit, any hit, and the visibility of points from views, over
// the tree of bvh_kernels.hpp (its packed 64-byte nodes and leaf records, unchanged).  The reference has neither a mesh nor a ray.
//
// The rule (include/badslam_hip.h "Mesh rays", DESIGN.md 8 "Mesh rays"): a watertight triangle test in the per-ray sheared frame
// (Woop, Benthin, Wald, "Watertight Ray/Triangle Intersection", JCGT 2013), and a slab function of the triangle's own box that is
// PART of the pair's value: hit(ray, t) needs a non-empty slab, and t_hit is the triangle's t clamped into [enter, exit].  The slab
// is monotone under inclusion of boxes AS FLOATS (fp32 subtraction, multiplication by one per-ray constant, min, max and a shift by
// a fixed number of representable floats are monotone), so [enter, exit] of a node contains that of every triangle below it, and
// skipping a subtree iff its slab is empty, or enter > min(best, t_max), or exit < t_min loses no hit and no tie: the result is a
// function of the rule alone, not of the tree's shape, the key width or the traversal order.  A brute-force restatement over all
// N x T pairs reproduces every bit.
//
// No kernel here waits on another thread: every traversal makes at most leaves - 1 passes, and a lane writes its own outputs once.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bvh_kernels.hpp"

namespace bslam {

constexpr int kRayPadUlps = 4;   // BSLAM_RAY_PAD_ULPS
constexpr uint32_t kRayNoView = 0xffffffffu;

__device__ __forceinline__ float ray_inf() { return __uint_as_float(0x7f800000u); }
__device__ __forceinline__ float ray_component(f3 v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

// x moved kRayPadUlps representable floats down or up, never beyond an infinity; -0 counts as +0.  x is no NaN.
template <bool kUp>
__device__ __forceinline__ float ray_pad(float x) {
  const uint32_t u = __float_as_uint(x + 0.f);
  uint32_t key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // the order-preserving key; -inf = 0x007fffff, +inf = 0xff800000
  key = kUp ? min(key + (uint32_t)kRayPadUlps, 0xff800000u) : max(key - (uint32_t)kRayPadUlps, 0x007fffffu);
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// What a ray computes once.
struct Ray {
  f3 o, d, inv;         // inv = 1 / d per component (+-inf where d is 0)
  float t_min, t_max;
  float sx, sy, sz;     // the shear: d[kx] / d[kz], d[ky] / d[kz], 1 / d[kz]
  int kx, ky, kz;
  bool valid;
};

__device__ __forceinline__ Ray ray_setup(f3 o, f3 d, float t_min, float t_max) {
  Ray r;
  r.o = o; r.d = d; r.t_min = t_min; r.t_max = t_max;
  r.valid = pmd_finite(o.x) && pmd_finite(o.y) && pmd_finite(o.z) && pmd_finite(d.x) && pmd_finite(d.y) && pmd_finite(d.z) &&
            (d.x != 0.f || d.y != 0.f || d.z != 0.f) && t_min <= t_max;   // a NaN bound fails the comparison
  const float mx = fabsf(d.x), my = fabsf(d.y), mz = fabsf(d.z);
  r.kz = (mx >= my && mx >= mz) ? 0 : (my >= mz ? 1 : 2);
  int kx = r.kz == 2 ? 0 : r.kz + 1, ky = kx == 2 ? 0 : kx + 1;
  const float dz = ray_component(d, r.kz);
  if (dz < 0.f) { const int s = kx; kx = ky; ky = s; }
  r.kx = kx; r.ky = ky;
  r.sx = ray_component(d, kx) / dz;
  r.sy = ray_component(d, ky) / dz;
  r.sz = 1.f / dz;
  r.inv = mk3(1.f / d.x, 1.f / d.y, 1.f / d.z);
  return r;
}

// One axis of the slab.
__device__ __forceinline__ void ray_slab_axis(float o, float d, float inv, float lo, float hi, float* enter, float* leave) {
  float near, far;
  if (d == 0.f) {
    const bool inside = lo <= o && o <= hi;
    near = inside ? -ray_inf() : ray_inf();
    far = inside ? ray_inf() : -ray_inf();
  } else {
    const float t0 = (lo - o) * inv, t1 = (hi - o) * inv;
    const bool free = t0 != t0 || t1 != t1;   // 0 x inf: the axis does not constrain
    near = free ? -ray_inf() : fminf(t0, t1);
    far = free ? ray_inf() : fmaxf(t0, t1);
  }
  *enter = fmaxf(*enter, near);
  *leave = fminf(*leave, far);
}

// slab(ray, box): (enter, exit), padded outward; empty iff enter > exit.
__device__ __forceinline__ void ray_slab(const Ray& r, f3 lo, f3 hi, float* enter, float* leave) {
  float e = -ray_inf(), l = ray_inf();
  ray_slab_axis(r.o.x, r.d.x, r.inv.x, lo.x, hi.x, &e, &l);
  ray_slab_axis(r.o.y, r.d.y, r.inv.y, lo.y, hi.y, &e, &l);
  ray_slab_axis(r.o.z, r.d.z, r.inv.z, lo.z, hi.z, &e, &l);
  *enter = ray_pad<false>(e);
  *leave = ray_pad<true>(l);
}

struct RayHit {
  float t;             // +inf: none
  uint32_t triangle;
  float u, v;
  bool front;
};

// hit(ray, t) of the rule for a triangle whose slab is (enter, exit), not empty: the sheared edge functions as differences of two
// plain products (nothing is contracted, so they are antisymmetric in the edge's two vertices), all three again in float64 where
// one is exactly 0, and t, u, v by correctly rounded division.  -> whether the pair hits; *hit is then filled but for the triangle.
__device__ __forceinline__ bool ray_triangle(const Ray& r, f3 a, f3 b, f3 c, float enter, float leave, RayHit* hit) {
  const f3 ra = sub3(a, r.o), rb = sub3(b, r.o), rc = sub3(c, r.o);
  const float az = ray_component(ra, r.kz), bz = ray_component(rb, r.kz), cz = ray_component(rc, r.kz);
  const float ax = ray_component(ra, r.kx) - r.sx * az, ay = ray_component(ra, r.ky) - r.sy * az;
  const float bx = ray_component(rb, r.kx) - r.sx * bz, by = ray_component(rb, r.ky) - r.sy * bz;
  const float cx = ray_component(rc, r.kx) - r.sx * cz, cy = ray_component(rc, r.ky) - r.sy * cz;
  float U = cx * by - cy * bx, V = ax * cy - ay * cx, W = bx * ay - by * ax;
  bool one_sign;
  if (U == 0.f || V == 0.f || W == 0.f) {
    const double u64 = (double)cx * (double)by - (double)cy * (double)bx;
    const double v64 = (double)ax * (double)cy - (double)ay * (double)cx;
    const double w64 = (double)bx * (double)ay - (double)by * (double)ax;
    one_sign = !((u64 < 0.0 || v64 < 0.0 || w64 < 0.0) && (u64 > 0.0 || v64 > 0.0 || w64 > 0.0));
    U = (float)u64; V = (float)v64; W = (float)w64;
  } else {
    one_sign = !((U < 0.f || V < 0.f || W < 0.f) && (U > 0.f || V > 0.f || W > 0.f));
  }
  const float det = (U + V) + W;
  if (!one_sign || det == 0.f) return false;
  const float T = (U * (r.sz * az) + V * (r.sz * bz)) + W * (r.sz * cz);
  const float t = T / det;
  if (t != t) return false;
  const float t_hit = fminf(fmaxf(t, enter), leave);
  if (!(t_hit >= r.t_min && t_hit <= r.t_max) || !pmd_finite(t_hit)) return false;
  hit->t = t_hit;
  hit->u = V / det;
  hit->v = W / det;
  hit->front = det > 0.f;
  return true;
}

// The tree as a traversal reads it.
struct RayTree {
  uint32_t leaves;          // 0: no valid triangle, every ray misses
  const float4* nodes;
  const float4* records;
};

// The traversal of one ray (valid; tree.leaves >= 1) with the shape of bvh_query_kernel: the current node in a register, the deferred
// siblings in this lane's column of the [depth][lane] LDS stack, one 64-byte fetch per node that decides both children.  A leaf child
// whose slab passes is evaluated at once with that slab -- the node holds the triangle's own box -- and an internal child that passes
// is entered, the nearer enter first, the other pushed.  kAny: stops at the first hit and leaves best->triangle alone.  Every pass
// fetches a node not fetched before on this lane: at most leaves - 1 passes, and at most one stack entry per level of the path.
template <bool kAny, bool kStats>
__device__ __forceinline__ void ray_traverse(const Ray& r, const RayTree& tree, uint32_t (*stack)[kBvhQueryBlock], int lane, RayHit* best, uint32_t* fetched,
                                             uint32_t* evaluated) {
  auto leaf = [&](uint32_t j, float enter, float leave) {
    if (j >= tree.leaves) return;   // never
    const float4 q0 = tree.records[kBvhLeafQuads * (size_t)j], q1 = tree.records[kBvhLeafQuads * (size_t)j + 1], q2 = tree.records[kBvhLeafQuads * (size_t)j + 2];
    if (kStats) ++*evaluated;
    RayHit h;
    if (!ray_triangle(r, mk3(q0.x, q0.y, q0.z), mk3(q1.x, q1.y, q1.z), mk3(q2.x, q2.y, q2.z), enter, leave, &h)) return;
    h.triangle = __float_as_uint(q0.w);
    if (h.t < best->t || (h.t == best->t && h.triangle < best->triangle)) *best = h;
  };
  // skipped iff the slab is empty, or enter > min(best, t_max), or exit < t_min; entered on equality
  auto passes = [&](float enter, float leave) { return !(enter > leave) && !(enter > fminf(best->t, r.t_max)) && !(leave < r.t_min); };
  if (tree.leaves == 1) {
    const float4 q0 = tree.records[0], q1 = tree.records[1], q2 = tree.records[2];
    const f3 a = mk3(q0.x, q0.y, q0.z), b = mk3(q1.x, q1.y, q1.z), c = mk3(q2.x, q2.y, q2.z);
    float enter, leave;
    ray_slab(r, mk3(fminf(fminf(a.x, b.x), c.x), fminf(fminf(a.y, b.y), c.y), fminf(fminf(a.z, b.z), c.z)),
             mk3(fmaxf(fmaxf(a.x, b.x), c.x), fmaxf(fmaxf(a.y, b.y), c.y), fmaxf(fmaxf(a.z, b.z), c.z)), &enter, &leave);
    if (passes(enter, leave)) leaf(0, enter, leave);
    return;
  }
  uint32_t node = 0;
  int depth = 0;
  for (uint32_t pass = 1; pass < tree.leaves; ++pass) {
    if (node >= tree.leaves - 1) break;   // never: no reference leaves the arrays
    const float4* nq = tree.nodes + kBvhNodeQuads * (size_t)node;
    const float4 n0 = nq[0], n1 = nq[1], n2 = nq[2], n3 = nq[3];
    if (kStats) ++*fetched;
    float e0, l0, e1, l1;
    ray_slab(r, mk3(n0.x, n0.y, n0.z), mk3(n0.w, n1.x, n1.y), &e0, &l0);
    ray_slab(r, mk3(n1.z, n1.w, n2.x), mk3(n2.y, n2.z, n2.w), &e1, &l1);
    const uint32_t r0 = __float_as_uint(n3.x), r1 = __float_as_uint(n3.y);
    const bool swap = e1 < e0;   // the nearer child first
    const float en = swap ? e1 : e0, ln = swap ? l1 : l0, ef = swap ? e0 : e1, lf = swap ? l0 : l1;
    const uint32_t rn = swap ? r1 : r0, rf = swap ? r0 : r1;
    if ((rn & kBvhLeafBit) && passes(en, ln)) leaf(rn & ~kBvhLeafBit, en, ln);
    if (kAny && pmd_finite(best->t)) return;
    if ((rf & kBvhLeafBit) && passes(ef, lf)) leaf(rf & ~kBvhLeafBit, ef, lf);
    if (kAny && pmd_finite(best->t)) return;
    const bool enter_near = !(rn & kBvhLeafBit) && passes(en, ln), enter_far = !(rf & kBvhLeafBit) && passes(ef, lf);
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

__device__ __forceinline__ RayHit ray_miss() {
  RayHit h;
  h.t = ray_inf(); h.triangle = kPmdNoTriangle; h.u = 0.f; h.v = 0.f; h.front = false;
  return h;
}

// {nodes fetched, triangles evaluated} of a wave into the cull statistics.
__device__ __forceinline__ void ray_stats(int lane, uint32_t fetched, uint32_t evaluated, unsigned long long* __restrict__ stats) {
  unsigned long long a = fetched, b = evaluated;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
  if (lane == 0 && (a | b)) { atomicAdd(&stats[0], a); atomicAdd(&stats[1], b); }
}

struct MeshRays {
  uint32_t rays;
  RayTree tree;
  const float* origins;      // [3 N]
  const float* directions;   // [3 N]
  const float* t_range;      // [2 N], or null: [0, +inf]
  float* out_t;              // closest: [N]
  uint32_t* out_triangle;    // closest, may be null
  float* out_uv;             // closest, may be null: [2 N]
  uint8_t* out_front;        // closest, may be null
  uint8_t* out_hit;          // any: [N]
};

// One ray per lane, one wave per block.
template <bool kAny, bool kStats>
__global__ __launch_bounds__(kBvhQueryBlock) void mesh_rays_kernel(MeshRays q, unsigned long long* __restrict__ stats) {
  __shared__ uint32_t stack[kBvhStack][kBvhQueryBlock];
  const int lane = (int)threadIdx.x;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < q.rays;
  RayHit best = ray_miss();
  uint32_t fetched = 0, evaluated = 0;
  if (live) {
    const f3 o = mk3(q.origins[3 * (size_t)i], q.origins[3 * (size_t)i + 1], q.origins[3 * (size_t)i + 2]);
    const f3 d = mk3(q.directions[3 * (size_t)i], q.directions[3 * (size_t)i + 1], q.directions[3 * (size_t)i + 2]);
    const float t_min = q.t_range ? q.t_range[2 * (size_t)i] : 0.f, t_max = q.t_range ? q.t_range[2 * (size_t)i + 1] : ray_inf();
    const Ray r = ray_setup(o, d, t_min, t_max);
    if (r.valid && q.tree.leaves != 0) ray_traverse<kAny, kStats>(r, q.tree, stack, lane, &best, &fetched, &evaluated);
    if (kAny) {
      q.out_hit[i] = pmd_finite(best.t) ? 1 : 0;
    } else {
      q.out_t[i] = best.t;
      if (q.out_triangle) q.out_triangle[i] = best.triangle;
      if (q.out_uv) { q.out_uv[2 * (size_t)i] = best.u; q.out_uv[2 * (size_t)i + 1] = best.v; }
      if (q.out_front) q.out_front[i] = best.front ? 1 : 0;
    }
  }
  if (kStats) ray_stats(lane, fetched, evaluated, stats);
}

struct MeshVisibility {
  uint32_t points;
  uint32_t views;
  RayTree tree;
  const float* xyz;          // [3 N]
  const float* normals;      // [3 N], or null
  const float4* view_rows;   // [4 K]: the three rows of camera_T_global, then (centre, 0)
  float fx, fy, cx, cy, width, height;
  float min_depth, max_depth, margin;
  uint32_t* out_count;       // [N]
  uint32_t* out_first;       // [N], may be null
};

// One point per lane, looping over the views: the view's rows are the same address for the whole wave, neighbouring points send
// neighbouring segments down the tree, and count and first need no atomic -- the lane writes both once.  A point is tested against a
// view's frustum (and its normal against the segment) before any access to the tree.
template <bool kStats>
__global__ __launch_bounds__(kBvhQueryBlock) void mesh_visibility_kernel(MeshVisibility q, unsigned long long* __restrict__ stats) {
  __shared__ uint32_t stack[kBvhStack][kBvhQueryBlock];
  const int lane = (int)threadIdx.x;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < q.points;
  uint32_t fetched = 0, evaluated = 0;
  if (live) {
    const f3 p = mk3(q.xyz[3 * (size_t)i], q.xyz[3 * (size_t)i + 1], q.xyz[3 * (size_t)i + 2]);
    f3 n = mk3(0.f, 0.f, 0.f);
    if (q.normals) n = mk3(q.normals[3 * (size_t)i], q.normals[3 * (size_t)i + 1], q.normals[3 * (size_t)i + 2]);
    uint32_t count = 0, first = kRayNoView;
    for (uint32_t k = 0; k < q.views; ++k) {
      const float4 m0 = q.view_rows[4 * (size_t)k], m1 = q.view_rows[4 * (size_t)k + 1], m2 = q.view_rows[4 * (size_t)k + 2], c = q.view_rows[4 * (size_t)k + 3];
      const float lx = ((m0.x * p.x + m0.y * p.y) + m0.z * p.z) + m0.w;
      const float ly = ((m1.x * p.x + m1.y * p.y) + m1.z * p.z) + m1.w;
      const float lz = ((m2.x * p.x + m2.y * p.y) + m2.z * p.z) + m2.w;
      if (!(lz >= q.min_depth && lz <= q.max_depth)) continue;
      const float px = q.fx * (lx / lz) + q.cx, py = q.fy * (ly / lz) + q.cy;
      if (!(px >= 0.f && px < q.width && py >= 0.f && py < q.height)) continue;
      const f3 o = mk3(c.x, c.y, c.z);
      const f3 d = sub3(p, o);
      if (q.normals && !(dot(n, d) < 0.f)) continue;
      const Ray r = ray_setup(o, d, 0.f, 1.f - q.margin / sqrtf(dot(d, d)));
      RayHit best = ray_miss();
      if (r.valid && q.tree.leaves != 0) ray_traverse<true, kStats>(r, q.tree, stack, lane, &best, &fetched, &evaluated);
      if (!pmd_finite(best.t)) {
        if (count == 0) first = k;
        ++count;
      }
    }
    q.out_count[i] = count;
    if (q.out_first) q.out_first[i] = first;
  }
  if (kStats) ray_stats(lane, fetched, evaluated, stats);
}

}  // namespace bslam
