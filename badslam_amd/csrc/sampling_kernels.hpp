// sampling_kernels.hpp -- points drawn uniformly by area from an indexed triangle mesh, for gfx950: a count pass with one triangle
// per lane, the scan over the counts (lifecycle_kernels.hpp), and an emit pass with one sample per lane that finds its triangle by
// searching the scanned offsets.  The reference has neither a mesh nor a way to measure one.
//
// The rule (include/badslam_hip.h "Surface sampling", DESIGN.md 8 "Surface sampling") is uint32 hashing and fp32 in one fixed
// expression order with explicit fused multiply-adds; a sample is a function of (seed, triangle, ordinal within the triangle) alone,
// so a brute-force restatement without a scan or a search reproduces every bit.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_math.hpp"
#include "distance_kernels.hpp"

namespace bslam {

// Words of the small device block of a call (u32 units).
constexpr int kSmpError = 0;       // kMeshBadIndex
constexpr int kSmpScanTotal = 1;   // the scan's 32-bit total (equals the low word of kSmpTotal once that was checked)
constexpr int kSmpTotal = 2;       // u64 (8 byte aligned): the number of samples
constexpr int kSmpWords = 4;

constexpr uint32_t kSmpStreamCount = 0, kSmpStreamFirst = 1, kSmpStreamSecond = 2;
constexpr uint32_t kSmpOne = 1u << 24;      // the fixed-point 1 of the two coordinates
constexpr float kSmpUnit = 0x1p-24f;

__host__ __device__ __forceinline__ uint32_t smp_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
// h(s, t, j) of the rule
__host__ __device__ __forceinline__ uint32_t smp_hash(uint32_t seed, uint32_t s, uint32_t t, uint32_t j) {
  return smp_mix(smp_mix((seed + s * 0x9e3779b9u) ^ smp_mix(t)) + j);
}

// What both passes need of triangle t, whose indices are known to be < V.
struct SmpTriangle {
  f3 a, u, v, n;
  float nn;
  bool valid;   // nine finite coordinates and nn > 0
};
__device__ __forceinline__ SmpTriangle smp_triangle(const float* __restrict__ positions, uint32_t i0, uint32_t i1, uint32_t i2) {
  SmpTriangle r;
  r.a = mk3(positions[3 * (size_t)i0], positions[3 * (size_t)i0 + 1], positions[3 * (size_t)i0 + 2]);
  const f3 b = mk3(positions[3 * (size_t)i1], positions[3 * (size_t)i1 + 1], positions[3 * (size_t)i1 + 2]);
  const f3 c = mk3(positions[3 * (size_t)i2], positions[3 * (size_t)i2 + 1], positions[3 * (size_t)i2 + 2]);
  const bool finite = pmd_finite(r.a.x) && pmd_finite(r.a.y) && pmd_finite(r.a.z) && pmd_finite(b.x) && pmd_finite(b.y) && pmd_finite(b.z) &&
                      pmd_finite(c.x) && pmd_finite(c.y) && pmd_finite(c.z);
  r.u = sub3(b, r.a);
  r.v = sub3(c, r.a);
  r.n = cross(r.u, r.v);
  r.nn = dot(r.n, r.n);
  r.valid = finite && r.nn > 0.f;
  return r;
}

// The count pass: the index check, the per-triangle counts (saturated to 32 bits: such a total is refused before it is used) and
// their 64-bit total, one integer atomic per wave.
__global__ __launch_bounds__(256) void sample_count_kernel(uint32_t vertices, uint32_t triangles, const float* __restrict__ positions,
                                                           const uint32_t* __restrict__ indices, float density, uint32_t seed, uint32_t* __restrict__ counts,
                                                           uint32_t* __restrict__ words) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long n = 0;
  if (t < triangles) {
    const uint32_t i0 = indices[3 * (size_t)t], i1 = indices[3 * (size_t)t + 1], i2 = indices[3 * (size_t)t + 2];
    if (i0 >= vertices || i1 >= vertices || i2 >= vertices) {
      atomicOr(&words[kSmpError], kMeshBadIndex);
    } else {
      const SmpTriangle tri = smp_triangle(positions, i0, i1, i2);
      if (tri.valid) {
        const float area = 0.5f * sqrtf(tri.nn);
        const float x = area * density;
        if (!(x < 4294967296.f)) {   // not finite, or 2^32 and more
          n = 1ull << 32;
        } else {
          const float k = floorf(x);
          const float r = (float)(smp_hash(seed, kSmpStreamCount, t, 0) >> 8) * kSmpUnit;
          n = (unsigned long long)k + (r < x - k ? 1u : 0u);
        }
      }
    }
    counts[t] = n > 0xffffffffull ? 0xffffffffu : (uint32_t)n;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
  if ((threadIdx.x & 63u) == 0 && n) atomicAdd((unsigned long long*)(words + kSmpTotal), n);
}

// The largest t in [lo, hi] with offset[t] <= i, given offset[lo] <= i; at most `steps` >= ceil(log2(hi - lo + 1)) rounds.
__device__ __forceinline__ uint32_t smp_search(const uint32_t* __restrict__ offset, uint32_t lo, uint32_t hi, uint32_t i, int steps) {
  for (int s = 0; s < steps && lo < hi; ++s) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (offset[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Sample i of triangle t.
__device__ __forceinline__ void smp_emit(uint32_t i, uint32_t t, uint32_t seed, const float* __restrict__ positions, const uint32_t* __restrict__ indices,
                                         const uint32_t* __restrict__ offset, float* __restrict__ out_points, float* __restrict__ out_normals,
                                         uint32_t* __restrict__ out_triangles) {
  const SmpTriangle tri = smp_triangle(positions, indices[3 * (size_t)t], indices[3 * (size_t)t + 1], indices[3 * (size_t)t + 2]);
  const uint32_t j = i - offset[t];
  uint32_t i1 = smp_hash(seed, kSmpStreamFirst, t, j) >> 8, i2 = smp_hash(seed, kSmpStreamSecond, t, j) >> 8;
  if (i1 + i2 > kSmpOne) { i1 = kSmpOne - i1; i2 = kSmpOne - i2; }
  const float w1 = (float)i1 * kSmpUnit, w2 = (float)i2 * kSmpUnit;
  float* p = out_points + 3 * (size_t)i;
  p[0] = __builtin_fmaf(w2, tri.v.x, __builtin_fmaf(w1, tri.u.x, tri.a.x));
  p[1] = __builtin_fmaf(w2, tri.v.y, __builtin_fmaf(w1, tri.u.y, tri.a.y));
  p[2] = __builtin_fmaf(w2, tri.v.z, __builtin_fmaf(w1, tri.u.z, tri.a.z));
  if (out_normals) {
    const float len = sqrtf(tri.nn);
    float* q = out_normals + 3 * (size_t)i;
    q[0] = tri.n.x / len; q[1] = tri.n.y / len; q[2] = tri.n.z / len;
  }
  if (out_triangles) out_triangles[i] = t;
}

// The emit pass: one sample per lane, so the load does not depend on how the area is spread over the triangles.  offset is the
// exclusive scan of the counts; sample i belongs to the largest t with offset[t] <= i (a triangle without samples shares its offset
// with its successor and is never that one).  A wave finds the triangles of its first and of its last sample with wave-uniform
// searches; where they are one triangle (a coarse mesh) no lane searches and the triangle is read through the scalar path, else
// each lane searches between the two.  The index check of the count pass has gone through: every index is < V.
__global__ __launch_bounds__(256) void sample_emit_kernel(uint32_t triangles, uint32_t samples, int steps, uint32_t seed, const float* __restrict__ positions,
                                                          const uint32_t* __restrict__ indices, const uint32_t* __restrict__ offset, float* __restrict__ out_points,
                                                          float* __restrict__ out_normals, uint32_t* __restrict__ out_triangles) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t first = __builtin_amdgcn_readfirstlane(i & ~63u);
  if (first >= samples) return;
  const uint32_t last = min(first + 63u, samples - 1u);
  const uint32_t t_first = __builtin_amdgcn_readfirstlane(smp_search(offset, 0u, triangles - 1u, first, steps));
  const uint32_t t_last = __builtin_amdgcn_readfirstlane(smp_search(offset, t_first, triangles - 1u, last, steps));
  if (t_first == t_last) {
    if (i < samples) smp_emit(i, t_first, seed, positions, indices, offset, out_points, out_normals, out_triangles);
  } else if (i < samples) {
    smp_emit(i, smp_search(offset, t_first, t_last, i, steps), seed, positions, indices, offset, out_points, out_normals, out_triangles);
  }
}

}  // namespace bslam
