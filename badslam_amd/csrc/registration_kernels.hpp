// registration_kernels.hpp -- the normal equations of one ICP step of a point set against a prepared mesh, for gfx950
// (include/badslam_hip.h "Surface registration", DESIGN.md 8 "Surface registration").  The correspondences come from the
// kTransform variant of pmd_query_kernel (distance_kernels.hpp), which writes (distance, triangle) at each point's original
// index; the kernels here walk the points in that original order, so that no sum depends on the order the counting sort left
// the points in.  The reference has no registration of surfaces.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_math.hpp"
#include "distance_kernels.hpp"
#include "pose_kernels.hpp"

namespace bslam {

constexpr int kRegH = 0;          // [21]: upper triangle of H, row-major
constexpr int kRegB = 21;         // [6]
constexpr int kRegCost = 27;      // sum of rho, once per pair
constexpr int kRegSquares = 28;   // sum of r * r over the rows
constexpr int kRegTerms = 29;     // columns in use of a kRow-float row
static_assert(kRow == 32, "a partial row of the step is a row of pose_reduce_kernel");

// u64 counters of a step
constexpr int kRegHits = 0, kRegUsed = 1, kRegDegenerate = 2, kRegCounters = 4;

struct RegStep {
  uint32_t points;
  const float* xyz;
  PmdTransform transform;
  const float4* records;
  const uint32_t* triangle;   // per point, at its original index: the winner, or kPmdNoTriangle
  float huber_k;
  float* partials;            // [waves][kRow]
  unsigned long long* counters;
};

// row(m, r, w) of the header into the thread's sums.
__device__ __forceinline__ void reg_row(f3 p, f3 m, float r, float w, float* acc) {
  const f3 c = cross(p, m);
  const float J[6] = {m.x, m.y, m.z, c.x, c.y, c.z};
  int k = kRegH;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const float wj = w * J[i];
#pragma unroll
    for (int j = i; j < 6; ++j) acc[k++] += wj * J[j];
    acc[kRegB + i] += wj * r;
  }
  acc[kRegSquares] += r * r;
}

// Huber weight and cost of a pair whose residual has the magnitude a.
__device__ __forceinline__ float reg_huber(float a, float k, float* rho) {
  const bool inside = a <= k;
  *rho = inside ? (0.5f * a) * a : k * (a - 0.5f * k);
  return inside ? 1.f : k / a;
}

// The offset vector v of the header from the record of the winning triangle: the terms of pmd_query_kernel's pair, in its
// order, for this one pair.
__device__ __forceinline__ f3 reg_offset(f3 p, const float4* __restrict__ rec) {
  const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2];
  const f3 wa = sub3(p, mk3(q0.x, q0.y, q0.z)), wb = sub3(p, mk3(q1.x, q1.y, q1.z)), wc = sub3(p, mk3(q2.x, q2.y, q2.z));
  const float4 eab = rec[4], ebc = rec[5], eca = rec[6], nq = rec[7];
  const f3 v0 = pmd_segment_offset(wa, eab), v1 = pmd_segment_offset(wb, ebc), v2 = pmd_segment_offset(wc, eca);
  const float s0 = dot(v0, v0), s1 = dot(v1, v1), s2 = dot(v2, v2);
  float d2 = __uint_as_float(0x7f800000u);
  f3 v = mk3(0.f, 0.f, 0.f);
  if (s0 < d2) { d2 = s0; v = v0; }
  if (s1 < d2) { d2 = s1; v = v1; }
  if (s2 < d2) { d2 = s2; v = v2; }
  const f3 n = mk3(nq.x, nq.y, nq.z);
  if (nq.w > 0.f && dot(cross(mk3(eab.x, eab.y, eab.z), wa), n) >= 0.f && dot(cross(mk3(ebc.x, ebc.y, ebc.z), wb), n) >= 0.f &&
      dot(cross(mk3(eca.x, eca.y, eca.z), wc), n) >= 0.f) {
    const float root = rec[8].x;
    const float d = dot(wa, n) / root;
    if (d * d < d2) {
      const float s = d / root;
      v = mk3(s * n.x, s * n.y, s * n.z);
    }
  }
  return v;
}

// One point per lane in original index order; every wave writes one row of kRow floats: its sums of the 29 terms (a fixed
// shuffle tree), zeros behind them.  Counters: ballots and one integer atomic per wave and counter.
template <int kMode>
__global__ __launch_bounds__(256) void reg_rows_kernel(RegStep s) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t t = i < s.points ? s.triangle[i] : kPmdNoTriangle;
  const bool hit = t != kPmdNoTriangle;
  bool used = false;
  float acc[kRegTerms];
#pragma unroll
  for (int k = 0; k < kRegTerms; ++k) acc[k] = 0.f;
  if (hit) {
    const f3 p = pmd_point<true>(s.xyz, s.transform, i);
    const float4* rec = s.records + (size_t)kPmdRecordQuads * t;
    float rho;
    if (kMode == BSLAM_REGISTRATION_PLANE) {
      const float4 nq = rec[7];
      if (nq.w > 0.f) {
        const float4 q0 = rec[0];
        const float root = rec[8].x;
        const f3 n = mk3(nq.x, nq.y, nq.z);
        const float d = dot(sub3(p, mk3(q0.x, q0.y, q0.z)), n) / root;
        const float w = reg_huber(fabsf(d), s.huber_k, &rho);
        reg_row(p, mk3(n.x / root, n.y / root, n.z / root), d, w, acc);
        acc[kRegCost] += rho;
        used = true;
      }
    } else {
      const f3 v = reg_offset(p, rec);
      const float w = reg_huber(sqrtf(dot(v, v)), s.huber_k, &rho);
      reg_row(p, mk3(1.f, 0.f, 0.f), v.x, w, acc);
      reg_row(p, mk3(0.f, 1.f, 0.f), v.y, w, acc);
      reg_row(p, mk3(0.f, 0.f, 1.f), v.z, w, acc);
      acc[kRegCost] += rho;
      used = true;
    }
  }
#pragma unroll
  for (int k = 0; k < kRegTerms; ++k) acc[k] = wave_sum(acc[k]);
  const unsigned long long hits = __ballot(hit), pairs = __ballot(used);
  if ((threadIdx.x & 63u) == 0) {
    float* row = s.partials + (size_t)(i >> 6) * kRow;
#pragma unroll
    for (int k = 0; k < kRow; ++k) row[k] = k < kRegTerms ? acc[k] : 0.f;
    if (hits) {
      atomicAdd(&s.counters[kRegHits], (unsigned long long)__popcll(hits));
      if (pairs) atomicAdd(&s.counters[kRegUsed], (unsigned long long)__popcll(pairs));
      if (hits != pairs) atomicAdd(&s.counters[kRegDegenerate], (unsigned long long)__popcll(hits & ~pairs));
    }
  }
}

// Stage B behind pose_reduce_kernel: sums[col] = the kReduceParts parts in their order.
__global__ __launch_bounds__(64) void reg_reduce_final_kernel(const float* __restrict__ parts, float* __restrict__ sums) {
  const int col = threadIdx.x;
  if (col >= kRow) return;
  float total = 0.f;
  for (int p = 0; p < kReduceParts; ++p) total += parts[(size_t)p * kRow + col];
  sums[col] = total;
}

}  // namespace bslam
