// distance_kernels.hpp -- the distance from each of N points to the nearest triangle of an indexed mesh, bounded by a search
// radius, for gfx950: a uniform grid of triangle lists, the points counting-sorted by cell, and a query in which the lanes of a
// wave walk one list together.  The reference has neither a mesh nor a way to measure one.
//
// The rule (include/badslam_hip.h "Surface evaluation", DESIGN.md 8 "Surface evaluation") is fp32 in one fixed expression order
// with explicit fused multiply-adds; the minimum over the candidates and the lowest-index tie do not depend on the order in which
// the candidates are met, so a brute-force restatement over all N x T pairs reproduces every bit.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_math.hpp"
#include "mesh_kernels.hpp"

namespace bslam {

// Words of the small device block of a call (u32 units).
constexpr int kPmdError = 0;       // kMeshBadIndex
constexpr int kPmdValid = 1;       // triangles with nine finite coordinates
constexpr int kPmdMinKey = 2;      // [3]: order-preserving keys of min(lo.a - R)
constexpr int kPmdMaxKey = 5;      // [3]: ... of max(hi.a + R)
constexpr int kPmdEntries = 8;     // u64 (8 byte aligned): (triangle, cell) entries
constexpr int kPmdWords = 16;

constexpr uint32_t kPmdNoTriangle = 0xffffffffu;
constexpr int kPmdTile = 64;          // records a wave stages at a time
constexpr int kPmdRecordQuads = 9;    // float4 per record

// The uniform grid: cell of coordinate x on axis a = floorf((x - origin[a]) * inv_cell), monotone non-decreasing in x under
// fp32 rounding (a subtraction of a constant, a multiplication by a positive constant and floorf each are).
struct PmdGrid {
  float origin[3];
  float inv_cell;
  int dim[3];
  uint32_t cells;
};

// One triangle as the query reads it, 9 float4: functions of the triangle alone, computed once.
//   q0 = a.xyz, lo.x - R     q1 = b.xyz, lo.y - R     q2 = c.xyz, lo.z - R
//   q3 = hi.xyz + R, bits of the triangle id (kPmdNoTriangle: not valid, in no cell)
//   q4 = e_ab, ee_ab         q5 = e_bc, ee_bc         q6 = e_ca, ee_ca       (e_xy = y - x, ee = dot(e, e))
//   q7 = n = cross(b - a, c - a), nn = dot(n, n)      q8 = sqrtf(nn), 0, 0, 0
struct PmdTriangle {
  bool valid;
  f3 a, b, c, lo, hi;   // lo, hi: the dilated box [lo - R, hi + R] as computed
};

__device__ __forceinline__ uint32_t pmd_key(float f) {   // unsigned order == float order (finite and infinite values)
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float pmd_cell(float x, float origin, float inv_cell) { return floorf((x - origin) * inv_cell); }

// Vertices and dilated box of triangle t.  *bad is set for an index >= V, which is never dereferenced.
__device__ __forceinline__ PmdTriangle pmd_load_triangle(uint32_t t, uint32_t vertices, const float* __restrict__ positions, const uint32_t* __restrict__ indices,
                                                         float R, bool* bad) {
  PmdTriangle r;
  r.valid = false;
  const uint32_t i0 = indices[3 * (size_t)t], i1 = indices[3 * (size_t)t + 1], i2 = indices[3 * (size_t)t + 2];
  if (i0 >= vertices || i1 >= vertices || i2 >= vertices) { *bad = true; return r; }
  r.a = mk3(positions[3 * (size_t)i0], positions[3 * (size_t)i0 + 1], positions[3 * (size_t)i0 + 2]);
  r.b = mk3(positions[3 * (size_t)i1], positions[3 * (size_t)i1 + 1], positions[3 * (size_t)i1 + 2]);
  r.c = mk3(positions[3 * (size_t)i2], positions[3 * (size_t)i2 + 1], positions[3 * (size_t)i2 + 2]);
  r.valid = pmd_finite(r.a.x) && pmd_finite(r.a.y) && pmd_finite(r.a.z) && pmd_finite(r.b.x) && pmd_finite(r.b.y) && pmd_finite(r.b.z) &&
            pmd_finite(r.c.x) && pmd_finite(r.c.y) && pmd_finite(r.c.z);
  if (!r.valid) return r;
  r.lo = mk3(fminf(fminf(r.a.x, r.b.x), r.c.x) - R, fminf(fminf(r.a.y, r.b.y), r.c.y) - R, fminf(fminf(r.a.z, r.b.z), r.c.z) - R);
  r.hi = mk3(fmaxf(fmaxf(r.a.x, r.b.x), r.c.x) + R, fmaxf(fmaxf(r.a.y, r.b.y), r.c.y) + R, fmaxf(fmaxf(r.a.z, r.b.z), r.c.z) + R);
  return r;
}

// Cell range of a dilated box, clamped to the grid (by monotonicity it lies inside already).
struct PmdRange { int x0, x1, y0, y1, z0, z1; };
__device__ __forceinline__ int pmd_clamp_cell(float c, int dim) { return (int)__builtin_amdgcn_fmed3f(c, 0.f, (float)(dim - 1)); }
__device__ __forceinline__ PmdRange pmd_range(const PmdGrid& g, f3 lo, f3 hi) {
  PmdRange r;
  r.x0 = pmd_clamp_cell(pmd_cell(lo.x, g.origin[0], g.inv_cell), g.dim[0]); r.x1 = pmd_clamp_cell(pmd_cell(hi.x, g.origin[0], g.inv_cell), g.dim[0]);
  r.y0 = pmd_clamp_cell(pmd_cell(lo.y, g.origin[1], g.inv_cell), g.dim[1]); r.y1 = pmd_clamp_cell(pmd_cell(hi.y, g.origin[1], g.inv_cell), g.dim[1]);
  r.z0 = pmd_clamp_cell(pmd_cell(lo.z, g.origin[2], g.inv_cell), g.dim[2]); r.z1 = pmd_clamp_cell(pmd_cell(hi.z, g.origin[2], g.inv_cell), g.dim[2]);
  return r;
}
__device__ __forceinline__ uint32_t pmd_cell_index(const PmdGrid& g, int x, int y, int z) { return ((uint32_t)z * (uint32_t)g.dim[1] + (uint32_t)y) * (uint32_t)g.dim[0] + (uint32_t)x; }

// Triangle pass 1: validity, the index check and the bounds reduction, by integer atomics on order-preserving keys.
__global__ __launch_bounds__(256) void pmd_bounds_kernel(uint32_t vertices, uint32_t triangles, const float* __restrict__ positions, const uint32_t* __restrict__ indices,
                                                         float R, uint32_t* __restrict__ words) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= triangles) return;
  bool bad = false;
  const PmdTriangle tri = pmd_load_triangle(t, vertices, positions, indices, R, &bad);
  if (bad) atomicOr(&words[kPmdError], kMeshBadIndex);
  if (!tri.valid) return;
  atomicAdd(&words[kPmdValid], 1u);
  atomicMin(&words[kPmdMinKey], pmd_key(tri.lo.x)); atomicMin(&words[kPmdMinKey + 1], pmd_key(tri.lo.y)); atomicMin(&words[kPmdMinKey + 2], pmd_key(tri.lo.z));
  atomicMax(&words[kPmdMaxKey], pmd_key(tri.hi.x)); atomicMax(&words[kPmdMaxKey + 1], pmd_key(tri.hi.y)); atomicMax(&words[kPmdMaxKey + 2], pmd_key(tri.hi.z));
}

// Triangle pass 2, the count pass: the number of (triangle, cell) entries, so that the budget is decided before a list is built.
__global__ __launch_bounds__(256) void pmd_entries_kernel(PmdGrid g, uint32_t vertices, uint32_t triangles, const float* __restrict__ positions,
                                                          const uint32_t* __restrict__ indices, float R, uint32_t* __restrict__ words) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long n = 0;
  if (t < triangles) {
    bool bad = false;
    const PmdTriangle tri = pmd_load_triangle(t, vertices, positions, indices, R, &bad);
    if (tri.valid) {
      const PmdRange r = pmd_range(g, tri.lo, tri.hi);
      n = (unsigned long long)(r.x1 - r.x0 + 1) * (unsigned long long)(r.y1 - r.y0 + 1) * (unsigned long long)(r.z1 - r.z0 + 1);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
  if ((threadIdx.x & 63u) == 0 && n) atomicAdd((unsigned long long*)(words + kPmdEntries), n);
}

// The per-triangle records, and the per-cell counts of the lists.
__global__ __launch_bounds__(256) void pmd_records_kernel(PmdGrid g, uint32_t vertices, uint32_t triangles, const float* __restrict__ positions,
                                                          const uint32_t* __restrict__ indices, float R, float4* __restrict__ records, uint32_t* __restrict__ cell_count) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= triangles) return;
  bool bad = false;
  const PmdTriangle tri = pmd_load_triangle(t, vertices, positions, indices, R, &bad);
  float4* rec = records + (size_t)kPmdRecordQuads * t;
  if (!tri.valid) {
    rec[3] = make_float4(0.f, 0.f, 0.f, __uint_as_float(kPmdNoTriangle));
    return;
  }
  const f3 eab = sub3(tri.b, tri.a), ebc = sub3(tri.c, tri.b), eca = sub3(tri.a, tri.c);
  const f3 n = cross(eab, sub3(tri.c, tri.a));
  const float nn = dot(n, n);
  rec[0] = make_float4(tri.a.x, tri.a.y, tri.a.z, tri.lo.x);
  rec[1] = make_float4(tri.b.x, tri.b.y, tri.b.z, tri.lo.y);
  rec[2] = make_float4(tri.c.x, tri.c.y, tri.c.z, tri.lo.z);
  rec[3] = make_float4(tri.hi.x, tri.hi.y, tri.hi.z, __uint_as_float(t));
  rec[4] = make_float4(eab.x, eab.y, eab.z, dot(eab, eab));
  rec[5] = make_float4(ebc.x, ebc.y, ebc.z, dot(ebc, ebc));
  rec[6] = make_float4(eca.x, eca.y, eca.z, dot(eca, eca));
  rec[7] = make_float4(n.x, n.y, n.z, nn);
  rec[8] = make_float4(sqrtf(nn), 0.f, 0.f, 0.f);
  const PmdRange r = pmd_range(g, tri.lo, tri.hi);
  for (int z = r.z0; z <= r.z1; ++z)
    for (int y = r.y0; y <= r.y1; ++y)
      for (int x = r.x0; x <= r.x1; ++x) atomicAdd(&cell_count[pmd_cell_index(g, x, y, z)], 1u);
}

// The fill: cell_count still holds the counts and serves as per-cell cursors counting down to 0, so that it can be used again
// for the points.  The order inside a cell depends on the schedule and cannot matter.
__global__ __launch_bounds__(256) void pmd_fill_kernel(PmdGrid g, uint32_t triangles, const float4* __restrict__ records, const uint32_t* __restrict__ cell_start,
                                                       uint32_t* __restrict__ cell_count, uint32_t entries, uint32_t* __restrict__ list) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= triangles) return;
  const float4* rec = records + (size_t)kPmdRecordQuads * t;
  const float4 q3 = rec[3];
  if (__float_as_uint(q3.w) == kPmdNoTriangle) return;
  const PmdRange r = pmd_range(g, mk3(rec[0].w, rec[1].w, rec[2].w), mk3(q3.x, q3.y, q3.z));
  for (int z = r.z0; z <= r.z1; ++z)
    for (int y = r.y0; y <= r.y1; ++y)
      for (int x = r.x0; x <= r.x1; ++x) {
        const uint32_t cell = pmd_cell_index(g, x, y, z);
        const uint32_t slot = cell_start[cell] + atomicSub(&cell_count[cell], 1u) - 1u;
        if (slot < entries) list[slot] = t;
      }
}

// Every point a miss (no valid triangle at all).
__global__ __launch_bounds__(256) void pmd_miss_kernel(uint32_t points, float* __restrict__ out_distance, uint32_t* __restrict__ out_triangle) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= points) return;
  out_distance[i] = __uint_as_float(0x7f800000u);
  if (out_triangle != nullptr) out_triangle[i] = kPmdNoTriangle;
}

// A rigid transform of the points, applied on the fly (bslam_registration_step): row-major 3 x 4.
struct PmdTransform { float m[12]; };

// Point i as the query sees it: the caller's point, or (kTransform) M applied to it,
//   p'.a = fmaf(M[a][2], p.z, fmaf(M[a][1], p.y, fmaf(M[a][0], p.x, M[a][3]))),
// the one expression every kernel that needs p' repeats, so that each of them holds the same bits.
template <bool kTransform>
__device__ __forceinline__ f3 pmd_point(const float* __restrict__ xyz, const PmdTransform& M, uint32_t i) {
  const f3 p = mk3(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
  if (!kTransform) return p;
  return mk3(__builtin_fmaf(M.m[2], p.z, __builtin_fmaf(M.m[1], p.y, __builtin_fmaf(M.m[0], p.x, M.m[3]))),
             __builtin_fmaf(M.m[6], p.z, __builtin_fmaf(M.m[5], p.y, __builtin_fmaf(M.m[4], p.x, M.m[7]))),
             __builtin_fmaf(M.m[10], p.z, __builtin_fmaf(M.m[9], p.y, __builtin_fmaf(M.m[8], p.x, M.m[11]))));
}

// The cell of every point.  A point outside the grid (a NaN fails every comparison) or in a cell without triangles is written as
// a miss here and is not sorted; the others are counted per cell.
template <bool kTransform>
__global__ __launch_bounds__(256) void pmd_point_cells_kernel(PmdGrid g, uint32_t points, const float* __restrict__ xyz, PmdTransform M,
                                                              const uint32_t* __restrict__ cell_start, uint32_t* __restrict__ cell_count,
                                                              uint32_t* __restrict__ point_cell, float* __restrict__ out_distance, uint32_t* __restrict__ out_triangle) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= points) return;
  const f3 p = pmd_point<kTransform>(xyz, M, i);
  const float cx = pmd_cell(p.x, g.origin[0], g.inv_cell), cy = pmd_cell(p.y, g.origin[1], g.inv_cell), cz = pmd_cell(p.z, g.origin[2], g.inv_cell);
  uint32_t cell = kPmdNoTriangle;
  if (cx >= 0.f && cx < (float)g.dim[0] && cy >= 0.f && cy < (float)g.dim[1] && cz >= 0.f && cz < (float)g.dim[2]) {
    cell = pmd_cell_index(g, (int)cx, (int)cy, (int)cz);
    if (cell_start[cell + 1] == cell_start[cell]) cell = kPmdNoTriangle;
  }
  point_cell[i] = cell;
  if (cell == kPmdNoTriangle) {
    out_distance[i] = __uint_as_float(0x7f800000u);
    if (out_triangle != nullptr) out_triangle[i] = kPmdNoTriangle;
    return;
  }
  atomicAdd(&cell_count[cell], 1u);
}

// Counting sort of the points by cell: sorted[point_start[cell] ...] = the points of the cell, in any order.
__global__ __launch_bounds__(256) void pmd_point_fill_kernel(uint32_t points, const uint32_t* __restrict__ point_cell, const uint32_t* __restrict__ point_start,
                                                             uint32_t* __restrict__ cell_count, uint32_t* __restrict__ sorted) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= points) return;
  const uint32_t cell = point_cell[i];
  if (cell == kPmdNoTriangle) return;
  const uint32_t slot = point_start[cell] + atomicSub(&cell_count[cell], 1u) - 1u;
  if (slot < points) sorted[slot] = i;
}

// seg(p, a, b) of the rule from w = p - a and the record's e = b - a, ee = dot(e, e).
// The q of the rule is the offset from the segment's nearest point to p.
__device__ __forceinline__ f3 pmd_segment_offset(f3 w, float4 e) {
  const f3 ev = mk3(e.x, e.y, e.z);
  const float we = dot(w, ev);
  float t = e.w > 0.f ? we / e.w : 0.f;
  t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
  return mk3(__builtin_fmaf(-t, ev.x, w.x), __builtin_fmaf(-t, ev.y, w.y), __builtin_fmaf(-t, ev.z, w.z));
}
__device__ __forceinline__ float pmd_segment(f3 w, float4 e) {
  const f3 q = pmd_segment_offset(w, e);
  return dot(q, q);
}

struct PmdQuery {
  uint32_t cells;
  const float* points;
  const uint32_t* point_cell;
  const uint32_t* point_start;   // [cells + 1]: the last entry is the number of sorted points
  const uint32_t* sorted;
  const uint32_t* cell_start;    // [cells + 1]
  const uint32_t* list;
  const float4* records;
  float r_squared;               // fl(R * R), formed on the host: of the call's R, which may be below the radius of the boxes
  PmdTransform transform;        // read by the kTransform variant only
  float* out_distance;
  uint32_t* out_triangle;        // may be null
};

// The query, one sorted point per lane.  Sorted points are grouped by cell, so a wave holds the points of one cell or of a few
// neighbouring short ones; it takes its cells one after the other (wave-uniform), stages the cell's list through its quarter of
// the block's LDS in tiles of kPmdTile records (one coalesced gather of 144 bytes per record), and every lane of that cell
// then reads the same record address -- a broadcast -- and runs box test -> three segments -> face against its own point.  The
// four waves of a block share nothing but the barriers, which keep the stage and the walk of a tile apart; a wave that has
// finished goes on attending them until the block's last wave has.  (best, triangle) stay in registers, every lane writes its own
// point once, at the point's original index.  No atomics but the profiling counters' (kStats: {pairs offered, pairs that passed
// the box test} of bslam_debug_cull_stats).  kTransform: the point is M applied to the caller's (bslam_registration_step).
template <bool kStats, bool kTransform>
__global__ __launch_bounds__(256) void pmd_query_kernel(PmdQuery q, unsigned long long* __restrict__ stats) {
  __shared__ float4 tiles[4][kPmdTile * kPmdRecordQuads];
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  float4* tile = tiles[wave];
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = slot < q.point_start[q.cells];
  uint32_t index = 0, my_cell = kPmdNoTriangle;
  f3 p = mk3(0.f, 0.f, 0.f);
  if (live) {
    index = q.sorted[slot];
    my_cell = q.point_cell[index];
    p = pmd_point<kTransform>(q.points, q.transform, index);
  }
  float best = __uint_as_float(0x7f800000u);
  uint32_t best_triangle = kPmdNoTriangle;
  uint32_t offered = 0, evaluated = 0;
  bool pending = live;
  uint32_t cur = kPmdNoTriangle, pos = 0, end = 0;   // wave-uniform: the cell being walked and what is left of its list
  for (;;) {
    if (pos >= end) {   // next cell of this wave
      const unsigned long long todo = __ballot(pending);
      if (todo != 0) {
        cur = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)my_cell, __builtin_ctzll(todo), 64));
        pos = q.cell_start[cur];
        end = q.cell_start[cur + 1];
        if (my_cell == cur) pending = false;
      } else {
        cur = kPmdNoTriangle;
      }
    }
    const bool busy = pos < end;
    if (!__syncthreads_or(busy ? 1 : 0)) break;   // also: the walk of the previous tile is over in every wave
    const int count = busy ? (int)min(end - pos, (uint32_t)kPmdTile) : 0;
    if (busy) {
      const uint32_t id = lane < count ? q.list[pos + lane] : 0u;
      for (int base = 0; base < count * kPmdRecordQuads; base += 64) {   // wave-uniform trip count: every source lane of the shuffle is active
        const int k = base + lane;
        const int r = min(k / kPmdRecordQuads, count - 1);
        const uint32_t t = (uint32_t)__shfl((int)id, r, 64);
        if (k < count * kPmdRecordQuads) tile[k] = q.records[(size_t)kPmdRecordQuads * t + (uint32_t)(k - r * kPmdRecordQuads)];
      }
    }
    __syncthreads();
    if (busy && live && my_cell == cur) {
      for (int r = 0; r < count; ++r) {
        const float4* rec = tile + r * kPmdRecordQuads;
        const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3];
        if (kStats) ++offered;
        if (!(p.x >= q0.w && p.x <= q3.x && p.y >= q1.w && p.y <= q3.y && p.z >= q2.w && p.z <= q3.z)) continue;
        if (kStats) ++evaluated;
        const f3 wa = sub3(p, mk3(q0.x, q0.y, q0.z)), wb = sub3(p, mk3(q1.x, q1.y, q1.z)), wc = sub3(p, mk3(q2.x, q2.y, q2.z));
        const float4 eab = rec[4], ebc = rec[5], eca = rec[6], nq = rec[7];
        float d2 = __uint_as_float(0x7f800000u);
        const float s0 = pmd_segment(wa, eab), s1 = pmd_segment(wb, ebc), s2 = pmd_segment(wc, eca);
        if (s0 < d2) d2 = s0;   // a NaN is no value
        if (s1 < d2) d2 = s1;
        if (s2 < d2) d2 = s2;
        const f3 n = mk3(nq.x, nq.y, nq.z);
        if (nq.w > 0.f && dot(cross(mk3(eab.x, eab.y, eab.z), wa), n) >= 0.f && dot(cross(mk3(ebc.x, ebc.y, ebc.z), wb), n) >= 0.f &&
            dot(cross(mk3(eca.x, eca.y, eca.z), wc), n) >= 0.f) {
          const float d = dot(wa, n) / rec[8].x;
          const float f = d * d;
          if (f < d2) d2 = f;
        }
        const uint32_t t = __float_as_uint(q3.w);
        if (d2 < best || (d2 == best && t < best_triangle)) { best = d2; best_triangle = t; }
      }
    }
    if (busy) pos += (uint32_t)count;
  }
  if (live) {
    const bool hit = best <= q.r_squared;
    q.out_distance[index] = hit ? sqrtf(best) : __uint_as_float(0x7f800000u);
    if (q.out_triangle != nullptr) q.out_triangle[index] = hit ? best_triangle : kPmdNoTriangle;
  }
  if (kStats) {
    unsigned long long a = offered, b = evaluated;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
    if (lane == 0 && a) { atomicAdd(&stats[0], a); atomicAdd(&stats[1], b); }
  }
}

}  // namespace bslam
