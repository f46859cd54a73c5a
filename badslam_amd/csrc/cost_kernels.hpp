// cost_kernels.hpp -- the objective of the bundle adjustment per keyframe (gfx950): the robust sum the Gauss-Newton steps are
// derived from, Tukey on the depth residuals (BS/cost_function.cuh:44-68) and kDescWeight * Huber on BOTH descriptor residuals
// (not the reference's debug quirk Q1, which counts only the first), over every (surfel, keyframe) pair that associates.
//
// The pass has the shape of pose_accumulate_kernel (pose_kernels.hpp): the same grid of (work slot) x (keyframe chunk)
// workgroups in the per-surfel Morton order, the same XCD slot mapping, the same block-level frustum culling with one visit word
// per (chunk, slot), the same association predicates (bit-exact against the oracle) and colour-bounds test.  Per pair it forms
// the residual VALUES only -- no Jacobians, no 27 H / b columns, no gradient half of the descriptor footprint -- so a thread
// carries two cost accumulators instead of 32, and a (slot, keyframe) row is 4 floats instead of 32: the two costs (wave sums
// through wave_column_sums_lds) and the two pair counts (from ballots).  ba_cost_reduce_kernel then sums each keyframe's visited
// rows in a fixed order: deterministic, no float atomics, the same bits with and without culling.  The depth term is the
// reference's Tukey function in a form without cancellation (objective_depth_term): near a converged pose, where the objective is
// read, the reference's fp32 form loses most digits of the small terms.
#pragma once

#include "pose_kernels.hpp"

namespace bslam {

constexpr int kCostCols = 4;          // per (slot, keyframe) row: depth cost, descriptor cost, depth pairs, descriptor pairs
constexpr int kCostRedCols = 4;       // columns per round of the wave reduction (two live columns: one round)
constexpr int kCostStashGroup = 8;    // keyframes per barrier: 8 rows x 4 columns = 32 storing threads

// active: the caller's per-surfel flags (only bit 0 counts), indexed by the caller's column (perm maps the sorted position to
// it), or nullptr: every surfel.  Deleted surfels (x = NaN) fail project_to_pixel and never count.
template <bool kDepth, bool kDesc, int kR>
__global__ __launch_bounds__(kPoseThreads) void ba_cost_kernel(CamConsts c_in, const KfDev* __restrict__ kfs, int kf_count, int kfs_per_block,
                                                               Schedule sc, SurfelRows s, const uint8_t* __restrict__ active,
                                                               const uint32_t* __restrict__ perm, float* __restrict__ partials, int rows_per_kf,
                                                               VisWord* __restrict__ vis) {
  CamConsts c = c_in;
  uint32_t chunk, slot;
  if (!chunk_and_slot_of_block(sc, &chunk, &slot)) return;
  const int kf_begin = (int)chunk * kfs_per_block;
  if (kf_begin >= kf_count) return;
  const int kf_end = min(kf_count, kf_begin + kfs_per_block);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  // the keyframes of the chunk this block visits, as in pose_accumulate_kernel (every keyframe is wanted, no keyframe list)
  __shared__ unsigned long long todo_shared;
  unsigned long long todo = pose_chunk_todo(c, kfs, kf_begin, kf_end, sc, slot, kR, chunk, nullptr, vis, nullptr, &todo_shared);
  if (todo == 0) return;

  // surfels of this thread, in registers: the cost path carries no accumulators to make room for
  f3 gp[kR], gn[kR];
  f3 tp1[kDesc ? kR : 1], tp2[kDesc ? kR : 1];
  float desc1[kDesc ? kR : 1], desc2[kDesc ? kR : 1];
  bool valid[kR];
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const uint32_t i = surfel_of_slot(sc, slot, r, kR);
    valid[r] = i < s.size;
    const uint32_t jj = valid[r] ? i : 0;
    if (active != nullptr && valid[r]) valid[r] = (active[perm ? perm[jj] : jj] & 1u) != 0;
    gp[r] = mk3(s.x[jj], s.y[jj], s.z[jj]);
    gn[r] = unpack_normal(s.normal[jj]);
    if constexpr (kDesc) {
      tangent_points(gp[r], gn[r], s.radius_squared[jj], &tp1[r], &tp2[r]);
      desc1[r] = s.d1[jj]; desc2[r] = s.d2[jj];
    }
  }

  __shared__ RowStash<kCostCols, kCostStashGroup, kCostRedCols> stash;
  RowStashCursor at;

  if constexpr (kDesc) BSLAM_HOIST_CAM_CENTRES(c);
  while (todo != 0) {   // uniform
    const int k = kf_begin + __builtin_ctzll(todo);
    todo &= todo - 1;
    KfDev kf = kfs[k];
    if constexpr (kDesc) BSLAM_HOIST_KF_TRANSLATION(kf);
    float cost[2];
    BSLAM_ZERO(cost[0]);
    BSLAM_ZERO(cost[1]);
    uint32_t n_depth = 0, n_desc = 0;   // uniform: pair counts of the wave, from ballots
#pragma unroll
    for (int r = 0; r < kR; ++r) {
      bool got_depth = false, got_desc = false;
      do {
        Proj p;
        DescSamples ds;
        f2 color_pxy, t1, t2;
        bool has_desc = false;
        if (!valid[r]) break;
        if constexpr (!kDesc) {
          if (!project_and_associate(c, kf, gp[r], gn[r], &p)) break;
        } else {
          // the pose kernel's order: record and the three quad gathers in flight together, the association test behind them
          if (!project_to_pixel(c, kf, gp[r], &p)) break;
          const PixelRecord rec = load_record(c, kf, p);
          has_desc = depth_to_color_pxy_in_bounds(c, p.pxy, &color_pxy);
          project_tangent_points(tp1[r], tp2[r], kf.frame_T_global, c, &t1, &t2);
          ds = descriptor_samples_issue(kf, c, color_pxy, t1, t2);
          asm volatile("" ::: "memory");
          if (!associate_with_record(c, kf, gn[r], rec, &p)) break;
        }
        if constexpr (kDepth) {
          cost[0] += objective_depth_term(depth_residual_value(c, p));
          got_depth = true;
        }
        if constexpr (kDesc) {
          if (has_desc) {
            float r1, r2;
            descriptor_samples_values(c, ds, desc1[r], desc2[r], &r1, &r2);
            cost[1] += weighted_desc_residual(r1) + weighted_desc_residual(r2);
            got_desc = true;
          }
        }
      } while (false);
      n_depth += (uint32_t)__builtin_popcountll(__ballot(got_depth));
      n_desc += (uint32_t)__builtin_popcountll(__ballot(got_desc));
    }

    float total = 0.f;
    int my_col;
    bool writer;
    wave_column_sums_owner<2, kCostRedCols>(&my_col, &writer);
    if (n_depth + n_desc != 0) total = wave_column_sums_lds<2, kCostRedCols>(cost, stash.tile[wave]);
    if (writer && my_col < 2) stash.put(at, my_col, total);
    if (lane == 0) {
      stash.put(at, 2, (float)n_depth);   // <= 64 * kR: exact
      stash.put(at, 3, (float)n_desc);
    }
    stash.next(at, k, partials, rows_per_kf, slot);
  }
  if (at.n) stash.flush(at, partials, rows_per_kf, slot);
}

// Row sums of keyframe k = blockIdx.x: the rows of the work slots that visited it (vis: bit place % kfs_per_block of the word
// [place / kfs_per_block][slot]; the other rows were never written), in a fixed order -- row r goes to thread (r % 256, column)
// and its partial sum (r / 256) % 4, the 256 x 4 partial sums of a column then meet in a fixed tree -- so the bits do not depend
// on what was culled (a row that is not visited would have been a row of zeros).  Costs add in fp32, counts in integers.
// Out: rows[k][4] = {depth cost, descriptor cost, depth pairs, descriptor pairs} (the counts as floats: what an exchange sums) and
// counts[k][2], exact.
constexpr int kCostReduceThreads = 1024;
__global__ __launch_bounds__(kCostReduceThreads) void ba_cost_reduce_kernel(const float* __restrict__ partials, int rows_per_kf, const VisWord* __restrict__ vis,
                                                                           int kfs_per_block, float* __restrict__ rows, uint32_t* __restrict__ counts) {
  const int k = blockIdx.x;
  const int col = threadIdx.x % kCostCols, sub = threadIdx.x / kCostCols;   // sub: 0 .. 255
  constexpr int kSubs = kCostReduceThreads / kCostCols;
  const VisWord* words = vis + (size_t)(k / kfs_per_block) * rows_per_kf;
  const uint32_t bit = (uint32_t)(k % kfs_per_block);
  const float* base = partials + (size_t)k * rows_per_kf * kCostCols + col;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  uint32_t n[4] = {0, 0, 0, 0};
  for (int r0 = 0; r0 < rows_per_kf; r0 += 4 * kSubs) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = r0 + u * kSubs + sub;
      const bool take = r < rows_per_kf && ((words[r] >> bit) & 1ull);
      const float x = take ? base[(size_t)r * kCostCols] : 0.f;
      v[u] += x;
      n[u] += col >= 2 ? (uint32_t)x : 0u;   // the per-row counts are small exact floats
    }
  }
  __shared__ float sv[kSubs][kCostCols];
  __shared__ uint32_t sn[kSubs][kCostCols];
  sv[sub][col] = (v[0] + v[1]) + (v[2] + v[3]);
  sn[sub][col] = (n[0] + n[1]) + (n[2] + n[3]);
  __syncthreads();
  for (int half = kSubs / 2; half > 0; half >>= 1) {
    if (sub < half) { sv[sub][col] += sv[sub + half][col]; sn[sub][col] += sn[sub + half][col]; }
    __syncthreads();
  }
  if (threadIdx.x < kCostCols) {
    rows[(size_t)k * kCostCols + col] = col < 2 ? sv[0][col] : (float)sn[0][col];
    if (col >= 2) counts[(size_t)k * 2 + (col - 2)] = sn[0][col];
  }
}

// bslam_debug_ba_cost_descriptor_residuals: for every surfel of one keyframe whose descriptor residuals the cost pass would
// evaluate, out[i] = {r1, r2} of descriptor_samples_finish and {r1, r2} of descriptor_samples_values (four floats; zeros for the
// other surfels).  Surfels in the caller's order.
__global__ __launch_bounds__(256) void ba_cost_descriptor_probe_kernel(CamConsts c, const KfDev* __restrict__ kfs, SurfelRows s, float* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.size) return;
  float o[4] = {0.f, 0.f, 0.f, 0.f};
  const KfDev& kf = kfs[0];
  const f3 gp = mk3(s.x[i], s.y[i], s.z[i]);
  const f3 gn = unpack_normal(s.normal[i]);
  Proj p;
  f2 color_pxy;
  if (project_and_associate(c, kf, gp, gn, &p) && depth_to_color_pxy_in_bounds(c, p.pxy, &color_pxy)) {
    f2 t1, t2;
    tangent_projections(gp, gn, s.radius_squared[i], kf.frame_T_global, c, &t1, &t2);
    const DescSamples ds = descriptor_samples_issue(kf, c, color_pxy, t1, t2);
    float gx1, gy1, gx2, gy2;
    descriptor_samples_finish(kf, c, ds, s.d1[i], s.d2[i], c.desc_gx_scale, c.desc_gy_scale, [&](f2 (&pts)[3]) {
      pts[0] = color_pxy; pts[1] = t1; pts[2] = t2; }, &o[0], &o[1], &gx1, &gy1, &gx2, &gy2);
    descriptor_samples_values(c, ds, s.d1[i], s.d2[i], &o[2], &o[3]);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) out[(size_t)i * 4 + q] = o[q];
}

}  // namespace bslam
