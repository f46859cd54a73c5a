// pcg_abi.inc -- PCG entry points of include/badslam_hip.h (included by badslam_hip.hip).

namespace bslam {

static int pcg_check(const bslam_context* ctx, const bslam_pcg_layout* l, const bslam_pcg_vectors* v) {
  if (!ctx || !l || !v) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (!v->r || !v->M || !v->delta || !v->g || !v->p || !v->alpha_n || !v->alpha_d || !v->beta_n)
    return fail(BSLAM_ERR_INVALID_ARGUMENT, "a PCG vector is null");
  if (!l->use_depth_residuals && !l->use_descriptor_residuals) return fail(BSLAM_ERR_INVALID_ARGUMENT, "need depth and/or descriptor residuals");
  return BSLAM_OK;
}

static PcgParams make_pcg_params(const bslam_pcg_layout* l, const bslam_pcg_vectors* v) {
  PcgParams P;
  P.unknown_count = l->unknown_count;
  P.surfel_start = l->surfel_unknown_start_index;
  P.depth_intr_start = l->depth_intrinsics_unknown_start_index;
  P.a_index = l->a_unknown_index;
  P.color_intr_start = l->color_intrinsics_unknown_start_index;
  P.gauge_kf = l->gauge_keyframe_id;
  P.optimize_poses = l->optimize_poses;
  P.optimize_geometry = l->optimize_geometry;
  P.optimize_depth_intr = l->optimize_depth_intrinsics;
  P.optimize_color_intr = l->optimize_color_intrinsics;
  P.per_surfel = l->use_descriptor_residuals ? 3 : 1;
  // sharded unknowns: the surfel entries, which end where the next group starts (BS/direct_ba_pcg.cc:270-306)
  P.shard_begin = P.shard_end = l->surfel_unknown_start_index;
  if (l->optimize_geometry) {
    P.shard_end = l->unknown_count;
    if (l->optimize_depth_intrinsics && l->depth_intrinsics_unknown_start_index != 0xffffffffu) P.shard_end = l->depth_intrinsics_unknown_start_index;
    else if (l->optimize_color_intrinsics && l->color_intrinsics_unknown_start_index != 0xffffffffu) P.shard_end = l->color_intrinsics_unknown_start_index;
  }
  P.r = v->r; P.M = v->M; P.delta = v->delta; P.g = v->g; P.p = v->p;
  P.alpha_n = v->alpha_n; P.alpha_d = v->alpha_d; P.beta_n = v->beta_n;
  P.cf_acc0 = P.cf_acc1 = nullptr;
  P.cf_cells = 0;
  P.perm = nullptr;
  return P;
}

// The instantiation of the surfel kernels for a pass (init / step 1), its residuals (depth and descriptors, depth only,
// descriptors only) and whether any intrinsics are unknowns.
typedef void (*PcgSurfelKernel)(CamConsts, const KfDev*, int, Schedule, SurfelRows, PcgParams, float*, float*);
template <bool kDepth, bool kDesc, bool kIntr>
static PcgSurfelKernel pcg_surfel_kernel_of(bool step1) { return step1 ? pcg_step1_kernel<kDepth, kDesc, kIntr> : pcg_init_kernel<kDepth, kDesc, kIntr>; }
template <bool kIntr>
static PcgSurfelKernel pcg_surfel_kernel_of(bool step1, bool depth, bool desc) {
  return depth && desc ? pcg_surfel_kernel_of<true, true, kIntr>(step1) : depth ? pcg_surfel_kernel_of<true, false, kIntr>(step1) : pcg_surfel_kernel_of<false, true, kIntr>(step1);
}

// Deterministic dot product tail: the two runs of block partials (shared | sharded) -> *out = shared + sum over
// ranks of sharded.  `pair` (2 floats of device scratch) receives {shared, sharded} when a hook is set.
static int pcg_final_sum(bslam_context* ctx, hipStream_t stream, const float* partial, int sb, int lb, float* out, float* pair) {
  if (!has_exchange(ctx)) {
    hipLaunchKernelGGL(pcg_final_sum_kernel, dim3(1), dim3(256), 0, stream, partial, sb, lb, out, 1);
    BSLAM_HIP_TRY(hipGetLastError());
    return BSLAM_OK;
  }
  hipLaunchKernelGGL(pcg_final_sum_kernel, dim3(1), dim3(256), 0, stream, partial, sb, lb, pair, 0);
  BSLAM_HIP_TRY(hipGetLastError());
  int rc = exchange_sum(ctx, stream, pair + 1, 1);
  if (rc) return rc;
  hipLaunchKernelGGL(pcg_add2_kernel, dim3(1), dim3(1), 0, stream, (const float*)pair, out);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

// Sums the shared unknowns of v0 (and v1) plus `extra_count` scalars at `extra` across ranks.
static int pcg_exchange_shared(bslam_context* ctx, hipStream_t stream, const PcgParams& P, float* v0, float* v1, float* extra, int extra_count) {
  const uint32_t shared = P.unknown_count - (P.shard_end - P.shard_begin);
  const size_t count = (size_t)shared * (v1 ? 2 : 1) + (size_t)extra_count;
  if (count == 0) return BSLAM_OK;
  int rc = ctx->exchange.reserve(count * sizeof(float));
  if (rc) return rc;
  float* stage = (float*)ctx->exchange.ptr;
  const unsigned blocks = (shared + 255) / 256;
  if (shared) {
    hipLaunchKernelGGL(pcg_pack_shared_kernel, dim3(blocks), dim3(256), 0, stream, (const float*)v0, (const float*)v1, P.unknown_count, P.shard_begin, P.shard_end, stage);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  float* tail = stage + (size_t)shared * (v1 ? 2 : 1);
  if (extra_count) BSLAM_HIP_TRY(hipMemcpyAsync(tail, extra, sizeof(float) * extra_count, hipMemcpyDeviceToDevice, stream));
  if ((rc = exchange_sum(ctx, stream, stage, count))) return rc;
  if (shared) {
    hipLaunchKernelGGL(pcg_unpack_shared_kernel, dim3(blocks), dim3(256), 0, stream, v0, v1, P.unknown_count, P.shard_begin, P.shard_end, (const float*)stage);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  if (extra_count) BSLAM_HIP_TRY(hipMemcpyAsync(extra, tail, sizeof(float) * extra_count, hipMemcpyDeviceToDevice, stream));
  return BSLAM_OK;
}

static int pcg_surfel_pass(bslam_context* ctx, hipStream_t stream, bool step1, const bslam_pcg_layout* layout,
                           const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera, const bslam_depth_params* dp,
                           int keyframe_count, const bslam_keyframe_view* keyframes, uint32_t surfels_size, const bslam_buffer2d* surfels,
                           const bslam_pcg_vectors* v) {
  if (keyframe_count <= 0 || !keyframes || !color_camera) return fail(BSLAM_ERR_INVALID_ARGUMENT, "need at least one keyframe");
  const uint32_t per = layout->use_descriptor_residuals ? 3u : 1u;
  if (layout->optimize_geometry && (uint64_t)layout->surfel_unknown_start_index + (uint64_t)per * surfels_size > layout->unknown_count)
    return fail(BSLAM_ERR_INVALID_ARGUMENT, "unknown layout too small for %u surfels", surfels_size);
  if (layout->optimize_poses && (layout->gauge_keyframe_id < 0 || layout->gauge_keyframe_id >= keyframe_count))
    return fail(BSLAM_ERR_INVALID_ARGUMENT, "gauge keyframe %d out of range", layout->gauge_keyframe_id);
  for (int k = 0; k < keyframe_count; ++k)
    if (keyframes[k].id != k) return fail(BSLAM_ERR_INVALID_ARGUMENT, "the PCG path needs keyframe ids 0..K-1 in list order (BS/direct_ba_pcg.cc:138-143)");
  CamConsts c;
  int rc = setup_keyframe_table(ctx, stream, color_camera, depth_camera, dp, keyframe_count, keyframes, layout->use_descriptor_residuals != 0,
                                surfels_size, surfels, &c);
  if (rc) return rc;
  PcgParams P = make_pcg_params(layout, v);
  if (layout->optimize_depth_intrinsics) {
    // fp64 scratch for the per-cell sums; zeroed on first use and left zero by pcg_cf_flush_kernel
    const size_t cells = (size_t)dp->cfactor_buffer.width * (size_t)dp->cfactor_buffer.height;
    if ((uint64_t)layout->depth_intrinsics_unknown_start_index + 5 + cells > layout->unknown_count)
      return fail(BSLAM_ERR_INVALID_ARGUMENT, "unknown layout too small for %zu cfactor cells", cells);
    const size_t bytes = cells * 2 * sizeof(double);
    const void* before = ctx->intr_cells.ptr;
    if ((rc = ctx->intr_cells.reserve(bytes))) return rc;
    if (ctx->intr_cells.ptr != before || ctx->intr_cells_owner != 1 || ctx->intr_cells_cells != cells)
      BSLAM_HIP_TRY(hipMemsetAsync(ctx->intr_cells.ptr, 0, bytes, stream));
    ctx->intr_cells_owner = 1;
    ctx->intr_cells_cells = cells;
    P.cf_acc0 = (double*)ctx->intr_cells.ptr;
    P.cf_acc1 = P.cf_acc0 + cells;
    P.cf_cells = (uint32_t)cells;
  }
  SurfelWork work;
  if ((rc = prepare_surfels(ctx, stream, surfels, surfels_size,
                            pcg_surfels_per_thread(layout->use_descriptor_residuals != 0, layout->optimize_depth_intrinsics || layout->optimize_color_intrinsics),
                            keyframe_count, &work, layout->use_descriptor_residuals != 0, /*same_surfels_as_last_call*/ step1))) return rc;
  const Schedule sc = work.sc;
  P.perm = work.perm;
  const int tiles = (int)sc.slots;
  const int pose_rows = tiles;   // one partial pose row per tile
  const size_t pose_floats = (size_t)pose_rows * keyframe_count * kPcgPoseRow;
  const size_t glob_floats = (size_t)tiles * kPcgGlobRow;
  if ((rc = ctx->partials.reserve((pose_floats + glob_floats + 64) * sizeof(float)))) return rc;
  float* pp = (float*)ctx->partials.ptr;
  float* pg = pp + pose_floats;
  const bool intr = layout->optimize_depth_intrinsics || layout->optimize_color_intrinsics;
  const bool depth = layout->use_depth_residuals != 0, desc = layout->use_descriptor_residuals != 0;
  const KfDev* kfs = (const KfDev*)ctx->kf_table.ptr;
  const SurfelRows rows = work.rows;
  const dim3 grid(8u * sc.slots_per_xcd);
  if (tiles > 0) {   // an empty shard of a multi-rank run only takes part in the reductions below
    ProfScope prof(ctx, stream, step1 ? 3 : 2);
    const PcgSurfelKernel kernel = intr ? pcg_surfel_kernel_of<true>(step1, depth, desc) : pcg_surfel_kernel_of<false>(step1, depth, desc);
    hipLaunchKernelGGL(kernel, grid, dim3(kPcgThreads), 0, stream, c, kfs, keyframe_count, sc, rows, P, pp, pg);
  }
  BSLAM_HIP_TRY(hipGetLastError());
  if (P.cf_cells) {
    hipLaunchKernelGGL(pcg_cf_flush_kernel, dim3((P.cf_cells + 255) / 256), dim3(256), 0, stream, P, step1 ? 1 : 0);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  if (layout->optimize_poses) {
    hipLaunchKernelGGL(pcg_pose_reduce_kernel, dim3((unsigned)keyframe_count), dim3(kPcgPoseReduceThreads), 0, stream, (const float*)pp, pose_rows, keyframe_count, kfs, P, step1 ? 1 : 0);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  // device scratch: [0..1] eps {shared, sharded}, [2] this rank's pair sum of alpha_d
  float* scratch = (float*)((uint8_t*)ctx->misc.ptr + kMiscPcgScratch);
  if (step1) {
    // epsilon term (added once per keyframe, quirk Q7, BS/kernel_pcg.cu:1102-1113)
    const int sb = (int)vec_shared_blocks(P), lb = (int)vec_local_blocks(P);
    if ((rc = ctx->coeffs.reserve(((size_t)sb + lb + 8) * sizeof(float)))) return rc;
    float* vpart = (float*)ctx->coeffs.ptr;
    if (sb + lb > 0) {
      hipLaunchKernelGGL(pcg_eps_kernel, dim3((unsigned)(sb + lb)), dim3(kVecThreads), 0, stream, P, vpart);
      BSLAM_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(pcg_final_sum_kernel, dim3(1), dim3(256), 0, stream, (const float*)vpart, sb, lb, scratch, 0);
    BSLAM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pcg_glob_reduce_kernel, dim3(1), dim3(kPcgGlobReduceThreads), 0, stream, (const float*)pg, tiles, P, 1, scratch + 2);
    BSLAM_HIP_TRY(hipGetLastError());
    // multi-rank: g of the shared unknowns, the sharded epsilon term and the pair sum are summed across ranks
    if (has_exchange(ctx) && (rc = pcg_exchange_shared(ctx, stream, P, v->g, nullptr, scratch + 1, 2))) return rc;
    hipLaunchKernelGGL(pcg_alpha_d_kernel, dim3(1), dim3(1), 0, stream, (const float*)(scratch + 2), (const float*)scratch, keyframe_count, v->alpha_d);
    BSLAM_HIP_TRY(hipGetLastError());
  } else {
    if (intr) {
      hipLaunchKernelGGL(pcg_glob_reduce_kernel, dim3(1), dim3(kPcgGlobReduceThreads), 0, stream, (const float*)pg, tiles, P, 0, (float*)nullptr);
      BSLAM_HIP_TRY(hipGetLastError());
    }
    // multi-rank: r0 and M of the shared unknowns are sums over all ranks' surfels
    if (has_exchange(ctx) && (rc = pcg_exchange_shared(ctx, stream, P, v->r, v->M, nullptr, 0))) return rc;
  }
  return BSLAM_OK;
}

}  // namespace bslam

extern "C" {

int bslam_pcg_init(bslam_context* ctx, void* stream_, const bslam_pcg_layout* layout,
                   const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera, const bslam_depth_params* depth_params,
                   int keyframe_count, const bslam_keyframe_view* keyframes, uint32_t surfels_size, const bslam_buffer2d* surfels,
                   const bslam_pcg_vectors* v) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = pcg_check(ctx, layout, v);
  if (rc) return rc;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  BSLAM_HIP_TRY(hipMemsetAsync(v->r, 0, (size_t)layout->unknown_count * sizeof(float), stream));   // BS/direct_ba_pcg.cc:315-316
  BSLAM_HIP_TRY(hipMemsetAsync(v->M, 0, (size_t)layout->unknown_count * sizeof(float), stream));
  if (surfels_size == 0 && !has_exchange(ctx)) return BSLAM_OK;                                    // BS/kernel_pcg.cu:536-538
  return pcg_surfel_pass(ctx, stream, false, layout, color_camera, depth_camera, depth_params, keyframe_count, keyframes, surfels_size, surfels, v);
}

int bslam_pcg_init2(bslam_context* ctx, void* stream_, const bslam_pcg_layout* layout, float a, const bslam_pcg_vectors* v) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = pcg_check(ctx, layout, v);
  if (rc) return rc;
  if (layout->unknown_count == 0) return BSLAM_OK;   // BS/kernel_pcg.cu:620-622
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const PcgParams P = make_pcg_params(layout, v);
  const int sb = (int)vec_shared_blocks(P), lb = (int)vec_local_blocks(P);
  if ((rc = ctx->coeffs.reserve(((size_t)sb + lb + 8) * sizeof(float)))) return rc;
  float* vpart = (float*)ctx->coeffs.ptr;
  hipLaunchKernelGGL(pcg_init2_kernel, dim3((unsigned)(sb + lb)), dim3(kVecThreads), 0, stream, P, a, vpart);
  BSLAM_HIP_TRY(hipGetLastError());
  return pcg_final_sum(ctx, stream, vpart, sb, lb, v->alpha_n, (float*)((uint8_t*)ctx->misc.ptr + kMiscPcgPair));
}

int bslam_pcg_step1(bslam_context* ctx, void* stream_, const bslam_pcg_layout* layout,
                    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera, const bslam_depth_params* depth_params,
                    int keyframe_count, const bslam_keyframe_view* keyframes, uint32_t surfels_size, const bslam_buffer2d* surfels,
                    const bslam_pcg_vectors* v, int clear_g) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = pcg_check(ctx, layout, v);
  if (rc) return rc;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  BSLAM_HIP_TRY(hipMemsetAsync(v->alpha_d, 0, sizeof(float), stream));                                        // BS/direct_ba_pcg.cc:383
  if (clear_g) BSLAM_HIP_TRY(hipMemsetAsync(v->g, 0, (size_t)layout->unknown_count * sizeof(float), stream));  // :393
  if (surfels_size == 0 && !has_exchange(ctx)) return BSLAM_OK;   // an empty shard still takes part in the exchange
  return pcg_surfel_pass(ctx, stream, true, layout, color_camera, depth_camera, depth_params, keyframe_count, keyframes, surfels_size, surfels, v);
}

int bslam_pcg_step2(bslam_context* ctx, void* stream_, const bslam_pcg_layout* layout, const bslam_pcg_vectors* v, float* beta_n_host) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = pcg_check(ctx, layout, v);
  if (rc) return rc;
  if (layout->unknown_count == 0) return BSLAM_OK;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const PcgParams P = make_pcg_params(layout, v);
  const int sb = (int)vec_shared_blocks(P), lb = (int)vec_local_blocks(P);
  if ((rc = ctx->coeffs.reserve(((size_t)sb + lb + 8) * sizeof(float)))) return rc;
  float* vpart = (float*)ctx->coeffs.ptr;
  hipLaunchKernelGGL(pcg_step2_kernel, dim3((unsigned)(sb + lb)), dim3(kVecThreads), 0, stream, P, vpart);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = pcg_final_sum(ctx, stream, vpart, sb, lb, v->beta_n, (float*)((uint8_t*)ctx->misc.ptr + kMiscPcgPair)))) return rc;
  if (beta_n_host) {
    const float* h = nullptr;
    if ((rc = read_back(ctx, stream, (const float*)v->beta_n, 1, &h))) return rc;   // BS/direct_ba_pcg.cc:441-443
    *beta_n_host = *h;
  }
  return BSLAM_OK;
}

int bslam_pcg_step3(bslam_context* ctx, void* stream_, const bslam_pcg_layout* layout, const bslam_pcg_vectors* v) {
  hipStream_t stream = (hipStream_t)stream_;
  int rc = pcg_check(ctx, layout, v);
  if (rc) return rc;
  if (layout->unknown_count == 0) return BSLAM_OK;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const PcgParams P = make_pcg_params(layout, v);
  const unsigned vblocks = vec_shared_blocks(P) + vec_local_blocks(P);
  hipLaunchKernelGGL(pcg_step3_kernel, dim3(vblocks), dim3(kVecThreads), 0, stream, P);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_update_surfels_from_pcg_delta(bslam_context* ctx, void* stream_, uint32_t surfels_size, const bslam_buffer2d* surfels,
                                        int use_descriptor_residuals, uint32_t surfel_unknown_start_index, const float* pcg_delta) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !surfels || !pcg_delta) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (surfels_size == 0) return BSLAM_OK;   // BS/kernel_pcg.cu:1343-1345
  int rc = check_surfels_size(surfels, surfels_size);
  if (rc) return rc;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  SurfelRowsRW s = surfel_rows_rw(surfels, nullptr, surfels_size);
  const dim3 grid((surfels_size + 255) / 256), block(256);
  if (use_descriptor_residuals) hipLaunchKernelGGL(pcg_update_surfels_kernel<true>, grid, block, 0, stream, s.x, s.y, s.z, (const uint32_t*)s.normal, s.d1, s.d2, surfels_size, surfel_unknown_start_index, pcg_delta);
  else hipLaunchKernelGGL(pcg_update_surfels_kernel<false>, grid, block, 0, stream, s.x, s.y, s.z, (const uint32_t*)s.normal, s.d1, s.d2, surfels_size, surfel_unknown_start_index, pcg_delta);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_update_cfactors_from_pcg_delta(bslam_context* ctx, void* stream_, const bslam_buffer2d* cfactor_buffer,
                                         uint32_t cfactor_unknown_start_index, const float* pcg_delta) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !cfactor_buffer || !cfactor_buffer->address || !pcg_delta) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const int n = cfactor_buffer->width * cfactor_buffer->height;
  hipLaunchKernelGGL(pcg_update_cfactors_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (uint8_t*)cfactor_buffer->address,
                     (uint32_t)cfactor_buffer->pitch, cfactor_buffer->width, cfactor_buffer->height, cfactor_unknown_start_index, pcg_delta);
  BSLAM_HIP_TRY(hipGetLastError());
  ctx->records_signature.clear();   // cfactor content changed: cached records (bslam_set_keyframe_cache) were built from the old one
  return BSLAM_OK;
}

}  // extern "C"
