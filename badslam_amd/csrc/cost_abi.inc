// cost_abi.inc -- bslam_compute_ba_cost and its descriptor probe (included by badslam_hip.hip).

extern "C" {

int bslam_compute_ba_cost(
    bslam_context* ctx, void* stream_, int use_depth_residuals, int use_descriptor_residuals,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera, const bslam_depth_params* depth_params,
    int keyframe_count, const bslam_keyframe_view* keyframes, uint32_t surfels_size, const bslam_buffer2d* surfels,
    const bslam_buffer2d* active_surfels, float* cost, uint32_t* counts, bslam_allreduce_fn allreduce, void* allreduce_user) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!use_depth_residuals && !use_descriptor_residuals) return fail(BSLAM_ERR_INVALID_ARGUMENT, "need depth and/or descriptor residuals");
  if (!color_camera) return fail(BSLAM_ERR_INVALID_ARGUMENT, "color_camera is null");
  if (!cost) return fail(BSLAM_ERR_INVALID_ARGUMENT, "cost is null");
  int rc = check_surfel_call(ctx, depth_camera, depth_params, surfels, surfels_size, active_surfels);
  if (rc) return rc;
  if (keyframe_count == 0) return BSLAM_OK;
  CamConsts c;
  if ((rc = setup_keyframe_table(ctx, stream, color_camera, depth_camera, depth_params, keyframe_count, keyframes, use_descriptor_residuals != 0,
                                 surfels_size, surfels, &c, active_surfels))) return rc;
  const size_t row_floats = (size_t)keyframe_count * kCostCols;
  const size_t out_bytes = row_floats * sizeof(float) + (size_t)keyframe_count * 2 * sizeof(uint32_t);
  if ((rc = ctx->coeffs.reserve(out_bytes))) return rc;
  float* d_rows = (float*)ctx->coeffs.ptr;
  uint32_t* d_counts = (uint32_t*)(d_rows + row_floats);

  if (surfels_size > 0) {
    const bool desc = use_descriptor_residuals != 0;
    const int R = pose_surfels_per_thread(desc, surfels_size);
    SurfelWork work;
    if ((rc = prepare_surfels(ctx, stream, surfels, surfels_size, R, keyframe_count, &work, desc))) return rc;
    const int rows_per_kf = (int)work.sc.slots;   // one row per (work slot, keyframe)
    if ((rc = ctx->partials.reserve((size_t)rows_per_kf * keyframe_count * kCostCols * sizeof(float)))) return rc;
    PoseGrid g;
    if ((rc = plan_pose_grid(ctx, work.sc, keyframe_count, 1, -1, &g))) return rc;
    const Schedule& sc = g.sc;
    const int per_block = g.per_block;
    const dim3 grid = g.grid;
    VisWord* vis = (VisWord*)ctx->vis.ptr;
    float* partials = (float*)ctx->partials.ptr;
    const KfDev* kfs = (const KfDev*)ctx->kf_table.ptr;
    const uint8_t* active = active_surfels ? (const uint8_t*)active_surfels->address : nullptr;
    {
      ProfScope prof(ctx, stream, BSLAM_PROF_BA_COST);
#define BSLAM_LAUNCH_COST(DEPTH, DESC, RR)                                                                                                        \
  hipLaunchKernelGGL((ba_cost_kernel<DEPTH, DESC, RR>), grid, dim3(kPoseThreads), 0, stream, c, kfs, keyframe_count, per_block, sc, work.rows, active, \
                     work.perm, partials, rows_per_kf, vis)
      if (use_depth_residuals && desc) BSLAM_LAUNCH_COST(true, true, kPoseRDesc);
      else if (desc) BSLAM_LAUNCH_COST(false, true, kPoseRDesc);
      else if (R == kPoseRGeoLarge) BSLAM_LAUNCH_COST(true, false, kPoseRGeoLarge);
      else BSLAM_LAUNCH_COST(true, false, kPoseRGeo);
#undef BSLAM_LAUNCH_COST
      BSLAM_HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(ba_cost_reduce_kernel, dim3((unsigned)keyframe_count), dim3(kCostReduceThreads), 0, stream, (const float*)partials, rows_per_kf,
                         (const VisWord*)vis, per_block, d_rows, d_counts);
      BSLAM_HIP_TRY(hipGetLastError());
    }
  } else {
    BSLAM_HIP_TRY(hipMemsetAsync(d_rows, 0, out_bytes, stream));   // an empty shard still takes part in the exchange
  }

  // Surfel-sharded runs: the K x 4 rows are summed over the ranks in place.  The counts travel as floats, exact below 2^24 per
  // keyframe and column; every rank sees the same sums and so returns the same error when one reaches the bound.
  const bool exchange = allreduce != nullptr || has_exchange(ctx);
  if (allreduce) {
    const int arc = allreduce(allreduce_user, d_rows, row_floats, stream);
    if (arc) return fail(BSLAM_ERR_HIP, "allreduce callback failed with %d", arc);
  } else if (exchange) {
    if ((rc = exchange_sum(ctx, stream, d_rows, row_floats))) return rc;
  }
  const float* rows = nullptr;
  if ((rc = read_back(ctx, stream, (const float*)d_rows, out_bytes / sizeof(float), &rows))) return rc;
  const uint32_t* exact = (const uint32_t*)(rows + row_floats);
  for (int k = 0; k < keyframe_count; ++k) {
    const float* row = rows + (size_t)k * kCostCols;
    if (exchange && !(row[2] < 16777216.f && row[3] < 16777216.f))
      return fail(BSLAM_ERR_INVALID_ARGUMENT, "keyframe %d: %.0f / %.0f pairs, the exchange counts exactly only below 2^24", k, row[2], row[3]);
    cost[2 * (size_t)k] = row[0];
    cost[2 * (size_t)k + 1] = row[1];
    if (counts) {
      counts[2 * (size_t)k] = exchange ? (uint32_t)row[2] : exact[2 * (size_t)k];
      counts[2 * (size_t)k + 1] = exchange ? (uint32_t)row[3] : exact[2 * (size_t)k + 1];
    }
  }
  return BSLAM_OK;
}

int bslam_debug_ba_cost_descriptor_residuals(
    bslam_context* ctx, void* stream_, const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera,
    const bslam_depth_params* depth_params, const bslam_keyframe_view* keyframe, uint32_t surfels_size, const bslam_buffer2d* surfels, float* out) {
  hipStream_t stream = (hipStream_t)stream_;
  if (surfels_size == 0) return BSLAM_OK;
  if (!keyframe || !out || !color_camera) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  CamConsts c;
  int rc = setup_keyframe_table(ctx, stream, color_camera, depth_camera, depth_params, 1, keyframe, true, surfels_size, surfels, &c);
  if (rc) return rc;
  hipLaunchKernelGGL(ba_cost_descriptor_probe_kernel, dim3((surfels_size + 255) / 256), dim3(256), 0, stream, c, (const KfDev*)ctx->kf_table.ptr,
                     surfel_rows(surfels, surfels_size), out);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

}  // extern "C"
