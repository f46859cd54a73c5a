// intrinsics_abi.inc -- bslam_optimize_intrinsics (included by badslam_hip.hip).

namespace bslam {

// 5x5 / 4x4 symmetric solve in double: pivoted LDL^T as Eigen's selfadjointView<Upper>().ldlt().solve()
// (BS/kernel_opt_intrinsics.cc:168, :269).  Host code.
static void solve_ldlt_upper_host(int n, const double* H_upper, const double* b, float* x) {
  double A[36];
  int idx = 0;
  for (int r = 0; r < n; ++r)
    for (int c = r; c < n; ++c) { A[r * n + c] = H_upper[idx]; A[c * n + r] = H_upper[idx]; ++idx; }
  int perm[6];
  for (int k = 0; k < n; ++k) {
    int p = k;
    double biggest = std::fabs(A[k * n + k]);
    for (int i = k + 1; i < n; ++i) { const double v = std::fabs(A[i * n + i]); if (v > biggest) { biggest = v; p = i; } }
    perm[k] = p;
    if (p != k) {
      for (int c = 0; c < n; ++c) std::swap(A[k * n + c], A[p * n + c]);
      for (int r = 0; r < n; ++r) std::swap(A[r * n + k], A[r * n + p]);
    }
    double temp[6];
    for (int j = 0; j < k; ++j) temp[j] = A[j * n + j] * A[k * n + j];
    double acc = 0.0;
    for (int j = 0; j < k; ++j) acc += A[k * n + j] * temp[j];
    const double dk = A[k * n + k] - acc;
    A[k * n + k] = dk;
    for (int i = k + 1; i < n; ++i) {
      double s = 0.0;
      for (int j = 0; j < k; ++j) s += A[i * n + j] * temp[j];
      const double v = A[i * n + k] - s;
      A[i * n + k] = (std::fabs(dk) > 0.0) ? v / dk : 0.0;
    }
  }
  double y[6];
  for (int i = 0; i < n; ++i) y[i] = b[i];
  for (int k = 0; k < n; ++k) if (perm[k] != k) std::swap(y[k], y[perm[k]]);
  for (int i = 0; i < n; ++i) for (int j = 0; j < i; ++j) y[i] -= A[i * n + j] * y[j];
  for (int i = 0; i < n; ++i) { const double d = A[i * n + i]; y[i] = (std::fabs(d) > 2.2250738585072014e-308) ? y[i] / d : 0.0; }
  for (int i = n - 1; i >= 0; --i) for (int j = i + 1; j < n; ++j) y[i] -= A[j * n + i] * y[j];
  for (int k = n - 1; k >= 0; --k) if (perm[k] != k) std::swap(y[k], y[perm[k]]);
  for (int i = 0; i < n; ++i) x[i] = (float)y[i];
}

// Test tap: `count` elements of device memory to the caller's host array once the stream has reached this point.  A null
// host pointer copies nothing and does not wait.
template <typename T>
static int tap_copy(hipStream_t stream, T* host, const T* dev, size_t count) {
  if (!host) return BSLAM_OK;
  BSLAM_HIP_TRY(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, stream));
  BSLAM_HIP_TRY(hipStreamSynchronize(stream));
  return BSLAM_OK;
}

// bslam_optimize_intrinsics and bslam_debug_optimize_intrinsics: one launch sequence; `tap` (null in the product call) names
// the host arrays that receive the intermediate values.
static int optimize_intrinsics_impl(
    bslam_context* ctx, void* stream_, int optimize_depth_intrinsics, int optimize_color_intrinsics,
    int keyframe_count, const bslam_keyframe_view* keyframes,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera, const bslam_depth_params* depth_params,
    uint32_t surfels_size, const bslam_buffer2d* surfels,
    bslam_camera4f* out_color_camera, bslam_camera4f* out_depth_camera, float* a, const bslam_intrinsics_tap* tap) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!optimize_depth_intrinsics && !optimize_color_intrinsics) return fail(BSLAM_ERR_INVALID_ARGUMENT, "nothing to optimise");   // BS/kernel_opt_intrinsics.cc:53
  int rc = check_surfel_call(ctx, depth_camera, depth_params, surfels, surfels_size);
  if (rc) return rc;
  if (surfels_size == 0 && !has_exchange(ctx)) return BSLAM_OK;                                                                       // :55-57 (an empty shard still takes part in the exchange)
  if (keyframe_count <= 0 || !keyframes || !color_camera || !a) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument / no keyframes");
  if (optimize_depth_intrinsics && !out_depth_camera) return fail(BSLAM_ERR_INVALID_ARGUMENT, "out_depth_camera is null");
  if (optimize_color_intrinsics && !out_color_camera) return fail(BSLAM_ERR_INVALID_ARGUMENT, "out_color_camera is null");
  // the caller's current a (DirectBA passes depth_params_.a by pointer, BS/direct_ba_alternating.cc:591), in place before the
  // upload: the derived pixel records are built from it
  bslam_depth_params dp = *depth_params;
  dp.a = *a;
  CamConsts c;
  if ((rc = setup_keyframe_table(ctx, stream, color_camera, depth_camera, &dp, keyframe_count, keyframes, optimize_color_intrinsics != 0,
                                 surfels_size, surfels, &c))) return rc;

  // the cell grid of the image; the cfactor buffer may be larger (check_surfel_call), its top-left grid is the image
  const int grid_w = (depth_camera->width - 1) / depth_params->sparse_surfel_cell_size + 1;
  const int ncells = grid_w * ((depth_camera->height - 1) / depth_params->sparse_surfel_cell_size + 1);
  const size_t cell_bytes = (size_t)ncells * (8 * sizeof(float) + 7 * sizeof(double));
  if ((rc = ctx->intr_cells.reserve(cell_bytes))) return rc;
  ctx->intr_cells_owner = 0;
  IntrinsicsCells cells;
  cells.B = (float*)ctx->intr_cells.ptr;
  cells.D = cells.B + (size_t)5 * ncells;
  cells.b2 = cells.D + ncells;
  cells.obs = (uint32_t*)(cells.b2 + ncells);
  cells.acc = (double*)(cells.obs + ncells);   // 8 * ncells floats precede it: 8-byte aligned
  cells.cells = ncells;
  cells.grid_width = grid_w;
  BSLAM_HIP_TRY(hipMemsetAsync(ctx->intr_cells.ptr, 0, cell_bytes, stream));   // :66-77

  SurfelWork work;
  if ((rc = prepare_surfels(ctx, stream, surfels, surfels_size, kIntrR, keyframe_count, &work))) return rc;
  const Schedule sc = work.sc;
  const int cell_blocks = (ncells + 255) / 256;
  const size_t rows = std::max<size_t>(sc.slots, (size_t)cell_blocks);
  if ((rc = ctx->partials.reserve((rows + 1) * kIntrRow * sizeof(double) + 2 * kIntrRow * sizeof(float)))) return rc;
  double* partial = (double*)ctx->partials.ptr;   // one row of float64 block sums per slot / per block of cells
  double* reduced = partial + rows * kIntrRow;    // [40]: the sums after the Schur correction of A and b1
  float* sums = (float*)(reduced + kIntrRow);     // [40]: A, b1, colour H, colour b, each rounded once
  float* x1_dev = sums + kIntrRow;                // [5]
  const SurfelRows srows = work.rows;
  const KfDev* kfs = (const KfDev*)ctx->kf_table.ptr;
  const dim3 grid(8u * sc.slots_per_xcd), block(kIntrThreads);
  if (sc.slots > 0) {
    if (optimize_depth_intrinsics && optimize_color_intrinsics) hipLaunchKernelGGL((intrinsics_accumulate_kernel<true, true>), grid, block, 0, stream, c, kfs, keyframe_count, sc, srows, cells, partial);
    else if (optimize_depth_intrinsics) hipLaunchKernelGGL((intrinsics_accumulate_kernel<true, false>), grid, block, 0, stream, c, kfs, keyframe_count, sc, srows, cells, partial);
    else hipLaunchKernelGGL((intrinsics_accumulate_kernel<false, true>), grid, block, 0, stream, c, kfs, keyframe_count, sc, srows, cells, partial);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(intrinsics_sum_rows_kernel, dim3(1), dim3(64), 0, stream, (const double*)partial, (int)sc.slots, sums, (double*)nullptr);
  BSLAM_HIP_TRY(hipGetLastError());
  if (optimize_depth_intrinsics) {
    hipLaunchKernelGGL(intrinsics_cells_round_kernel, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, stream, cells);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  if (has_exchange(ctx)) {
    // surfel-sharded run: the normal-equation blocks are sums over all ranks' surfels.  The observation counts are
    // integers; they travel as exactly representable floats (< 2^24 observations per cell).
    int arc = exchange_sum(ctx, stream, sums, kIntrRow);
    if (arc) return arc;
    if (optimize_depth_intrinsics) {
      hipLaunchKernelGGL(intrinsics_obs_convert_kernel, dim3((unsigned)cell_blocks), dim3(256), 0, stream, cells.obs, ncells, 0);
      BSLAM_HIP_TRY(hipGetLastError());
      arc = exchange_sum(ctx, stream, (float*)ctx->intr_cells.ptr, (size_t)ncells * 8);
      if (arc) return arc;
      hipLaunchKernelGGL(intrinsics_obs_convert_kernel, dim3((unsigned)cell_blocks), dim3(256), 0, stream, cells.obs, ncells, 1);
      BSLAM_HIP_TRY(hipGetLastError());
    }
  }

  if (tap) {
    if ((rc = tap_copy(stream, tap->sums, (const float*)sums, kIntrRow))) return rc;
    if (optimize_depth_intrinsics) {
      if ((rc = tap_copy(stream, tap->cells, (const float*)cells.B, (size_t)7 * ncells))) return rc;   // B[5], D, b2 are contiguous
      if ((rc = tap_copy(stream, tap->obs, (const uint32_t*)cells.obs, (size_t)ncells))) return rc;
    }
  }

  if (optimize_depth_intrinsics) {
    // Schur complement: A -= B D^-1 B^T, b1 -= B D^-1 b2 (:110-118)
    hipLaunchKernelGGL(intrinsics_intermediate_kernel, dim3((unsigned)cell_blocks), dim3(256), 0, stream, cells, partial);
    BSLAM_HIP_TRY(hipGetLastError());
    if (tap && (rc = tap_copy(stream, tap->schur_cells, (const float*)cells.B, (size_t)6 * ncells))) return rc;
  }
  // reduced = sums - the Schur terms (none without depth intrinsics), in float64 from here to the solves
  hipLaunchKernelGGL(intrinsics_sum_rows_kernel, dim3(1), dim3(64), 0, stream, (const double*)partial, optimize_depth_intrinsics ? cell_blocks : 0, sums, reduced);
  BSLAM_HIP_TRY(hipGetLastError());
  if (tap && (rc = tap_copy(stream, tap->schur_sums, (const double*)reduced, kIntrRow))) return rc;
  const double* h = nullptr;
  if ((rc = read_back(ctx, stream, (const double*)reduced, kIntrRow, &h))) return rc;

  if (optimize_depth_intrinsics) {
    double A[15], b1[5];
    float x1[5];
    std::memcpy(A, h, sizeof(A));
    std::memcpy(b1, h + 15, sizeof(b1));
    constexpr float kAPriorWeight = 10;                       // :143-155
    A[14] += kAPriorWeight * kAPriorWeight;
    b1[4] += kAPriorWeight * kAPriorWeight * (*a);
    solve_ldlt_upper_host(5, A, b1, x1);                      // :168
    const float new_fx = 1.0f / (c.fx_inv - x1[0]);           // :183-186
    const float new_fy = 1.0f / (c.fy_inv - x1[1]);
    const float new_cx = -(new_fx * (c.cx_inv - x1[2])) + 0.5f;
    const float new_cy = -(new_fy * (c.cy_inv - x1[3])) + 0.5f;
    *out_depth_camera = bslam_camera4f{new_fx, new_fy, new_cx, new_cy, depth_camera->width, depth_camera->height};
    *a -= x1[4];
    if (tap && tap->x1) std::memcpy(tap->x1, x1, sizeof(x1));
    float* x1_stage = (float*)ctx->staging2.ptr;
    std::memcpy(x1_stage, x1, sizeof(x1));
    BSLAM_HIP_TRY(hipMemcpyAsync(x1_dev, x1_stage, sizeof(x1), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(intrinsics_pixel_update_kernel, dim3((unsigned)cell_blocks), dim3(256), 0, stream, cells, (const float*)x1_dev,
                       (uint8_t*)depth_params->cfactor_buffer.address, (uint32_t)depth_params->cfactor_buffer.pitch);
    BSLAM_HIP_TRY(hipGetLastError());
    BSLAM_HIP_TRY(hipStreamSynchronize(stream));              // the staging is re-used below / by the next call
    ctx->records_signature.clear();                           // cfactor content changed
  }
  if (optimize_color_intrinsics) {
    if ((rc = read_back(ctx, stream, (const double*)reduced, kIntrRow, &h))) return rc;
    double H[10], b[4];
    float x[4];
    std::memcpy(H, h + 20, sizeof(H));
    std::memcpy(b, h + 30, sizeof(b));
    solve_ldlt_upper_host(4, H, b, x);                        // :269
    if (tap && tap->x) std::memcpy(tap->x, x, sizeof(x));
    *out_color_camera = bslam_camera4f{color_camera->fx - x[0], color_camera->fy - x[1], color_camera->cx - x[2], color_camera->cy - x[3],
                                       color_camera->width, color_camera->height};
  }
  return BSLAM_OK;
}

}  // namespace bslam

extern "C" {

int bslam_optimize_intrinsics(
    bslam_context* ctx, void* stream, int optimize_depth_intrinsics, int optimize_color_intrinsics,
    int keyframe_count, const bslam_keyframe_view* keyframes,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera, const bslam_depth_params* depth_params,
    uint32_t surfels_size, const bslam_buffer2d* surfels,
    bslam_camera4f* out_color_camera, bslam_camera4f* out_depth_camera, float* a) {
  return bslam::optimize_intrinsics_impl(ctx, stream, optimize_depth_intrinsics, optimize_color_intrinsics, keyframe_count, keyframes, color_camera,
                                         depth_camera, depth_params, surfels_size, surfels, out_color_camera, out_depth_camera, a, nullptr);
}

int bslam_debug_optimize_intrinsics(
    bslam_context* ctx, void* stream, int optimize_depth_intrinsics, int optimize_color_intrinsics,
    int keyframe_count, const bslam_keyframe_view* keyframes,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera, const bslam_depth_params* depth_params,
    uint32_t surfels_size, const bslam_buffer2d* surfels,
    bslam_camera4f* out_color_camera, bslam_camera4f* out_depth_camera, float* a, const bslam_intrinsics_tap* tap) {
  return bslam::optimize_intrinsics_impl(ctx, stream, optimize_depth_intrinsics, optimize_color_intrinsics, keyframe_count, keyframes, color_camera,
                                         depth_camera, depth_params, surfels_size, surfels, out_color_camera, out_depth_camera, a, tap);
}

}  // extern "C"
