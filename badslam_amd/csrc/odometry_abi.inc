// odometry_abi.inc -- pairwise frame tracking entry points of include/badslam_hip.h (included by badslam_hip.hip).

namespace bslam {

static int pair_images(const bslam_buffer2d* frame_depth, const bslam_buffer2d* frame_normals, const bslam_buffer2d* frame_color,
                       const bslam_buffer2d* surfel_depth, const bslam_buffer2d* surfel_normals, const bslam_buffer2d* surfel_color,
                       const bslam_camera4f* depth_camera, const bslam_camera4f* color_camera, PairImages* im) {
  int rc;
  if ((rc = make_img(frame_depth, 4, "frame depth", &im->frame_depth))) return rc;
  if ((rc = make_img(frame_normals, 2, "frame normals", &im->frame_normals))) return rc;
  if ((rc = make_img(frame_color, 1, "frame color", &im->frame_color))) return rc;
  if ((rc = make_img(surfel_depth, 4, "surfel depth", &im->surfel_depth))) return rc;
  if ((rc = make_img(surfel_normals, 2, "surfel normals", &im->surfel_normals))) return rc;
  if ((rc = make_img(surfel_color, 1, "surfel color", &im->surfel_color))) return rc;
  if (im->frame_depth.width != depth_camera->width || im->frame_depth.height != depth_camera->height || !same_shape(im->frame_depth, im->frame_normals) ||
      !same_shape(im->frame_depth, im->surfel_depth) || !same_shape(im->frame_depth, im->surfel_normals) || !same_shape(im->frame_depth, im->surfel_color))
    return fail(BSLAM_ERR_INVALID_ARGUMENT, "depth-sized images do not match the (scaled) depth camera %dx%d", depth_camera->width, depth_camera->height);
  if (im->frame_color.width != color_camera->width || im->frame_color.height != color_camera->height)
    return fail(BSLAM_ERR_INVALID_ARGUMENT, "frame colour image does not match the (scaled) colour camera %dx%d", color_camera->width, color_camera->height);
  return BSLAM_OK;
}

// The residual sets of one output kind: depth and descriptor, depth alone, descriptor alone (kGradMag only changes the descriptor).
template <bool kCoeffs, bool kGradMag>
static void launch_pairs(bool use_depth, bool use_desc, dim3 grid, hipStream_t stream, const CamConsts& c, float threshold_factor, float* partials, const PairBatch& batch) {
  if (use_depth && use_desc) hipLaunchKernelGGL((pair_accumulate_kernel<true, true, kCoeffs, kGradMag>), grid, dim3(256), 0, stream, c, threshold_factor, partials, batch);
  else if (use_depth) hipLaunchKernelGGL((pair_accumulate_kernel<true, false, kCoeffs, false>), grid, dim3(256), 0, stream, c, threshold_factor, partials, batch);
  else hipLaunchKernelGGL((pair_accumulate_kernel<false, true, kCoeffs, kGradMag>), grid, dim3(256), 0, stream, c, threshold_factor, partials, batch);
}

// The driver of every image-pair entry point, which has checked its own pointers and pair_count (1 ... kMaxPairBatch): pair p
// tracks tracked_*[p] with transforms[p] against the base images.  Returns the pair_count reduced rows (kRow floats each) in
// *rows_out, on the host and valid until the next call on the context.  coeffs: H, b and the visible count, else cost and residual
// count; gradmag: the one colour residual on gradient-magnitude images in place of the two descriptor residuals.
static int run_pairs(bslam_context* ctx, hipStream_t stream, bool coeffs, bool gradmag, int use_depth, int use_desc, const bslam_camera4f* color_camera,
                     const bslam_camera4f* depth_camera, float baseline_fx, float threshold_factor, int pair_count, const bslam_buffer2d* tracked_depth,
                     const bslam_buffer2d* tracked_normals, const bslam_buffer2d* tracked_color, const bslam_mat3x4* transforms,
                     const bslam_buffer2d* base_depth, const bslam_buffer2d* base_normals, const bslam_buffer2d* base_color, const float** rows_out) {
  if (!use_depth && !use_desc) return fail(BSLAM_ERR_INVALID_ARGUMENT, "need depth and/or descriptor residuals");
  PairBatch batch;
  std::memset(&batch, 0, sizeof(batch));
  int rc;
  for (int p = 0; p < pair_count; ++p) {
    if ((rc = pair_images(&tracked_depth[p], &tracked_normals[p], &tracked_color[p], base_depth, base_normals, base_color, depth_camera, color_camera, &batch.im[p])))
      return rc;
    std::memcpy(batch.im[p].frame_T_surfel.m, transforms[p].m, sizeof(float) * 12);
  }
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const CamConsts c = depth_only_consts(ctx, color_camera, depth_camera, baseline_fx);
  // every pair's tracked colour as luma quads (one 8-byte gather per bilinear sample), one launch: pair_images checked that
  // all have the colour camera's size
  const int cw = color_camera->width, ch = color_camera->height;
  const size_t quad_count = (size_t)(cw + 1) * (ch + 1);
  if (!quad_table_addressable(cw, ch)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "colour image %dx%d is beyond the luma quad table's 32-bit addressing", cw, ch);
  if ((rc = ctx->quads_aux.reserve((size_t)pair_count * quad_count * sizeof(QuadEntry)))) return rc;
  for (int p = 0; p < pair_count; ++p) batch.im[p].frame_quads = (const QuadEntry*)ctx->quads_aux.ptr + (size_t)p * quad_count;
  hipLaunchKernelGGL(build_quads_u8_batched_kernel, dim3((unsigned)((cw + 1 + 255) / 256), (unsigned)(ch + 1), (unsigned)pair_count), dim3(256), 0, stream,
                     (QuadEntry*)ctx->quads_aux.ptr, quad_count, batch);
  BSLAM_HIP_TRY(hipGetLastError());
  const int pixels = depth_camera->width * depth_camera->height;
  const int blocks = (pixels + 255) / 256;
  const int rows = blocks * 4;   // per pair: one per wave
  const size_t partial_floats = (size_t)pair_count * rows * kRow;
  if ((rc = ctx->partials.reserve((partial_floats + (size_t)pair_count * kReduceParts * kRow) * sizeof(float)))) return rc;
  if ((rc = ctx->coeffs.reserve((size_t)pair_count * kRow * sizeof(float)))) return rc;
  float* partials = (float*)ctx->partials.ptr;
  const dim3 grid((unsigned)blocks, (unsigned)pair_count);
  if (gradmag && use_desc) {
    if (coeffs) launch_pairs<true, true>(use_depth, use_desc, grid, stream, c, threshold_factor, partials, batch);
    else launch_pairs<false, true>(use_depth, use_desc, grid, stream, c, threshold_factor, partials, batch);
  } else {
    if (coeffs) launch_pairs<true, false>(use_depth, use_desc, grid, stream, c, threshold_factor, partials, batch);
    else launch_pairs<false, false>(use_depth, use_desc, grid, stream, c, threshold_factor, partials, batch);
  }
  BSLAM_HIP_TRY(hipGetLastError());
  float* parts = partials + partial_floats;
  hipLaunchKernelGGL(pose_reduce_kernel, dim3((unsigned)pair_count, kReduceParts), dim3(256), 0, stream, (const float*)partials, rows, parts);
  BSLAM_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(pose_reduce_final_kernel, dim3((unsigned)pair_count), dim3(64), 0, stream, (const float*)parts, (float*)ctx->coeffs.ptr);
  BSLAM_HIP_TRY(hipGetLastError());
  return read_back(ctx, stream, (const float*)ctx->coeffs.ptr, (size_t)pair_count * kRow, rows_out);   // results valid on return (BS/kernel_opt_pose.cc:189-191)
}

// The single-pair entry points: a batch of one.
static int run_pair(bslam_context* ctx, void* stream, bool coeffs, bool gradmag, int use_depth, int use_desc, const bslam_camera4f* color_camera,
                    const bslam_camera4f* depth_camera, float baseline_fx, float threshold_factor, const bslam_buffer2d* frame_depth,
                    const bslam_buffer2d* frame_normals, const bslam_buffer2d* frame_color, const bslam_mat3x4* estimate_frame_T_surfel_frame,
                    const bslam_buffer2d* surfel_depth, const bslam_buffer2d* surfel_normals, const bslam_buffer2d* surfel_color, const float** row) {
  if (!ctx || !color_camera || !depth_camera || !estimate_frame_T_surfel_frame) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  return run_pairs(ctx, (hipStream_t)stream, coeffs, gradmag, use_depth, use_desc, color_camera, depth_camera, baseline_fx, threshold_factor, 1, frame_depth,
                   frame_normals, frame_color, estimate_frame_T_surfel_frame, surfel_depth, surfel_normals, surfel_color, row);
}

// What the entry points copy out of a row.
static void copy_coeffs(const float* row, uint32_t* visible_count, float* H, float* b) {
  std::memcpy(H, row, 21 * sizeof(float));
  std::memcpy(b, row + 21, 6 * sizeof(float));
  if (visible_count) *visible_count = read_row_count(row);
}
static void copy_cost(const float* row, uint32_t* residual_count, float* residual_sum) {
  *residual_count = read_row_count(row);
  *residual_sum = row[kRowCost];
}

}  // namespace bslam

extern "C" {

int bslam_compute_brightness_from_color(bslam_context* ctx, void* stream_, const bslam_buffer2d* color_buffer, const bslam_buffer2d* intensity_buffer) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx) return fail(BSLAM_ERR_INVALID_ARGUMENT, "context is null");
  Img color, out;
  int rc = make_img(color_buffer, 4, "color", &color);
  if (rc) return rc;
  if ((rc = make_img(intensity_buffer, 1, "intensity", &out))) return rc;
  if (!same_shape(color, out)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "color and intensity buffers differ in size");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(normalize_byte_kernel<uint32_t>, image_grid(out), dim3(256), 0, stream, color, out);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_set_to_read_mode_normalized(bslam_context* ctx, void* stream_, const bslam_buffer2d* input_u8, const bslam_buffer2d* output_u8) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx) return fail(BSLAM_ERR_INVALID_ARGUMENT, "context is null");
  Img in, out;
  int rc = make_img(input_u8, 1, "input", &in);
  if (rc) return rc;
  if ((rc = make_img(output_u8, 1, "output", &out))) return rc;
  if (!same_shape(in, out)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "buffers differ in size");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(normalize_byte_kernel<uint8_t>, image_grid(out), dim3(256), 0, stream, in, out);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_calibrate_depth(bslam_context* ctx, void* stream_, const bslam_depth_params* depth_params, const bslam_buffer2d* depth_buffer,
                          const bslam_buffer2d* out_depth) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !depth_params || !depth_params->cfactor_buffer.address) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  Img in, out;
  int rc = make_img(depth_buffer, 2, "depth", &in);
  if (rc) return rc;
  if ((rc = make_img(out_depth, 4, "output depth", &out))) return rc;
  if (!same_shape(in, out)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "buffers differ in size");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const bslam_camera4f cam = {1.f, 1.f, 0.f, 0.f, in.width, in.height};
  const CamConsts c = make_cam_consts(ctx, nullptr, &cam, depth_params);
  hipLaunchKernelGGL((calibrate_depth_kernel<false>), image_grid(out), dim3(256), 0, stream, c, in, in, out, out);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_calibrate_depth_and_transform_color_to_depth(bslam_context* ctx, void* stream_, const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera,
                                                       const bslam_depth_params* depth_params, const bslam_buffer2d* depth_buffer,
                                                       const bslam_buffer2d* color_u8, const bslam_buffer2d* out_depth, const bslam_buffer2d* out_color) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !color_camera || !depth_camera || !depth_params || !depth_params->cfactor_buffer.address) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  Img in, col, out, outc;
  int rc = make_img(depth_buffer, 2, "depth", &in);
  if (rc) return rc;
  if ((rc = make_img(color_u8, 1, "color", &col))) return rc;
  if ((rc = make_img(out_depth, 4, "output depth", &out))) return rc;
  if ((rc = make_img(out_color, 1, "output color", &outc))) return rc;
  if (!same_shape(in, out) || !same_shape(in, outc)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "buffers differ in size");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const CamConsts c = make_cam_consts(ctx, color_camera, depth_camera, depth_params);
  hipLaunchKernelGGL((calibrate_depth_kernel<true>), image_grid(out), dim3(256), 0, stream, c, in, col, out, outc);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_downsample_images(bslam_context* ctx, void* stream_, const bslam_buffer2d* depth_buffer, const bslam_buffer2d* normals_buffer,
                            const bslam_buffer2d* color_u8, const bslam_buffer2d* downsampled_depth, const bslam_buffer2d* downsampled_normals,
                            const bslam_buffer2d* downsampled_color) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx) return fail(BSLAM_ERR_INVALID_ARGUMENT, "context is null");
  Img d, n, col, od, on, oc;
  int rc;
  if ((rc = make_img(depth_buffer, 4, "depth", &d)) || (rc = make_img(normals_buffer, 2, "normals", &n)) || (rc = make_img(color_u8, 1, "color", &col)) ||
      (rc = make_img(downsampled_depth, 4, "downsampled depth", &od)) || (rc = make_img(downsampled_normals, 2, "downsampled normals", &on)) ||
      (rc = make_img(downsampled_color, 1, "downsampled color", &oc)))
    return rc;
  if (!same_shape(d, n) || !same_shape(od, on) || 2 * od.width > d.width || 2 * od.height > d.height)
    return fail(BSLAM_ERR_INVALID_ARGUMENT, "pyramid level sizes do not fit");
  // a colour pyramid of its own size (colour camera of another pyramid level than the depth camera) halves like the depth one
  if (!same_shape(od, oc) && (2 * oc.width > col.width || 2 * oc.height > col.height)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "colour pyramid level sizes do not fit");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const dim3 grid((unsigned)((std::max(od.width, oc.width) + 255) / 256), (unsigned)std::max(od.height, oc.height));
  hipLaunchKernelGGL(downsample_kernel, grid, dim3(256), 0, stream, d, n, col, ctx->tex_mode, od, on, oc);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_accumulate_pose_coeffs_from_images(
    bslam_context* ctx, void* stream, int use_depth_residuals, int use_descriptor_residuals, const bslam_camera4f* color_camera,
    const bslam_camera4f* depth_camera, float baseline_fx, float threshold_factor, const bslam_buffer2d* downsampled_depth,
    const bslam_buffer2d* downsampled_normals, const bslam_buffer2d* downsampled_color, const bslam_mat3x4* estimate_frame_T_surfel_frame,
    const bslam_buffer2d* surfel_depth, const bslam_buffer2d* surfel_normals, const bslam_buffer2d* surfel_color, uint32_t* visible_count, float* H, float* b) {
  if (!H || !b) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null output");
  const float* row = nullptr;
  int rc = run_pair(ctx, stream, true, false, use_depth_residuals, use_descriptor_residuals, color_camera, depth_camera, baseline_fx, threshold_factor,
                    downsampled_depth, downsampled_normals, downsampled_color, estimate_frame_T_surfel_frame, surfel_depth, surfel_normals, surfel_color, &row);
  if (rc) return rc;
  copy_coeffs(row, visible_count, H, b);
  return BSLAM_OK;
}

int bslam_compute_cost_and_residual_count_from_images(
    bslam_context* ctx, void* stream, int use_depth_residuals, int use_descriptor_residuals, const bslam_camera4f* color_camera,
    const bslam_camera4f* depth_camera, float baseline_fx, float threshold_factor, const bslam_buffer2d* downsampled_depth,
    const bslam_buffer2d* downsampled_normals, const bslam_buffer2d* downsampled_color, const bslam_mat3x4* estimate_frame_T_surfel_frame,
    const bslam_buffer2d* surfel_depth, const bslam_buffer2d* surfel_normals, const bslam_buffer2d* surfel_color, uint32_t* residual_count, float* residual_sum) {
  if (!residual_count || !residual_sum) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null output");
  const float* row = nullptr;
  int rc = run_pair(ctx, stream, false, false, use_depth_residuals, use_descriptor_residuals, color_camera, depth_camera, baseline_fx, threshold_factor,
                    downsampled_depth, downsampled_normals, downsampled_color, estimate_frame_T_surfel_frame, surfel_depth, surfel_normals, surfel_color, &row);
  if (rc) return rc;
  copy_cost(row, residual_count, residual_sum);
  return BSLAM_OK;
}

int bslam_accumulate_pose_coeffs_from_images_gradmag(
    bslam_context* ctx, void* stream, int use_depth_residuals, int use_descriptor_residuals, const bslam_camera4f* color_camera,
    const bslam_camera4f* depth_camera, float baseline_fx, float threshold_factor, const bslam_buffer2d* downsampled_depth,
    const bslam_buffer2d* downsampled_normals, const bslam_buffer2d* downsampled_color, const bslam_mat3x4* estimate_frame_T_surfel_frame,
    const bslam_buffer2d* surfel_depth, const bslam_buffer2d* surfel_normals, const bslam_buffer2d* surfel_color, uint32_t* visible_count, float* H, float* b) {
  if (!H || !b) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null output");
  const float* row = nullptr;
  int rc = run_pair(ctx, stream, true, true, use_depth_residuals, use_descriptor_residuals, color_camera, depth_camera, baseline_fx, threshold_factor,
                    downsampled_depth, downsampled_normals, downsampled_color, estimate_frame_T_surfel_frame, surfel_depth, surfel_normals, surfel_color, &row);
  if (rc) return rc;
  copy_coeffs(row, visible_count, H, b);
  return BSLAM_OK;
}

int bslam_compute_cost_and_residual_count_from_images_gradmag(
    bslam_context* ctx, void* stream, int use_depth_residuals, int use_descriptor_residuals, const bslam_camera4f* color_camera,
    const bslam_camera4f* depth_camera, float baseline_fx, float threshold_factor, const bslam_buffer2d* downsampled_depth,
    const bslam_buffer2d* downsampled_normals, const bslam_buffer2d* downsampled_color, const bslam_mat3x4* estimate_frame_T_surfel_frame,
    const bslam_buffer2d* surfel_depth, const bslam_buffer2d* surfel_normals, const bslam_buffer2d* surfel_color, uint32_t* residual_count, float* residual_sum) {
  if (!residual_count || !residual_sum) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null output");
  const float* row = nullptr;
  int rc = run_pair(ctx, stream, false, true, use_depth_residuals, use_descriptor_residuals, color_camera, depth_camera, baseline_fx, threshold_factor,
                    downsampled_depth, downsampled_normals, downsampled_color, estimate_frame_T_surfel_frame, surfel_depth, surfel_normals, surfel_color, &row);
  if (rc) return rc;
  copy_cost(row, residual_count, residual_sum);
  return BSLAM_OK;
}

int bslam_accumulate_pose_coeffs_from_images_batched(
    bslam_context* ctx, void* stream, int use_depth_residuals, int use_descriptor_residuals, const bslam_camera4f* color_camera,
    const bslam_camera4f* depth_camera, float baseline_fx, float threshold_factor, int pair_count, const bslam_buffer2d* tracked_depth,
    const bslam_buffer2d* tracked_normals, const bslam_buffer2d* tracked_color, const bslam_mat3x4* estimates_frame_T_surfel_frame,
    const bslam_buffer2d* base_depth, const bslam_buffer2d* base_normals, const bslam_buffer2d* base_color, uint32_t* visible_counts, float* H, float* b) {
  if (!ctx || !color_camera || !depth_camera || !estimates_frame_T_surfel_frame || !tracked_depth || !tracked_normals || !tracked_color)
    return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (!H || !b) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null output");
  if (pair_count < 1 || pair_count > kMaxPairBatch) return fail(BSLAM_ERR_INVALID_ARGUMENT, "pair_count %d outside [1, %d]", pair_count, kMaxPairBatch);
  const float* rows = nullptr;
  int rc = run_pairs(ctx, (hipStream_t)stream, true, false, use_depth_residuals, use_descriptor_residuals, color_camera, depth_camera, baseline_fx, threshold_factor,
                     pair_count, tracked_depth, tracked_normals, tracked_color, estimates_frame_T_surfel_frame, base_depth, base_normals, base_color, &rows);
  if (rc) return rc;
  for (int p = 0; p < pair_count; ++p) copy_coeffs(rows + (size_t)p * kRow, visible_counts ? visible_counts + p : nullptr, H + 21 * p, b + 6 * p);
  return BSLAM_OK;
}

int bslam_compute_sobel_gradient_magnitude(bslam_context* ctx, void* stream_, const bslam_buffer2d* color_buffer, const bslam_buffer2d* gradmag_buffer) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx) return fail(BSLAM_ERR_INVALID_ARGUMENT, "context is null");
  Img color, out;
  int rc = make_img(color_buffer, 4, "color", &color);
  if (rc) return rc;
  if ((rc = make_img(gradmag_buffer, 1, "gradmag", &out))) return rc;
  if (!same_shape(color, out)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "color and gradmag buffers differ in size");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(sobel_gradient_magnitude_kernel, image_grid(out), dim3(256), 0, stream, color, out);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_calibrate_and_downsample_images(bslam_context* ctx, void* stream_, int downsample_color, const bslam_depth_params* depth_params,
                                          const bslam_buffer2d* depth_buffer, const bslam_buffer2d* normals_buffer, const bslam_buffer2d* color_u8,
                                          const bslam_buffer2d* downsampled_depth, const bslam_buffer2d* downsampled_normals,
                                          const bslam_buffer2d* downsampled_color) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !depth_params || !depth_params->cfactor_buffer.address) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  Img d, n, col, od, on, oc;
  int rc;
  if ((rc = make_img(depth_buffer, 2, "depth", &d)) || (rc = make_img(normals_buffer, 2, "normals", &n)) || (rc = make_img(color_u8, 1, "color", &col)) ||
      (rc = make_img(downsampled_depth, 4, "downsampled depth", &od)) || (rc = make_img(downsampled_normals, 2, "downsampled normals", &on)) ||
      (rc = make_img(downsampled_color, 1, "downsampled color", &oc)))
    return rc;
  if (!same_shape(d, n) || !same_shape(od, on) || !same_shape(od, oc) || 2 * od.width > d.width || 2 * od.height > d.height)
    return fail(BSLAM_ERR_INVALID_ARGUMENT, "pyramid level sizes do not fit");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const bslam_camera4f cam = {1.f, 1.f, 0.f, 0.f, d.width, d.height};
  const CamConsts c = make_cam_consts(ctx, nullptr, &cam, depth_params);
  if (downsample_color) hipLaunchKernelGGL((calibrate_and_downsample_kernel<true>), image_grid(od), dim3(256), 0, stream, c, d, n, col, od, on, oc);
  else hipLaunchKernelGGL((calibrate_and_downsample_kernel<false>), image_grid(od), dim3(256), 0, stream, c, d, n, col, od, on, oc);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

}  // extern "C"
