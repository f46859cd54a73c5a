// preprocess_abi.inc -- keyframe preprocessing entry points of include/badslam_hip.h (included by badslam_hip.hip).

namespace bslam {

// The pyramid level L (1 ... 3) with in = out * 2^L in both dimensions; 0 if there is none.
static int pyramid_level(const Img& in, const Img& out) {
  for (int level = 1; level <= 3; ++level)
    if (in.width == (int64_t)out.width << level && in.height == (int64_t)out.height << level) return level;
  return 0;
}

}  // namespace bslam

extern "C" {

int bslam_median_filter_and_densify_depth(bslam_context* ctx, void* stream_, const bslam_buffer2d* input_depth, const bslam_buffer2d* output_depth) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx) return fail(BSLAM_ERR_INVALID_ARGUMENT, "context is null");
  Img in, out;
  int rc = make_img(input_depth, 2, "input depth", &in);
  if (rc) return rc;
  if ((rc = make_img(output_depth, 2, "output depth", &out))) return rc;
  if (!same_shape(in, out) || overlap(in, out)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "input and output depth must be buffers of one size that do not overlap");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const int quads_per_row = (in.width + 3) / 4;
  hipLaunchKernelGGL(median_densify_kernel, flat_grid((size_t)quads_per_row * in.height), dim3(256), 0, stream, in, out, quads_per_row,
                     rows_aligned(in, 8) && rows_aligned(out, 8));
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_downscale_depth_median(bslam_context* ctx, void* stream_, const bslam_buffer2d* input_depth, const bslam_buffer2d* output_depth) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx) return fail(BSLAM_ERR_INVALID_ARGUMENT, "context is null");
  Img in, out;
  int rc = make_img(input_depth, 2, "input depth", &in);
  if (rc) return rc;
  if ((rc = make_img(output_depth, 2, "output depth", &out))) return rc;
  const int level = pyramid_level(in, out);
  if (!level || overlap(in, out)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "input depth must have 2^L times the output size, L = 1 ... 3, and not overlap the output");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const dim3 grid = flat_grid((size_t)out.width * out.height);
  if (level == 1) hipLaunchKernelGGL(downscale_depth_median_kernel<1>, grid, dim3(256), 0, stream, in, out, rows_aligned(in, 4));
  else if (level == 2) hipLaunchKernelGGL(downscale_depth_median_kernel<2>, grid, dim3(256), 0, stream, in, out, rows_aligned(in, 8));
  else hipLaunchKernelGGL(downscale_depth_median_kernel<3>, grid, dim3(256), 0, stream, in, out, rows_aligned(in, 16));
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_downscale_rgb(bslam_context* ctx, void* stream_, const bslam_buffer2d* input_rgb, const bslam_buffer2d* output_rgb) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx) return fail(BSLAM_ERR_INVALID_ARGUMENT, "context is null");
  Img in, out;
  int rc = make_img(input_rgb, 3, "input rgb", &in);
  if (rc) return rc;
  if ((rc = make_img(output_rgb, 3, "output rgb", &out))) return rc;
  const int level = pyramid_level(in, out);
  if (!level || overlap(in, out)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "input rgb must have 2^L times the output size, L = 1 ... 3, and not overlap the output");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const dim3 grid = flat_grid((size_t)out.width * 3 * out.height);
  if (level == 1) hipLaunchKernelGGL(downscale_rgb_kernel<1>, grid, dim3(256), 0, stream, in, out);
  else if (level == 2) hipLaunchKernelGGL(downscale_rgb_kernel<2>, grid, dim3(256), 0, stream, in, out);
  else hipLaunchKernelGGL(downscale_rgb_kernel<3>, grid, dim3(256), 0, stream, in, out);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_compute_brightness(bslam_context* ctx, void* stream_, const bslam_buffer2d* rgb_buffer, const bslam_buffer2d* color_buffer) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx) return fail(BSLAM_ERR_INVALID_ARGUMENT, "context is null");
  Img rgb, color;
  int rc = make_img(rgb_buffer, 3, "rgb", &rgb);
  if (rc) return rc;
  if ((rc = make_img(color_buffer, 4, "color", &color))) return rc;
  if (!same_shape(rgb, color)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "rgb and color buffers differ in size");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(brightness_kernel, image_grid(color), dim3(256), 0, stream, rgb, color);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_bilateral_filter_and_depth_cutoff(bslam_context* ctx, void* stream_, float sigma_xy, float sigma_value, float radius_factor,
                                            uint16_t max_depth, float raw_to_float_depth, const bslam_buffer2d* input_depth,
                                            const bslam_buffer2d* output_depth) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx) return fail(BSLAM_ERR_INVALID_ARGUMENT, "context is null");
  Img in, out;
  int rc = make_img(input_depth, 2, "input depth", &in);
  if (rc) return rc;
  if ((rc = make_img(output_depth, 2, "output depth", &out))) return rc;
  if (!same_shape(in, out) || in.base == out.base) return fail(BSLAM_ERR_INVALID_ARGUMENT, "input and output depth must be distinct buffers of one size");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const int radius = (int)(radius_factor * sigma_xy + 0.5f);   // BS/cuda_depth_processing.cu:113
  hipLaunchKernelGGL(bilateral_kernel, image_grid(out), dim3(256), 0, stream, 2.0f * sigma_xy * sigma_xy, 2.0f * sigma_value * sigma_value, radius,
                     radius * radius, (uint32_t)max_depth, raw_to_float_depth, in, out);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_compute_normals(bslam_context* ctx, void* stream_, const bslam_camera4f* depth_camera, const bslam_depth_params* depth_params,
                          const bslam_buffer2d* input_depth, const bslam_buffer2d* output_depth, const bslam_buffer2d* normals_buffer) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !depth_camera || !depth_params || !depth_params->cfactor_buffer.address) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  Img in, out, nrm;
  int rc = make_img(input_depth, 2, "input depth", &in);
  if (rc) return rc;
  if ((rc = make_img(output_depth, 2, "output depth", &out))) return rc;
  if ((rc = make_img(normals_buffer, 2, "normals", &nrm))) return rc;
  if (!same_shape(in, out) || !same_shape(in, nrm) || in.base == out.base || in.base == nrm.base || out.base == nrm.base)
    return fail(BSLAM_ERR_INVALID_ARGUMENT, "depth / normals buffers must be distinct and of one size");
  if (in.width != depth_camera->width || in.height != depth_camera->height) return fail(BSLAM_ERR_INVALID_ARGUMENT, "depth image does not match the camera");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const CamConsts c = make_cam_consts(ctx, nullptr, depth_camera, depth_params);
  hipLaunchKernelGGL(normals_kernel, image_grid(in), dim3(256), 0, stream, c, in, out, nrm);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_compute_point_radii_and_remove_isolated_pixels(bslam_context* ctx, void* stream_, const bslam_camera4f* depth_camera, float raw_to_float_depth,
                                                         const bslam_buffer2d* depth_buffer, const bslam_buffer2d* radius_buffer,
                                                         const bslam_buffer2d* out_depth) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !depth_camera) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  Img in, rad, out;
  int rc = make_img(depth_buffer, 2, "depth", &in);
  if (rc) return rc;
  if ((rc = make_img(radius_buffer, 2, "radius", &rad))) return rc;
  if ((rc = make_img(out_depth, 2, "output depth", &out))) return rc;
  if (!same_shape(in, rad) || !same_shape(in, out) || in.base == out.base || in.base == rad.base || rad.base == out.base)
    return fail(BSLAM_ERR_INVALID_ARGUMENT, "depth / radius buffers must be distinct and of one size");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const CamConsts c = depth_only_consts(ctx, nullptr, depth_camera, 0.f);
  hipLaunchKernelGGL(radii_kernel, image_grid(in), dim3(256), 0, stream, c, raw_to_float_depth, in, rad, out);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_compute_min_max_depth(bslam_context* ctx, void* stream_, const bslam_buffer2d* depth_buffer, float raw_to_float_depth, float* min_depth,
                                float* max_depth) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !min_depth || !max_depth) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  Img in;
  int rc = make_img(depth_buffer, 2, "depth", &in);
  if (rc) return rc;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  if ((rc = ctx->staging2.reserve(64))) return rc;
  uint32_t* result = (uint32_t*)((uint8_t*)ctx->misc.ptr + kMiscMinMaxDepth);
  const uint32_t init[2] = {0x7f800000u, 0u};   // +inf, 0 (ComputeMinMaxDepthCUDA_InitializeBuffers)
  std::memcpy(ctx->staging2.ptr, init, sizeof(init));
  BSLAM_HIP_TRY(hipMemcpyAsync(result, ctx->staging2.ptr, sizeof(init), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(min_max_depth_kernel, image_grid(in), dim3(256), 0, stream, raw_to_float_depth, in, result);
  BSLAM_HIP_TRY(hipGetLastError());
  const uint32_t* h = nullptr;
  if ((rc = read_back(ctx, stream, (const uint32_t*)result, 2, &h))) return rc;   // results valid on return (BS/cuda_depth_processing.cu:455-464)
  std::memcpy(min_depth, h, 4);
  std::memcpy(max_depth, h + 1, 4);
  return BSLAM_OK;
}

}  // extern "C"
