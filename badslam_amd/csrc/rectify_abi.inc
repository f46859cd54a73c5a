// rectify_abi.inc -- sensor rectification entry points of include/badslam_hip.h (included by badslam_hip.hip).

namespace bslam {

static bool finite_positive(float v) { return v > 0.0f && v <= 3.4028235e38f; }

}  // namespace bslam

extern "C" {

int bslam_build_undistortion_map(bslam_context* ctx, void* stream_, const bslam_radtan_camera* source, const bslam_camera4f* target,
                                 const bslam_buffer2d* map_buffer) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !source || !target) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  Img map;
  int rc = make_img(map_buffer, sizeof(MapEntry), "undistortion map", &map);
  if (rc) return rc;
  if (map.width != target->width || map.height != target->height) return fail(BSLAM_ERR_INVALID_ARGUMENT, "undistortion map does not have the target camera's size");
  if (!rows_aligned(map, 4)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "undistortion map rows must be 4 byte aligned");
  if (source->width < 2 || source->height < 2) return fail(BSLAM_ERR_INVALID_ARGUMENT, "source camera must be at least 2 x 2");
  if (!finite_positive(target->fx) || !finite_positive(target->fy)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "target focal lengths must be positive");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(undistortion_map_kernel, image_grid(map), dim3(256), 0, stream, *source, *target, map);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_undistort_rgb(bslam_context* ctx, void* stream_, const bslam_buffer2d* input_rgb, const bslam_buffer2d* map_buffer,
                        const bslam_buffer2d* output_rgb) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx) return fail(BSLAM_ERR_INVALID_ARGUMENT, "context is null");
  Img in, map, out;
  int rc = make_img(input_rgb, 3, "input rgb", &in);
  if (rc) return rc;
  if ((rc = make_img(map_buffer, sizeof(MapEntry), "undistortion map", &map))) return rc;
  if ((rc = make_img(output_rgb, 3, "output rgb", &out))) return rc;
  if (!same_shape(map, out)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "undistortion map and output rgb differ in size");
  if (!rows_aligned(map, 4)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "undistortion map rows must be 4 byte aligned");
  if (in.width < 2 || in.height < 2) return fail(BSLAM_ERR_INVALID_ARGUMENT, "input rgb must be at least 2 x 2");
  if (overlap(in, out) || overlap(map, out)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "output rgb must not overlap the input or the map");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(undistort_rgb_kernel, image_grid(out), dim3(256), 0, stream, in, map, out);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_reproject_depth(bslam_context* ctx, void* stream_, const bslam_buffer2d* input_depth, float input_depth_to_metres,
                          const bslam_buffer2d* unprojection_map, const bslam_mat3x4* target_T_depth, const bslam_camera4f* target,
                          float depth_difference_threshold, float output_metres_to_depth, const bslam_buffer2d* output_depth) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !target) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  Img in, map, out;
  int rc = make_img(input_depth, 2, "input depth", &in);
  if (rc) return rc;
  if ((rc = make_img(unprojection_map, sizeof(MapEntry), "unprojection map", &map))) return rc;
  if ((rc = make_img(output_depth, 2, "output depth", &out))) return rc;
  if (!same_shape(in, map)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "unprojection map does not have the input depth's size");
  if (!rows_aligned(map, 4)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "unprojection map rows must be 4 byte aligned");
  if (out.width != target->width || out.height != target->height) return fail(BSLAM_ERR_INVALID_ARGUMENT, "output depth does not have the target camera's size");
  if (overlap(in, out) || overlap(map, out) || overlap(in, map)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "input depth, unprojection map and output depth must not overlap");
  if (!finite_positive(depth_difference_threshold)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "depth_difference_threshold must be > 0");
  if (!finite_positive(input_depth_to_metres) || !finite_positive(output_metres_to_depth)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "depth scales must be > 0");
  if ((int64_t)out.width * out.height > 0x7fffffff) return fail(BSLAM_ERR_INVALID_ARGUMENT, "output depth is too large");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const int pixels = out.width * out.height;
  if ((rc = ctx->zbuffer.reserve((size_t)pixels * sizeof(uint32_t)))) return rc;
  uint32_t* zbuffer = (uint32_t*)ctx->zbuffer.ptr;
  bslam_mat3x4 T = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
  if (target_T_depth) T = *target_T_depth;
  hipLaunchKernelGGL(zbuffer_clear_kernel, flat_grid((size_t)pixels), dim3(256), 0, stream, zbuffer, pixels);
  if (in.width >= 2 && in.height >= 2) {
    const dim3 tiles((unsigned)((in.width - 1 + kRasterTile - 1) / kRasterTile), (unsigned)((in.height - 1 + kRasterTile - 1) / kRasterTile));
    hipLaunchKernelGGL(reproject_depth_kernel, tiles, dim3(256), 0, stream, in, input_depth_to_metres, map, T, *target, depth_difference_threshold, zbuffer);
  }
  hipLaunchKernelGGL(zbuffer_resolve_kernel, image_grid(out), dim3(256), 0, stream, (const uint32_t*)zbuffer, output_metres_to_depth, out);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

}  // extern "C"
