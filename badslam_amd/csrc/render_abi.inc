// render_abi.inc -- model view entry point of include/badslam_hip.h (included by badslam_hip.hip after rectify_abi.inc,
// whose argument helpers it uses).

namespace bslam {

// An optional output image of the camera's size: *out keeps base == nullptr when the caller passed none.
static int make_view(const bslam_buffer2d* b, size_t elem, size_t align, const char* name, const bslam_camera4f* cam, Img* out) {
  out->base = nullptr; out->pitch = 0; out->width = 0; out->height = 0;
  if (!b) return BSLAM_OK;
  int rc = make_img(b, elem, name, out);
  if (rc) return rc;
  if (out->width != cam->width || out->height != cam->height) return fail(BSLAM_ERR_INVALID_ARGUMENT, "%s does not have the camera's size", name);
  if (!rows_aligned(*out, align)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "%s rows must be %zu byte aligned", name, align);
  return BSLAM_OK;
}

}  // namespace bslam

extern "C" {

int bslam_render_surfels(bslam_context* ctx, void* stream_, const bslam_mat3x4* camera_T_global, const bslam_camera4f* camera, uint32_t surfels_size,
                         const bslam_buffer2d* surfels, float min_depth, float max_depth, float radius_scale, float metres_to_depth,
                         const bslam_buffer2d* out_depth, const bslam_buffer2d* out_index, const bslam_buffer2d* out_color,
                         const bslam_buffer2d* out_normal) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !camera_T_global || !camera || !surfels || !surfels->address) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (!out_depth && !out_index && !out_color && !out_normal) return fail(BSLAM_ERR_INVALID_ARGUMENT, "no output view was asked for");
  if (camera->width <= 0 || camera->height <= 0 || (int64_t)camera->width * camera->height > 0x7fffffff)
    return fail(BSLAM_ERR_INVALID_ARGUMENT, "the camera must have between 1 and 2^31 - 1 pixels");
  if (!finite_positive(camera->fx) || !finite_positive(camera->fy)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "focal lengths must be positive");
  if (!finite_positive(radius_scale) || !finite_positive(metres_to_depth)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "radius_scale and metres_to_depth must be > 0");
  if (!(min_depth > 0.0f) || !(max_depth >= min_depth)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "need 0 < min_depth <= max_depth");
  if (surfels->height <= BSLAM_SURFEL_COLOR || surfels->width < 0 || surfels->pitch < (size_t)surfels->width * sizeof(float))
    return fail(BSLAM_ERR_INVALID_ARGUMENT, "surfel buffer needs the rows up to BSLAM_SURFEL_COLOR and a pitch that holds them");
  int rc = check_surfels_size(surfels, surfels_size);
  if (rc) return rc;
  Img rows_img;   // the surfel rows as an image of floats, for the alignment and overlap tests
  rows_img.base = (uint8_t*)surfels->address; rows_img.pitch = (uint32_t)surfels->pitch; rows_img.width = surfels->width; rows_img.height = surfels->height;
  if (surfels->pitch > 0xffffffffu || !rows_aligned(rows_img, sizeof(float))) return fail(BSLAM_ERR_INVALID_ARGUMENT, "surfel rows must be 4 byte aligned");
  Img view[4];
  if ((rc = make_view(out_depth, 2, 2, "depth view", camera, &view[0]))) return rc;
  if ((rc = make_view(out_index, 4, 4, "index view", camera, &view[1]))) return rc;
  if ((rc = make_view(out_color, 4, 4, "colour view", camera, &view[2]))) return rc;
  if ((rc = make_view(out_normal, 12, 4, "normal view", camera, &view[3]))) return rc;
  for (int a = 0; a < 4; ++a) {
    if (!view[a].base) continue;
    if (overlap(view[a], rows_img)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "an output view overlaps the surfel rows");
    for (int b = a + 1; b < 4; ++b)
      if (view[b].base && overlap(view[a], view[b])) return fail(BSLAM_ERR_INVALID_ARGUMENT, "two output views overlap");
  }
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const int pixels = camera->width * camera->height;
  if ((rc = ctx->zbuffer.reserve((size_t)pixels * sizeof(unsigned long long)))) return rc;
  unsigned long long* keys = (unsigned long long*)ctx->zbuffer.ptr;
  const SurfelRowsAll all = surfel_rows_all(surfels);   // the descriptor rows may lie beyond this buffer: their addresses are not used
  const RenderRows rows{all.x, all.y, all.z, all.normal, all.radius_squared, all.color, surfels_size};
  hipLaunchKernelGGL(render_clear_kernel, flat_grid((size_t)pixels), dim3(256), 0, stream, keys, pixels);
  if (surfels_size > 0)
    hipLaunchKernelGGL(render_splat_kernel, flat_grid((size_t)surfels_size), dim3(256), 0, stream, rows, *camera_T_global, *camera, min_depth, max_depth,
                       radius_scale, keys);
  hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((camera->width + 255) / 256), (unsigned)camera->height), dim3(256), 0, stream,
                     (const unsigned long long*)keys, rows, *camera_T_global, metres_to_depth, camera->width, camera->height, view[0], view[1], view[2], view[3]);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

}  // extern "C"
