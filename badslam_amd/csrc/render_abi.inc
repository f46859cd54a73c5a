// render_abi.inc -- model view entry point of include/badslam_hip.h (included by badslam_hip.hip).

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

// A camera and its optional output views: the camera's pixel count and focal lengths, every view of `specs` through make_view
// into views[], and no view may share a byte with another view or with one of `inputs` (named by inputs_name in the message).
struct ViewSpec { const bslam_buffer2d* buffer; size_t elem, align; const char* name; };
static int load_views(const bslam_camera4f* cam, std::initializer_list<ViewSpec> specs, std::initializer_list<Img> inputs, const char* inputs_name, Img* views) {
  if (cam->width <= 0 || cam->height <= 0 || (int64_t)cam->width * cam->height > 0x7fffffff)
    return fail(BSLAM_ERR_INVALID_ARGUMENT, "the camera must have between 1 and 2^31 - 1 pixels");
  if (!finite_positive(cam->fx) || !finite_positive(cam->fy)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "focal lengths must be positive");
  int n = 0, rc;
  for (const ViewSpec& s : specs)
    if ((rc = make_view(s.buffer, s.elem, s.align, s.name, cam, &views[n++]))) return rc;
  for (int a = 0; a < n; ++a) {   // an absent view is an empty Img, which overlaps nothing
    for (const Img& in : inputs)
      if (overlap(views[a], in)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "an output view overlaps %s", inputs_name);
    for (int b = a + 1; b < n; ++b)
      if (overlap(views[a], views[b])) return fail(BSLAM_ERR_INVALID_ARGUMENT, "two output views overlap");
  }
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
  if ((rc = load_views(camera, {{out_depth, 2, 2, "depth view"}, {out_index, 4, 4, "index view"}, {out_color, 4, 4, "colour view"}, {out_normal, 12, 4, "normal view"}},
                       {rows_img}, "the surfel rows", view))) return rc;
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
