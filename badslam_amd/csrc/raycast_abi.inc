// raycast_abi.inc -- surface view entry points of include/badslam_hip.h (included by badslam_hip.hip after render_abi.inc
// and fusion_abi.inc, whose argument helpers it uses).

namespace bslam {

// Layout of the caller's aux buffer: block flags, padded to 256 bytes, then the validity words.
struct RayAuxLayout {
  uint32_t words_x, groups_y, groups_z;   // 64-cell words per row; groups (and blocks) of 8 cells along y and z
  size_t flag_bytes, bits_offset, bytes;
};
static RayAuxLayout ray_aux_layout(const VolumeDev& v) {
  RayAuxLayout l;
  l.words_x = (uint32_t)(v.nx - 1 + 63) / 64;
  l.groups_y = (uint32_t)(v.ny - 1 + 7) / 8;
  l.groups_z = (uint32_t)(v.nz - 1 + 7) / 8;
  l.flag_bytes = (size_t)l.words_x * l.groups_y * l.groups_z;
  l.bits_offset = (l.flag_bytes + 255) & ~(size_t)255;
  l.bytes = l.bits_offset + (size_t)l.words_x * (size_t)(v.ny - 1) * (size_t)(v.nz - 1) * sizeof(unsigned long long);
  return l;
}

// The aux bytes as an image of one row (more beyond 2^32 - 1 bytes), for the overlap tests.
static Img aux_img(const void* aux, size_t bytes) {
  Img a;
  a.base = (uint8_t*)aux; a.pitch = (uint32_t)std::min<size_t>(bytes, 0xffffffffu); a.width = 0; a.height = (int)((bytes + a.pitch - 1) / a.pitch);
  return a;
}

// N = the number of k >= 0 with fmaf(float(k), step, min_depth) <= max_depth (t is monotone in k); refused above kRayMaxSamples.
static int ray_sample_count(float min_depth, float max_depth, float step, int* out) {
  const double estimate = std::floor(((double)max_depth - (double)min_depth) / (double)step);
  if (!(estimate <= (double)kRayMaxSamples + 2.0)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "more than %d samples per ray: raise step or narrow the depth range", kRayMaxSamples);
  int n = (int)estimate + 1;
  while (n > 1 && std::fmaf((float)(n - 1), step, min_depth) > max_depth) --n;
  while (n <= kRayMaxSamples && std::fmaf((float)n, step, min_depth) <= max_depth) ++n;
  if (n > kRayMaxSamples) return fail(BSLAM_ERR_INVALID_ARGUMENT, "more than %d samples per ray: raise step or narrow the depth range", kRayMaxSamples);
  *out = n;
  return BSLAM_OK;
}

}  // namespace bslam

extern "C" {

int bslam_volume_views_aux_bytes(const bslam_volume* volume, size_t* bytes) {
  if (!bytes) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  VolumeDev vol;
  int rc = check_volume(volume, &vol);
  if (rc) return rc;
  *bytes = ray_aux_layout(vol).bytes;
  return BSLAM_OK;
}

int bslam_prepare_volume_views(bslam_context* ctx, void* stream_, const bslam_volume* volume, const bslam_buffer2d* tsdf, const bslam_buffer2d* count,
                               uint32_t min_count, void* aux, size_t aux_bytes) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !tsdf || !count || !aux) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (min_count < 1) return fail(BSLAM_ERR_INVALID_ARGUMENT, "min_count must be >= 1");
  VolumeArgs v;
  int rc = load_volume(volume, tsdf, count, nullptr, &v);
  if (rc) return rc;
  const RayAuxLayout l = ray_aux_layout(v.vol);
  if ((uintptr_t)aux % 8 != 0) return fail(BSLAM_ERR_INVALID_ARGUMENT, "the aux buffer must be 8 byte aligned");
  if (aux_bytes < l.bytes) return fail(BSLAM_ERR_INVALID_ARGUMENT, "the aux buffer has %zu bytes, the volume needs %zu", aux_bytes, l.bytes);
  const Img a = aux_img(aux, l.bytes);
  if (overlap(a, v.tsdf) || overlap(a, v.count)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "the aux buffer overlaps a volume");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  // <= 2^30 / 8 / 8 / 2 groups: words_x * 64 <= nx + 62 and every dimension is >= 2
  hipLaunchKernelGGL(raycast_prepare_kernel, dim3((unsigned)l.flag_bytes), dim3(256), 0, stream, v.vol, v.tsdf, v.count, min_count, l.words_x, l.groups_y,
                     (unsigned long long*)((uint8_t*)aux + l.bits_offset), (uint8_t*)aux);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_raycast_volume(bslam_context* ctx, void* stream_, const bslam_volume* volume, const bslam_buffer2d* tsdf, const bslam_buffer2d* color, const void* aux,
                         const bslam_mat3x4* global_T_camera, const bslam_camera4f* camera, float min_depth, float max_depth, float step, float metres_to_depth,
                         const bslam_buffer2d* out_depth, const bslam_buffer2d* out_color, const bslam_buffer2d* out_normal) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !tsdf || !aux || !global_T_camera || !camera) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (!out_depth && !out_color && !out_normal) return fail(BSLAM_ERR_INVALID_ARGUMENT, "no output view was asked for");
  VolumeArgs v;
  int rc = load_volume(volume, tsdf, nullptr, color, &v);
  if (rc) return rc;
  const VolumeDev& vol = v.vol;
  if (!finite_positive(step) || !finite_positive(metres_to_depth)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "step and metres_to_depth must be finite and > 0");
  if (!finite_positive(min_depth) || !finite_positive(max_depth) || !(min_depth < max_depth)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "need 0 < min_depth < max_depth, both finite");
  RayParams p;
  if ((rc = ray_sample_count(min_depth, max_depth, step, &p.samples))) return rc;
  if ((uintptr_t)aux % 8 != 0) return fail(BSLAM_ERR_INVALID_ARGUMENT, "the aux buffer must be 8 byte aligned");
  const RayAuxLayout l = ray_aux_layout(vol);
  Img view[3];
  if ((rc = load_views(camera, {{out_depth, 2, 2, "depth view"}, {out_color, 4, 4, "colour view"}, {out_normal, 12, 4, "normal view"}},
                       {v.tsdf, v.color, aux_img(aux, l.bytes)}, "the volume or the aux buffer", view))) return rc;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  p.min_depth = min_depth; p.step = step; p.metres_to_depth = metres_to_depth;
  p.inv_voxel = 1.0f / vol.voxel;   // IEEE single division on the host
  p.widen = (int)std::min(std::ceil(1.1920928955078125e-07 * (double)max_depth / (double)step) + 2.0, (double)kRayMaxSamples);
  p.fnx = (float)(vol.nx - 2); p.fny = (float)(vol.ny - 2); p.fnz = (float)(vol.nz - 2);
  RayAux ra;
  ra.flags = (const uint8_t*)aux;
  ra.bits = (const uint32_t*)((const uint8_t*)aux + l.bits_offset);
  ra.words_x = l.words_x; ra.groups_x = l.words_x; ra.blocks_y = l.groups_y;
  const RayCam cam{camera->fx, camera->fy, camera->cx, camera->cy, camera->width, camera->height};
  const uint32_t tiles_x = (uint32_t)(camera->width + 15) / 16, tiles_y = (uint32_t)(camera->height + 15) / 16;   // <= 2^31 / 16 tiles in all
  hipLaunchKernelGGL(raycast_march_kernel, dim3(tiles_x * tiles_y), dim3(256), 0, stream, *global_T_camera, cam, vol, p, ra, ctx->culling ? 1 : 0, tiles_x, v.tsdf, v.color,
                     view[0], view[1], view[2], cull_stats_ptr(ctx));
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

}  // extern "C"
