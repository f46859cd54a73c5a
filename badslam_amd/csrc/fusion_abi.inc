// fusion_abi.inc -- volumetric fusion and mesh extraction entry points of include/badslam_hip.h (included by badslam_hip.hip
// after lifecycle_abi.inc, whose device_scan it uses).

namespace bslam {

constexpr int64_t kMaxVoxels = (int64_t)1 << 30;

static int check_volume(const bslam_volume* v, VolumeDev* out) {
  if (!v) return fail(BSLAM_ERR_INVALID_ARGUMENT, "volume is null");
  if (!finite_positive(v->voxel_size)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "voxel_size must be finite and > 0");
  for (int i = 0; i < 3; ++i)
    if (!(std::fabs(v->origin[i]) <= 3.4028235e38f)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "the volume's origin must be finite");
  if (v->nx < 2 || v->ny < 2 || v->nz < 2) return fail(BSLAM_ERR_INVALID_ARGUMENT, "every volume dimension must be >= 2");
  if ((int64_t)v->nx * v->ny > kMaxVoxels || (int64_t)v->nx * v->ny * v->nz > kMaxVoxels)
    return fail(BSLAM_ERR_INVALID_ARGUMENT, "a volume of %d x %d x %d voxels exceeds 2^30", v->nx, v->ny, v->nz);
  out->ox = v->origin[0]; out->oy = v->origin[1]; out->oz = v->origin[2]; out->voxel = v->voxel_size;
  out->nx = v->nx; out->ny = v->ny; out->nz = v->nz;
  return BSLAM_OK;
}

// A volume buffer of 4-byte elements: nz * ny rows of nx elements, rows 4 byte aligned.
static int make_volume_img(const bslam_buffer2d* b, const VolumeDev& v, const char* name, Img* out) {
  int rc = make_img(b, 4, name, out);
  if (rc) return rc;
  if (out->width != v.nx || out->height != v.nz * v.ny) return fail(BSLAM_ERR_INVALID_ARGUMENT, "%s must have nz * ny = %d rows of nx = %d elements", name, v.nz * v.ny, v.nx);
  if (b->pitch > 0xffffffffu || !rows_aligned(*out, 4)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "%s rows must be 4 byte aligned", name);
  return BSLAM_OK;
}

// A volume and its buffers as a call takes them: the tsdf image always, the count and colour images where given; an absent one
// stays an empty Img, which overlaps nothing.
struct VolumeArgs { VolumeDev vol; Img tsdf, count, color; };
static int load_volume(const bslam_volume* v, const bslam_buffer2d* tsdf, const bslam_buffer2d* count, const bslam_buffer2d* color, VolumeArgs* out) {
  *out = VolumeArgs{};
  int rc = check_volume(v, &out->vol);
  if (rc) return rc;
  if ((rc = make_volume_img(tsdf, out->vol, "tsdf volume", &out->tsdf))) return rc;
  if (count && (rc = make_volume_img(count, out->vol, "count volume", &out->count))) return rc;
  if (color && (rc = make_volume_img(color, out->vol, "colour volume", &out->color))) return rc;
  return BSLAM_OK;
}

}  // namespace bslam

extern "C" {

int bslam_fuse_keyframes(bslam_context* ctx, void* stream_, const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera,
                         const bslam_depth_params* depth_params, int keyframe_count, const bslam_keyframe_view* keyframes, const bslam_volume* volume,
                         float truncation, const bslam_buffer2d* tsdf, const bslam_buffer2d* count, const bslam_buffer2d* color) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !depth_camera || !depth_params || !tsdf || !count) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (color && !color_camera) return fail(BSLAM_ERR_INVALID_ARGUMENT, "a colour volume needs the colour camera");
  VolumeArgs v;
  int rc = load_volume(volume, tsdf, count, color, &v);
  if (rc) return rc;
  const VolumeDev& vol = v.vol;
  if (!finite_positive(truncation)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "truncation must be finite and > 0");
  if (overlap(v.tsdf, v.count) || overlap(v.tsdf, v.color) || overlap(v.count, v.color)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "two output volumes overlap");
  // The keyframe list goes through the setup of every call that walks one; fusion reads no surfels, so it hands that setup an
  // empty surfel buffer of the required height.
  bslam_buffer2d no_surfels;
  no_surfels.address = nullptr; no_surfels.height = BSLAM_SURFEL_DATA_ATTRIBUTE_COUNT; no_surfels.width = 0; no_surfels.pitch = 0;
  CamConsts c;
  if ((rc = setup_keyframe_table(ctx, stream, color_camera, depth_camera, depth_params, keyframe_count, keyframes, color != nullptr, 0, &no_surfels, &c))) return rc;
  const uint32_t bricks_x = (uint32_t)(vol.nx + kBrickX - 1) / kBrickX, bricks_y = (uint32_t)(vol.ny + kBrickY - 1) / kBrickY,
                 bricks_z = (uint32_t)(vol.nz + kBrickZ - 1) / kBrickZ;
  const dim3 grid(bricks_x * bricks_y * bricks_z);   // <= 2^30 / 2 bricks (every dimension is >= 2)
  if (color)
    hipLaunchKernelGGL(fuse_keyframes_kernel<true>, grid, dim3(256), 0, stream, c, (const KfDev*)ctx->kf_table.ptr, keyframe_count, vol, truncation,
                       ctx->culling ? 1 : 0, bricks_x, bricks_y, v.tsdf, v.count, v.color, cull_stats_ptr(ctx));
  else
    hipLaunchKernelGGL(fuse_keyframes_kernel<false>, grid, dim3(256), 0, stream, c, (const KfDev*)ctx->kf_table.ptr, keyframe_count, vol, truncation,
                       ctx->culling ? 1 : 0, bricks_x, bricks_y, v.tsdf, v.count, v.color, cull_stats_ptr(ctx));
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_extract_mesh(bslam_context* ctx, void* stream_, const bslam_volume* volume, const bslam_buffer2d* tsdf, const bslam_buffer2d* count,
                       const bslam_buffer2d* color, uint32_t min_count, uint32_t vertex_capacity, uint32_t triangle_capacity, float* positions,
                       float* normals, void* colors, uint32_t* indices, uint32_t* vertex_count, uint32_t* triangle_count) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !tsdf || !count || !vertex_count || !triangle_count) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (min_count < 1) return fail(BSLAM_ERR_INVALID_ARGUMENT, "min_count must be >= 1");
  VolumeArgs v;
  int rc = load_volume(volume, tsdf, count, color, &v);
  if (rc) return rc;
  MeshVolume m;
  m.vol = v.vol; m.tsdf = v.tsdf; m.count = v.count; m.color = v.color;
  m.min_count = min_count;
  m.cells = (uint32_t)(m.vol.nx - 1) * (uint32_t)(m.vol.ny - 1) * (uint32_t)(m.vol.nz - 1);
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  // scratch: active u8[cells] | quads u8[cells] | vertex_id u32[cells] | quad_offset u32[cells] | tile sums | totals u32[2]
  const size_t n = ((size_t)m.cells + 63) & ~(size_t)63, tiles = n / kScanTile + 2;   // the cells padded to 64: every array starts 64 byte aligned
  uint8_t *active, *quads;
  uint32_t *vertex_id, *quad_offset, *tile_sums, *totals;
  if ((rc = carve(ctx->fusion, [&](Carver& c) {
         active = c.take<uint8_t>(n, 64); quads = c.take<uint8_t>(n, 64); vertex_id = c.take<uint32_t>(n, 64); quad_offset = c.take<uint32_t>(n, 64);
         tile_sums = c.take<uint32_t>(tiles); totals = c.take<uint32_t>(16);
       }))) return rc;
  const dim3 grid = flat_grid(m.cells), block(256);
  hipLaunchKernelGGL(mesh_flag_cells_kernel, grid, block, 0, stream, m, active);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = device_scan(stream, 0, active, m.cells, true, vertex_id, tile_sums, totals))) return rc;
  hipLaunchKernelGGL(mesh_count_quads_kernel, grid, block, 0, stream, m, (const uint8_t*)active, quads);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = device_scan(stream, 0, quads, m.cells, true, quad_offset, tile_sums, totals + 1))) return rc;
  const uint32_t* host = nullptr;
  if ((rc = read_back(ctx, stream, (const uint32_t*)totals, 2, &host))) return rc;
  const uint32_t vertices = host[0], quad_total = host[1];
  if (quad_total > 0x7fffffffu) return fail(BSLAM_ERR_INVALID_ARGUMENT, "the mesh has more than 2^32 - 1 triangles");
  *vertex_count = vertices;
  *triangle_count = 2 * quad_total;
  if (!positions || !indices || vertices > vertex_capacity || 2 * quad_total > triangle_capacity || vertices == 0) return BSLAM_OK;   // counts only
  hipLaunchKernelGGL(mesh_emit_kernel, grid, block, 0, stream, m, (const uint8_t*)active, (const uint32_t*)vertex_id, (const uint32_t*)quad_offset, positions,
                     normals, m.color.base ? (uint32_t*)colors : nullptr, indices);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

}  // extern "C"
