// render_mesh_abi.inc -- mesh view entry points of include/badslam_hip.h (included by badslam_hip.hip after render_abi.inc and
// mesh_abi.inc: load_views, the mesh spans and the error word).

extern "C" {

int bslam_set_render_mesh_tuning(bslam_context* ctx, int small_box, int wave_box, int project_once, int resolve_reads_projected) {
  if (!ctx) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null context");
  if (small_box < 0 || wave_box < 0) return fail(BSLAM_ERR_INVALID_ARGUMENT, "small_box and wave_box must be >= 0");
  if (resolve_reads_projected && !project_once) return fail(BSLAM_ERR_INVALID_ARGUMENT, "the resolve pass can only read projected vertices that the vertex pass wrote");
  ctx->render_mesh_small_box = small_box;
  ctx->render_mesh_wave_box = wave_box;
  ctx->render_mesh_project_once = project_once != 0;
  ctx->render_mesh_resolve_projected = resolve_reads_projected != 0;
  return BSLAM_OK;
}

int bslam_render_mesh(bslam_context* ctx, void* stream_, const bslam_mat3x4* camera_T_global, const bslam_camera4f* camera, uint32_t vertex_count,
                      const float* positions, const float* normals, const void* colors, uint32_t triangle_count, const uint32_t* indices, float min_depth,
                      float max_depth, int cull_backfaces, float metres_to_depth, const bslam_buffer2d* out_depth, const bslam_buffer2d* out_index,
                      const bslam_buffer2d* out_color, const bslam_buffer2d* out_normal) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !camera_T_global || !camera) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (!out_depth && !out_index && !out_color && !out_normal) return fail(BSLAM_ERR_INVALID_ARGUMENT, "no output view was asked for");
  if (out_color && !colors) return fail(BSLAM_ERR_INVALID_ARGUMENT, "a colour view needs vertex colours");
  if (!finite_positive(min_depth) || !finite_positive(max_depth) || !finite_positive(metres_to_depth))
    return fail(BSLAM_ERR_INVALID_ARGUMENT, "min_depth, max_depth and metres_to_depth must be finite and > 0");
  if (min_depth > max_depth) return fail(BSLAM_ERR_INVALID_ARGUMENT, "need min_depth <= max_depth");
  if (cull_backfaces != 0 && cull_backfaces != 1) return fail(BSLAM_ERR_INVALID_ARGUMENT, "cull_backfaces must be 0 or 1");
  const size_t V = vertex_count, T = triangle_count;
  const MeshSpan spans[4] = {{positions, 12 * V, "positions", false}, {normals, normals ? 12 * V : 0, "normals", false}, {colors, colors ? 4 * V : 0, "colors", false},
                             {indices, 12 * T, "indices", false}};
  int rc = check_mesh_spans(spans, 4);
  if (rc) return rc;
  Img view[4];
  if ((rc = load_views(camera, {{out_depth, 2, 2, "depth view"}, {out_index, 4, 4, "index view"}, {out_color, 4, 4, "colour view"}, {out_normal, 12, 4, "normal view"}}, {},
                       "the mesh", view))) return rc;
  for (const Img& v : view) {   // an absent view is an empty Img, which overlaps nothing
    const uintptr_t v0 = (uintptr_t)v.base, v1 = v0 + (size_t)v.height * v.pitch;
    for (const MeshSpan& s : spans)
      if (s.bytes != 0 && v0 < (uintptr_t)s.ptr + s.bytes && (uintptr_t)s.ptr < v1) return fail(BSLAM_ERR_INVALID_ARGUMENT, "an output view overlaps %s", s.name);
  }
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const int pixels = camera->width * camera->height;
  const bool draw = V != 0 && T != 0, project_once = draw && ctx->render_mesh_project_once;
  // scratch: keys u64[pixels] | words u32[16] = {error bits, queued triangles} | queue u32[T] | projected RasterVertex[V], when the vertex pass runs
  const bool use_queue = draw && ctx->render_mesh_wave_box != INT_MAX;
  unsigned long long* keys = nullptr;
  uint32_t *words = nullptr, *queue = nullptr;
  RasterVertex* projected = nullptr;
  if ((rc = carve(ctx->zbuffer, [&](Carver& c) {
         keys = c.take<unsigned long long>((size_t)pixels); words = c.take<uint32_t>(16); queue = c.take<uint32_t>(use_queue ? T : 0);
         projected = project_once ? c.take<RasterVertex>(V, 16) : nullptr;
       }))) return rc;
  MeshView mesh{positions, normals, (const uint32_t*)colors, indices, nullptr, vertex_count, triangle_count};
  const dim3 block(256);
  BSLAM_HIP_TRY(hipMemsetAsync(words, 0, 2 * sizeof(uint32_t), stream));
  hipLaunchKernelGGL(render_clear_kernel, flat_grid((size_t)pixels), block, 0, stream, keys, pixels);
  if (project_once) hipLaunchKernelGGL(render_mesh_vertex_kernel, flat_grid(V), block, 0, stream, mesh, *camera_T_global, *camera, projected);
  mesh.projected = projected;
  if (draw)
    hipLaunchKernelGGL(render_mesh_draw_kernel, flat_grid(T), block, 0, stream, mesh, *camera_T_global, *camera, min_depth, max_depth, cull_backfaces,
                       ctx->render_mesh_small_box, ctx->render_mesh_wave_box, keys, words, queue);
  if (use_queue)
    hipLaunchKernelGGL(render_mesh_queue_kernel, dim3(kMeshQueueBlocks), block, 0, stream, mesh, *camera_T_global, *camera, min_depth, max_depth, cull_backfaces, keys,
                       (const uint32_t*)words, (const uint32_t*)queue);
  if (!ctx->render_mesh_resolve_projected) mesh.projected = nullptr;
  hipLaunchKernelGGL(render_mesh_resolve_kernel, dim3((unsigned)((camera->width + 255) / 256), (unsigned)camera->height), block, 0, stream,
                     (const unsigned long long*)keys, mesh, *camera_T_global, *camera, metres_to_depth, view[0], view[1], view[2], view[3]);
  BSLAM_HIP_TRY(hipGetLastError());
  if (V == 0) return empty_mesh(stream, T, "bslam_render_mesh");   // the views are empty; any triangle names a vertex that does not exist
  const uint32_t* host = nullptr;
  if ((rc = read_back(ctx, stream, (const uint32_t*)words, 1, &host))) return rc;
  return mesh_error(host[0], "bslam_render_mesh");
}

}  // extern "C"
