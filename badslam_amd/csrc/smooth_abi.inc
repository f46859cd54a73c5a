// smooth_abi.inc -- bslam_smooth_mesh of include/badslam_hip.h (included by badslam_hip.hip after mesh_abi.inc:
// check_mesh_spans, mesh_error, empty_mesh, pad64, vertex_id_bits, mesh_sort; device_scan, flat_grid, read_back, carve).

extern "C" {

int bslam_smooth_mesh(bslam_context* ctx, void* stream_, uint32_t vertex_count, uint32_t triangle_count, const float* positions, const float* normals,
                      const uint32_t* indices, uint32_t iterations, float lambda, float mu, uint32_t boundary_mode, float* out_positions, float* out_normals) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* call = "bslam_smooth_mesh";
  if (!ctx) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (!std::isfinite(lambda) || !(lambda > 0.f && lambda <= 1.f)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "lambda must be finite and lie in (0, 1]");
  if (!std::isfinite(mu) || !(mu >= -1.f && mu <= 0.f)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "mu must be finite and lie in [-1, 0]");
  if (boundary_mode > 2u) return fail(BSLAM_ERR_INVALID_ARGUMENT, "boundary_mode must be 0 (fixed), 1 (rim) or 2 (free)");
  if (iterations > 65535u) return fail(BSLAM_ERR_INVALID_ARGUMENT, "more than 65535 iterations");
  const size_t V = vertex_count, T = triangle_count;
  // one thread per vertex / per directed pair (six per triangle) in blocks of 256, and a scan of 32-bit ranks over the pairs
  if (V > 0xffffff00ull || 6 * T > 0xffffff00ull) return fail(BSLAM_ERR_INVALID_ARGUMENT, "more than 2^32 - 256 vertices or adjacency entries");
  const MeshSpan spans[5] = {{positions, 12 * V, "positions", false}, {normals, normals ? 12 * V : 0, "normals", false}, {indices, 12 * T, "indices", false},
                             {out_positions, 12 * V, "out_positions", true}, {out_normals, out_normals ? 12 * V : 0, "out_normals", true}};
  int rc = check_mesh_spans(spans, 5);
  if (rc) return rc;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  for (float& ms : ctx->smooth_stage_ms) ms = 0.f;
  if (V == 0) return empty_mesh(stream, T, call);
  const unsigned bits = vertex_id_bits(V);
  const uint32_t steps = T == 0 ? 0u : iterations * (mu != 0.f ? 2u : 1u);
  const bool fans = T != 0 && out_normals != nullptr;
  // scratch: words | per directed pair (P = 6 T): keys, sorted keys, ids, slots, head flags, ranks, neighbours, rim flags | per corner (3 T), when
  //          normals are asked for: keys, sorted keys, the fans | per vertex: list and fan ends, boundary flags | the working positions of the steps
  //          between the first and the last | scan sums | the sort's own
  const size_t P = 6 * T, C3 = fans ? 3 * T : 0, nv = pad64(V), np = pad64(P), nc = pad64(C3), tiles = np / kScanTile + 2;
  size_t sort_bytes = 0;
  if ((rc = mesh_sort_bytes(std::max<size_t>(P, 1), stream, &sort_bytes))) return rc;
  SmoothState s = {};
  uint32_t* tile_sums;
  uint8_t* sort_temp;
  float* work[2] = {nullptr, nullptr};
  if ((rc = carve(ctx->smooth, [&](Carver& c) {
         s.words = c.take<uint32_t>(kSmoothWords, 16);
         s.pair_keys = c.take<unsigned long long>(np, 64); s.sorted_pairs = c.take<unsigned long long>(np, 64); s.ids = c.take<uint32_t>(np, 64);
         s.pair_slots = c.take<uint32_t>(np, 64); s.head = c.take<uint8_t>(np, 64); s.rank = c.take<uint32_t>(np, 64); s.neighbour = c.take<uint32_t>(np, 64);
         s.single = c.take<uint8_t>(np, 64);
         if (fans) { s.fan_keys = c.take<unsigned long long>(nc, 64); s.sorted_fans = c.take<unsigned long long>(nc, 64); s.fan = c.take<uint32_t>(nc, 64); }
         s.list_start = c.take<uint32_t>(nv, 64); s.list_end = c.take<uint32_t>(nv, 64); s.fan_start = c.take<uint32_t>(nv, 64); s.fan_end = c.take<uint32_t>(nv, 64);
         s.boundary = c.take<uint8_t>(nv, 64);
         if (steps >= 2) work[0] = c.take<float>(3 * nv, 64);
         if (steps >= 3) work[1] = c.take<float>(3 * nv, 64);
         tile_sums = c.take<uint32_t>(tiles, 16); sort_temp = c.take<uint8_t>(sort_bytes, 256);
       }))) return rc;
  s.vertices = vertex_count; s.triangles = triangle_count; s.pairs = (uint32_t)P; s.corners = (uint32_t)(3 * T); s.bits = bits; s.tri = indices;
  const dim3 block(256);
  BSLAM_HIP_TRY(hipMemsetAsync(s.words, 0, kSmoothWords * sizeof(uint32_t), stream));
  if ((rc = ctx->smooth_events.mark(ctx->profiling, stream, 0))) return rc;
  hipLaunchKernelGGL(mesh_check_positions_kernel, flat_grid(V), block, 0, stream, vertex_count, positions, s.words + kSmoothError);
  BSLAM_HIP_TRY(hipGetLastError());
  if (T != 0) {
    hipLaunchKernelGGL(smooth_keys_kernel, flat_grid(T), block, 0, stream, s);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  if ((rc = ctx->smooth_events.mark(ctx->profiling, stream, 1))) return rc;
  if (T != 0) {
    // stable: the fan of a vertex stays in ascending slot, so in ascending triangle
    if ((rc = mesh_sort(call, sort_temp, sort_bytes, s.pair_keys, s.sorted_pairs, s.ids, s.pair_slots, P, 2 * bits, stream))) return rc;
    if (fans && (rc = mesh_sort(call, sort_temp, sort_bytes, s.fan_keys, s.sorted_fans, s.ids, s.fan, 3 * T, bits + 1, stream))) return rc;
  }
  if ((rc = ctx->smooth_events.mark(ctx->profiling, stream, 2))) return rc;
  if (T != 0) {
    BSLAM_HIP_TRY(hipMemsetAsync(s.list_start, 0, V * sizeof(uint32_t), stream));
    BSLAM_HIP_TRY(hipMemsetAsync(s.list_end, 0, V * sizeof(uint32_t), stream));
    BSLAM_HIP_TRY(hipMemsetAsync(s.boundary, 0, V, stream));
    hipLaunchKernelGGL(smooth_heads_kernel, flat_grid(P), block, 0, stream, s);
    BSLAM_HIP_TRY(hipGetLastError());
    if ((rc = device_scan(stream, 0, s.head, s.pairs, false, s.rank, tile_sums, s.words + kSmoothPairs))) return rc;
    hipLaunchKernelGGL(smooth_lists_kernel, flat_grid(P), block, 0, stream, s);
    BSLAM_HIP_TRY(hipGetLastError());
    if (fans) {
      BSLAM_HIP_TRY(hipMemsetAsync(s.fan_start, 0, V * sizeof(uint32_t), stream));
      BSLAM_HIP_TRY(hipMemsetAsync(s.fan_end, 0, V * sizeof(uint32_t), stream));
      hipLaunchKernelGGL(smooth_fans_kernel, flat_grid(3 * T), block, 0, stream, s);
      BSLAM_HIP_TRY(hipGetLastError());
    }
  }
  if ((rc = ctx->smooth_events.mark(ctx->profiling, stream, 3))) return rc;
  // the one read-back: nothing is written to the outputs before the error word is known
  const uint32_t* host = nullptr;
  if ((rc = read_back(ctx, stream, (const uint32_t*)s.words, 2, &host))) return rc;
  if ((rc = mesh_error(host[kSmoothError], call))) return rc;
  if ((rc = ctx->smooth_events.mark(ctx->profiling, stream, 4))) return rc;
  if (steps == 0) {
    BSLAM_HIP_TRY(hipMemcpyAsync(out_positions, positions, 12 * V, hipMemcpyDeviceToDevice, stream));
  } else {
    const float* from = positions;
    for (uint32_t k = 0; k < steps; ++k) {
      float* to = k + 1 == steps ? out_positions : work[k & 1u];
      const float factor = (mu != 0.f && (k & 1u)) ? mu : lambda;
      hipLaunchKernelGGL(smooth_step_kernel, flat_grid(V), block, 0, stream, s, from, to, (double)factor, boundary_mode);
      BSLAM_HIP_TRY(hipGetLastError());
      from = to;
    }
  }
  if ((rc = ctx->smooth_events.mark(ctx->profiling, stream, 5))) return rc;
  if (out_normals != nullptr) {
    hipLaunchKernelGGL(smooth_normals_kernel, flat_grid(V), block, 0, stream, s, (const float*)out_positions, normals, out_normals, fans ? 1 : 0);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  if ((rc = ctx->smooth_events.mark(ctx->profiling, stream, 6))) return rc;
  BSLAM_HIP_TRY(hipStreamSynchronize(stream));
  if (ctx->profiling) {
    const int from[5] = {0, 1, 2, 4, 5};
    for (int st = 0; st < 5; ++st)
      if ((rc = ctx->smooth_events.elapsed(from[st], from[st] + 1, &ctx->smooth_stage_ms[st]))) return rc;
  }
  return BSLAM_OK;
}

int bslam_smooth_stage_times(bslam_context* ctx, float* stage_ms5) {
  if (!ctx || !stage_ms5) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  std::memcpy(stage_ms5, ctx->smooth_stage_ms, sizeof(ctx->smooth_stage_ms));
  return BSLAM_OK;
}

}  // extern "C"
