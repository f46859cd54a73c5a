// bvh_abi.inc -- bslam_nearest_triangle and bslam_debug_nearest_triangle_tree of include/badslam_hip.h (included by badslam_hip.hip
// after distance_abi.inc: pmd_unkey, pmd_miss_kernel; mesh_abi.inc: check_mesh_spans, mesh_error, empty_mesh, mesh_sort; flat_grid,
// read_back, carve, cull_stats_ptr).  The build and the query are separate functions: a later call may keep a tree.

namespace bslam {

// The triangle side: census (one read-back), keys, the sort, the radix tree, the boxes and the packed nodes, into ctx->bvh; fills
// ctx->bvh_tree.  tree.leaves == 0: no valid triangle, nothing was built.  Nothing is synchronised behind the census.
static int bvh_build(bslam_context* ctx, hipStream_t stream, const char* call, uint32_t vertex_count, const float* positions, uint32_t triangle_count,
                     const uint32_t* indices, bool want_height) {
  const dim3 block(256);
  const size_t T = triangle_count;
  bslam_context::BvhTree& tree = ctx->bvh_tree;
  tree = bslam_context::BvhTree();
  int rc;
  if ((rc = ctx->bvh.reserve(kBvhWords * sizeof(uint32_t)))) return rc;
  uint32_t* words = (uint32_t*)ctx->bvh.ptr;
  BSLAM_HIP_TRY(hipMemsetAsync(words, 0, kBvhWords * sizeof(uint32_t), stream));
  BSLAM_HIP_TRY(hipMemsetAsync(words + kBvhMinKey, 0xff, 3 * sizeof(uint32_t), stream));
  hipLaunchKernelGGL(bvh_census_kernel, flat_grid(T), block, 0, stream, vertex_count, triangle_count, positions, indices, words);
  BSLAM_HIP_TRY(hipGetLastError());
  const uint32_t* host = nullptr;
  if ((rc = read_back(ctx, stream, (const uint32_t*)words, (size_t)kBvhWords, &host))) return rc;
  if ((rc = mesh_error(host[kBvhError], call))) return rc;
  const size_t L = host[kBvhValid];
  if (L == 0) return BSLAM_OK;
  // a child reference keeps its top bit for the leaf flag
  if (L > 0x80000000ull) return fail(BSLAM_ERR_INVALID_ARGUMENT, "%s: %zu valid triangles, more than the 2^31 a tree holds", call, L);
  BvhQuantiser qz;
  for (int a = 0; a < 3; ++a) {
    qz.origin[a] = pmd_unkey(host[kBvhMinKey + a]);
    const float extent = pmd_unkey(host[kBvhMaxKey + a]) - qz.origin[a];
    const float scale = (float)(1 << kBvhAxisBits) / extent;
    qz.scale[a] = extent > 0.f && std::isfinite(extent) && std::isfinite(scale) ? scale : 0.f;
  }
  // scratch (every piece 64 byte aligned): words | keys, sorted keys u64[T] | ids, sorted ids u32[T] | parents u32[L - 1], u32[L] |
  //   children u32[2 (L - 1)] | box keys u32[3 (L - 1)] twice | leaf boxes f32[3 L] twice | nodes float4[4 (L - 1)] | records float4[3 L] | the sort's own
  size_t sort_bytes = 0;
  if ((rc = mesh_sort_bytes(T, stream, &sort_bytes))) return rc;
  unsigned long long *keys, *sorted_keys;
  uint32_t *ids, *sorted_ids;
  uint8_t* sort_temp;
  BvhBuild b;
  b.leaves = (uint32_t)L;
  if ((rc = carve(ctx->bvh, [&](Carver& c) {
         words = c.take<uint32_t>(kBvhWords, 64); keys = c.take<unsigned long long>(T, 64); sorted_keys = c.take<unsigned long long>(T, 64);
         ids = c.take<uint32_t>(T, 64); sorted_ids = c.take<uint32_t>(T, 64);
         b.parent_internal = c.take<uint32_t>(L - 1, 64); b.parent_leaf = c.take<uint32_t>(L, 64); b.children = c.take<uint32_t>(2 * (L - 1), 64);
         b.box_min = c.take<uint32_t>(3 * (L - 1), 64); b.box_max = c.take<uint32_t>(3 * (L - 1), 64);
         b.leaf_lo = c.take<float>(3 * L, 64); b.leaf_hi = c.take<float>(3 * L, 64);
         b.nodes = c.take<float4>((size_t)kBvhNodeQuads * (L - 1), 64); b.records = c.take<float4>((size_t)kBvhLeafQuads * L, 64);
         sort_temp = c.take<uint8_t>(sort_bytes, 256);
       }))) return rc;
  b.sorted_keys = sorted_keys;
  b.sorted_ids = sorted_ids;
  BSLAM_HIP_TRY(hipMemsetAsync(words, 0, kBvhWords * sizeof(uint32_t), stream));   // the slab may have moved; kBvhHeight starts at 0
  hipLaunchKernelGGL(bvh_keys_kernel, flat_grid(T), block, 0, stream, qz, vertex_count, triangle_count, positions, indices, keys, ids);
  BSLAM_HIP_TRY(hipGetLastError());
  // stable: equal codes stay in ascending triangle id, and the invalid triangles, of the one key beyond every code, end up behind
  if ((rc = mesh_sort(call, sort_temp, sort_bytes, keys, sorted_keys, ids, sorted_ids, T, kBvhKeyBits + 1, stream))) return rc;
  if (L > 1) {
    hipLaunchKernelGGL(bvh_tree_kernel, flat_grid(L - 1), block, 0, stream, b);
    BSLAM_HIP_TRY(hipGetLastError());
    BSLAM_HIP_TRY(hipMemsetAsync(b.box_min, 0xff, 3 * (L - 1) * sizeof(uint32_t), stream));   // the empty box
    BSLAM_HIP_TRY(hipMemsetAsync(b.box_max, 0, 3 * (L - 1) * sizeof(uint32_t), stream));
  }
  if (want_height) hipLaunchKernelGGL(bvh_boxes_kernel<true>, flat_grid(L), block, 0, stream, b, vertex_count, positions, indices, words);
  else hipLaunchKernelGGL(bvh_boxes_kernel<false>, flat_grid(L), block, 0, stream, b, vertex_count, positions, indices, words);
  BSLAM_HIP_TRY(hipGetLastError());
  if (L > 1) {
    hipLaunchKernelGGL(bvh_pack_kernel, flat_grid(L - 1), block, 0, stream, b);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  tree.leaves = b.leaves;
  tree.words = words; tree.sorted_ids = sorted_ids; tree.parent_internal = b.parent_internal; tree.parent_leaf = b.parent_leaf;
  tree.box_min = b.box_min; tree.box_max = b.box_max; tree.leaf_lo = b.leaf_lo; tree.leaf_hi = b.leaf_hi; tree.nodes = b.nodes; tree.records = b.records;
  return BSLAM_OK;
}

// The point side against ctx->bvh_tree (leaves >= 1).  Nothing is synchronised.
static int bvh_query(bslam_context* ctx, hipStream_t stream, uint32_t point_count, const float* points, float r_squared, float* out_distance, uint32_t* out_triangle) {
  const bslam_context::BvhTree& tree = ctx->bvh_tree;
  BvhQuery q;
  q.points = point_count; q.leaves = tree.leaves; q.xyz = points; q.nodes = (const float4*)tree.nodes; q.records = (const float4*)tree.records;
  q.r_squared = r_squared; q.out_distance = out_distance; q.out_triangle = out_triangle;
  const dim3 grid((unsigned)(((size_t)point_count + kBvhQueryBlock - 1) / kBvhQueryBlock)), block(kBvhQueryBlock);
  if (ctx->profiling) hipLaunchKernelGGL(bvh_query_kernel<true>, grid, block, 0, stream, q, cull_stats_ptr(ctx));
  else hipLaunchKernelGGL(bvh_query_kernel<false>, grid, block, 0, stream, q, (unsigned long long*)nullptr);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

}  // namespace bslam

extern "C" {

int bslam_nearest_triangle(bslam_context* ctx, void* stream_, uint32_t point_count, const float* points, uint32_t vertex_count, const float* positions,
                           uint32_t triangle_count, const uint32_t* indices, float max_distance, float* out_distance, uint32_t* out_triangle, uint32_t* leaves,
                           uint32_t* height) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* call = "bslam_nearest_triangle";
  if (!ctx) return fail(BSLAM_ERR_INVALID_ARGUMENT, "context is null");
  if (!(max_distance > 0.f)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "max_distance must be > 0 (+infinity: no radius)");
  if (!out_distance) return fail(BSLAM_ERR_INVALID_ARGUMENT, "out_distance is null");
  const size_t N = point_count, V = vertex_count, T = triangle_count;
  // one thread per point / per triangle in blocks of 256: the rounded-up thread index has to fit 32 bits
  if (N > 0xffffff00ull || T > 0xffffff00ull) return fail(BSLAM_ERR_INVALID_ARGUMENT, "more than 2^32 - 256 points or triangles");
  const MeshSpan spans[5] = {{points, 12 * N, "points", false}, {positions, 12 * V, "positions", false}, {indices, 12 * T, "indices", false},
                             {out_distance, 4 * N, "out_distance", true}, {out_triangle, out_triangle ? 4 * N : 0, "out_triangle", true}};
  int rc = check_mesh_spans(spans, 5);
  if (rc) return rc;
  const float r_squared = max_distance * max_distance;   // +inf stays +inf
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  if (leaves) *leaves = 0;
  if (height) *height = 0;
  ctx->bvh_tree = bslam_context::BvhTree();
  if (T != 0) {
    if (V == 0) return empty_mesh(stream, T, call);   // every index is beyond
    if ((rc = bvh_build(ctx, stream, call, vertex_count, positions, triangle_count, indices, height != nullptr))) return rc;
  }
  const uint32_t L = ctx->bvh_tree.leaves;
  if (leaves) *leaves = L;
  if (N != 0) {
    if (L == 0) {   // nothing to be near to
      hipLaunchKernelGGL(pmd_miss_kernel, flat_grid(N), dim3(256), 0, stream, point_count, out_distance, out_triangle);
      BSLAM_HIP_TRY(hipGetLastError());
    } else if ((rc = bvh_query(ctx, stream, point_count, points, r_squared, out_distance, out_triangle))) {
      return rc;
    }
  }
  if (height && L != 0) {
    const uint32_t* host = nullptr;
    if ((rc = read_back(ctx, stream, (const uint32_t*)ctx->bvh_tree.words, (size_t)kBvhWords, &host))) return rc;   // waits for the stream
    *height = host[kBvhHeight];
    ctx->bvh_tree.height = host[kBvhHeight];
    return BSLAM_OK;
  }
  BSLAM_HIP_TRY(hipStreamSynchronize(stream));
  return BSLAM_OK;
}

int bslam_debug_nearest_triangle_tree(bslam_context* ctx, uint32_t leaf_capacity, uint32_t* parent, uint32_t* children, float* boxes, uint32_t* leaf_triangle,
                                      uint32_t* leaves) {
  if (!ctx || !leaves) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  const bslam_context::BvhTree& tree = ctx->bvh_tree;
  const size_t L = tree.leaves;
  *leaves = tree.leaves;
  if (L == 0 || L > leaf_capacity) return BSLAM_OK;   // the caller sizes its arrays from *leaves and asks again
  if (!parent || !children || !boxes || !leaf_triangle) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  BSLAM_HIP_TRY(hipDeviceSynchronize());
  const size_t I = L - 1;
  // nodes 0 .. L - 2 are the internal ones, node L - 1 + j is leaf j
  BSLAM_HIP_TRY(hipMemcpy(leaf_triangle, tree.sorted_ids, L * sizeof(uint32_t), hipMemcpyDeviceToHost));
  BSLAM_HIP_TRY(hipMemcpy(parent + I, tree.parent_leaf, L * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (I == 0) {
    parent[0] = kBvhNoNode;
    BSLAM_HIP_TRY(hipMemcpy(boxes, tree.leaf_lo, 3 * sizeof(float), hipMemcpyDeviceToHost));
    BSLAM_HIP_TRY(hipMemcpy(boxes + 3, tree.leaf_hi, 3 * sizeof(float), hipMemcpyDeviceToHost));
    return BSLAM_OK;
  }
  BSLAM_HIP_TRY(hipMemcpy(parent, tree.parent_internal, I * sizeof(uint32_t), hipMemcpyDeviceToHost));
  // the boxes and the children as the query reads them: from the packed nodes.  The root's box, which no node holds, from its keys.
  std::vector<float> nodes(16 * I);
  uint32_t root[6];
  BSLAM_HIP_TRY(hipMemcpy(nodes.data(), tree.nodes, nodes.size() * sizeof(float), hipMemcpyDeviceToHost));
  BSLAM_HIP_TRY(hipMemcpy(root, tree.box_min, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  BSLAM_HIP_TRY(hipMemcpy(root + 3, tree.box_max, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (int a = 0; a < 6; ++a) boxes[a] = pmd_unkey(root[a]);
  for (size_t i = 0; i < I; ++i) {
    const float* n = nodes.data() + 16 * i;
    for (int c = 0; c < 2; ++c) {
      uint32_t ref;
      std::memcpy(&ref, n + 12 + c, sizeof(ref));
      const size_t node = (ref & kBvhLeafBit) ? I + (ref & ~kBvhLeafBit) : ref;
      children[2 * i + c] = (uint32_t)node;
      if (node < I + L && node != 0) std::memcpy(boxes + 6 * node, n + 6 * c, 6 * sizeof(float));
    }
  }
  return BSLAM_OK;
}

}  // extern "C"
