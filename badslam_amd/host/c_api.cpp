// c_api.cpp -- flat C API over bslam_host::DirectBA so that the Python tests (ctypes) and other
// FFIs can drive the C++ host class.  Exceptions never cross the boundary: they are turned into a
// negative return code + bsh_last_error().
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <string>

#include "bad_slam.hpp"
#include "direct_ba.hpp"
#include "io.hpp"
#include "loop_closure.hpp"
#include "pairwise_frame_tracking.hpp"
#include "place_recognition.hpp"
#include "pose_graph.hpp"
#include "rectification.hpp"

using namespace bslam_host;

static thread_local std::string g_err;

#define BSH_TRY(...)                          \
  try { __VA_ARGS__; return 0; }              \
  catch (const std::exception& e) { g_err = e.what(); return -1; } \
  catch (...) { g_err = "unknown exception"; return -1; }

// Copy of a whole vector into a caller's array that may be null (an output that is not wanted).
template <typename T, typename U>
static void copy_out(T* dst, const std::vector<U>& v) { if (dst) std::memcpy(dst, v.data(), v.size() * sizeof(U)); }
static SE3f pose_from7(const float* p) { bslam_se3f q; std::memcpy(q.q, p, 16); std::memcpy(q.t, p + 4, 12); return SE3f::FromPod(q); }
static void pose_to7(const SE3f& T, float* p) { const bslam_se3f q = T.ToPod(); std::memcpy(p, q.q, 16); std::memcpy(p + 4, q.t, 12); }

extern "C" {

const char* bsh_last_error(void) { return g_err.c_str(); }

void* bsh_create(int max_surfel_count, float raw_to_float_depth, float baseline_fx, int sparse_surfel_cell_size,
                 float surfel_merge_dist_factor, int min_obs_boot1, int min_obs_boot2, int min_obs,
                 const float* color_params, int color_w, int color_h, const float* depth_params, int depth_w, int depth_h,
                 int pyramid_level_for_color, int use_depth_residuals, int use_descriptor_residuals, int device) {
  try {
    return new DirectBA(max_surfel_count, raw_to_float_depth, baseline_fx, sparse_surfel_cell_size, surfel_merge_dist_factor, min_obs_boot1,
                        min_obs_boot2, min_obs, PinholeCamera4f(color_w, color_h, color_params), PinholeCamera4f(depth_w, depth_h, depth_params),
                        pyramid_level_for_color, use_depth_residuals != 0, use_descriptor_residuals != 0, nullptr, SE3f(), device);
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}

static std::map<void*, std::unique_ptr<std::ofstream>> g_timings;
void bsh_destroy(void* ba) { delete static_cast<DirectBA*>(ba); g_timings.erase(ba); }

// the kernel library's context of this DirectBA (bslam_profile_* on the BA's own launches)
void* bsh_context(void* ba) { return static_cast<DirectBA*>(ba)->context(); }

int bsh_add_keyframe(void* ba_, void* stream, uint32_t frame_index, float min_depth, float max_depth, const uint16_t* depth,
                     const uint16_t* normals, const uint16_t* radius, const uint8_t* color, const float* pose7) {
  DirectBA* ba = static_cast<DirectBA*>(ba_);
  try {
    auto kf = std::make_shared<Keyframe>(static_cast<hipStream_t>(stream), frame_index, min_depth, max_depth, ba->depth_camera().width(),
                                         ba->depth_camera().height(), depth, normals, radius, reinterpret_cast<const uchar4_t*>(color),
                                         pose_from7(pose7));
    ba->AddKeyframe(kf);
    return kf->id();
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

int bsh_set_surfels(void* ba, void* stream, const float* rows, size_t pitch_bytes, uint32_t count) {
  BSH_TRY(static_cast<DirectBA*>(ba)->SetSurfels(static_cast<hipStream_t>(stream), rows, pitch_bytes, count));
}
int bsh_get_surfels(void* ba, void* stream, float* rows, size_t pitch_bytes, int nrows) {
  BSH_TRY(static_cast<DirectBA*>(ba)->GetSurfels(static_cast<hipStream_t>(stream), rows, pitch_bytes, nrows));
}
int bsh_get_active_surfels(void* ba, void* stream, uint8_t* out) {
  BSH_TRY(static_cast<DirectBA*>(ba)->GetActiveSurfels(static_cast<hipStream_t>(stream), out));
}
uint32_t bsh_surfels_size(void* ba) { return static_cast<DirectBA*>(ba)->surfels_size(); }
int bsh_keyframe_count(void* ba) { return static_cast<int>(static_cast<DirectBA*>(ba)->keyframes().size()); }

int bsh_get_keyframe_pose(void* ba, int id, float* pose7) {
  BSH_TRY(pose_to7(static_cast<DirectBA*>(ba)->keyframes().at(id)->global_T_frame(), pose7));
}
int bsh_set_keyframe_pose(void* ba, int id, const float* pose7) {
  BSH_TRY(static_cast<DirectBA*>(ba)->keyframes().at(id)->set_global_T_frame(pose_from7(pose7)));
}
int bsh_get_keyframe_activation(void* ba, int id) { return static_cast<int>(static_cast<DirectBA*>(ba)->keyframes().at(id)->activation()); }
int bsh_set_keyframe_activation(void* ba, int id, int activation) {
  BSH_TRY(static_cast<DirectBA*>(ba)->keyframes().at(id)->SetActivation(static_cast<Keyframe::Activation>(activation)));
}
int bsh_keyframe_covisibility(void* ba, int id, int* out, int capacity) {
  auto& list = static_cast<DirectBA*>(ba)->keyframes().at(id)->co_visibility_list();
  const int n = static_cast<int>(list.size());
  for (int i = 0; i < n && i < capacity; ++i) out[i] = list[i];
  return n;
}
// Replaces a keyframe's depth / normals image (the reference's tests do this through const_cast, e.g.
// BS/test/test_geometry_optimization_geometric_residual.cc:124-139).
int bsh_upload_keyframe_depth(void* ba, void* stream, int id, const uint16_t* depth) {
  BSH_TRY({
    auto& kf = static_cast<DirectBA*>(ba)->keyframes().at(id);
    kf->mutable_depth_buffer().Upload(static_cast<hipStream_t>(stream), depth, static_cast<size_t>(kf->depth_buffer().width()) * 2);
    static_cast<DirectBA*>(ba)->InvalidateKeyframeCache();
  });
}
int bsh_upload_keyframe_normals(void* ba, void* stream, int id, const uint16_t* normals) {
  BSH_TRY({
    auto& kf = static_cast<DirectBA*>(ba)->keyframes().at(id);
    kf->mutable_normals_buffer().Upload(static_cast<hipStream_t>(stream), normals, static_cast<size_t>(kf->normals_buffer().width()) * 2);
    static_cast<DirectBA*>(ba)->InvalidateKeyframeCache();
  });
}

int bsh_add_keyframe_from_images(void* ba_, void* stream, uint32_t frame_index, const uint16_t* depth, const uint8_t* rgb, const float* pose7) {
  DirectBA* ba = static_cast<DirectBA*>(ba_);
  try {
    return ba->AddKeyframeFromImages(static_cast<hipStream_t>(stream), frame_index, depth, rgb, pose_from7(pose7))->id();
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}
int bsh_get_keyframe_images(void* ba, void* stream, int id, uint16_t* depth, uint16_t* normals, uint16_t* radius, uint8_t* color, float* min_max) {
  BSH_TRY({
    const auto& kf = static_cast<DirectBA*>(ba)->keyframes().at(id);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t w = static_cast<size_t>(kf->depth_buffer().width());
    kf->depth_buffer().Download(s, depth, w * 2);
    kf->normals_buffer().Download(s, normals, w * 2);
    kf->radius_buffer().Download(s, radius, w * 2);
    kf->color_buffer().Download(s, reinterpret_cast<uchar4_t*>(color), static_cast<size_t>(kf->color_buffer().width()) * 4);
    min_max[0] = kf->min_depth();
    min_max[1] = kf->max_depth();
  });
}
// Keyframe management and export (BS/direct_ba.h:95-116, 123-126)
int bsh_keyframe_is_deleted(void* ba, int id) { return static_cast<DirectBA*>(ba)->keyframes().at(id) ? 0 : 1; }
int bsh_delete_keyframe(void* ba, int id) { BSH_TRY(static_cast<DirectBA*>(ba)->DeleteKeyframe(id)); }
int bsh_merge_keyframes(void* ba, void* stream, uint64_t approx_merge_count, int* deleted_ids, int capacity, int* deleted_count) {
  BSH_TRY({
    const std::vector<int> ids = static_cast<DirectBA*>(ba)->MergeKeyframes(static_cast<hipStream_t>(stream), static_cast<size_t>(approx_merge_count));
    for (size_t i = 0; i < ids.size() && static_cast<int>(i) < capacity; ++i) deleted_ids[i] = ids[i];
    *deleted_count = static_cast<int>(ids.size());
  });
}
int bsh_update_keyframe_covisibility(void* ba, int id) {
  BSH_TRY({
    DirectBA* b = static_cast<DirectBA*>(ba);
    if (!b->keyframes().at(id)) throw std::invalid_argument("keyframe was deleted");
    b->UpdateKeyframeCoVisibility(b->keyframes().at(id));
  });
}
int bsh_assign_colors(void* ba, void* stream) { BSH_TRY(static_cast<DirectBA*>(ba)->AssignColors(static_cast<hipStream_t>(stream))); }
// Fills up to `capacity` points; *count receives the number of valid surfels.
int bsh_export_point_cloud(void* ba, void* stream, uint64_t capacity, float* positions, uint8_t* colors, float* normals, uint64_t* count) {
  BSH_TRY({
    DirectBA::PointCloud cloud;
    static_cast<DirectBA*>(ba)->ExportToPointCloud(static_cast<hipStream_t>(stream), &cloud);
    const size_t n = std::min<size_t>(cloud.size(), capacity);
    if (positions) std::memcpy(positions, cloud.positions.data(), n * 3 * sizeof(float));
    if (colors) std::memcpy(colors, cloud.colors.data(), n * 3);
    if (normals) std::memcpy(normals, cloud.normals.data(), n * 3 * sizeof(float));
    *count = cloud.size();
  });
}
// size2: width, height of the depth camera
int bsh_depth_camera_size(void* ba, int* size2) {
  BSH_TRY({
    size2[0] = static_cast<DirectBA*>(ba)->depth_camera().width();
    size2[1] = static_cast<DirectBA*>(ba)->depth_camera().height();
  });
}
// DirectBA::RenderModel.  camera: fx, fy, cx, cy (pixel-corner) + size; options: min_depth, max_depth, radius_scale.  Each output is a
// row-major host image of the camera's size, or null for a view that is not wanted; camera_T_global (12 floats, may be null)
// receives the matrix the kernels took.
static void views_out(const DirectBA::ModelViews& v, uint16_t* depth, uint32_t* index, uint8_t* color, float* normal) {
  copy_out(depth, v.depth); copy_out(index, v.index); copy_out(color, v.color); copy_out(normal, v.normal);
}
int bsh_render_model(void* ba, void* stream, const float* global_T_camera_pose7, const float* camera_params4, int width, int height, const float* options3,
                     uint16_t* depth, uint32_t* index, uint8_t* color, float* normal, float* camera_T_global) {
  BSH_TRY({
    DirectBA::RenderOptions o;
    o.min_depth = options3[0]; o.max_depth = options3[1]; o.radius_scale = options3[2];
    o.depth = depth != nullptr; o.index = index != nullptr; o.color = color != nullptr; o.normal = normal != nullptr;
    DirectBA::ModelViews v;
    static_cast<DirectBA*>(ba)->RenderModel(static_cast<hipStream_t>(stream), pose_from7(global_T_camera_pose7), PinholeCamera4f(width, height, camera_params4), o, &v);
    views_out(v, depth, index, color, normal);
    if (camera_T_global) std::memcpy(camera_T_global, v.camera_T_global.m, sizeof(v.camera_T_global.m));
  });
}
// DirectBA::RenderVolume.  camera as in bsh_render_model; options3: min_depth, max_depth, step (0: the voxel size).  Each output
// is a row-major host image of the camera's size, or null for a view that is not wanted; global_T_camera (12 floats, may be
// null) receives the matrix the kernel took.
int bsh_render_volume(void* ba, void* stream, const float* global_T_camera_pose7, const float* camera_params4, int width, int height, const float* options3,
                      uint32_t min_count, uint16_t* depth, uint8_t* color, float* normal, float* global_T_camera) {
  BSH_TRY({
    DirectBA::VolumeViewOptions o;
    o.min_depth = options3[0]; o.max_depth = options3[1]; o.step = options3[2];
    o.min_count = min_count;
    o.depth = depth != nullptr; o.color = color != nullptr; o.normal = normal != nullptr;
    DirectBA::ModelViews v;
    static_cast<DirectBA*>(ba)->RenderVolume(static_cast<hipStream_t>(stream), pose_from7(global_T_camera_pose7), PinholeCamera4f(width, height, camera_params4), o, &v);
    views_out(v, depth, nullptr, color, normal);
    if (global_T_camera) std::memcpy(global_T_camera, v.global_T_camera.m, sizeof(v.global_T_camera.m));
  });
}
// DirectBA::ModelBounds.  bounds6: min x y z, max x y z; returns 1 when there is a valid surfel, 0 when none, -1 on error.
int bsh_model_bounds(void* ba, void* stream, float* bounds6) {
  try { return static_cast<DirectBA*>(ba)->ModelBounds(static_cast<hipStream_t>(stream), bounds6, bounds6 + 3) ? 1 : 0; }
  catch (const std::exception& e) { g_err = e.what(); return -1; }
}
// DirectBA::FuseKeyframes.  origin3: x y z of the volume's corner; dims3: nx ny nz.
int bsh_fuse_keyframes(void* ba, void* stream, const float* origin3, float voxel_size, const int* dims3, float truncation) {
  BSH_TRY({
    DirectBA::VolumeSpec spec;
    std::memcpy(spec.origin, origin3, sizeof(spec.origin));
    spec.voxel_size = voxel_size;
    spec.nx = dims3[0]; spec.ny = dims3[1]; spec.nz = dims3[2];
    static_cast<DirectBA*>(ba)->FuseKeyframes(static_cast<hipStream_t>(stream), spec, truncation);
  });
}
// DirectBA::ExtractMesh in two steps: bsh_extract_mesh extracts, keeps the mesh for this thread and reports counts2 = {vertices,
// triangles}; bsh_mesh_copy copies it out (positions, normals: 3 floats per vertex; colors: 4 bytes per vertex; indices: 3 per
// triangle) and drops it.
static thread_local DirectBA::Mesh g_mesh;
// DirectBA::ExtractMesh with MeshOptions: as bsh_extract_mesh, then bsh_mesh_copy.  report3 (may be null; with it the report is
// computed and kept for this thread) receives {components, removed vertices, removed triangles} of the mesh as extracted;
// bsh_mesh_component_sizes then copies out the vertex count of every component in descending order (`components` entries).
static thread_local DirectBA::MeshComponentReport g_mesh_report;
static void extract_mesh(void* ba, void* stream, uint32_t min_count, uint32_t min_component_vertices, uint64_t* counts2, uint32_t* report3) {
  static_cast<DirectBA*>(ba)->ExtractMesh(static_cast<hipStream_t>(stream), DirectBA::MeshOptions{min_count, min_component_vertices}, &g_mesh,
                                          report3 ? &g_mesh_report : nullptr);
  counts2[0] = g_mesh.vertex_count();
  counts2[1] = g_mesh.triangle_count();
  if (report3) { report3[0] = g_mesh_report.components; report3[1] = g_mesh_report.removed_vertices; report3[2] = g_mesh_report.removed_triangles; }
}
int bsh_extract_mesh(void* ba, void* stream, uint32_t min_count, uint64_t* counts2) { BSH_TRY(extract_mesh(ba, stream, min_count, 0, counts2, nullptr)); }
int bsh_extract_mesh_filtered(void* ba, void* stream, uint32_t min_count, uint32_t min_component_vertices, uint64_t* counts2, uint32_t* report3) {
  BSH_TRY({
    g_mesh_report = DirectBA::MeshComponentReport();
    extract_mesh(ba, stream, min_count, min_component_vertices, counts2, report3);
  });
}
int bsh_mesh_component_sizes(uint32_t* sizes, uint32_t capacity) {
  BSH_TRY({
    std::memcpy(sizes, g_mesh_report.sizes_descending.data(), std::min<size_t>(g_mesh_report.sizes_descending.size(), capacity) * sizeof(uint32_t));
    g_mesh_report = DirectBA::MeshComponentReport();
  });
}
// DirectBA::MeshComponents of a host mesh of `vertices` vertices and `triangles` index triples: labels, sizes (vertices entries
// each, either may be null) and *components.
int bsh_mesh_components(void* ba, void* stream, uint32_t vertices, uint32_t triangles, const uint32_t* indices, uint32_t* labels, uint32_t* sizes,
                        uint32_t* components) {
  BSH_TRY({
    DirectBA::Mesh mesh;
    mesh.positions.assign(3 * static_cast<size_t>(vertices), 0.f);
    mesh.indices.assign(indices, indices + 3 * static_cast<size_t>(triangles));
    std::vector<uint32_t> l, s;
    *components = static_cast<DirectBA*>(ba)->MeshComponents(static_cast<hipStream_t>(stream), mesh, labels ? &l : nullptr, sizes ? &s : nullptr);
    copy_out(labels, l);
    copy_out(sizes, s);
  });
}
int bsh_mesh_copy(float* positions, float* normals, uint8_t* colors, uint32_t* indices) {
  BSH_TRY({
    copy_out(positions, g_mesh.positions);
    copy_out(normals, g_mesh.normals);
    copy_out(colors, g_mesh.colors);
    copy_out(indices, g_mesh.indices);
    g_mesh = DirectBA::Mesh();
  });
}
// A host mesh from a caller's arrays: normals, colors (4 bytes per vertex) and indices may be null.
static DirectBA::Mesh mesh_from(uint64_t vertices, const float* positions, const float* normals, const uint8_t* colors, uint64_t triangles, const uint32_t* indices) {
  DirectBA::Mesh mesh;
  mesh.positions.assign(positions, positions + 3 * vertices);
  if (normals) mesh.normals.assign(normals, normals + 3 * vertices);
  if (colors) {
    mesh.colors.resize(vertices);
    std::memcpy(mesh.colors.data(), colors, 4 * vertices);
  }
  if (triangles) mesh.indices.assign(indices, indices + 3 * triangles);
  return mesh;
}
// DirectBA::RenderMesh of host arrays (normals and colors -- 4 bytes per vertex -- may be null).  camera and outputs as in
// bsh_render_model; options2: min_depth, max_depth.
int bsh_render_mesh(void* ba, void* stream, uint64_t vertices, const float* positions, const float* normals, const uint8_t* colors, uint64_t triangles,
                    const uint32_t* indices, const float* global_T_camera_pose7, const float* camera_params4, int width, int height, const float* options2,
                    int cull_backfaces, uint16_t* depth, uint32_t* index, uint8_t* color, float* normal, float* camera_T_global) {
  BSH_TRY({
    DirectBA::MeshViewOptions o;
    o.min_depth = options2[0]; o.max_depth = options2[1];
    o.cull_backfaces = cull_backfaces != 0;
    o.depth = depth != nullptr; o.index = index != nullptr; o.color = color != nullptr; o.normal = normal != nullptr;
    const DirectBA::Mesh mesh = mesh_from(vertices, positions, normals, colors, triangles, indices);
    DirectBA::ModelViews v;
    static_cast<DirectBA*>(ba)->RenderMesh(static_cast<hipStream_t>(stream), mesh, pose_from7(global_T_camera_pose7), PinholeCamera4f(width, height, camera_params4), o, &v);
    views_out(v, depth, index, color, normal);
    if (camera_T_global) std::memcpy(camera_T_global, v.camera_T_global.m, sizeof(v.camera_T_global.m));
  });
}
// DirectBA::SimplifyMesh of host arrays in two steps, like the mesh: bsh_simplify_mesh (normals, colors -- 4 bytes per vertex --
// and indices may be null; origin3: x y z) keeps the result for this thread and reports counts2 = {vertices, triangles};
// bsh_simplified_copy copies it out (normals and colors only where the input had them; vertex_cluster: one entry per input vertex;
// any pointer may be null) and drops it.
static thread_local DirectBA::Mesh g_simplified;
static thread_local std::vector<uint32_t> g_simplified_cluster;
int bsh_simplify_mesh(void* ba, void* stream, uint64_t vertices, const float* positions, const float* normals, const uint8_t* colors, uint64_t triangles,
                      const uint32_t* indices, const float* origin3, float cell_size, uint64_t* counts2) {
  BSH_TRY({
    g_simplified = DirectBA::Mesh();
    g_simplified_cluster.clear();
    const DirectBA::Mesh mesh = mesh_from(vertices, positions, normals, colors, triangles, indices);
    static_cast<DirectBA*>(ba)->SimplifyMesh(static_cast<hipStream_t>(stream), mesh, origin3, cell_size, &g_simplified, &g_simplified_cluster);
    counts2[0] = g_simplified.vertex_count();
    counts2[1] = g_simplified.triangle_count();
  });
}
int bsh_simplified_copy(float* positions, float* normals, uint8_t* colors, uint32_t* indices, uint32_t* vertex_cluster) {
  BSH_TRY({
    copy_out(positions, g_simplified.positions);
    copy_out(normals, g_simplified.normals);
    copy_out(colors, g_simplified.colors);
    copy_out(indices, g_simplified.indices);
    copy_out(vertex_cluster, g_simplified_cluster);
    g_simplified = DirectBA::Mesh();
    g_simplified_cluster = std::vector<uint32_t>();
  });
}
// DirectBA::DecimateMesh of host arrays in the same two steps: bsh_decimate_mesh keeps the result for this thread and reports
// counts3 = {vertices, triangles, rounds}; bsh_decimated_copy copies it out (vertex_map: one entry per input vertex; any pointer may
// be null) and drops it.
static thread_local DirectBA::Mesh g_decimated;
static thread_local std::vector<uint32_t> g_decimated_map;
int bsh_decimate_mesh(void* ba, void* stream, uint64_t vertices, const float* positions, const float* normals, const uint8_t* colors, uint64_t triangles,
                      const uint32_t* indices, uint32_t target_vertices, float boundary_weight, float max_cost, uint32_t max_rounds, uint64_t* counts3) {
  BSH_TRY({
    g_decimated = DirectBA::Mesh();
    g_decimated_map.clear();
    const DirectBA::Mesh mesh = mesh_from(vertices, positions, normals, colors, triangles, indices);
    DirectBA::DecimateOptions options;
    options.target_vertices = target_vertices;
    options.boundary_weight = boundary_weight;
    options.max_cost = max_cost;
    options.max_rounds = max_rounds;
    counts3[2] = static_cast<DirectBA*>(ba)->DecimateMesh(static_cast<hipStream_t>(stream), mesh, options, &g_decimated, &g_decimated_map);
    counts3[0] = g_decimated.vertex_count();
    counts3[1] = g_decimated.triangle_count();
  });
}
int bsh_decimated_copy(float* positions, float* normals, uint8_t* colors, uint32_t* indices, uint32_t* vertex_map) {
  BSH_TRY({
    copy_out(positions, g_decimated.positions);
    copy_out(normals, g_decimated.normals);
    copy_out(colors, g_decimated.colors);
    copy_out(indices, g_decimated.indices);
    copy_out(vertex_map, g_decimated_map);
    g_decimated = DirectBA::Mesh();
    g_decimated_map = std::vector<uint32_t>();
  });
}
// DirectBA::CleanMesh of host arrays in the same two steps: bsh_clean_mesh (flags3: weld, remove_duplicates, remove_unreferenced) keeps
// the result for this thread and reports counts6 = {vertices, triangles, welded vertices, unreferenced vertices, degenerate triangles,
// duplicate triangles}; bsh_cleaned_copy copies it out (vertex_map, triangle_map: one entry per input vertex and triangle; any pointer
// may be null) and drops it.
static thread_local DirectBA::Mesh g_cleaned;
static thread_local std::vector<uint32_t> g_cleaned_vertex_map, g_cleaned_triangle_map;
int bsh_clean_mesh(void* ba, void* stream, uint64_t vertices, const float* positions, const float* normals, const uint8_t* colors, uint64_t triangles,
                   const uint32_t* indices, const int* flags3, uint64_t* counts6) {
  BSH_TRY({
    g_cleaned = DirectBA::Mesh();
    g_cleaned_vertex_map.clear();
    g_cleaned_triangle_map.clear();
    const DirectBA::Mesh mesh = mesh_from(vertices, positions, normals, colors, triangles, indices);
    DirectBA::CleanOptions options;
    options.weld = flags3[0] != 0;
    options.remove_duplicates = flags3[1] != 0;
    options.remove_unreferenced = flags3[2] != 0;
    DirectBA::CleanReport report;
    static_cast<DirectBA*>(ba)->CleanMesh(static_cast<hipStream_t>(stream), mesh, options, &g_cleaned, &g_cleaned_vertex_map, &g_cleaned_triangle_map, &report);
    counts6[0] = g_cleaned.vertex_count();
    counts6[1] = g_cleaned.triangle_count();
    counts6[2] = report.welded_vertices;
    counts6[3] = report.unreferenced_vertices;
    counts6[4] = report.degenerate_triangles;
    counts6[5] = report.duplicate_triangles;
  });
}
int bsh_cleaned_copy(float* positions, float* normals, uint8_t* colors, uint32_t* indices, uint32_t* vertex_map, uint32_t* triangle_map) {
  BSH_TRY({
    copy_out(positions, g_cleaned.positions);
    copy_out(normals, g_cleaned.normals);
    copy_out(colors, g_cleaned.colors);
    copy_out(indices, g_cleaned.indices);
    copy_out(vertex_map, g_cleaned_vertex_map);
    copy_out(triangle_map, g_cleaned_triangle_map);
    g_cleaned = DirectBA::Mesh();
    g_cleaned_vertex_map = std::vector<uint32_t>();
    g_cleaned_triangle_map = std::vector<uint32_t>();
  });
}
// DirectBA::MeshTopology of `triangles` index triples over `vertices` vertices: *report (a bslam_mesh_report), edge_uses and loop_of_slot
// (3 * triangles entries each, either may be null).
int bsh_mesh_topology(void* ba, void* stream, uint64_t vertices, uint64_t triangles, const uint32_t* indices, void* report, uint32_t* edge_uses, uint32_t* loop_of_slot) {
  BSH_TRY({
    std::vector<uint32_t> triples, uses, loops;
    if (triangles) triples.assign(indices, indices + 3 * static_cast<size_t>(triangles));
    static_cast<DirectBA*>(ba)->MeshTopology(static_cast<hipStream_t>(stream), static_cast<size_t>(vertices), triples, static_cast<bslam_mesh_report*>(report),
                                             edge_uses ? &uses : nullptr, loop_of_slot ? &loops : nullptr);
    copy_out(edge_uses, uses);
    copy_out(loop_of_slot, loops);
  });
}
// DirectBA::OrientMesh of host arrays (normals may be null unless mode is 1): out_indices (3 * triangles entries), flipped and
// patch_of_triangle (one entry per triangle, either may be null) and *report (a bslam_orient_report, may be null).
int bsh_orient_mesh(void* ba, void* stream, uint64_t vertices, const float* positions, const float* normals, uint64_t triangles, const uint32_t* indices, int mode,
                    uint32_t* out_indices, uint8_t* flipped, uint32_t* patch_of_triangle, void* report) {
  BSH_TRY({
    if (mode < 0 || mode > 2) throw std::invalid_argument("OrientMesh: mode must be 0 (majority), 1 (normals) or 2 (volume)");
    const DirectBA::Mesh mesh = mesh_from(vertices, positions, normals, nullptr, triangles, indices);
    std::vector<uint32_t> oriented, patches;
    std::vector<uint8_t> flips;
    static_cast<DirectBA*>(ba)->OrientMesh(static_cast<hipStream_t>(stream), mesh, static_cast<DirectBA::OrientMode>(mode), &oriented, flipped ? &flips : nullptr,
                                           patch_of_triangle ? &patches : nullptr, static_cast<bslam_orient_report*>(report));
    copy_out(out_indices, oriented);
    copy_out(flipped, flips);
    copy_out(patch_of_triangle, patches);
  });
}
// DirectBA::FillMeshHoles of host arrays in the same two steps: bsh_fill_mesh_holes keeps the result for this thread and reports
// counts3 = {vertices, triangles, holes filled}; bsh_filled_copy copies it out (any pointer may be null) and drops it.
static thread_local DirectBA::Mesh g_filled;
int bsh_fill_mesh_holes(void* ba, void* stream, uint64_t vertices, const float* positions, const float* normals, const uint8_t* colors, uint64_t triangles,
                        const uint32_t* indices, uint32_t max_hole_edges, uint64_t* counts3) {
  BSH_TRY({
    g_filled = DirectBA::Mesh();
    const DirectBA::Mesh mesh = mesh_from(vertices, positions, normals, colors, triangles, indices);
    counts3[2] = static_cast<DirectBA*>(ba)->FillMeshHoles(static_cast<hipStream_t>(stream), mesh, max_hole_edges, &g_filled);
    counts3[0] = g_filled.vertex_count();
    counts3[1] = g_filled.triangle_count();
  });
}
int bsh_filled_copy(float* positions, float* normals, uint8_t* colors, uint32_t* indices) {
  BSH_TRY({
    copy_out(positions, g_filled.positions);
    copy_out(normals, g_filled.normals);
    copy_out(colors, g_filled.colors);
    copy_out(indices, g_filled.indices);
    g_filled = DirectBA::Mesh();
  });
}
// DirectBA::SmoothMesh of host arrays in the same two steps: bsh_smooth_mesh (normals and indices may be null; boundary 0 fixed, 1 rim,
// 2 free) keeps the new positions and normals for this thread; bsh_smoothed_copy copies them out (either pointer may be null) and
// drops them.  Colours and indices are the caller's own.
static thread_local DirectBA::Mesh g_smoothed;
static DirectBA::SmoothOptions smooth_options(uint32_t iterations, float lambda, float mu, uint32_t boundary) {
  if (boundary > 2u) throw std::invalid_argument("SmoothMesh: boundary must be 0 (fixed), 1 (rim) or 2 (free)");
  DirectBA::SmoothOptions options;
  options.iterations = iterations;
  options.lambda = lambda;
  options.mu = mu;
  options.boundary = static_cast<DirectBA::SmoothBoundary>(boundary);
  return options;
}
int bsh_smooth_mesh(void* ba, void* stream, uint64_t vertices, const float* positions, const float* normals, uint64_t triangles, const uint32_t* indices,
                    uint32_t iterations, float lambda, float mu, uint32_t boundary) {
  BSH_TRY({
    g_smoothed = DirectBA::Mesh();
    const DirectBA::SmoothOptions options = smooth_options(iterations, lambda, mu, boundary);
    const DirectBA::Mesh mesh = mesh_from(vertices, positions, normals, nullptr, triangles, indices);
    static_cast<DirectBA*>(ba)->SmoothMesh(static_cast<hipStream_t>(stream), mesh, options, &g_smoothed);
  });
}
// DirectBA::SmoothMeshOnDevice of the mesh the last ExtractMesh left on the device: *vertices receives its vertex count, and
// bsh_smoothed_copy copies the result out as above.
int bsh_smooth_extracted_mesh(void* ba, void* stream, uint32_t iterations, float lambda, float mu, uint32_t boundary, uint64_t* vertices) {
  BSH_TRY({
    g_smoothed = DirectBA::Mesh();
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const DirectBA::DeviceMesh d = static_cast<DirectBA*>(ba)->SmoothMeshOnDevice(s, smooth_options(iterations, lambda, mu, boundary));
    g_smoothed.positions.resize(size_t{3} * d.vertices);
    g_smoothed.normals.resize(size_t{3} * d.vertices);
    d.positions->Download(s, g_smoothed.positions.data(), g_smoothed.positions.size());
    d.normals->Download(s, g_smoothed.normals.data(), g_smoothed.normals.size());
    if (hipStreamSynchronize(s) != hipSuccess) throw std::runtime_error("SmoothMeshOnDevice: the download failed");
    *vertices = d.vertices;
  });
}
int bsh_smoothed_copy(float* positions, float* normals) {
  BSH_TRY({
    copy_out(positions, g_smoothed.positions);
    copy_out(normals, g_smoothed.normals);
    g_smoothed = DirectBA::Mesh();
  });
}
// DirectBA::PointMeshDistance of host arrays: points 3 per point, positions 3 per vertex, indices 3 per triangle; distance and
// triangle receive `points_count` entries; *cell_used the grid cell of the call that succeeded, grid2 = {cells, entries}.
static void grid_out(const DirectBA::PointMeshResult& result, float* cell_used, uint64_t* grid2) {
  if (cell_used) *cell_used = result.cell_size;
  if (grid2) { grid2[0] = result.grid_cells; grid2[1] = result.grid_entries; }
}
int bsh_point_mesh_distance(void* ba, void* stream, uint64_t point_count, const float* points, uint64_t vertices, const float* positions, uint64_t triangles,
                            const uint32_t* indices, float max_distance, float cell_size, uint64_t max_grid_entries, float* distance, uint32_t* triangle,
                            float* cell_used, uint64_t* grid2) {
  BSH_TRY({
    DirectBA::Mesh mesh;
    mesh.positions.assign(positions, positions + 3 * vertices);
    mesh.indices.assign(indices, indices + 3 * triangles);
    const DirectBA::PointMeshOptions options{max_distance, cell_size, max_grid_entries};
    DirectBA::PointMeshResult result;
    static_cast<DirectBA*>(ba)->PointMeshDistance(static_cast<hipStream_t>(stream), points, point_count, mesh, options, &result);
    copy_out(distance, result.distance);
    copy_out(triangle, result.triangle);
    grid_out(result, cell_used, grid2);
  });
}
// DirectBA::NearestTriangle of host arrays shaped as above; max_distance may be +infinity; tree2 = {leaves, height}.
int bsh_nearest_triangle(void* ba, void* stream, uint64_t point_count, const float* points, uint64_t vertices, const float* positions, uint64_t triangles,
                         const uint32_t* indices, float max_distance, float* distance, uint32_t* triangle, uint32_t* tree2) {
  BSH_TRY({
    DirectBA::Mesh mesh;
    mesh.positions.assign(positions, positions + 3 * vertices);
    mesh.indices.assign(indices, indices + 3 * triangles);
    DirectBA::NearestTriangleResult result;
    static_cast<DirectBA*>(ba)->NearestTriangle(static_cast<hipStream_t>(stream), points, point_count, mesh, max_distance, &result);
    copy_out(distance, result.distance);
    copy_out(triangle, result.triangle);
    if (tree2) { tree2[0] = result.leaves; tree2[1] = result.height; }
  });
}
// DirectBA::RayCastMesh of host arrays: origins, directions 3 per ray, t_range 2 per ray or null; any_hit 0 fills t, triangle, uv (2 per
// ray) and front, any_hit 1 fills hit; the arrays of the other mode are not touched; tree2 = {leaves, height}.
int bsh_mesh_rays(void* ba, void* stream, uint64_t ray_count, const float* origins, const float* directions, const float* t_range, uint64_t vertices,
                  const float* positions, uint64_t triangles, const uint32_t* indices, int any_hit, float* t, uint32_t* triangle, float* uv, uint8_t* front, uint8_t* hit,
                  uint32_t* tree2) {
  BSH_TRY({
    DirectBA::Mesh mesh;
    mesh.positions.assign(positions, positions + 3 * vertices);
    mesh.indices.assign(indices, indices + 3 * triangles);
    DirectBA::RayCastResult result;
    static_cast<DirectBA*>(ba)->RayCastMesh(static_cast<hipStream_t>(stream), origins, directions, t_range, ray_count, mesh, any_hit != 0, &result);
    copy_out(t, result.t);
    copy_out(triangle, result.triangle);
    copy_out(uv, result.uv);
    copy_out(front, result.front);
    copy_out(hit, result.hit);
    if (tree2) { tree2[0] = result.leaves; tree2[1] = result.height; }
  });
}
// DirectBA::MeshVisibility of host arrays: points and (or null) normals 3 per point, camera_T_global 12 per view (row-major 3 x 4),
// centres 3 per view, camera_params4 = fx fy cx cy, options3 = min_depth, max_depth, margin; count and first one per point.
int bsh_mesh_visibility(void* ba, void* stream, uint64_t point_count, const float* points, const float* normals, uint64_t vertices, const float* positions,
                        uint64_t triangles, const uint32_t* indices, uint64_t views, const float* camera_T_global, const float* centres, const float* camera_params4,
                        int width, int height, const float* options3, uint32_t* count, uint32_t* first, uint32_t* tree2) {
  BSH_TRY({
    DirectBA::Mesh mesh;
    mesh.positions.assign(positions, positions + 3 * vertices);
    mesh.indices.assign(indices, indices + 3 * triangles);
    std::vector<bslam_mat3x4> rows(views);
    for (uint64_t k = 0; k < views; ++k) std::memcpy(rows[k].m, camera_T_global + 12 * k, sizeof(rows[k].m));
    const std::vector<float> centre(centres, centres + 3 * views);
    DirectBA::VisibilityOptions options;
    options.min_depth = options3[0]; options.max_depth = options3[1]; options.margin = options3[2];
    DirectBA::VisibilityResult result;
    static_cast<DirectBA*>(ba)->MeshVisibility(static_cast<hipStream_t>(stream), points, normals, point_count, mesh, rows, centre, PinholeCamera4f(width, height, camera_params4),
                                               options, &result);
    copy_out(count, result.count);
    copy_out(first, result.first);
    if (tree2) { tree2[0] = result.leaves; tree2[1] = result.height; }
  });
}
// DirectBA::SurfelMeshDistance in two steps, like the mesh: the call keeps its result for this thread and reports *count (the
// valid surfels), *cell_used and grid2; bsh_distance_copy copies distance and triangle out (`count` entries each) and drops it.
static thread_local DirectBA::PointMeshResult g_distance;
int bsh_surfel_mesh_distance(void* ba, void* stream, float max_distance, float cell_size, uint64_t max_grid_entries, uint64_t* count, float* cell_used,
                             uint64_t* grid2) {
  BSH_TRY({
    g_distance = DirectBA::PointMeshResult();
    static_cast<DirectBA*>(ba)->SurfelMeshDistance(static_cast<hipStream_t>(stream), DirectBA::PointMeshOptions{max_distance, cell_size, max_grid_entries}, &g_distance);
    *count = g_distance.distance.size();
    grid_out(g_distance, cell_used, grid2);
  });
}
int bsh_distance_copy(float* distance, uint32_t* triangle) {
  BSH_TRY({
    copy_out(distance, g_distance.distance);
    copy_out(triangle, g_distance.triangle);
    g_distance = DirectBA::PointMeshResult();
  });
}
// DirectBA::SampleMesh of host arrays in two steps, like the mesh: bsh_sample_mesh keeps the samples for this thread and reports
// *count; bsh_samples_copy copies them out (positions, normals: 3 floats per sample; triangle: 1 per sample) and drops them.
static thread_local DirectBA::MeshSamples g_samples;
int bsh_sample_mesh(void* ba, void* stream, uint64_t vertices, const float* positions, uint64_t triangles, const uint32_t* indices, float density, uint32_t seed,
                    uint64_t* count) {
  BSH_TRY({
    g_samples = DirectBA::MeshSamples();
    DirectBA::Mesh mesh;
    mesh.positions.assign(positions, positions + 3 * vertices);
    if (triangles) mesh.indices.assign(indices, indices + 3 * triangles);
    static_cast<DirectBA*>(ba)->SampleMesh(static_cast<hipStream_t>(stream), mesh, density, seed, &g_samples);
    *count = g_samples.count();
  });
}
int bsh_samples_copy(float* positions, float* normals, uint32_t* triangle) {
  BSH_TRY({
    copy_out(positions, g_samples.positions);
    copy_out(normals, g_samples.normals);
    copy_out(triangle, g_samples.triangles);
    g_samples = DirectBA::MeshSamples();
  });
}
// DirectBA::RegisterPoints of host arrays, in two steps like the mesh.  options8 = {max_distance, min_distance (0: max / 8), mode
// (-1: by the mesh), huber (0: half the stage's radius), shrink, iterations_per_stage, cell_size (0: doubling), max_grid_entries};
// initial16 and transform16 are row-major 4 x 4; status3 = {steps, converged, DirectBA::RegistrationEnd}; grid3 = {cell used, cells,
// entries}.  bsh_registration_history copies 7 doubles per step (radius, hits, used, cost, rmse, step translation, step rotation)
// and drops them; bsh_registration_reason names an end.
static thread_local std::vector<DirectBA::RegistrationStep> g_registration;
int bsh_register_points(void* ba, void* stream, uint64_t point_count, const float* points, uint64_t vertices, const float* positions, uint64_t triangles,
                        const uint32_t* indices, const double* options8, const double* initial16, double* transform16, int32_t* status3, double* grid3) {
  BSH_TRY({
    DirectBA::Mesh mesh;
    mesh.positions.assign(positions, positions + 3 * vertices);
    if (triangles) mesh.indices.assign(indices, indices + 3 * triangles);
    DirectBA::RegistrationOptions options;
    options.max_distance = static_cast<float>(options8[0]);
    options.min_distance = static_cast<float>(options8[1]);
    options.mode = static_cast<int>(options8[2]);
    options.huber = static_cast<float>(options8[3]);
    options.shrink = options8[4];
    options.iterations_per_stage = static_cast<int>(options8[5]);
    options.cell_size = static_cast<float>(options8[6]);
    options.max_grid_entries = static_cast<uint64_t>(options8[7]);
    std::copy(initial16, initial16 + 16, options.initial);
    DirectBA::RegistrationResult result;
    static_cast<DirectBA*>(ba)->RegisterPoints(static_cast<hipStream_t>(stream), points, point_count, mesh, options, &result);
    std::copy(result.target_T_source, result.target_T_source + 16, transform16);
    status3[0] = static_cast<int32_t>(result.history.size());
    status3[1] = result.converged ? 1 : 0;
    status3[2] = result.end;
    if (grid3) { grid3[0] = result.cell_size; grid3[1] = static_cast<double>(result.grid_cells); grid3[2] = static_cast<double>(result.grid_entries); }
    g_registration = std::move(result.history);
  });
}
int bsh_registration_history(double* rows7) {
  BSH_TRY({
    for (size_t i = 0; i < g_registration.size(); ++i) {
      const DirectBA::RegistrationStep& s = g_registration[i];
      const double row[7] = {s.radius, static_cast<double>(s.hits), static_cast<double>(s.used), s.cost, s.rmse, s.step_translation, s.step_rotation};
      std::copy(row, row + 7, rows7 + 7 * i);
    }
    g_registration.clear();
  });
}
const char* bsh_registration_reason(int end) { return DirectBA::RegistrationReason(end); }
// LoadPLY in two steps: bsh_load_ply reads the file, keeps it for this thread and reports counts4 = {vertices, triangles, has
// normals, has colours}; bsh_ply_copy copies it out (positions, normals: 3 floats per vertex; colors: 3 bytes per vertex; indices:
// 3 per triangle; any may be null) and drops it.
static thread_local PlyMesh g_ply;
int bsh_load_ply(const char* path, uint64_t* counts4) {
  BSH_TRY({
    std::string error;
    if (!LoadPLY(path, &g_ply, &error)) { g_ply = PlyMesh(); throw std::runtime_error(error); }
    counts4[0] = g_ply.vertex_count(); counts4[1] = g_ply.triangle_count(); counts4[2] = g_ply.has_normals; counts4[3] = g_ply.has_colors;
  });
}
int bsh_ply_copy(float* positions, float* normals, uint8_t* colors, uint32_t* indices) {
  BSH_TRY({
    copy_out(positions, g_ply.positions);
    copy_out(normals, g_ply.normals);
    copy_out(colors, g_ply.colors_rgb);
    copy_out(indices, g_ply.indices);
    g_ply = PlyMesh();
  });
}
// DirectBA::Volume.  With tsdf == null only the description is returned: dims3 = nx ny nz, floats5 = origin x y z, voxel size,
// truncation; else the three arrays of nx * ny * nz elements (colour: 4 bytes each) are filled as well.
int bsh_volume(void* ba, void* stream, int* dims3, float* floats5, float* tsdf, uint32_t* count, uint8_t* color) {
  BSH_TRY({
    DirectBA::VolumeData v;
    static_cast<DirectBA*>(ba)->Volume(static_cast<hipStream_t>(stream), &v);
    dims3[0] = v.spec.nx; dims3[1] = v.spec.ny; dims3[2] = v.spec.nz;
    std::memcpy(floats5, v.spec.origin, 12);
    floats5[3] = v.spec.voxel_size; floats5[4] = v.truncation;
    copy_out(tsdf, v.tsdf);
    copy_out(count, v.count);
    copy_out(color, v.color);
  });
}
int bsh_save_point_cloud_ply(const char* path, uint64_t count, const float* positions, const uint8_t* colors_rgb, const float* normals) {
  BSH_TRY(if (!SavePointCloudAsPLY(path, count, positions, colors_rgb, normals)) throw std::runtime_error(std::string("cannot write ") + path));
}
int bsh_save_mesh_ply(const char* path, uint64_t vertex_count, const float* positions, const float* normals, const uint8_t* colors_rgba, uint64_t triangle_count,
                      const uint32_t* indices) {
  BSH_TRY(if (!SaveMeshAsPLY(path, vertex_count, positions, normals, colors_rgba, triangle_count, indices))
            throw std::runtime_error(std::string("cannot write ") + path + " (or an index is out of range)"));
}
int bsh_set_scheme_end_tasks(void* ba, int enable) { BSH_TRY(static_cast<DirectBA*>(ba)->SetSchemeEndTasks(enable != 0)); }
int bsh_create_surfels_for_keyframe(void* ba, void* stream, int filter_new_surfels, int keyframe_id) {
  BSH_TRY({
    DirectBA* b = static_cast<DirectBA*>(ba);
    b->CreateSurfelsForKeyframe(static_cast<hipStream_t>(stream), filter_new_surfels != 0, b->keyframes().at(keyframe_id));
  });
}

int bsh_set_options(void* ba, int batched_pose_optimization, int pcg_gauge_keyframe, int texture_mode) {
  BSH_TRY({
    DirectBA* b = static_cast<DirectBA*>(ba);
    b->SetBatchedPoseOptimization(batched_pose_optimization != 0);
    b->SetPCGGaugeKeyframe(pcg_gauge_keyframe);
    b->SetTextureMode(texture_mode);
  });
}
// --save_timings (BS/main.cc:660-662): the BA phase timing lines of BS/direct_ba_alternating.cc:630-688 go to `path`
// (nullptr / "": stop).  The stream lives as long as the DirectBA it was set on.
int bsh_set_timings_file(void* ba, const char* path) {
  BSH_TRY({
    DirectBA* b = static_cast<DirectBA*>(ba);
    b->SetTimingsStream(nullptr);
    g_timings.erase(ba);
    if (path && *path) {
      auto f = std::make_unique<std::ofstream>(path);
      if (!*f) throw std::runtime_error(std::string("cannot open ") + path);
      b->SetTimingsStream(f.get());
      g_timings[ba] = std::move(f);
    }
  });
}
int bsh_set_allreduce(void* ba, bslam_allreduce_fn fn, void* user) { BSH_TRY(static_cast<DirectBA*>(ba)->SetAllReduce(fn, user)); }
int bsh_comm_init(void* ba, const void* unique_id, int rank, int world_size) { BSH_TRY(static_cast<DirectBA*>(ba)->InitComm(unique_id, rank, world_size)); }
int bsh_comm_destroy(void* ba) { BSH_TRY(static_cast<DirectBA*>(ba)->DestroyComm()); }

int bsh_estimate_frame_pose(void* ba_, void* stream, int keyframe_id, const float* init7, float* out7) {
  BSH_TRY({
    DirectBA* ba = static_cast<DirectBA*>(ba_);
    const auto& kf = ba->keyframes().at(keyframe_id);
    SE3f out;
    ba->EstimateFramePose(static_cast<hipStream_t>(stream), pose_from7(init7), kf->depth_buffer(), kf->normals_buffer(), kf->color_buffer(), &out, false);
    pose_to7(out, out7);
  });
}

int bsh_bundle_adjustment(void* ba, void* stream, int optimize_depth_intrinsics, int optimize_color_intrinsics, int do_surfel_updates,
                          int optimize_poses, int optimize_geometry, int min_iterations, int max_iterations, int use_pcg,
                          int active_keyframe_window_start, int active_keyframe_window_end, int increase_ba_iteration_count,
                          int pcg_max_inner_iterations, int* iterations_done, int* converged) {
  BSH_TRY({
    bool conv = false;
    int iters = 0;
    static_cast<DirectBA*>(ba)->BundleAdjustment(static_cast<hipStream_t>(stream), optimize_depth_intrinsics != 0, optimize_color_intrinsics != 0,
                                                 do_surfel_updates != 0, optimize_poses != 0, optimize_geometry != 0, min_iterations, max_iterations,
                                                 use_pcg != 0, active_keyframe_window_start, active_keyframe_window_end,
                                                 increase_ba_iteration_count != 0, &iters, &conv, 0, nullptr, pcg_max_inner_iterations);
    if (iterations_done) *iterations_done = iters;
    if (converged) *converged = conv ? 1 : 0;
  });
}

// DirectBA::ComputeCost: ids[n], cost[n][2], counts[n][2] for the n <= capacity non-deleted keyframes, totals[2] = (depth, descriptor).
int bsh_compute_cost(void* ba_, void* stream, int active_surfels_only, int capacity, int* ids, float* cost, uint32_t* counts, int* n, double* totals) {
  BSH_TRY({
    DirectBA::CostReport r;
    static_cast<DirectBA*>(ba_)->ComputeCost(static_cast<hipStream_t>(stream), active_surfels_only != 0, &r);
    const int K = static_cast<int>(r.keyframe_ids.size());
    if (K > capacity) throw std::invalid_argument("bsh_compute_cost: more keyframes than capacity");
    for (int k = 0; k < K; ++k) {
      ids[k] = r.keyframe_ids[k];
      for (int j = 0; j < 2; ++j) { cost[2 * k + j] = r.cost[2 * k + j]; counts[2 * k + j] = r.counts[2 * k + j]; }
    }
    *n = K;
    totals[0] = r.depth_total;
    totals[1] = r.descriptor_total;
  });
}
int bsh_set_cost_tracking(void* ba, int enable) { BSH_TRY(static_cast<DirectBA*>(ba)->SetCostTracking(enable != 0)); }
// DirectBA::cost_history: totals[i][2] = (depth, descriptor) of entry i < min(n, capacity); n = the entries of the last BundleAdjustment
int bsh_cost_history(void* ba, int capacity, double* totals, int* n) {
  BSH_TRY({
    const auto& h = static_cast<DirectBA*>(ba)->cost_history();
    *n = static_cast<int>(h.size());
    for (int i = 0; i < *n && i < capacity; ++i) { totals[2 * i] = h[i].depth_total; totals[2 * i + 1] = h[i].descriptor_total; }
  });
}

int bsh_set_intrinsics(void* ba_, const float* color4, const float* depth4, float a) {
  BSH_TRY({
    DirectBA* ba = static_cast<DirectBA*>(ba_);
    if (color4) ba->SetColorCamera(PinholeCamera4f(ba->color_camera().width(), ba->color_camera().height(), color4));
    if (depth4) ba->SetDepthCamera(PinholeCamera4f(ba->depth_camera().width(), ba->depth_camera().height(), depth4));
    ba->SetA(a);
  });
}
int bsh_get_cfactor(void* ba_, void* stream, float* out) {
  BSH_TRY({
    DirectBA* ba = static_cast<DirectBA*>(ba_);
    ba->cfactor_buffer().Download(static_cast<hipStream_t>(stream), out, static_cast<size_t>(ba->cfactor_buffer().width()) * sizeof(float));
  });
}

int bsh_get_intrinsics(void* ba_, float* color4, float* depth4, float* a) {
  BSH_TRY({
    DirectBA* ba = static_cast<DirectBA*>(ba_);
    std::memcpy(color4, ba->color_camera().parameters(), 16);
    std::memcpy(depth4, ba->depth_camera().parameters(), 16);
    *a = ba->a();
  });
}

// ---- file formats (io.hpp) ----
int bsh_png_info(const char* path, int* whbc /* width, height, bit depth, channels */) {
  PngInfo info;
  if (!ReadPngInfo(path, &info)) { g_err = std::string("cannot read PNG header of ") + path; return -1; }
  whbc[0] = info.width; whbc[1] = info.height; whbc[2] = info.bit_depth; whbc[3] = info.channels;
  return 0;
}
int bsh_read_png_gray16(const char* path, uint16_t* out, size_t capacity) {
  int w, h;
  std::vector<uint16_t> img;
  if (!ReadPngGray16(path, &w, &h, &img) || img.size() > capacity) { g_err = std::string("cannot read 16-bit PNG ") + path; return -1; }
  std::memcpy(out, img.data(), img.size() * sizeof(uint16_t));
  return 0;
}
int bsh_read_png_rgb8(const char* path, uint8_t* out, size_t capacity) {
  int w, h;
  std::vector<uint8_t> img;
  if (!ReadPngRgb8(path, &w, &h, &img) || img.size() > capacity) { g_err = std::string("cannot read 8-bit PNG ") + path; return -1; }
  std::memcpy(out, img.data(), img.size());
  return 0;
}
void* bsh_tum_open(const char* folder, const char* trajectory_filename) {
  auto ds = std::make_unique<TumDataset>();
  if (!ReadTUMRGBDDatasetAssociatedAndCalibrated(folder, trajectory_filename ? trajectory_filename : "", ds.get())) {
    g_err = std::string("cannot read TUM RGB-D dataset ") + folder;
    return nullptr;
  }
  return ds.release();
}
void bsh_tum_close(void* ds) { delete static_cast<TumDataset*>(ds); }
int bsh_tum_frame_count(void* ds) { return static_cast<int>(static_cast<TumDataset*>(ds)->frames.size()); }
int bsh_tum_camera(void* ds_, float* params4, int* width, int* height) {
  const TumDataset* ds = static_cast<TumDataset*>(ds_);
  std::memcpy(params4, ds->camera_parameters, 16);
  *width = ds->width; *height = ds->height;
  return 0;
}
int bsh_tum_frame(void* ds_, int i, char* rgb_path, char* depth_path, char* rgb_ts, char* depth_ts, size_t capacity, float* rgb_pose7, float* depth_pose7) {
  const TumDataset* ds = static_cast<TumDataset*>(ds_);
  if (i < 0 || i >= static_cast<int>(ds->frames.size())) { g_err = "frame index out of range"; return -1; }
  const TumFrame& f = ds->frames[static_cast<size_t>(i)];
  std::snprintf(rgb_path, capacity, "%s", f.rgb_path.c_str());
  std::snprintf(depth_path, capacity, "%s", f.depth_path.c_str());
  std::snprintf(rgb_ts, capacity, "%s", f.rgb_timestamp_string.c_str());
  std::snprintf(depth_ts, capacity, "%s", f.depth_timestamp_string.c_str());
  pose_to7(f.rgb_global_T_frame, rgb_pose7);
  pose_to7(f.depth_global_T_frame, depth_pose7);
  return 0;
}
int bsh_save_poses(int count, const char* const* timestamp_strings, const float* poses7, int start_frame, const char* path) {
  std::vector<std::string> ts(static_cast<size_t>(count));
  std::vector<SE3f> poses(static_cast<size_t>(count));
  for (int i = 0; i < count; ++i) { ts[i] = timestamp_strings[i]; poses[i] = pose_from7(poses7 + 7 * i); }
  if (!SavePoses(ts, poses, start_frame, path)) { g_err = std::string("cannot write ") + path; return -1; }
  return 0;
}
int bsh_save_calibration_arrays(const char* base, const float* depth4, const float* color4, float a, int w, int h, const float* cfactor) {
  if (!SaveCalibration(base, depth4, color4, a, w, h, cfactor)) { g_err = std::string("cannot write calibration ") + base; return -1; }
  return 0;
}
int bsh_load_calibration_arrays(const char* base, float* depth4, float* color4, float* a, int w, int h, float* cfactor) {
  if (!LoadCalibration(base, depth4, color4, a, w, h, cfactor)) { g_err = std::string("cannot read calibration ") + base; return -1; }
  return 0;
}
// SaveCalibration / LoadCalibration of BS/io.cc:570-700 on a DirectBA
int bsh_save_calibration(void* ba_, void* stream, const char* base) {
  BSH_TRY({
    DirectBA* ba = static_cast<DirectBA*>(ba_);
    const int w = ba->cfactor_buffer().width(), h = ba->cfactor_buffer().height();
    std::vector<float> cf(static_cast<size_t>(w) * h);
    ba->cfactor_buffer().Download(static_cast<hipStream_t>(stream), cf.data(), static_cast<size_t>(w) * sizeof(float));
    if (!SaveCalibration(base, ba->depth_camera().parameters(), ba->color_camera().parameters(), ba->a(), w, h, cf.data()))
      throw std::runtime_error(std::string("cannot write calibration ") + base);
  });
}
int bsh_load_calibration(void* ba_, void* stream, const char* base) {
  BSH_TRY({
    DirectBA* ba = static_cast<DirectBA*>(ba_);
    const int w = ba->cfactor_buffer().width(), h = ba->cfactor_buffer().height();
    std::vector<float> cf(static_cast<size_t>(w) * h);
    float d[4], c[4], a = 0.f;
    if (!LoadCalibration(base, d, c, &a, w, h, cf.data())) throw std::runtime_error(std::string("cannot read calibration ") + base);
    ba->SetDepthCamera(PinholeCamera4f(ba->depth_camera().width(), ba->depth_camera().height(), d));
    ba->SetColorCamera(PinholeCamera4f(ba->color_camera().width(), ba->color_camera().height(), c));
    ba->SetA(a);
    ba->UploadCFactor(static_cast<hipStream_t>(stream), cf.data());
  });
}

// ---- state file v1 ----
void* bsh_state_load(const char* path) {
  auto st = std::make_unique<StateV1>();
  std::string err;
  if (!LoadState(path, st.get(), &err)) { g_err = err; return nullptr; }
  return st.release();
}
void bsh_state_free(void* st) { delete static_cast<StateV1*>(st); }
int bsh_state_save(void* st, const char* path) {
  if (!SaveState(*static_cast<StateV1*>(st), path)) { g_err = std::string("cannot write ") + path; return -1; }
  return 0;
}
// ints: base_kf_id, last_frame_index, frame count, keyframe count, surfel_count, surfels_size, ba_iteration_count, cell size;
// floats: a, raw_to_float_depth, baseline_fx, depth camera (4), colour camera (4)
int bsh_state_summary(void* st_, int32_t* ints8, float* floats11) {
  const StateV1* st = static_cast<StateV1*>(st_);
  ints8[0] = st->base_kf_id; ints8[1] = st->last_frame_index; ints8[2] = static_cast<int32_t>(st->frame_global_T_frame.size());
  ints8[3] = static_cast<int32_t>(st->keyframes.size()); ints8[4] = st->surfel_count; ints8[5] = st->surfels_size; ints8[6] = st->ba_iteration_count;
  ints8[7] = st->sparse_surfel_cell_size;
  floats11[0] = st->a; floats11[1] = st->raw_to_float_depth; floats11[2] = st->baseline_fx;
  std::memcpy(floats11 + 3, st->depth_camera_parameters, 16);
  std::memcpy(floats11 + 7, st->color_camera_parameters, 16);
  return 0;
}
// The DirectBA part of SaveState (BS/io.cc:106-178): cameras, deformation, keyframe metadata, surfels, BA counters.  The SLAM
// front-end fields (config, motion model, queue) keep their defaults; frame poses = the keyframes' poses at their frame indices.
int bsh_state_save_from_ba(void* ba_, void* stream_, int frame_count, const char* path) {
  BSH_TRY({
    DirectBA* ba = static_cast<DirectBA*>(ba_);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StateV1 st;
    st.frame_global_T_frame.assign(static_cast<size_t>(frame_count), SE3f());
    st.config.raw_to_float_depth = ba->depth_params().raw_to_float_depth;
    st.config.baseline_fx = ba->depth_params().baseline_fx;
    st.config.sparse_surfel_cell_size = ba->depth_params().sparse_surfel_cell_size;
    st.config.use_geometric_residuals = ba->use_depth_residuals();
    st.config.use_photometric_residuals = ba->use_descriptor_residuals();
    st.color_camera_width = ba->color_camera().width(); st.color_camera_height = ba->color_camera().height();
    st.depth_camera_width = ba->depth_camera().width(); st.depth_camera_height = ba->depth_camera().height();
    std::memcpy(st.color_camera_parameters, ba->color_camera().parameters(), 16);
    std::memcpy(st.depth_camera_parameters, ba->depth_camera().parameters(), 16);
    st.cfactor_width = ba->cfactor_buffer().width(); st.cfactor_height = ba->cfactor_buffer().height();
    st.cfactor.resize(static_cast<size_t>(st.cfactor_width) * st.cfactor_height);
    ba->cfactor_buffer().Download(stream, st.cfactor.data(), static_cast<size_t>(st.cfactor_width) * sizeof(float));
    const bslam_depth_params dp = ba->depth_params();
    st.a = dp.a; st.raw_to_float_depth = dp.raw_to_float_depth; st.baseline_fx = dp.baseline_fx; st.sparse_surfel_cell_size = dp.sparse_surfel_cell_size;
    for (const auto& kf : ba->keyframes()) {
      StateKeyframeV1 k;
      if (kf) {
        k.id = kf->id(); k.frame_index = static_cast<int32_t>(kf->frame_index()); k.activation = static_cast<int32_t>(kf->activation());
        k.last_active_in_ba_iteration = kf->last_active_in_ba_iteration(); k.last_covis_in_ba_iteration = kf->last_covis_in_ba_iteration();
        if (k.frame_index < 0 || k.frame_index >= frame_count) throw std::invalid_argument("keyframe frame index outside the frame list");
        st.frame_global_T_frame[static_cast<size_t>(k.frame_index)] = kf->global_T_frame();
      }
      st.keyframes.push_back(k);
    }
    st.surfel_count = static_cast<int32_t>(ba->surfel_count()); st.surfels_size = static_cast<int32_t>(ba->surfels_size());
    st.surfels.resize(static_cast<size_t>(8) * st.surfels_size);
    if (st.surfels_size) ba->GetSurfels(stream, st.surfels.data(), static_cast<size_t>(st.surfels_size) * sizeof(float), 8);
    st.ba_iteration_count = ba->ba_iteration_count(); st.last_ba_iteration_count = ba->last_ba_iteration_count();
    st.use_depth_residuals = ba->use_depth_residuals(); st.use_descriptor_residuals = ba->use_descriptor_residuals();
    st.min_observation_count_while_bootstrapping_1 = ba->min_observation_count_while_bootstrapping_1();
    st.min_observation_count_while_bootstrapping_2 = ba->min_observation_count_while_bootstrapping_2();
    st.min_observation_count = ba->min_observation_count();
    st.surfel_merge_dist_factor = ba->surfel_merge_dist_factor();
    if (!SaveState(st, path)) throw std::runtime_error(std::string("cannot write ") + path);
  });
}
// The DirectBA part of LoadState (BS/io.cc:300-372, 446-475): the keyframes must already exist (the reference re-creates them
// from the dataset images); their poses come from the per-frame pose list.
int bsh_state_load_into_ba(void* ba_, void* stream_, const char* path) {
  BSH_TRY({
    DirectBA* ba = static_cast<DirectBA*>(ba_);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StateV1 st;
    std::string err;
    if (!LoadState(path, &st, &err)) throw std::runtime_error(err);
    if (st.cfactor_width != ba->cfactor_buffer().width() || st.cfactor_height != ba->cfactor_buffer().height())
      throw std::runtime_error("cfactor buffer size mismatch");                      // BS/io.cc:331-335
    if (st.keyframes.size() != ba->keyframes().size()) throw std::runtime_error("keyframe count mismatch");
    if (static_cast<u32>(st.surfels_size) > static_cast<u32>(ba->max_surfel_count())) throw std::runtime_error("surfel count exceeds max_surfel_count");   // :452-455
    ba->SetColorCamera(PinholeCamera4f(st.color_camera_width, st.color_camera_height, st.color_camera_parameters));
    ba->SetDepthCamera(PinholeCamera4f(st.depth_camera_width, st.depth_camera_height, st.depth_camera_parameters));
    ba->SetA(st.a);
    ba->UploadCFactor(stream, st.cfactor.data());
    for (size_t i = 0; i < st.keyframes.size(); ++i) {
      const StateKeyframeV1& k = st.keyframes[i];
      const auto& kf = ba->keyframes()[i];
      if ((k.id < 0) != (kf == nullptr)) throw std::runtime_error("keyframe list mismatch");
      if (!kf) continue;
      kf->SetActivation(static_cast<Keyframe::Activation>(k.activation));
      kf->SetLastActiveInBAIteration(k.last_active_in_ba_iteration);
      kf->SetLastCovisInBAIteration(k.last_covis_in_ba_iteration);
      kf->set_global_T_frame(st.frame_global_T_frame.at(static_cast<size_t>(k.frame_index)));
    }
    ba->SetSurfels(stream, st.surfels.data(), static_cast<size_t>(st.surfels_size) * sizeof(float), static_cast<u32>(st.surfels_size));
    ba->SetBAIterationCounts(st.ba_iteration_count, st.last_ba_iteration_count);
  });
}

// TrackFramePairwise on two keyframes of a DirectBA (base = the reference keyframe, tracked = the frame to localise):
// out = base_T_tracked.  iterations: num_scales ints (may be null).
int bsh_track_keyframe_pair_ex(void* ba_, void* stream, int tracked_id, int base_id, int num_scales, int test_different_initial_estimates,
                               const float* init1_pose7, const float* init2_pose7, float* out_pose7, int* iterations, int use_pyramid_level_0, int use_gradmag) {
  BSH_TRY({
    DirectBA* ba = static_cast<DirectBA*>(ba_);
    const auto& tracked = ba->keyframes().at(tracked_id);
    const auto& base = ba->keyframes().at(base_id);
    PairwiseFrameTrackingBuffers buffers(ba->depth_camera().width(), ba->depth_camera().height(), ba->color_camera().width(), ba->color_camera().height(),
                                         num_scales);
    SE3f out;
    const bslam_depth_params dp = ba->depth_params();
    for (int s = 0; s < num_scales; ++s) iterations[s] = 0;
    TrackFramePairwise(ba->context(), static_cast<hipStream_t>(stream), &buffers, ba->color_camera(), ba->depth_camera(), dp, ba->use_depth_residuals(),
                       ba->use_descriptor_residuals(), tracked->depth_buffer(), tracked->normals_buffer(), tracked->color_buffer(), base->depth_buffer(),
                       base->normals_buffer(), base->color_buffer(), test_different_initial_estimates != 0, pose_from7(init1_pose7),
                       pose_from7(init2_pose7 ? init2_pose7 : init1_pose7), &out, iterations, use_pyramid_level_0 != 0, use_gradmag != 0);
    pose_to7(out, out_pose7);
  });
}

int bsh_track_keyframe_pair(void* ba_, void* stream, int tracked_id, int base_id, int num_scales, int test_different_initial_estimates,
                            const float* init1_pose7, const float* init2_pose7, float* out_pose7, int* iterations) {
  BSH_TRY({
    DirectBA* ba = static_cast<DirectBA*>(ba_);
    const auto& tracked = ba->keyframes().at(tracked_id);
    const auto& base = ba->keyframes().at(base_id);
    PairwiseFrameTrackingBuffers buffers(ba->depth_camera().width(), ba->depth_camera().height(), ba->color_camera().width(), ba->color_camera().height(),
                                         num_scales);
    SE3f out;
    const bslam_depth_params dp = ba->depth_params();
    TrackFramePairwise(ba->context(), static_cast<hipStream_t>(stream), &buffers, ba->color_camera(), ba->depth_camera(), dp, ba->use_depth_residuals(),
                       ba->use_descriptor_residuals(), tracked->depth_buffer(), tracked->normals_buffer(), tracked->color_buffer(), base->depth_buffer(),
                       base->normals_buffer(), base->color_buffer(), test_different_initial_estimates != 0, pose_from7(init1_pose7),
                       pose_from7(init2_pose7 ? init2_pose7 : init1_pose7), &out, iterations);
    pose_to7(out, out_pose7);
  });
}

// TrackFramesPairwiseBatched of keyframes tracked_ids[0..n) against keyframe base_id: out_pose7[7 * p] = base_T_tracked[p],
// iterations[num_scales * p + s].
int bsh_track_keyframes_batched(void* ba_, void* stream, int base_id, int n, const int* tracked_ids, const float* inits_pose7, int num_scales,
                                float* out_pose7, int* iterations) {
  BSH_TRY({
    DirectBA* ba = static_cast<DirectBA*>(ba_);
    const auto& base = ba->keyframes().at(base_id);
    if (!base) throw std::invalid_argument("base keyframe is deleted");
    std::vector<TrackedFrameImages> tracked;
    std::vector<SE3f> inits;
    for (int p = 0; p < n; ++p) {
      const auto& kf = ba->keyframes().at(tracked_ids[p]);
      if (!kf) throw std::invalid_argument("tracked keyframe is deleted");
      tracked.push_back(TrackedFrameImages{&kf->depth_buffer(), &kf->normals_buffer(), &kf->color_buffer()});
      inits.push_back(pose_from7(inits_pose7 + 7 * p));
    }
    std::vector<std::unique_ptr<PairwiseFrameTrackingBuffers>> buffers;
    std::vector<SE3f> out;
    std::vector<std::vector<int>> its;
    TrackFramesPairwiseBatched(ba->context(), static_cast<hipStream_t>(stream), &buffers, num_scales, ba->color_camera(), ba->depth_camera(), ba->depth_params(),
                               ba->use_depth_residuals(), ba->use_descriptor_residuals(), tracked, base->depth_buffer(), base->normals_buffer(),
                               base->color_buffer(), inits, &out, &its);
    for (int p = 0; p < n; ++p) {
      pose_to7(out[p], out_pose7 + 7 * p);
      for (int s = 0; s < num_scales; ++s) iterations[num_scales * p + s] = its[p][s];
    }
  });
}

// LoopClosureResult as flat arrays.  ints: [status, old ids (3), pixel_count, chi2 count, iterations (3 x num_scales)];
// floats: [refined pose7 x 3, averaged pose7, mean pixel distance]; chi2: up to kLoopPoseGraphIterations doubles.
static void loop_result_out(const LoopClosureResult& r, int num_scales, int* ints, float* floats, double* chi2) {
  ints[0] = static_cast<int>(r.status);
  for (int i = 0; i < 3; ++i) ints[1 + i] = r.old_keyframe_ids[i];
  ints[4] = r.pixel_count;
  ints[5] = static_cast<int>(r.chi2.size());
  for (int i = 0; i < 3; ++i)
    for (int s = 0; s < num_scales; ++s) ints[6 + num_scales * i + s] = (i < static_cast<int>(r.tracking_iterations.size())) ? r.tracking_iterations[i][s] : 0;
  for (int i = 0; i < 3; ++i) pose_to7(r.cur_T_old_refined[i], floats + 7 * i);
  pose_to7(r.cur_T_old_averaged, floats + 21);
  floats[28] = r.mean_pixel_distance;
  for (size_t i = 0; i < r.chi2.size() && i < static_cast<size_t>(kLoopPoseGraphIterations); ++i) chi2[i] = r.chi2[i];
}

int bsh_close_loop(void* ba_, void* stream, int current_id, int matched_id, const float* old_T_cur_initial_pose7, int num_scales, int* ints, float* floats,
                   double* chi2) {
  BSH_TRY({
    LoopClosureResult r;
    CloseLoop(*static_cast<DirectBA*>(ba_), static_cast<hipStream_t>(stream), current_id, matched_id, pose_from7(old_T_cur_initial_pose7), num_scales, &r);
    loop_result_out(r, num_scales, ints, floats, chi2);
  });
}

// ---- place recognition (host/place_recognition.hpp) ----
// options: [min_keyframe_gap, score_threshold, max_distance, min_matches, ransac_iterations, ransac_min_inliers]
static PlaceRecognitionOptions place_options_in(const int64_t* options6, double ransac_inlier_threshold) {
  PlaceRecognitionOptions o;
  o.min_keyframe_gap = static_cast<int>(options6[0]); o.score_threshold = options6[1]; o.max_distance = static_cast<int>(options6[2]);
  o.min_matches = static_cast<int>(options6[3]); o.ransac_iterations = static_cast<int>(options6[4]); o.ransac_min_inliers = static_cast<int>(options6[5]);
  o.ransac_inlier_threshold = ransac_inlier_threshold;
  return o;
}
// the defaults of PlaceRecognitionOptions in the layout above
int bsh_place_default_options(int64_t* options6, double* ransac_inlier_threshold) {
  const PlaceRecognitionOptions o;
  options6[0] = o.min_keyframe_gap; options6[1] = o.score_threshold; options6[2] = o.max_distance; options6[3] = o.min_matches;
  options6[4] = o.ransac_iterations; options6[5] = o.ransac_min_inliers;
  *ransac_inlier_threshold = o.ransac_inlier_threshold;
  return 0;
}
// EstimateRelativePose (no GPU): points as n x 3 doubles; pose7 = old_T_cur [qx qy qz qw tx ty tz]; inliers: n bytes (may be null).
// Returns 1 when an estimate was found, 0 when it was rejected, -1 on error.
int bsh_estimate_relative_pose(int current_id, int matched_id, int n, const double* p_cur, const double* p_old, int iterations, double inlier_threshold,
                               int min_inliers, double* pose7, int* inlier_count, uint8_t* inliers) {
  int found = 0;
  const int rc = [&]() -> int {
    BSH_TRY({
      RelativePoseEstimate e;
      EstimateRelativePose(current_id, matched_id, n, p_cur, p_old, iterations, inlier_threshold, min_inliers, &e);
      for (int i = 0; i < 4; ++i) pose7[i] = e.q[i];
      for (int i = 0; i < 3; ++i) pose7[4 + i] = e.t[i];
      *inlier_count = e.inlier_count;
      copy_out(inliers, e.inliers);
      found = e.found ? 1 : 0;
    });
  }();
  return rc < 0 ? rc : found;
}
uint32_t bsh_place_ransac_seed(int current_id, int matched_id) { return PlaceRansacSeed(current_id, matched_id); }
int bsh_place_cells(void* ba) {
  int cells = 0;
  const int rc = [&]() -> int { BSH_TRY(cells = static_cast<DirectBA*>(ba)->place_recognizer().cells()); }();
  return rc < 0 ? rc : cells;
}
// xy: cells words, desc: cells x 8 words (bsh_place_cells)
int bsh_extract_keyframe_features(void* ba, void* stream, int keyframe_id, int64_t score_threshold, uint32_t* xy, uint32_t* desc) {
  BSH_TRY({
    std::vector<u32> x, d;
    static_cast<DirectBA*>(ba)->ExtractKeyframeFeatures(static_cast<hipStream_t>(stream), keyframe_id, score_threshold, &x, &d);
    std::memcpy(xy, x.data(), x.size() * sizeof(u32));
    std::memcpy(desc, d.data(), d.size() * sizeof(u32));
  });
}
// match: n x cells, count: n
int bsh_match_keyframe_features(void* ba, void* stream, int query_id, int n, const int* ids, int max_distance, int32_t* match, uint32_t* count) {
  BSH_TRY({
    std::vector<int32_t> m;
    std::vector<u32> c;
    static_cast<DirectBA*>(ba)->MatchKeyframeFeatures(static_cast<hipStream_t>(stream), query_id, std::vector<int>(ids, ids + n), max_distance, &m, &c);
    std::memcpy(match, m.data(), m.size() * sizeof(int32_t));
    std::memcpy(count, c.data(), c.size() * sizeof(u32));
  });
}
// out5: [candidate id, match count, inlier count, pose found, loop attempted]; pose7: the RANSAC old_T_cur in double;
// ints / floats / chi2: the LoopClosureResult as bsh_close_loop reports it (meaningful with loop attempted).
int bsh_recognize_place(void* ba, void* stream, int current_id, const int64_t* options6, double ransac_inlier_threshold, int num_scales, int* out5, double* pose7,
                        int* ints, float* floats, double* chi2) {
  BSH_TRY({
    PlaceRecognitionResult r;
    static_cast<DirectBA*>(ba)->RecognizePlace(static_cast<hipStream_t>(stream), current_id, place_options_in(options6, ransac_inlier_threshold), num_scales, &r);
    out5[0] = r.candidate_id; out5[1] = r.match_count; out5[2] = r.pose.inlier_count; out5[3] = r.pose.found ? 1 : 0; out5[4] = r.loop_attempted ? 1 : 0;
    for (int i = 0; i < 4; ++i) pose7[i] = r.pose.q[i];
    for (int i = 0; i < 3; ++i) pose7[4 + i] = r.pose.t[i];
    loop_result_out(r.loop, num_scales, ints, floats, chi2);
  });
}

// ---- pose graph (host/pose_graph.hpp); poses as double pose7 [qx qy qz qw tx ty tz] ----
static Pose3d pose3d_from7(const double* p) { return Pose3d::FromQuaternion(p[0], p[1], p[2], p[3], p[4], p[5], p[6]); }
static void pose3d_to7(const Pose3d& T, double* p) {
  T.ToQuaternion(p, p + 1, p + 2, p + 3);
  p[4] = T.t[0]; p[5] = T.t[1]; p[6] = T.t[2];
}
static void report_pose_graph(const PoseGraphResult& res, double* chi2, double* initial_chi2, long long* factor_blocks) {
  if (chi2) for (size_t i = 0; i < res.chi2.size(); ++i) chi2[i] = res.chi2[i];
  if (initial_chi2) *initial_chi2 = res.initial_chi2;
  if (factor_blocks) *factor_blocks = static_cast<long long>(res.factor_blocks);
}

// OptimizePoseGraph on an explicit graph.  poses7: vertex_count x 7 (in / out); edges: edge_count x (from, to);
// measurements7: edge_count x 7 (from_T_to).  chi2: `iterations` values (may be null).
int bsh_optimize_pose_graph(int vertex_count, double* poses7, int edge_count, const int* edges, const double* measurements7, int fixed_vertex, int iterations,
                            double* chi2, double* initial_chi2, long long* factor_blocks) {
  BSH_TRY({
    std::vector<Pose3d> poses(static_cast<size_t>(vertex_count));
    for (int v = 0; v < vertex_count; ++v) poses[v] = pose3d_from7(poses7 + 7 * v);
    std::vector<PoseGraphEdge> e(static_cast<size_t>(edge_count));
    for (int i = 0; i < edge_count; ++i) e[i] = PoseGraphEdge{edges[2 * i], edges[2 * i + 1], pose3d_from7(measurements7 + 7 * i)};
    PoseGraphResult res;
    OptimizePoseGraph(&poses, e, fixed_vertex, iterations, &res);
    for (int v = 0; v < vertex_count; ++v)
      if (v != fixed_vertex) pose3d_to7(poses[v], poses7 + 7 * v);   // the gauge is returned untouched
    report_pose_graph(res, chi2, initial_chi2, factor_blocks);
  });
}

// OptimizeKeyframePoseGraph: exists[i] = 0 for a deleted keyframe; loop_edges: loop_count x (from_id, to_id).
// Returns the gauge keyframe id (>= 0) or -1 on error.
int bsh_optimize_keyframe_pose_graph(int keyframe_count, const int* exists, double* poses7, int loop_count, const int* loop_edges,
                                     const double* loop_measurements7, int iterations, double* chi2, double* initial_chi2, long long* factor_blocks) {
  int gauge = -1;
  int rc = [&]() -> int {
    BSH_TRY({
      std::vector<Pose3d> poses(static_cast<size_t>(keyframe_count));
      std::vector<bool> ex(static_cast<size_t>(keyframe_count));
      for (int i = 0; i < keyframe_count; ++i) {
        ex[i] = exists[i] != 0;
        if (ex[i]) poses[i] = pose3d_from7(poses7 + 7 * i);
      }
      std::vector<KeyframeLoopEdge> loops(static_cast<size_t>(loop_count));
      for (int i = 0; i < loop_count; ++i) loops[i] = KeyframeLoopEdge{loop_edges[2 * i], loop_edges[2 * i + 1], pose3d_from7(loop_measurements7 + 7 * i)};
      PoseGraphResult res;
      gauge = OptimizeKeyframePoseGraph(&poses, ex, loops, iterations, &res);
      if (gauge < 0) throw std::invalid_argument("no keyframe exists");
      for (int i = 0; i < keyframe_count; ++i)
        if (ex[i] && i != gauge) pose3d_to7(poses[i], poses7 + 7 * i);
      report_pose_graph(res, chi2, initial_chi2, factor_blocks);
    });
  }();
  return rc < 0 ? rc : gauge;
}

// AveragePose (BS/util.cc:110-129) of count double pose7s.
int bsh_average_pose(int count, const double* poses7, double* out7) {
  BSH_TRY({
    std::vector<Pose3d> poses;
    for (int i = 0; i < count; ++i) poses.push_back(pose3d_from7(poses7 + 7 * i));
    pose3d_to7(AveragePose(poses), out7);
  });
}

// ---- BadSlam front end (host/bad_slam.hpp) ----
// cfg: [keyframe_interval, max_num_ba_iterations_per_keyframe, num_scales, max_surfel_count, sparse_surfel_cell_size, use_motion_model,
//       use_geometric_residuals, use_photometric_residuals, do_surfel_updates, use_pcg, optimize_intrinsics, disable_deactivation, start_frame,
//       pyramid_level_for_depth, pyramid_level_for_color, median_filter_and_densify_iterations]
// fcfg: [raw_to_float_depth, max_depth, baseline_fx]
void* bsh_slam_create(const int* cfg, const float* fcfg, int color_width, int color_height, const float* color_params, int depth_width, int depth_height,
                      const float* depth_params, int device) {
  try {
    BadSlamConfigV1 c;
    c.keyframe_interval = cfg[0]; c.max_num_ba_iterations_per_keyframe = cfg[1]; c.num_scales = cfg[2]; c.max_surfel_count = cfg[3];
    c.sparse_surfel_cell_size = cfg[4]; c.use_motion_model = cfg[5] != 0; c.use_geometric_residuals = cfg[6] != 0;
    c.use_photometric_residuals = cfg[7] != 0; c.do_surfel_updates = cfg[8] != 0; c.use_pcg = cfg[9] != 0; c.optimize_intrinsics = cfg[10] != 0;
    c.disable_deactivation = cfg[11] != 0; c.start_frame = cfg[12];
    c.pyramid_level_for_depth = cfg[13]; c.pyramid_level_for_color = cfg[14]; c.median_filter_and_densify_iterations = cfg[15];
    c.raw_to_float_depth = fcfg[0]; c.max_depth = fcfg[1]; c.baseline_fx = fcfg[2];
    return new BadSlam(c, PinholeCamera4f(color_width, color_height, color_params), PinholeCamera4f(depth_width, depth_height, depth_params), device);
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
void bsh_slam_destroy(void* slam) { delete static_cast<BadSlam*>(slam); }
void* bsh_slam_direct_ba(void* slam) { return &static_cast<BadSlam*>(slam)->direct_ba(); }
int bsh_slam_process_frame(void* slam, int frame_index, const uint16_t* depth, const uint8_t* rgb, int force_keyframe) {
  BSH_TRY(static_cast<BadSlam*>(slam)->ProcessFrame(frame_index, depth, rgb, force_keyframe != 0));
}
// BadSlam::PreprocessFrame alone, finished on return (for timing the stage)
int bsh_slam_preprocess_frame(void* slam, const uint16_t* depth, const uint8_t* rgb) {
  BSH_TRY({
    BadSlam* s = static_cast<BadSlam*>(slam);
    s->PreprocessFrame(depth, rgb);
    if (hipStreamSynchronize(s->stream()) != hipSuccess) throw std::runtime_error("hipStreamSynchronize failed");
  });
}
// Sensor rectification (host/rectification.hpp).  cameras: [colour, depth]; color_T_depth: 12 floats, row-major 3x4; enable = 0 switches it off
// and reads nothing else.
int bsh_slam_set_sensor_rectification(void* slam, int enable, const bslam_radtan_camera* cameras, const float* color_T_depth,
                                      float depth_difference_threshold, float raw_depth_to_metres) {
  BSH_TRY({
    BadSlam* s = static_cast<BadSlam*>(slam);
    if (!enable) { s->SetSensorRectification(nullptr); return 0; }
    SensorRectification r;
    r.color_camera = cameras[0];
    r.depth_camera = cameras[1];
    std::memcpy(r.color_T_depth.m, color_T_depth, sizeof(r.color_T_depth.m));
    r.depth_difference_threshold = depth_difference_threshold;
    r.raw_depth_to_metres = raw_depth_to_metres;
    s->SetSensorRectification(&r);
  });
}
// params4: fx, fy, cx, cy (pixel-corner); size2: width, height
int bsh_decide_undistorted_camera(const bslam_radtan_camera* camera, int avoid_invalid_pixels, float* params4, int* size2) {
  BSH_TRY({
    const PinholeCamera4f c = DecideUndistortedCamera(*camera, avoid_invalid_pixels != 0);
    std::memcpy(params4, c.parameters(), 4 * sizeof(float));
    size2[0] = c.width();
    size2[1] = c.height();
  });
}
// map: height x width x 2 floats
int bsh_make_unprojection_map(const bslam_radtan_camera* camera, float* map) {
  BSH_TRY({
    const std::vector<float> m = MakeUnprojectionMap(*camera);
    std::memcpy(map, m.data(), m.size() * sizeof(float));
  });
}
// count normalised points (x, y) through the distortion (inverse = 0) or its inverse (inverse = 1), in double
int bsh_radtan_points(const bslam_radtan_camera* camera, int inverse, int count, const double* in_xy, double* out_xy) {
  BSH_TRY({
    for (int i = 0; i < count; ++i) {
      if (inverse) RadtanUndistort(*camera, in_xy[2 * i], in_xy[2 * i + 1], &out_xy[2 * i], &out_xy[2 * i + 1]);
      else RadtanDistort(*camera, in_xy[2 * i], in_xy[2 * i + 1], &out_xy[2 * i], &out_xy[2 * i + 1]);
    }
  });
}
int bsh_slam_run_bundle_adjustment(void* slam, int frame_index, int optimize_depth_intrinsics, int optimize_color_intrinsics, int optimize_poses,
                                   int optimize_geometry, int min_iterations, int max_iterations, int window_start, int window_end,
                                   int increase_ba_iteration_count, int* iterations_done, int* converged) {
  BSH_TRY({
    bool conv = false;
    int done = 0;
    static_cast<BadSlam*>(slam)->RunBundleAdjustment(static_cast<uint32_t>(frame_index), optimize_depth_intrinsics != 0, optimize_color_intrinsics != 0,
                                                     optimize_poses != 0, optimize_geometry != 0, min_iterations, max_iterations, window_start, window_end,
                                                     increase_ba_iteration_count != 0, &done, &conv);
    if (iterations_done) *iterations_done = done;
    if (converged) *converged = conv ? 1 : 0;
  });
}
int bsh_slam_close_loop(void* slam, int matched_id, const float* old_T_cur_initial_pose7, int* ints, float* floats, double* chi2) {
  BSH_TRY({
    BadSlam* s = static_cast<BadSlam*>(slam);
    LoopClosureResult r;
    s->CloseLoop(matched_id, pose_from7(old_T_cur_initial_pose7), &r);
    loop_result_out(r, s->config().num_scales, ints, floats, chi2);
  });
}
int bsh_slam_set_loop_candidate_search(void* slam, int enable, int min_keyframe_gap) {
  BSH_TRY(static_cast<BadSlam*>(slam)->SetLoopCandidateSearch(enable != 0, min_keyframe_gap));
}
int bsh_slam_loop_log_size(void* slam) { return static_cast<int>(static_cast<BadSlam*>(slam)->loop_closure_log().size()); }
// entries x [keyframe id, candidate id, status]; distances: entries floats
int bsh_slam_loop_log(void* slam, int* entries3, float* distances, int capacity) {
  BSH_TRY({
    const auto& log = static_cast<BadSlam*>(slam)->loop_closure_log();
    for (size_t i = 0; i < log.size() && static_cast<int>(i) < capacity; ++i) {
      entries3[3 * i] = log[i].keyframe_id;
      entries3[3 * i + 1] = log[i].candidate_id;
      entries3[3 * i + 2] = static_cast<int>(log[i].status);
      distances[i] = log[i].mean_pixel_distance;
    }
  });
}
int bsh_slam_set_place_recognition(void* slam, int enable, const int64_t* options6, double ransac_inlier_threshold) {
  BSH_TRY(static_cast<BadSlam*>(slam)->SetPlaceRecognition(enable != 0, enable ? place_options_in(options6, ransac_inlier_threshold) : PlaceRecognitionOptions()));
}
int bsh_slam_place_log_size(void* slam) { return static_cast<int>(static_cast<BadSlam*>(slam)->place_recognition_log().size()); }
// entries x [keyframe id, candidate id, match count, inlier count, pose found, loop attempted, status]; distances: entries floats; poses7: entries x 7 doubles
int bsh_slam_place_log(void* slam, int* entries7, float* distances, double* poses7, int capacity) {
  BSH_TRY({
    const auto& log = static_cast<BadSlam*>(slam)->place_recognition_log();
    for (size_t i = 0; i < log.size() && static_cast<int>(i) < capacity; ++i) {
      int* e = entries7 + 7 * i;
      e[0] = log[i].keyframe_id; e[1] = log[i].candidate_id; e[2] = log[i].match_count; e[3] = log[i].inlier_count; e[4] = log[i].pose_found ? 1 : 0;
      e[5] = log[i].loop_attempted ? 1 : 0; e[6] = static_cast<int>(log[i].status);
      distances[i] = log[i].mean_pixel_distance;
      for (int j = 0; j < 7; ++j) poses7[7 * i + j] = log[i].old_T_cur[j];
    }
  });
}
int bsh_slam_frame_count(void* slam) { return static_cast<int>(static_cast<BadSlam*>(slam)->frame_poses().size()); }
int bsh_slam_get_frame_poses(void* slam, float* poses7, int capacity) {
  BSH_TRY({
    const auto& poses = static_cast<BadSlam*>(slam)->frame_poses();
    for (size_t i = 0; i < poses.size() && static_cast<int>(i) < capacity; ++i) pose_to7(poses[i], poses7 + 7 * i);
  });
}
// state: [keyframe_created, pose_estimated, num_planned_ba_iterations, base keyframe id or -1, motion model length]
int bsh_slam_state(void* slam, int* state) {
  BSH_TRY({
    BadSlam* s = static_cast<BadSlam*>(slam);
    state[0] = s->keyframe_created(); state[1] = s->pose_estimated(); state[2] = s->num_planned_ba_iterations();
    state[3] = s->base_kf() ? s->base_kf()->id() : -1;
    state[4] = static_cast<int>(s->motion_model_base_kf_tr_frame().size());
  });
}

}  // extern "C"
