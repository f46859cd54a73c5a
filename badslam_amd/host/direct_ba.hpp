// direct_ba.hpp -- C++ host side of the bundle-adjustment hot path on MI355X.
//
// Mirrors the reference's class DirectBA (BS/direct_ba.h:65-550, BS = applications/badslam/src/
// badslam of pangfumin/badslam) for the part of its interface that lies on the hot path:
// constructor argument list, AddKeyframe, EstimateFramePose, BundleAdjustment (alternating and
// PCG), the accessors callers use.  All device work goes through the C ABI of
// include/badslam_hip.h; this class owns the scene state exactly as the reference's does
// (surfel SoA, active mask, cfactor image, PCG vectors, keyframe buffers).
//
// Not on the hot path and therefore absent ("out of scope" / "next" rows): surfel
// creation / merge / deletion / compaction (do_surfel_updates must be false, surfels are
// uploaded with SetSurfels), keyframe merging, the on-screen visualisation (off-screen views of the
// model: RenderModel).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/badslam_hip.h"
#include "se3.hpp"

namespace bslam_host {

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;

// = vis::PinholeCamera4f (libvis/src/libvis/camera.h:1740-1743): fx, fy, cx, cy (pixel-corner
// convention) + image size.
class PinholeCamera4f {
 public:
  PinholeCamera4f() : width_(0), height_(0), p_{0, 0, 0, 0} {}
  PinholeCamera4f(int width, int height, const float* parameters) : width_(width), height_(height) {
    for (int i = 0; i < 4; ++i) p_[i] = parameters[i];
  }
  int width() const { return width_; }
  int height() const { return height_; }
  const float* parameters() const { return p_; }
  bslam_camera4f pod() const { return bslam_camera4f{p_[0], p_[1], p_[2], p_[3], width_, height_}; }

 private:
  int width_, height_;
  float p_[4];
};

// Device image with the layout of vis::CUDABuffer<T> (pitched 2-D).
template <typename T>
class DeviceBuffer {
 public:
  DeviceBuffer(int height, int width);
  ~DeviceBuffer();
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  int width() const { return width_; }
  int height() const { return height_; }
  size_t pitch() const { return pitch_; }
  T* address() const { return data_; }
  bslam_buffer2d ToPod() const { return bslam_buffer2d{data_, height_, width_, pitch_}; }
  void Upload(hipStream_t stream, const T* host, size_t host_pitch_bytes);
  void Download(hipStream_t stream, T* host, size_t host_pitch_bytes) const;
  void Clear(int byte_value, hipStream_t stream);

 private:
  T* data_;
  int height_, width_;
  size_t pitch_;
};

inline void ThrowOnHipError(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// Flat device array of `count` elements (plain hipMalloc; count 0 is allowed and still has an address).  Upload and Download
// enqueue asynchronous copies of the first n elements: the caller waits for the stream once, where it needs the data.
template <typename T>
class DeviceArray {
 public:
  explicit DeviceArray(size_t count) : data_(nullptr), count_(count) {
    ThrowOnHipError(hipMalloc(reinterpret_cast<void**>(&data_), std::max<size_t>(count * sizeof(T), 1)), "hipMalloc");
  }
  ~DeviceArray() { hipError_t e = hipFree(data_); (void)e; }
  DeviceArray(const DeviceArray&) = delete;
  DeviceArray& operator=(const DeviceArray&) = delete;
  size_t count() const { return count_; }
  T* address() const { return data_; }
  void Upload(hipStream_t stream, const T* host, size_t n) { Copy(data_, host, n, hipMemcpyHostToDevice, stream); }
  void Download(hipStream_t stream, T* host, size_t n) const { Copy(host, data_, n, hipMemcpyDeviceToHost, stream); }

 private:
  static void Copy(void* to, const void* from, size_t n, hipMemcpyKind kind, hipStream_t stream) {
    if (n) ThrowOnHipError(hipMemcpyAsync(to, from, n * sizeof(T), kind, stream), "hipMemcpyAsync");
  }
  T* data_;
  size_t count_;
};

struct uchar4_t { u8 x, y, z, w; };

// = vis::Keyframe (BS/keyframe.h) reduced to what the path reads.
class Keyframe {
 public:
  enum class Activation { kActive = 0, kCovisibleActive = 1, kInactive = 2 };   // BS/keyframe.h:54-67

  // Mirrors the reference constructor that takes prepared buffers (BS/keyframe.cc:35-80); the
  // images are HOST arrays in the formats of SURVEY.md A.2 and are uploaded.
  Keyframe(hipStream_t stream, u32 frame_index, float min_depth, float max_depth, int width, int height,
           const u16* depth, const u16* normals, const u16* radius, const uchar4_t* color, const SE3f& global_T_frame);

  // Mirrors the reference constructor from raw images (BS/keyframe.cc:82-161): uploads the u16 depth and the
  // 3-byte rgb image (HOST arrays) and runs ComputeBrightness, ComputeNormals, ComputePointRadiiAndRemoveIsolatedPixels
  // and ComputeMinMaxDepth through the C ABI of `ctx`.
  Keyframe(bslam_context* ctx, hipStream_t stream, u32 frame_index, const bslam_depth_params& depth_params, const bslam_camera4f& depth_camera,
           const u16* depth_image, int color_width, int color_height, const u8* rgb_image, const SE3f& global_T_frame);

  // The reference's prepared-buffer constructor proper (BS/keyframe.cc:35-80): DEVICE images, copied on `stream`.
  Keyframe(hipStream_t stream, u32 frame_index, float min_depth, float max_depth, const DeviceBuffer<u16>& depth, const DeviceBuffer<u16>& normals,
           const DeviceBuffer<u16>& radius, const DeviceBuffer<uchar4_t>& color, const SE3f& global_T_frame);

  const DeviceBuffer<u16>& depth_buffer() const { return depth_; }
  const DeviceBuffer<u16>& normals_buffer() const { return normals_; }
  const DeviceBuffer<u16>& radius_buffer() const { return radius_; }
  const DeviceBuffer<uchar4_t>& color_buffer() const { return color_; }
  DeviceBuffer<u16>& mutable_depth_buffer() { return depth_; }
  DeviceBuffer<u16>& mutable_normals_buffer() { return normals_; }

  const SE3f& global_T_frame() const { return global_T_frame_; }
  const SE3f& frame_T_global() const { return frame_T_global_; }
  void set_global_T_frame(const SE3f& T) { global_T_frame_ = T; frame_T_global_ = T.Inverse(); }   // BS/keyframe.h:160-173

  Activation activation() const { return activation_; }
  void SetActivation(Activation a) { activation_ = a; }
  int id() const { return id_; }
  void SetID(int id) { id_ = id; }
  u32 frame_index() const { return frame_index_; }
  float min_depth() const { return min_depth_; }
  float max_depth() const { return max_depth_; }
  std::vector<int>& co_visibility_list() { return co_visibility_list_; }
  int last_active_in_ba_iteration() const { return last_active_in_ba_iteration_; }
  void SetLastActiveInBAIteration(int v) { last_active_in_ba_iteration_ = v; }
  int last_covis_in_ba_iteration() const { return last_covis_in_ba_iteration_; }
  void SetLastCovisInBAIteration(int v) { last_covis_in_ba_iteration_ = v; }

  bslam_keyframe_view view() const;

 private:
  u32 frame_index_;
  int id_ = -1;
  int last_active_in_ba_iteration_ = -1, last_covis_in_ba_iteration_ = -1;
  float min_depth_, max_depth_;
  DeviceBuffer<u16> depth_, normals_, radius_;
  DeviceBuffer<uchar4_t> color_;
  SE3f global_T_frame_, frame_T_global_;
  Activation activation_ = Activation::kActive;
  std::vector<int> co_visibility_list_;
};

// = vis::CameraFrustum (libvis/src/libvis/camera_frustum.h): bounding-box test, then the
// separating-axis test on planes and edge cross products.
class CameraFrustum {
 public:
  CameraFrustum(const PinholeCamera4f& camera, float min_depth, float max_depth, const SE3f& global_T_camera);
  bool Intersects(CameraFrustum* other);

 private:
  void ComputeAxesAndPlanes();
  Vec3f points_[8];
  Vec3f axes_[6];
  Vec3f plane_n_[6];
  float plane_d_[6];
  bool computed_ = false;
  float bb_min_[3], bb_max_[3];
};

class PlaceRecognizer;            // host/place_recognition.hpp
struct PlaceRecognitionOptions;
struct PlaceRecognitionResult;

class Timer;   // reference API placeholder (BS/direct_ba.h:158); only a null pointer is accepted

class DirectBA {
 public:
  // Argument list of BS/direct_ba.h:73-88 (render_window must be null: no display on the GPU box).
  DirectBA(int max_surfel_count, float raw_to_float_depth, float baseline_fx, int sparse_surfel_cell_size,
           float surfel_merge_dist_factor, int min_observation_count_while_bootstrapping_1,
           int min_observation_count_while_bootstrapping_2, int min_observation_count,
           const PinholeCamera4f& color_camera_initial_estimate, const PinholeCamera4f& depth_camera_initial_estimate,
           int pyramid_level_for_color, bool use_depth_residuals, bool use_descriptor_residuals,
           void* render_window, const SE3f& global_T_anchor_frame, int device = 0);
  ~DirectBA();

  void AddKeyframe(const std::shared_ptr<Keyframe>& new_keyframe);   // BS/direct_ba.cc:196-204

  // BS/direct_ba_alternating.cc:42-283: Gauss-Newton on one frame against the surfel model, host
  // loop with one accumulation call + double LDLT + SE3 update per iteration, as the reference.
  void EstimateFramePose(hipStream_t stream, const SE3f& global_T_frame_initial_estimate, const DeviceBuffer<u16>& depth_buffer,
                         const DeviceBuffer<u16>& normals_buffer, const DeviceBuffer<uchar4_t>& color_buffer,
                         SE3f* out_global_T_frame_estimate, bool called_within_ba);

  // BS/direct_ba.h:143-162 / BS/direct_ba.cc:407-453
  void BundleAdjustment(hipStream_t stream, bool optimize_depth_intrinsics, bool optimize_color_intrinsics, bool do_surfel_updates,
                        bool optimize_poses, bool optimize_geometry, int min_iterations, int max_iterations, bool use_pcg,
                        int active_keyframe_window_start, int active_keyframe_window_end, bool increase_ba_iteration_count,
                        int* iterations_done = nullptr, bool* converged = nullptr, double time_limit = 0, Timer* timer = nullptr,
                        int pcg_max_inner_iterations = 30, int pcg_max_keyframes = 2500,
                        std::function<bool(int)> progress_function = nullptr);

  // Keyframe management of the outer seam (BS/direct_ba.h:95-116).  The reference's LoopDetector* parameters are
  // dropped: loop detection stays with the caller, which removes the image from its own detector.
  void DeleteKeyframe(int keyframe_index);                                    // BS/direct_ba.cc:207-229
  // Deletes up to approx_merge_count keyframes that are close to both neighbours on the trajectory (never keyframe 0);
  // returns the deleted ids in the order of deletion.                         // BS/direct_ba.cc:251-338
  std::vector<int> MergeKeyframes(hipStream_t stream, size_t approx_merge_count);
  void UpdateKeyframeCoVisibility(const std::shared_ptr<Keyframe>& keyframe);  // BS/direct_ba.cc:710-737
  void AssignColors(hipStream_t stream);                                       // BS/direct_ba.cc:456-459
  // ExportToPointCloud (BS/direct_ba.cc:461-546): the valid (non-NaN) surfels as host arrays; normals are
  // re-normalised 10-bit normals as in the reference.
  struct PointCloud {
    std::vector<float> positions;   // 3 per point
    std::vector<u8> colors;         // 3 per point (r, g, b)
    std::vector<float> normals;     // 3 per point
    size_t size() const { return positions.size() / 3; }
  };
  void ExportToPointCloud(hipStream_t stream, PointCloud* cloud) const;

  // Views of the surfel model from a pose (bslam_render_surfels; in place of the reference's render window): oriented
  // discs, nearest surface per pixel, identical bits from call to call.  metres_to_depth is 1 / raw_to_float_depth, so
  // the depth view has the units of a keyframe's depth image.  The device images are kept and re-used between calls.
  // On a surfel-sharded (multi-GPU) object this renders the local shard only.
  struct RenderOptions {
    float min_depth = 0.05f, max_depth = 50.f;   // metres; a surfel whose ball leaves the range is dropped
    float radius_scale = 1.f;
    bool depth = true, index = false, color = true, normal = false;   // the views wanted, at least one
  };
  struct ModelViews {   // row-major host images of the camera's size; a view not asked for is empty
    int width = 0, height = 0;
    bslam_mat3x4 camera_T_global;   // global_T_camera.Inverse() as the kernels took it
    std::vector<u16> depth;
    std::vector<u32> index;       // 0xFFFFFFFF: nothing drawn
    std::vector<uchar4_t> color;
    std::vector<float> normal;    // 3 per pixel, camera frame
    bslam_mat3x4 global_T_camera; // set by RenderVolume only: the matrix its kernel took
  };
  void RenderModel(hipStream_t stream, const SE3f& global_T_camera, const PinholeCamera4f& camera, const RenderOptions& options, ModelViews* views);

  // Volumetric fusion and meshing (bslam_fuse_keyframes, bslam_extract_mesh; the reference ends at the point cloud).  The
  // volume is fused from scratch from all keyframes that are not deleted, at their current poses and with the object's
  // cameras and depth parameters -- call it after bundle adjustment.  The device volume is kept by the object and re-used
  // while its dimensions stay the same; an object that never calls these allocates and launches nothing for them.
  // Keyframes are replicated on a surfel-sharded object, so every rank fuses the same volume and nothing is exchanged.
  struct VolumeSpec {
    float origin[3] = {0.f, 0.f, 0.f};   // sample (x, y, z) lies at origin + (i + 0.5) * voxel_size per axis
    float voxel_size = 0.01f;
    int nx = 0, ny = 0, nz = 0;
  };
  struct VolumeData {   // host copy of the fused volume, element (z * ny + y) * nx + x
    VolumeSpec spec;
    float truncation = 0.f;
    std::vector<float> tsdf;
    std::vector<u32> count;
    std::vector<uchar4_t> color;
  };
  struct Mesh {
    std::vector<float> positions, normals;   // 3 per vertex
    std::vector<uchar4_t> colors;            // 1 per vertex
    std::vector<u32> indices;                // 3 per triangle, counter-clockwise seen from free space
    size_t vertex_count() const { return positions.size() / 3; }
    size_t triangle_count() const { return indices.size() / 3; }
  };
  // A mesh on the device: positions and normals 3 floats per vertex, colours 1, indices 3 per triangle, each null where the mesh has
  // none.  The arrays may have room for more than the `vertices` and `triangles` in use (the result of an operator has room for its
  // input's counts).  vertex_map, where an operator gives one: the output vertex of every input vertex; rounds: of a decimation.
  struct DeviceMesh {
    std::unique_ptr<DeviceArray<float>> positions, normals;
    std::unique_ptr<DeviceArray<uchar4_t>> colors;
    std::unique_ptr<DeviceArray<u32>> indices, vertex_map;
    std::unique_ptr<DeviceArray<u32>> triangle_map;   // of a cleaning: the output triangle of every input triangle
    u32 vertices = 0, triangles = 0, rounds = 0;
    u32 filled_holes = 0;                             // of a hole filling
    DeviceMesh() = default;
    DeviceMesh(u32 v, u32 t) : positions(new DeviceArray<float>(size_t{3} * v)), normals(new DeviceArray<float>(size_t{3} * v)), colors(new DeviceArray<uchar4_t>(v)),
                               indices(new DeviceArray<u32>(size_t{3} * t)), vertices(v), triangles(t) {}
  };
  void FuseKeyframes(hipStream_t stream, const VolumeSpec& spec, float truncation);
  void ExtractMesh(hipStream_t stream, u32 min_count, Mesh* mesh);   // of the volume of the last FuseKeyframes
  // Extraction with clean-up (bslam_mesh_components, bslam_filter_mesh): the extracted mesh stays on the device, is labelled by
  // connected component -- vertices are joined iff a triangle holds both -- and, from min_component_vertices = 2 on, loses every
  // component of fewer vertices (flying pixels at occlusion edges, single noisy blobs) before the one download; the kept
  // vertices and triangles keep their order.  With min_component_vertices 0 or 1 and no report this is ExtractMesh(stream,
  // min_count, mesh): nothing else is launched.  The report describes the mesh as extracted, before anything was dropped.
  struct MeshOptions {
    u32 min_count = 1;
    u32 min_component_vertices = 0;
  };
  struct MeshComponentReport {
    u32 components = 0, removed_vertices = 0, removed_triangles = 0;
    std::vector<u32> sizes_descending;   // vertices per component
  };
  void ExtractMesh(hipStream_t stream, const MeshOptions& options, Mesh* mesh, MeshComponentReport* report = nullptr);
  // Components of a caller's mesh: labels[v] = the smallest vertex id of v's component, sizes[v] = its vertex count (either may
  // be null).  Returns the number of components.
  u32 MeshComponents(hipStream_t stream, const Mesh& mesh, std::vector<u32>* labels, std::vector<u32>* sizes);
  // Mesh simplification (bslam_simplify_mesh): vertex clustering on the uniform grid of cells of cell_size from origin.  All
  // vertices of a cell become one -- the mean position, the normalised normal sum, the rounded mean colour, each over the members
  // in ascending vertex id --, clusters are numbered in ascending (c_z, c_y, c_x), triangles are remapped and kept iff their three
  // clusters differ.  A mesh without triangles is a point cloud: voxel-grid down-sampling.  Every vertex has to lie at or above
  // origin and within 2^21 cells of it on every axis.
  // Host arrays: mesh.normals and mesh.colors may be empty, and so may mesh.indices; *out gets what the input has.  vertex_cluster
  // (may be null) receives the cluster of every input vertex.
  void SimplifyMesh(hipStream_t stream, const Mesh& mesh, const float origin[3], float cell_size, Mesh* out, std::vector<u32>* vertex_cluster);
  // The same on device arrays (4 byte aligned; normals and colors may be null; see bslam_simplify_mesh); the result stays on the
  // device, its vertex_map the cluster of every input vertex.
  DeviceMesh SimplifyMeshOnDevice(hipStream_t stream, u32 vertices, u32 triangles, const float* positions, const float* normals, const uchar4_t* colors,
                                  const u32* indices, const float origin[3], float cell_size);
  // Mesh decimation (bslam_decimate_mesh): quadric-error edge collapse in rounds of pairwise non-adjacent collapses until
  // target_vertices are left, no edge may collapse any more or max_rounds (0: no limit) have run.  Boundary edges are held by a
  // quadric of weight boundary_weight; an edge whose cost exceeds max_cost never collapses.
  struct DecimateOptions {
    u32 target_vertices = 0;
    float boundary_weight = 1.f;
    float max_cost = std::numeric_limits<float>::infinity();
    u32 max_rounds = 0;
  };
  // Host arrays: mesh.normals and mesh.colors may be empty; *out gets what the input has.  vertex_map (may be null) receives the
  // output vertex of every input vertex.  Returns the number of rounds.
  u32 DecimateMesh(hipStream_t stream, const Mesh& mesh, const DecimateOptions& options, Mesh* out, std::vector<u32>* vertex_map);
  // The same on device arrays (4 byte aligned; normals and colors may be null; see bslam_decimate_mesh); the result stays on the device.
  DeviceMesh DecimateMeshOnDevice(hipStream_t stream, u32 vertices, u32 triangles, const float* positions, const float* normals, const uchar4_t* colors,
                                  const u32* indices, const DecimateOptions& options);
  // Mesh smoothing (bslam_smooth_mesh): `iterations` of a one-ring step with lambda followed, unless mu is 0, by one with mu (Taubin;
  // mu = 0 is plain Laplacian smoothing), then vertex normals from the smoothed geometry.  Counts, indices and colours stay.  The
  // defaults have been tried on synthetic meshes only and are provisional.
  enum SmoothBoundary : u32 { kSmoothFixed = 0, kSmoothRim = 1, kSmoothFree = 2 };   // boundary vertices: held, smoothed along the rim, smoothed like any other
  struct SmoothOptions {
    u32 iterations = 10;
    float lambda = 0.5f, mu = -0.53f;
    SmoothBoundary boundary = kSmoothFixed;
  };
  // Host arrays: mesh.normals (the fall-back where the geometry gives no normal) and mesh.colors may be empty; *out gets new positions
  // and normals, and the input's colours and indices.
  void SmoothMesh(hipStream_t stream, const Mesh& mesh, const SmoothOptions& options, Mesh* out);
  // The same on the mesh the last ExtractMesh left on the device, which stays as it is; the result -- positions and normals -- stays
  // on the device.
  DeviceMesh SmoothMeshOnDevice(hipStream_t stream, const SmoothOptions& options);
  // ... and on a caller's device arrays (4 byte aligned; normals may be null; see bslam_smooth_mesh).
  DeviceMesh SmoothMeshOnDevice(hipStream_t stream, u32 vertices, u32 triangles, const float* positions, const float* normals, const u32* indices,
                                const SmoothOptions& options);
  // Mesh repair (bslam_clean_mesh): with weld, vertices with equal coordinates become the one with the smallest id; triangles that repeat a
  // vertex are dropped; with remove_duplicates, of the triangles on the same three vertices the first stays; with remove_unreferenced,
  // vertices that no surviving triangle names are dropped (never those of a point cloud).  What stays keeps its order and its bits.
  struct CleanOptions {
    bool weld = true, remove_duplicates = true, remove_unreferenced = true;
  };
  struct CleanReport {
    u32 welded_vertices = 0, unreferenced_vertices = 0, degenerate_triangles = 0, duplicate_triangles = 0;
  };
  // Host arrays: mesh.normals and mesh.colors may be empty; *out gets what the input has.  vertex_map and triangle_map (may be null)
  // receive the output id of every input vertex and triangle, 0xffffffff where it was dropped; report may be null.
  void CleanMesh(hipStream_t stream, const Mesh& mesh, const CleanOptions& options, Mesh* out, std::vector<u32>* vertex_map, std::vector<u32>* triangle_map,
                 CleanReport* report);
  // The same on device arrays (4 byte aligned; normals and colors may be null; see bslam_clean_mesh); the result stays on the device.
  DeviceMesh CleanMeshOnDevice(hipStream_t stream, u32 vertices, u32 triangles, const float* positions, const float* normals, const uchar4_t* colors, const u32* indices,
                               const CleanOptions& options, CleanReport* report);
  // The census of the edges and boundary loops of mesh.indices (bslam_mesh_topology); edge_uses and loop_of_slot, one entry per
  // triangle corner, may be null.  Triangles that repeat a vertex are refused: clean first.
  void MeshTopology(hipStream_t stream, const Mesh& mesh, bslam_mesh_report* report, std::vector<u32>* edge_uses, std::vector<u32>* loop_of_slot);
  // The same of index triples over vertex_count vertices, for a caller that has no positions at hand.
  void MeshTopology(hipStream_t stream, size_t vertex_count, const std::vector<u32>& indices, bslam_mesh_report* report, std::vector<u32>* edge_uses,
                    std::vector<u32>* loop_of_slot);
  // Hole filling (bslam_fill_mesh_holes): every boundary loop of at most max_hole_edges (3 .. 4096) edges gets a vertex at the centroid of
  // its vertices and a fan of triangles; the input comes first and unchanged.  Returns the number of holes filled.
  u32 FillMeshHoles(hipStream_t stream, const Mesh& mesh, u32 max_hole_edges, Mesh* out);
  // The same on device arrays; two calls, the first for the counts.  The result stays on the device.
  DeviceMesh FillMeshHolesOnDevice(hipStream_t stream, u32 vertices, u32 triangles, const float* positions, const float* normals, const uchar4_t* colors,
                                   const u32* indices, u32 max_hole_edges);
  // Mesh orientation (bslam_orient_mesh): every orientable patch -- triangles joined over edges that two triangles use -- gets one
  // winding, and `mode` says which: the one most of its triangles have, the one the vertex normals vote for (mesh.normals is needed),
  // or the one with a positive enclosed volume (closed patches; others fall back to the majority).  A patch that cannot be oriented
  // stays as it is.  *indices gets the triangles in their order, a flipped one (a, b, c) as (a, c, b); flipped (0 / 1) and
  // patch_of_triangle (the smallest triangle id of the patch) have one entry per triangle and may be null, and so may report.
  enum OrientMode : int { kOrientMajority = 0, kOrientNormals = 1, kOrientVolume = 2 };
  void OrientMesh(hipStream_t stream, const Mesh& mesh, OrientMode mode, std::vector<u32>* indices, std::vector<u8>* flipped, std::vector<u32>* patch_of_triangle,
                  bslam_orient_report* report);
  // Surface evaluation (bslam_point_mesh_distance): the distance of every point to the nearest triangle of a mesh within
  // max_distance, +infinity and triangle 0xffffffff beyond.  cell_size 0: the grid cell starts at max_distance and doubles while
  // the call reports that the grid exceeds max_grid_entries (or its cap on the cells); the result names the cell that was used.
  struct PointMeshOptions {
    float max_distance = 0.1f;
    float cell_size = 0.f;
    uint64_t max_grid_entries = 1ull << 28;
  };
  struct PointMeshResult {
    std::vector<float> distance;
    std::vector<u32> triangle;
    float cell_size = 0.f;
    uint64_t grid_cells = 0, grid_entries = 0;
  };
  // Host arrays: points float[3 point_count] and a mesh whose normals and colours are not looked at; a point cloud is a mesh with
  // the triangles (i, i, i).
  void PointMeshDistance(hipStream_t stream, const float* points, size_t point_count, const Mesh& mesh, const PointMeshOptions& options, PointMeshResult* result);
  // The same on device arrays (4 byte aligned; see bslam_point_mesh_distance); the results are downloaded.
  void PointMeshDistanceOnDevice(hipStream_t stream, size_t point_count, const float* points, u32 vertices, const float* positions, u32 triangles,
                                 const u32* indices, const PointMeshOptions& options, PointMeshResult* result);
  // Nearest triangle (bslam_nearest_triangle): the same distance through a bounding-volume hierarchy, for any max_distance > 0,
  // +infinity included: no radius, every point hits a mesh that has a valid triangle.  leaves: the valid triangles; height: of the tree.
  struct NearestTriangleResult {
    std::vector<float> distance;
    std::vector<u32> triangle;
    u32 leaves = 0, height = 0;
  };
  void NearestTriangle(hipStream_t stream, const float* points, size_t point_count, const Mesh& mesh, float max_distance, NearestTriangleResult* result);
  // Mesh rays (bslam_mesh_rays): what each of ray_count rays (host arrays: origins and directions float[3 n], t_range float[2 n] or
  // null for [0, +inf]) hits on `mesh`.  Closest hit fills t (+inf: a miss), triangle (0xffffffff), uv and front; any_hit fills hit alone.
  struct RayCastResult {
    std::vector<float> t, uv;
    std::vector<u32> triangle;
    std::vector<uint8_t> front, hit;
    u32 leaves = 0, height = 0;
  };
  void RayCastMesh(hipStream_t stream, const float* origins, const float* directions, const float* t_range, size_t ray_count, const Mesh& mesh, bool any_hit,
                   RayCastResult* result);
  // Visible points (bslam_mesh_visibility): from how many of the views each point (host arrays: points and, or null, normals
  // float[3 n]) is seen past `mesh`, and the lowest such view (0xffffffff: none).  A view is camera_T_global and its centre, the
  // translation of global_T_camera; the second form derives both from global_T_camera poses as RenderMesh does.
  struct VisibilityOptions {
    float min_depth = 0.05f, max_depth = 50.f, margin = 0.02f;
  };
  struct VisibilityResult {
    std::vector<u32> count, first;
    u32 leaves = 0, height = 0;
  };
  void MeshVisibility(hipStream_t stream, const float* points, const float* normals, size_t point_count, const Mesh& mesh, const std::vector<bslam_mat3x4>& camera_T_global,
                      const std::vector<float>& centres, const PinholeCamera4f& camera, const VisibilityOptions& options, VisibilityResult* result);
  void MeshVisibility(hipStream_t stream, const float* points, const float* normals, size_t point_count, const Mesh& mesh, const std::vector<SE3f>& global_T_camera,
                      const PinholeCamera4f& camera, const VisibilityOptions& options, VisibilityResult* result);
  // The centres of the valid surfels (the points of ExportToPointCloud, in its order) against the mesh the last ExtractMesh
  // returned, which stays on the device for this: how far the surfels that bundle adjustment optimised lie from the surface the
  // volume produced -- a consistency figure that needs no ground truth.  Throws std::logic_error if no mesh was extracted.
  void SurfelMeshDistance(hipStream_t stream, const PointMeshOptions& options, PointMeshResult* result);
  // Surface sampling (bslam_sample_mesh): points drawn uniformly by area, `density` per square unit on average, a function of
  // (seed, triangle, ordinal within the triangle) alone; ordered by triangle.  Degenerate triangles -- a point cloud -- yield nothing.
  struct MeshSamples {
    std::vector<float> positions, normals;   // 3 per sample; the normal is the triangle's, cross(b - a, c - a) normalised
    std::vector<u32> triangles;              // 1 per sample
    size_t count() const { return triangles.size(); }
  };
  struct DeviceSamples {   // the same on the device
    std::unique_ptr<DeviceArray<float>> positions, normals;
    std::unique_ptr<DeviceArray<u32>> triangles;
    uint64_t count = 0;
  };
  // Host arrays: the count call, the allocation, the emit call and one download.
  void SampleMesh(hipStream_t stream, const Mesh& mesh, float density, u32 seed, MeshSamples* samples);
  // The same on device arrays (4 byte aligned; see bslam_sample_mesh); the samples stay on the device, where
  // PointMeshDistanceOnDevice takes them as its points.
  DeviceSamples SampleMeshOnDevice(hipStream_t stream, u32 vertices, const float* positions, u32 triangles, const u32* indices, float density, u32 seed);
  // ... of the mesh the last ExtractMesh returned, which is still on the device.  Throws std::logic_error if no mesh was extracted.
  DeviceSamples SampleMeshOnDevice(hipStream_t stream, float density, u32 seed);
  // Surface registration (bslam_registration_prepare / bslam_registration_step): the rigid motion target_T_source that lays the
  // points onto the mesh, by iterative closest point from `initial`.  The points are uploaded and the mesh is prepared once, at
  // max_distance (with the cell doubling of PointMeshDistance while over budget); stages run at the radii max_distance, shrink *
  // that, ... down to min_distance, each until the step falls below kRegistrationStepTranslation / Rotation or
  // iterations_per_stage steps were taken.  Per step the normal equations come from the device, delta = (translation, rotation)
  // solves H delta = -b (SolveLDLTUpper) and the estimate becomes Exp(delta) * estimate, in double.  A mesh without triangles is a
  // point cloud: every vertex is the triangle (i, i, i).  The defaults below -- and the stage schedule -- are provisional: they
  // were tried on synthetic scenes only.
  static constexpr double kRegistrationStepTranslation = 1e-5;   // metres: IsScale1PoseEstimationConverged's form of test, the
  static constexpr double kRegistrationStepRotation = 1e-6;      // rotation weighing 10 x, at a scale that fits a scan in metres
  static constexpr double kRegistrationSingularShare = 1e-5;     // a pivot that keeps less of its variable's diagonal: singular
  struct RegistrationOptions {
    float max_distance = 0.1f;
    float min_distance = 0.f;          // 0: max_distance / 8
    int mode = -1;                     // BSLAM_REGISTRATION_PLANE / _POINT; -1: PLANE for a mesh with triangles, POINT for a cloud
    float huber = 0.f;                 // 0: half the radius of the stage
    double shrink = 0.5;
    int iterations_per_stage = 20;
    float cell_size = 0.f;
    uint64_t max_grid_entries = 1ull << 28;
    double initial[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // row-major 4 x 4
  };
  struct RegistrationStep {
    double radius = 0.0;
    uint64_t hits = 0, used = 0;
    double cost = 0.0, rmse = 0.0;                                // rmse: sqrt(sum r^2 / used); NaN without a pair
    double step_translation = 0.0, step_rotation = 0.0;           // norms of the step's parts; NaN when none was taken
  };
  enum RegistrationEnd { kRegistrationConverged = 0, kRegistrationIterationsExhausted = 1, kRegistrationTooFewPairs = 2, kRegistrationSingular = 3 };
  static const char* RegistrationReason(int end);
  struct RegistrationResult {
    double target_T_source[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    bool converged = false;            // the last stage ended by the convergence test
    int end = kRegistrationIterationsExhausted;
    std::vector<RegistrationStep> history;   // one entry per step
    float cell_size = 0.f;
    uint64_t grid_cells = 0, grid_entries = 0;
  };
  // Too few pairs (< 6) or a singular system end the loop: converged = false, the last valid estimate is returned, nothing throws.
  void RegisterPoints(hipStream_t stream, const float* points, size_t point_count, const Mesh& mesh, const RegistrationOptions& options, RegistrationResult* result);
  void Volume(hipStream_t stream, VolumeData* volume) const;         // download of that volume
  // Views of the volume of the last FuseKeyframes from a pose (bslam_raycast_volume): per pixel the first front-facing zero
  // crossing of the trilinear interpolant along the ray, as depth (units of a keyframe's depth image), colour and normal -- no
  // holes where surfels are sparse, comparable pixel by pixel with a keyframe's depth image.  Samples seen by fewer than
  // min_count keyframes are unobserved.  The object owns the prepared aux buffer and prepares it again only after a new fusion
  // or for a new min_count; the device images are those of RenderModel.  Throws std::logic_error if nothing was fused.
  struct VolumeViewOptions {
    float min_depth = 0.05f, max_depth = 50.f;   // metres of depth; at most 65536 steps between them
    float step = 0.f;                            // metres of depth between samples; 0: the voxel size
    u32 min_count = 1;
    bool depth = true, color = true, normal = false;   // the views wanted, at least one
  };
  void RenderVolume(hipStream_t stream, const SE3f& global_T_camera, const PinholeCamera4f& camera, const VolumeViewOptions& options, ModelViews* views);
  // Views of a triangle mesh from a pose (bslam_render_mesh): the nearest triangle per pixel as depth (units of a keyframe's depth
  // image), triangle id, perspective-correct colour and normal -- of the result of ExtractMesh, SmoothMesh, SimplifyMesh, DecimateMesh
  // or LoadPLY alike.  Without vertex normals the normal view shows face normals; a colour view of a mesh without colours throws
  // std::invalid_argument.  The mesh is uploaded per call; the device images are those of RenderModel.
  struct MeshViewOptions {
    float min_depth = 0.05f, max_depth = 50.f;   // metres; a triangle with a vertex outside the range is dropped, not clipped
    bool cull_backfaces = true;                  // draw only triangles seen counter-clockwise (from free space, for an extracted mesh)
    bool depth = true, index = false, color = true, normal = false;   // the views wanted, at least one
  };
  void RenderMesh(hipStream_t stream, const Mesh& mesh, const SE3f& global_T_camera, const PinholeCamera4f& camera, const MeshViewOptions& options, ModelViews* views);
  // Axis-aligned box of the valid (non-NaN) surfels; false when there is none.
  bool ModelBounds(hipStream_t stream, float min[3], float max[3]) const;

  // Place recognition (host/place_recognition.hpp; the methods are defined in place_recognition.cpp).  The database of
  // keyframe features is created by the first of these calls; an object that never calls them allocates and launches
  // nothing for it.
  // Extracts keyframe_id's features into its database slot and, with xy and desc given, downloads them: xy[cells],
  // desc[cells][8] as bslam_extract_keyframe_features writes them.
  void ExtractKeyframeFeatures(hipStream_t stream, int keyframe_id, int64_t score_threshold, std::vector<u32>* xy, std::vector<u32>* desc);
  // One match launch of keyframe query_id against the extracted keyframes `ids`: match[ids.size()][cells], count[ids.size()].
  void MatchKeyframeFeatures(hipStream_t stream, int query_id, const std::vector<int>& ids, int max_distance, std::vector<int32_t>* match, std::vector<u32>* count);
  // Adds every keyframe up to current_id that the database lacks, picks the candidate (PlaceRecognizer::Query), estimates
  // old_T_cur from the matched pixels' depths (EstimateRelativePose) and hands it to CloseLoop.  Keyframe poses change
  // only when result->loop.status is kLoopClosed.
  void RecognizePlace(hipStream_t stream, int current_id, const PlaceRecognitionOptions& options, int num_scales, PlaceRecognitionResult* result);
  PlaceRecognizer& place_recognizer();
  void ResetPlaceRecognizer();   // releases the database

  // The objective the BA minimises (bslam_compute_ba_cost: Tukey depth terms and kDescWeight * Huber on both descriptor
  // residuals) at the keyframes' current poses, intrinsics and cfactors: every non-deleted keyframe whatever its activation, every
  // non-deleted surfel -- with active_surfels_only, only those the last geometry step flagged active.  Only reads the scene.
  struct CostReport {
    std::vector<int> keyframe_ids;
    std::vector<float> cost;        // 2 per keyframe: depth, descriptor
    std::vector<uint32_t> counts;   // 2 per keyframe: depth-associated pairs, pairs with valid descriptor residuals
    double depth_total = 0, descriptor_total = 0;
    double total() const { return depth_total + descriptor_total; }
  };
  void ComputeCost(hipStream_t stream, bool active_surfels_only, CostReport* report);
  // Off by default.  On: BundleAdjustment (alternating and PCG) evaluates the objective before its first iteration and after
  // every iteration into cost_history(), which each BundleAdjustment call restarts.  The poses and surfels it computes do not
  // change (the evaluation only reads); it costs one surfel x keyframe pass and a host round trip per iteration.
  void SetCostTracking(bool enable) { cost_tracking_ = enable; }
  const std::vector<CostReport>& cost_history() const { return cost_history_; }

  // Scene state in / out.
  void SetSurfels(hipStream_t stream, const float* host_rows, size_t host_pitch_bytes, u32 count);
  void GetSurfels(hipStream_t stream, float* host_rows, size_t host_pitch_bytes, int rows) const;
  void GetActiveSurfels(hipStream_t stream, u8* host) const;

  // Pose phase of the alternating scheme: true (default) = all keyframes advance in lock-step in
  // one launch per Gauss-Newton iteration (bslam_estimate_frame_poses_batched); false = the
  // reference's sequential EstimateFramePose calls.
  void SetBatchedPoseOptimization(bool enable) { batched_pose_optimization_ = enable; }
  // PerformBASchemeEndTasks (merge / delete / radius update / compaction at the end of a BA scheme) is on as in the
  // reference; switching it off keeps the surfel set fixed across BundleAdjustment calls (parity tests against plain loops).
  void SetSchemeEndTasks(bool enable) { scheme_end_tasks_ = enable; }
  // DirectBA::CreateSurfelsForKeyframe (BS/direct_ba.h:118-121)
  void CreateSurfelsForKeyframe(hipStream_t stream, bool filter_new_surfels, const std::shared_ptr<Keyframe>& keyframe);
  // new Keyframe(stream, frame_index, depth_params(), depth_camera(), depth_image, color_image, pose) + AddKeyframe
  // (the idiom of the reference's tests, e.g. BS/test/test_pose_optimization_geometric_residual.cc:108-118)
  std::shared_ptr<Keyframe> AddKeyframeFromImages(hipStream_t stream, u32 frame_index, const u16* depth_image, const u8* rgb_image, const SE3f& global_T_frame);
  // The reference picks the PCG gauge keyframe with rand() % K (BS/direct_ba_pcg.cc:328); a fixed
  // id >= 0 makes runs reproducible.
  void SetPCGGaugeKeyframe(int id) { fixed_gauge_keyframe_ = id; }
  void SetTextureMode(int mode);
  // Must be called after rewriting the content of a keyframe's depth / normal image or of the
  // cfactor image in place (the class does it itself for the changes it makes).
  void InvalidateKeyframeCache();
  void SetTimingsStream(std::ostream* s) { timings_stream_ = s; }   // --save_timings format of BS/direct_ba_alternating.cc:630-688
  // Surfel-sharded multi-GPU runs: `fn` sums device buffers across ranks (RCCL / torch.distributed); it is
  // used by the batched pose step and, through the context, by the PCG and intrinsics entry points.
  void SetAllReduce(bslam_allreduce_fn fn, void* user);
  // The library's own exchange: an RCCL communicator in this DirectBA's kernel context (bslam_comm_init).  rank 0 obtains the
  // 128-byte id with bslam_comm_get_unique_id and hands it to every rank; after InitComm every BA scheme of this object
  // (alternating pose step, PCG, intrinsics) sums its shared quantities over the ranks on the BA stream -- no callback.
  void InitComm(const void* unique_id, int rank, int world_size);
  void DestroyComm();

  void Lock() const { ba_thread_mutex_.lock(); }
  void Unlock() const { ba_thread_mutex_.unlock(); }
  const std::vector<std::shared_ptr<Keyframe>>& keyframes() const { return keyframes_; }
  const PinholeCamera4f& depth_camera() const { return depth_camera_; }
  const PinholeCamera4f& color_camera() const { return color_camera_; }
  bslam_depth_params depth_params() const;
  float a() const { return a_; }
  void SetA(float a) { a_ = a; }
  void SetDepthCamera(const PinholeCamera4f& camera) { depth_camera_ = camera; }   // BS/direct_ba.h (used by the intrinsics tests)
  void SetColorCamera(const PinholeCamera4f& camera) { color_camera_ = camera; }
  const DeviceBuffer<float>& cfactor_buffer() const { return *cfactor_buffer_; }
  // host row-major cfactor image -> device (LoadCalibration, BS/io.cc:694); invalidates the derived records
  void UploadCFactor(hipStream_t stream, const float* host) {
    cfactor_buffer_->Upload(stream, host, static_cast<size_t>(cfactor_buffer_->width()) * sizeof(float));
    InvalidateKeyframeCache();
  }
  u32 surfels_size() const { return surfels_size_; }
  u32 surfel_count() const { return surfel_count_; }
  const DeviceBuffer<float>& surfels() const { return *surfels_; }
  bool use_depth_residuals() const { return use_depth_residuals_; }
  bool use_descriptor_residuals() const { return use_descriptor_residuals_; }
  int ba_iteration_count() const { return ba_iteration_count_; }
  int last_ba_iteration_count() const { return last_ba_iteration_count_; }
  void SetBAIterationCounts(int count, int last) { ba_iteration_count_ = count; last_ba_iteration_count_ = last; }   // LoadState, BS/io.cc:466-467
  int max_surfel_count() const { return surfels_->width(); }
  int min_observation_count_while_bootstrapping_1() const { return min_observation_count_while_bootstrapping_1_; }
  int min_observation_count_while_bootstrapping_2() const { return min_observation_count_while_bootstrapping_2_; }
  int min_observation_count() const { return min_observation_count_; }
  float surfel_merge_dist_factor() const { return surfel_merge_dist_factor_; }
  int GetMinObservationCount() const {   // BS/direct_ba.h:212-218
    return (keyframes_.size() < 10) ? ((keyframes_.size() < 5) ? min_observation_count_while_bootstrapping_1_
                                                              : min_observation_count_while_bootstrapping_2_)
                                    : min_observation_count_;
  }
  bslam_context* context() const { return ctx_; }

 private:
  void BundleAdjustmentAlternating(hipStream_t stream, bool optimize_depth_intrinsics, bool optimize_color_intrinsics, bool do_surfel_updates,
                                   bool optimize_poses, bool optimize_geometry, int min_iterations, int max_iterations,
                                   int active_keyframe_window_start, int active_keyframe_window_end, bool increase_ba_iteration_count,
                                   int* num_iterations_done, bool* converged, double time_limit, std::function<bool(int)> progress_function);
  void BundleAdjustmentPCG(hipStream_t stream, bool optimize_depth_intrinsics, bool optimize_color_intrinsics, bool do_surfel_updates,
                           bool optimize_poses, bool optimize_geometry, int min_iterations, int max_iterations, int max_inner_iterations,
                           int max_keyframe_count, int active_keyframe_window_start, int active_keyframe_window_end,
                           bool increase_ba_iteration_count, int* num_iterations_done, bool* converged, double time_limit,
                           std::function<bool(int)> progress_function);
  void DetermineNewKeyframeCoVisibility(const std::shared_ptr<Keyframe>& new_keyframe);   // BS/direct_ba.cc:231-249
  void DetermineCovisibleActiveKeyframes();                                               // BS/direct_ba.cc:548-564
  std::vector<bslam_keyframe_view> KeyframeViews() const;
  // Merge for the keyframes last active in this BA iteration, DeleteSurfelsAndUpdateRadii, Compact (BS/direct_ba.cc:566-653)
  void PerformBASchemeEndTasks(hipStream_t stream, bool do_surfel_updates);
  // DetermineSupportingSurfelsAndMergeSurfelsCUDA for the given keyframes, then CompactSurfelsCUDA incl. the active flags
  // (BS/direct_ba_alternating.cc:486-533)
  void MergeAndCompact(hipStream_t stream, const std::vector<u32>& keyframe_ids);
  void Check(int rc, const char* what) const;

  bslam_context* ctx_ = nullptr;
  int device_;
  PinholeCamera4f color_camera_, depth_camera_;
  int pyramid_level_for_color_;
  bool use_depth_residuals_, use_descriptor_residuals_;
  int min_observation_count_while_bootstrapping_1_, min_observation_count_while_bootstrapping_2_, min_observation_count_;
  float surfel_merge_dist_factor_;
  SE3f global_T_anchor_frame_;
  float a_ = 0.f, raw_to_float_depth_, baseline_fx_;
  int sparse_surfel_cell_size_;
  std::unique_ptr<DeviceBuffer<float>> cfactor_buffer_;
  std::unique_ptr<DeviceBuffer<float>> surfels_;
  std::unique_ptr<DeviceBuffer<u8>> active_surfels_;
  u32 surfels_size_ = 0, surfel_count_ = 0;
  int ba_iteration_count_ = 0, last_ba_iteration_count_ = -1;
  std::vector<std::shared_ptr<Keyframe>> keyframes_;
  mutable std::mutex ba_thread_mutex_;
  // PCG vectors, allocated lazily (BS/direct_ba_pcg.cc:255-268)
  std::unique_ptr<DeviceBuffer<float>> pcg_r_, pcg_M_, pcg_delta_, pcg_g_, pcg_p_, pcg_scalars_;
  bool cost_tracking_ = false;
  std::vector<CostReport> cost_history_;
  void TrackCost(hipStream_t stream);   // appends ComputeCost(stream, false) to cost_history_ when tracking is on
  bool batched_pose_optimization_ = true;
  bool scheme_end_tasks_ = true;
  int fixed_gauge_keyframe_ = -1;
  std::ostream* timings_stream_ = nullptr;
  // device images of RenderModel, re-allocated when the camera's size changes
  std::unique_ptr<DeviceBuffer<u16>> render_depth_;
  std::unique_ptr<DeviceBuffer<u32>> render_index_;
  std::unique_ptr<DeviceBuffer<uchar4_t>> render_color_;
  std::unique_ptr<DeviceBuffer<float>> render_normal_;   // 3 floats per pixel
  std::unique_ptr<PlaceRecognizer> place_recognizer_;   // null until place recognition is used
  // device volume of FuseKeyframes: nz * ny rows of nx elements each; null until fusion is used
  std::unique_ptr<DeviceBuffer<float>> volume_tsdf_;
  std::unique_ptr<DeviceBuffer<u32>> volume_count_;
  std::unique_ptr<DeviceBuffer<uchar4_t>> volume_color_;
  VolumeSpec volume_spec_;
  float volume_truncation_ = 0.f;
  // the fused volume as the library takes it; throws "<caller>: no fused volume (call FuseKeyframes first)" if there is none
  struct FusedVolume { bslam_volume vol; bslam_buffer2d tsdf, count, color; };
  FusedVolume Fused(const char* caller) const;
  // prepared aux buffer of RenderVolume and the min_count it was prepared for (0: stale -- a new fusion, or never prepared)
  std::unique_ptr<DeviceArray<u8>> volume_aux_;
  u32 volume_aux_min_count_ = 0;
  // The views a render call wants: ViewImages gives their render_*_ images the camera's size and fills pods[] (depth, index,
  // colour, normal) for them; DownloadViews copies them into `views`, whose size is set.
  struct ViewSet { bool depth, index, color, normal; };
  void ViewImages(int w, int h, const ViewSet& want, bslam_buffer2d pods[4]);
  void DownloadViews(hipStream_t stream, const ViewSet& want, ModelViews* views) const;
  // Which arrays of a host mesh a call takes to the device.
  enum MeshPart : unsigned { kMeshPositions = 1, kMeshNormals = 2, kMeshColors = 4, kMeshIndices = 8, kMeshAll = 15 };
  // Throws std::invalid_argument in the name of `who` unless positions and indices hold whole vertices and triangles and, like a
  // caller's `points` points, fit one device image, and the normals and colours `what` names have one entry per vertex or none.
  static void CheckMeshSizes(const Mesh& mesh, const char* who, unsigned what, size_t points = 0);
  // CheckMeshSizes in the name of `who` (null: the caller has checked by a rule of its own), then uploads the parts `what` names
  // -- normals and colours only where the mesh has them; `indices`, when given, in place of the mesh's -- and waits once: the host
  // arrays are the caller's and pageable.
  DeviceMesh UploadMesh(hipStream_t stream, const Mesh& mesh, const char* who, unsigned what, const std::vector<u32>* indices = nullptr);
  // The `vertices` and `triangles` in use of what `mesh` holds into *out, sized to fit, and its vertex map into *map (may be null);
  // everything is enqueued, then the stream is waited for once.
  void DownloadMesh(hipStream_t stream, const DeviceMesh& mesh, Mesh* out, std::vector<u32>* map);
  // The extraction: the count call, the allocations and the emit call.  Forgets the kept mesh once the count call is through.
  DeviceMesh ExtractDeviceMesh(hipStream_t stream, u32 min_count);
  // device copy of the mesh the last ExtractMesh returned (positions 3 V floats, indices 3 T), for SurfelMeshDistance
  std::unique_ptr<DeviceArray<float>> mesh_positions_;
  std::unique_ptr<DeviceArray<u32>> mesh_indices_;
  u32 mesh_vertices_ = 0, mesh_triangles_ = 0;
  bool mesh_extracted_ = false;
  void KeepDeviceMesh(DeviceMesh mesh);   // keeps its positions and indices
  // xyz of the valid surfels (a deleted one carries NaN in x), in the order of ExportToPointCloud
  std::vector<float> ValidSurfelCentres(hipStream_t stream) const;
  bool comm_ = false, sharded_ = false;
  bslam_allreduce_fn allreduce_ = nullptr;
  void* allreduce_user_ = nullptr;
  // phase timing (BS/direct_ba.h:513-532)
  // phase timing events of a BA iteration (--save_timings lines): [0,1] activation, [2,3] geometry, [4,5] poses, [6,7] PCG,
  // [8,9] surfel creation, [10,11] initial surfel merge, [12,13] surfel compaction, [14,15] intrinsics
  hipEvent_t ev_[16];
};

}  // namespace bslam_host
