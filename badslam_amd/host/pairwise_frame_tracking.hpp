// pairwise_frame_tracking.hpp -- host side of the odometry: the coarse-to-fine direct alignment
// of a tracked frame against a base keyframe.  Mirrors vis::TrackFramePairwise (BS/pairwise_frame_tracking.cc:256-678)
// with both of its switches (use_pyramid_level_0, use_gradmag; BadSlam::RunOdometry passes true / false), plus the input
// preparation BadSlam::RunOdometry does before the call (BS/bad_slam.cc:859-897).  The kernels are behind the C ABI (include/badslam_hip.h, odometry section).
#pragma once

#include <memory>
#include <vector>

#include "direct_ba.hpp"

namespace bslam_host {

// vis::PairwiseFrameTrackingBuffers (BS/pairwise_frame_tracking.h): per-scale images of both frames.  Everything has the
// depth image's size halved per scale, except tracked_color, which has the colour image's (the two cameras may differ).
struct PairwiseFrameTrackingBuffers {
  PairwiseFrameTrackingBuffers(int depth_width, int depth_height, int color_width, int color_height, int num_scales);
  int num_scales;
  std::vector<std::unique_ptr<DeviceBuffer<float>>> base_depth, tracked_depth;
  std::vector<std::unique_ptr<DeviceBuffer<u16>>> base_normals, tracked_normals;   // level 0 unused: the frames' own buffers
  std::vector<std::unique_ptr<DeviceBuffer<u8>>> base_color, tracked_color;
  std::unique_ptr<DeviceBuffer<u8>> base_gradmag, tracked_gradmag;                  // luma of the two uchar4 images
};

// out_base_T_frame: pose of the tracked frame in the base frame.  iterations_per_scale (may be null) receives
// num_scales entries.  Inputs are the keyframe-format device images (depth u16, normals u16, colour uchar4).
void TrackFramePairwise(bslam_context* ctx, hipStream_t stream, PairwiseFrameTrackingBuffers* buffers, const PinholeCamera4f& color_camera,
                        const PinholeCamera4f& depth_camera, const bslam_depth_params& depth_params, bool use_depth_residuals,
                        bool use_descriptor_residuals, const DeviceBuffer<u16>& tracked_depth, const DeviceBuffer<u16>& tracked_normals,
                        const DeviceBuffer<uchar4_t>& tracked_color, const DeviceBuffer<u16>& base_depth, const DeviceBuffer<u16>& base_normals,
                        const DeviceBuffer<uchar4_t>& base_color, bool test_different_initial_estimates, const SE3f& base_T_frame_initial_estimate_1,
                        const SE3f& base_T_frame_initial_estimate_2, SE3f* out_base_T_frame, int* iterations_per_scale,
                        bool use_pyramid_level_0 = true, bool use_gradmag = false);

// Keyframe-format device images of one tracked frame.
struct TrackedFrameImages {
  const DeviceBuffer<u16>* depth;
  const DeviceBuffer<u16>* normals;
  const DeviceBuffer<uchar4_t>* color;
};

// Loop verification (BS/loop_detector.cc:495-546): tracks tracked.size() (1..BSLAM_MAX_PAIR_BATCH) frames against ONE base
// frame in lockstep, with test_different_initial_estimates = false, use_pyramid_level_0 = true, use_gradmag = false.
// The base pyramid is built once.  Each Gauss-Newton iteration makes one bslam_accumulate_pose_coeffs_from_images_batched
// call over the pairs still iterating at that scale; each pair keeps its own damping, solve, convergence test and
// iteration count, so out_base_T_frame[p] and iterations_per_scale[p] are bit-identical to a TrackFramePairwise call of
// pair p alone.  buffers: grown to tracked.size() entries if shorter (entry 0 also holds the base pyramid).
void TrackFramesPairwiseBatched(bslam_context* ctx, hipStream_t stream, std::vector<std::unique_ptr<PairwiseFrameTrackingBuffers>>* buffers, int num_scales,
                                const PinholeCamera4f& color_camera, const PinholeCamera4f& depth_camera, const bslam_depth_params& depth_params,
                                bool use_depth_residuals, bool use_descriptor_residuals, const std::vector<TrackedFrameImages>& tracked,
                                const DeviceBuffer<u16>& base_depth, const DeviceBuffer<u16>& base_normals, const DeviceBuffer<uchar4_t>& base_color,
                                const std::vector<SE3f>& base_T_frame_initial_estimates, std::vector<SE3f>* out_base_T_frame,
                                std::vector<std::vector<int>>* iterations_per_scale);

}  // namespace bslam_host
