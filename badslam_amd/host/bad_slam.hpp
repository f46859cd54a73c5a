// bad_slam.hpp -- the sequential front end around DirectBA: vis::BadSlam (BS/bad_slam.{h,cc}) without its threads,
// GUI and loop detector.  Per frame: device preprocessing (BS/bad_slam.cc:639-760), pairwise tracking against the last
// keyframe with the constant-motion initial estimates (:763-950), a keyframe every `keyframe_interval` frames
// (:953-1097) and the planned bundle-adjustment iterations (:212-282, :481-536), after which the poses of the
// non-keyframes follow their neighbouring keyframes (BS/trajectory_deformation.cc:45-146).
//
// Loop closure: CloseLoop (host/loop_closure.hpp) for a caller-supplied candidate; an opt-in geometric candidate
// search (SetLoopCandidateSearch) that closes drift within the tracker's basin; and opt-in place recognition
// (SetPlaceRecognition, host/place_recognition.hpp), which finds the candidate and the start pose from the images alone
// and so closes drift of any size.
//
// Input conditioning (BS/bad_slam.cc:645-685): median_filter_and_densify_iterations, pyramid_level_for_depth and
// pyramid_level_for_color (each level 0 ... 3) run as kernels on the uploaded full-resolution frame, where the
// reference works on the host.  As there, median iterations and a depth level exclude each other.  The two streams may
// use different levels (cameras of different sizes).
//
// Sensor rectification (SetSensorRectification, off by default): the frames arrive as a raw sensor streams them, from a
// distorted colour camera and a distorted depth camera beside it, and are undistorted / reprojected into the cameras
// of this object on the stream, in front of the input conditioning (the reference: host code in its input threads,
// BS/undistortion.cc and BS/input_structure.cc:196-298).
//
// Not built: parallel_ba (BA thread), real-time pacing (target_frame_rate), the reference's own loop detector (DBoW2
// vocabulary, opengv RANSAC; enable_loop_detection stays off -- SetPlaceRecognition is this project's stand-in), keyframe
// merging on low memory.  Those switches must keep their "off" values.
#pragma once

#include <memory>
#include <vector>

#include "direct_ba.hpp"
#include "io.hpp"
#include "loop_closure.hpp"
#include "pairwise_frame_tracking.hpp"
#include "place_recognition.hpp"
#include "rectification.hpp"

namespace bslam_host {

class BadSlam {
 public:
  // config: BS/bad_slam_config.h (defaults of BadSlamConfigV1).  Cameras in the pixel-corner convention of
  // PinholeCamera4f, already scaled to the pyramid levels in use (config.pyramid_level_for_color / _depth).
  BadSlam(const BadSlamConfigV1& config, const PinholeCamera4f& color_camera, const PinholeCamera4f& depth_camera, int device = 0);
  ~BadSlam();

  // vis::BadSlam::ProcessFrame (BS/bad_slam.cc:170-282).  depth_image: raw u16 depth (0 = no measurement, as in the
  // dataset PNGs), rgb_image: 3 bytes per pixel; both HOST arrays at full resolution, i.e. of the cameras' sizes
  // times 2^level of their stream (width << level, height << level).  Frames must arrive with consecutive indices
  // starting at config.start_frame.
  void ProcessFrame(int frame_index, const u16* depth_image, const u8* rgb_image, bool force_keyframe = false);

  // The first stage of ProcessFrame on its own (BS/bad_slam.cc:639-760): upload, input conditioning and the preprocessing
  // kernels, enqueued on the stream.  The images as for ProcessFrame.  It overwrites the buffers of the frame being
  // processed (depth, normals, radius, colour) and nothing else, so a call between two ProcessFrame calls is harmless
  // only because the next ProcessFrame uploads its own frame first.  Public for timing the stage.
  void PreprocessFrame(const u16* depth_image, const u8* rgb_image);
  hipStream_t stream() const { return stream_; }

  // Switches the sensor rectification on (null: off again, the staging buffers are released).  While it is on,
  // ProcessFrame / PreprocessFrame take the RAW frames: depth of rectification->depth_camera's size in units of
  // raw_depth_to_metres, rgb of rectification->color_camera's size.  The depth mesh is reprojected into, and the
  // colour image undistorted into, the camera DecideUndistortedCamera(color_camera, avoid_invalid_pixels = true), as
  // the reference does (BS/input_structure.cc:418-422); the depth comes out in units of config.raw_to_float_depth.
  // That camera, scaled by the pyramid level of each stream, is what this object must have been constructed with: its
  // size must equal the cameras' sizes times 2^level (std::invalid_argument otherwise).  The undistortion map and the
  // unprojection map are built and uploaded here, once.
  void SetSensorRectification(const SensorRectification* rectification);
  bool sensor_rectification() const { return rectify_; }

  // vis::BadSlam::RunBundleAdjustment (BS/bad_slam.cc:481-536)
  void RunBundleAdjustment(u32 frame_index, bool optimize_depth_intrinsics, bool optimize_color_intrinsics, bool optimize_poses, bool optimize_geometry,
                           int min_iterations, int max_iterations, int active_keyframe_window_start, int active_keyframe_window_end,
                           bool increase_ba_iteration_count, int* iterations_done, bool* converged);

  // The closure half of LoopDetector::AddImage (BS/loop_detector.cc:440-712) for the newest keyframe against keyframe
  // matched_id; old_T_cur_initial = the newest keyframe's pose in matched_id's frame.  With status kLoopClosed, the
  // non-keyframe poses follow their keyframes (:685-708).
  void CloseLoop(int matched_id, const SE3f& old_T_cur_initial, LoopClosureResult* result);

  // Opt-in geometric loop candidates (off by default): when a keyframe is added, before its BA iterations, the
  // existing keyframe with id <= new id - min_keyframe_gap whose frustum intersects the new one and whose camera centre
  // is nearest (ties: lower id) is tried with CloseLoop, initial estimate from the current poses.  Closes drift the
  // pairwise tracker can still converge over; it does not recognise places.
  struct LoopLogEntry {
    int keyframe_id, candidate_id;
    LoopClosureStatus status;
    float mean_pixel_distance;
  };
  void SetLoopCandidateSearch(bool enable, int min_keyframe_gap);
  const std::vector<LoopLogEntry>& loop_closure_log() const { return loop_log_; }

  // Opt-in place recognition (off by default; while it is off nothing is allocated or launched for it): every new
  // keyframe's features enter the database, and before its BA iterations DirectBA::RecognizePlace looks for an older
  // keyframe showing the same place, estimates the start pose and tries CloseLoop.  With status kLoopClosed the
  // non-keyframe poses follow their keyframes.  Switching it off releases the database.  It excludes
  // SetLoopCandidateSearch: enabling one while the other is on throws std::invalid_argument.
  struct PlaceLogEntry {
    int keyframe_id, candidate_id;   // candidate_id = -1: no place recognised
    int match_count, inlier_count;
    bool pose_found, loop_attempted;
    LoopClosureStatus status;        // meaningful with loop_attempted
    float mean_pixel_distance;
    double old_T_cur[7];             // qx qy qz qw tx ty tz of the RANSAC start pose (with pose_found)
  };
  void SetPlaceRecognition(bool enable, const PlaceRecognitionOptions& options);
  const std::vector<PlaceLogEntry>& place_recognition_log() const { return place_log_; }

  DirectBA& direct_ba() { return *direct_ba_; }
  const BadSlamConfigV1& config() const { return config_; }
  // global_T_frame of every processed frame (index = frame_index - config.start_frame)
  const std::vector<SE3f>& frame_poses() const { return frame_global_T_frame_; }
  int last_frame_index() const { return last_frame_index_; }
  bool keyframe_created() const { return keyframe_created_; }
  bool pose_estimated() const { return pose_estimated_; }
  int num_planned_ba_iterations() const { return num_planned_ba_iterations_; }
  const Keyframe* base_kf() const { return base_kf_; }
  const std::vector<SE3f>& motion_model_base_kf_tr_frame() const { return base_kf_tr_frame_; }

 private:
  void PredictFramePose(SE3f* estimate_1, SE3f* estimate_2) const;                          // :763-825
  void RunOdometry(int frame_index);                                                        // :827-950
  std::shared_ptr<Keyframe> CreateKeyframe(int frame_index);                                // :953-1097
  void CloseLoopUpTo(int frame_index, int matched_id, const SE3f& old_T_cur_initial, LoopClosureResult* result);
  void SearchLoopCandidate(int frame_index, const Keyframe& new_keyframe);
  void RunPlaceRecognition(int frame_index, const Keyframe& new_keyframe);
  SE3f& FramePose(int frame_index) { return frame_global_T_frame_.at(static_cast<size_t>(frame_index - config_.start_frame)); }

  BadSlamConfigV1 config_;
  std::unique_ptr<DirectBA> direct_ba_;
  hipStream_t stream_ = nullptr;

  // buffers of the frame being processed (BS/bad_slam.h:283-296)
  std::unique_ptr<DeviceBuffer<u8>> rgb_buffer_;
  std::unique_ptr<DeviceBuffer<uchar4_t>> color_buffer_;
  std::unique_ptr<DeviceBuffer<u16>> depth_buffer_, filtered_depth_buffer_A_, filtered_depth_buffer_B_, normals_buffer_, radius_buffer_;
  // full-resolution staging for the input conditioning; null while the switch that needs it is off
  std::unique_ptr<DeviceBuffer<u8>> raw_rgb_buffer_;
  std::unique_ptr<DeviceBuffer<u16>> raw_depth_buffer_, median_depth_buffer_;
  // sensor rectification; the buffers exist only while it is on
  bool rectify_ = false;
  SensorRectification rectification_;
  bslam_camera4f rectified_camera_ = {};   // the full-resolution target of both streams
  std::unique_ptr<DeviceBuffer<u8>> sensor_rgb_buffer_;
  std::unique_ptr<DeviceBuffer<u16>> sensor_depth_buffer_;
  std::unique_ptr<DeviceBuffer<float>> undistortion_map_, unprojection_map_;   // 2 floats per pixel
  std::unique_ptr<PairwiseFrameTrackingBuffers> pairwise_tracking_buffers_;

  Keyframe* base_kf_ = nullptr;
  SE3f base_kf_global_T_frame_;
  std::vector<SE3f> base_kf_tr_frame_;   // motion model: poses of the last (up to three) frames relative to the base keyframe, newest last
  std::vector<SE3f> frame_global_T_frame_;
  int last_frame_index_ = -1;
  int num_planned_ba_iterations_ = 0;
  int bundle_adjustment_counter_ = 0;
  bool pose_estimated_ = false, keyframe_created_ = false;
  bool loop_candidate_search_ = false;
  int loop_min_keyframe_gap_ = 0;
  std::vector<LoopLogEntry> loop_log_;
  bool place_recognition_ = false;
  PlaceRecognitionOptions place_options_;
  std::vector<PlaceLogEntry> place_log_;
};

// BS/trajectory_deformation.cc:33-43 / :45-146 on a plain pose vector (frame_poses[i] = pose of frame start_frame + i)
void RememberKeyframePoses(const DirectBA& ba, std::vector<SE3f>* original_keyframe_T_global);
void ExtrapolateAndInterpolateKeyframePoseChanges(u32 start_frame, u32 end_frame, const DirectBA& ba, const std::vector<SE3f>& original_keyframe_T_global,
                                                  std::vector<SE3f>* frame_poses);

}  // namespace bslam_host
