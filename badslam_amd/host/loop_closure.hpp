// loop_closure.hpp -- the closure half of vis::LoopDetector::AddImage (BS/loop_detector.cc:440-712, after the RANSAC
// step): verify a loop candidate with three direct pairwise trackings, average them, decide whether bundle adjustment
// could close the loop by itself, and otherwise close it with a keyframe pose graph (host/pose_graph.hpp).  The
// candidate and the initial pose come from the caller: host/place_recognition.hpp finds both from the images (in place of
// the reference's DBoW2 query and opengv RANSAC).
#pragma once

#include <vector>

#include "direct_ba.hpp"

namespace bslam_host {

enum LoopClosureStatus {
  kLoopClosed = 0,                   // the pose graph was optimised and every keyframe pose written back
  kLoopIgnoredSmall = 1,             // the averaged estimate moves the grid points by <= 1 px on average: left to BA
  kLoopRejectedNoNeighbours = 2,     // the matched keyframe has no next (or second) existing keyframe for verification
  kLoopRejectedInconsistent = 3,     // the three refined relative poses disagree (> 10 degrees optical axis or > 2 cm)
};

struct LoopClosureResult {
  LoopClosureStatus status = kLoopRejectedNoNeighbours;
  int old_keyframe_ids[3] = {-1, -1, -1};      // matched, next, previous (or the one after next)
  SE3f cur_T_old_refined[3];                   // relative pose of the matched keyframe per verification tracking
  SE3f cur_T_old_averaged;
  float mean_pixel_distance = 0.f;             // over the grid points counted (0 if none)
  int pixel_count = 0;
  std::vector<double> chi2;                    // pose-graph chi^2 after each iteration (empty unless closed)
  std::vector<std::vector<int>> tracking_iterations;   // [3][num_scales]
};

// Grid of the pixel-distance test: every kLoopGridStride-th pixel in x and y, starting at kLoopGridStride / 2.
constexpr int kLoopGridStride = 8;
constexpr int kLoopPoseGraphIterations = 20;

// Closes a loop from keyframe current_id (the tracking base) to keyframe matched_id.  old_T_cur_initial: initial
// estimate of current_id's pose in matched_id's frame (the reference's RANSAC result).  Changes keyframe poses only
// with status kLoopClosed; the lowest-id existing keyframe is the gauge and keeps its pose bit for bit.
void CloseLoop(DirectBA& ba, hipStream_t stream, int current_id, int matched_id, const SE3f& old_T_cur_initial, int num_scales, LoopClosureResult* result);

}  // namespace bslam_host
