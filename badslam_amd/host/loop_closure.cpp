// loop_closure.cpp -- see loop_closure.hpp.
#include "loop_closure.hpp"

#include <algorithm>
#include <cmath>
#include <memory>
#include <stdexcept>

#include "pairwise_frame_tracking.hpp"
#include "pose_graph.hpp"

namespace bslam_host {

namespace {
Pose3d ToPose3d(const SE3f& T) { return Pose3d::FromQuaternion(T.qx, T.qy, T.qz, T.qw, T.tx, T.ty, T.tz); }
SE3f ToSE3f(const Pose3d& P) {
  double qx, qy, qz, qw;
  P.ToQuaternion(&qx, &qy, &qz, &qw);
  SE3f T;
  T.qx = static_cast<float>(qx); T.qy = static_cast<float>(qy); T.qz = static_cast<float>(qz); T.qw = static_cast<float>(qw);
  T.tx = static_cast<float>(P.t[0]); T.ty = static_cast<float>(P.t[1]); T.tz = static_cast<float>(P.t[2]);
  return T;
}
// PinholeCamera::ProjectToPixelCornerConvIfVisible(p, 0.f, &out) (libvis camera.h)
bool ProjectIfVisible(const PinholeCamera4f& cam, Vec3f p, float* px, float* py) {
  if (!(p.z > 0.f)) return false;
  const float* k = cam.parameters();
  *px = k[0] * (p.x / p.z) + k[2];
  *py = k[1] * (p.y / p.z) + k[3];
  return *px >= 0.f && *py >= 0.f && *px < cam.width() && *py < cam.height();
}
}  // namespace

void CloseLoop(DirectBA& ba, hipStream_t stream, int current_id, int matched_id, const SE3f& old_T_cur_initial, int num_scales, LoopClosureResult* result) {
  LoopClosureResult r;
  const auto& kfs = ba.keyframes();
  const int n = static_cast<int>(kfs.size());
  if (current_id < 0 || current_id >= n || !kfs[current_id] || matched_id < 0 || matched_id >= n || !kfs[matched_id] || current_id == matched_id)
    throw std::invalid_argument("CloseLoop: current and matched keyframes must be two different existing keyframes");
  Keyframe& current = *kfs[current_id];
  // --- 1. the three old keyframes (BS/loop_detector.cc:440-494): matched, next, previous (or the one after next)
  Keyframe* old_kf[3] = {kfs[matched_id].get(), nullptr, nullptr};
  int next_index = -1;
  for (int i = matched_id + 1; i < n; ++i)
    if (kfs[i] && i != current_id) { old_kf[1] = kfs[i].get(); next_index = i; break; }
  if (old_kf[1]) {
    for (int i = matched_id - 1; i >= 0; --i)
      if (kfs[i] && i != current_id) { old_kf[2] = kfs[i].get(); break; }
    if (!old_kf[2])
      for (int i = next_index + 1; i < n; ++i)
        if (kfs[i] && i != current_id) { old_kf[2] = kfs[i].get(); break; }
  }
  if (!old_kf[1] || !old_kf[2]) {
    r.status = kLoopRejectedNoNeighbours;
    *result = r;
    return;
  }
  // --- 2. three trackings, base = current keyframe, tracked = old keyframes (:495-546), in one lockstep batch
  std::vector<TrackedFrameImages> tracked;
  std::vector<SE3f> inits, matched_T_this(3);
  for (int i = 0; i < 3; ++i) {
    r.old_keyframe_ids[i] = old_kf[i]->id();
    matched_T_this[i] = (i == 0) ? SE3f() : (old_kf[0]->frame_T_global() * old_kf[i]->global_T_frame());
    tracked.push_back(TrackedFrameImages{&old_kf[i]->depth_buffer(), &old_kf[i]->normals_buffer(), &old_kf[i]->color_buffer()});
    inits.push_back(old_T_cur_initial.Inverse() * matched_T_this[i]);
  }
  std::vector<std::unique_ptr<PairwiseFrameTrackingBuffers>> buffers;
  std::vector<SE3f> cur_T_tracked;
  TrackFramesPairwiseBatched(ba.context(), stream, &buffers, num_scales, ba.color_camera(), ba.depth_camera(), ba.depth_params(), ba.use_depth_residuals(),
                             ba.use_descriptor_residuals(), tracked, current.depth_buffer(), current.normals_buffer(), current.color_buffer(), inits,
                             &cur_T_tracked, &r.tracking_iterations);
  for (int i = 0; i < 3; ++i) r.cur_T_old_refined[i] = (matched_T_this[i] * cur_T_tracked[i].Inverse()).Inverse();
  // --- 3. consistency (:571-604): angle between the third rotation columns (the optical axes) and translation distance
  constexpr float kMaxAngleDifference = static_cast<float>(M_PI) / 180.f * 10.f;
  constexpr float kMaxEuclideanDistance = 0.02f;
  for (int i = 0; i < 2; ++i)
    for (int k = i + 1; k < 3; ++k) {
      float Ri[9], Rk[9];
      r.cur_T_old_refined[i].RotationMatrix(Ri);
      r.cur_T_old_refined[k].RotationMatrix(Rk);
      const float dot = Ri[2] * Rk[2] + Ri[5] * Rk[5] + Ri[8] * Rk[8];
      const float angle = std::acos(std::min(1.f, std::max(-1.f, dot)));
      const SE3f& a = r.cur_T_old_refined[i];
      const SE3f& b = r.cur_T_old_refined[k];
      const float dx = a.tx - b.tx, dy = a.ty - b.ty, dz = a.tz - b.tz;
      if (angle > kMaxAngleDifference || std::sqrt(dx * dx + dy * dy + dz * dz) > kMaxEuclideanDistance) {
        r.status = kLoopRejectedInconsistent;
        *result = r;
        return;
      }
    }
  // --- 4. average (:606-609), in double
  std::vector<Pose3d> refined;
  for (int i = 0; i < 3; ++i) refined.push_back(ToPose3d(r.cur_T_old_refined[i]));
  r.cur_T_old_averaged = ToSE3f(AveragePose(refined));
  // --- 5. would BA handle it? (:623-669)  The reference moves its matched ORB keypoints; there are none here, so the
  // points are a fixed grid of the current keyframe's valid raw depth pixels (raw depth * raw_to_float_depth, no cfactor,
  // as the reference's keypoint depths), unprojected with the depth camera's pixel-centre convention.
  const SE3f cur_T_global_estimate = r.cur_T_old_averaged * old_kf[0]->frame_T_global();
  const SE3f est_T_actual = cur_T_global_estimate * current.global_T_frame();
  const DeviceBuffer<u16>& depth = current.depth_buffer();
  std::vector<u16> raw(static_cast<size_t>(depth.width()) * depth.height());
  depth.Download(stream, raw.data(), static_cast<size_t>(depth.width()) * sizeof(u16));
  const float* dk = ba.depth_camera().parameters();
  const float raw_to_float = ba.depth_params().raw_to_float_depth;
  float distance_sum = 0.f;
  int distance_count = 0;
  for (int y = kLoopGridStride / 2; y < depth.height(); y += kLoopGridStride)
    for (int x = kLoopGridStride / 2; x < depth.width(); x += kLoopGridStride) {
      const u16 d = raw[static_cast<size_t>(y) * depth.width() + x];
      if (d == 0 || (d & BSLAM_INVALID_DEPTH_BIT)) continue;
      const float z = raw_to_float * d;
      const Vec3f p{z * ((x + 0.5f - dk[2]) / dk[0]), z * ((y + 0.5f - dk[3]) / dk[1]), z};
      const Vec3f q0 = est_T_actual.Rotate(p);
      const Vec3f q{q0.x + est_T_actual.tx, q0.y + est_T_actual.ty, q0.z + est_T_actual.tz};
      float ex, ey, cx, cy;
      if (ProjectIfVisible(ba.color_camera(), q, &ex, &ey) && ProjectIfVisible(ba.color_camera(), p, &cx, &cy)) {
        distance_sum += std::sqrt((ex - cx) * (ex - cx) + (ey - cy) * (ey - cy));
        ++distance_count;
      }
    }
  r.pixel_count = distance_count;
  r.mean_pixel_distance = distance_count ? distance_sum / distance_count : 0.f;
  constexpr float kAveragePixelDistanceThreshold = 1.0f;
  if (distance_count >= 5 && r.mean_pixel_distance <= kAveragePixelDistanceThreshold) {
    r.status = kLoopIgnoredSmall;
    *result = r;
    return;
  }
  // --- 6. pose graph from the current state + the loop edge current -> matched (:671-700)
  std::vector<Pose3d> poses(static_cast<size_t>(n));
  std::vector<bool> exists(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) {
    exists[i] = kfs[i] != nullptr;
    if (exists[i]) poses[i] = ToPose3d(kfs[i]->global_T_frame());
  }
  PoseGraphResult pg;
  const int gauge = OptimizeKeyframePoseGraph(&poses, exists, {KeyframeLoopEdge{current_id, matched_id, ToPose3d(r.cur_T_old_averaged)}},
                                              kLoopPoseGraphIterations, &pg);
  for (int i = 0; i < n; ++i)
    if (exists[i] && i != gauge) kfs[i]->set_global_T_frame(ToSE3f(poses[i]));
  r.chi2 = pg.chi2;
  r.status = kLoopClosed;
  *result = r;
}

}  // namespace bslam_host
