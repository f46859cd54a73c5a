// pairwise_frame_tracking.cpp -- see pairwise_frame_tracking.hpp.
#include "pairwise_frame_tracking.hpp"

#include <cmath>
#include <stdexcept>
#include <string>

namespace bslam_host {

namespace {
void Check(int rc, const char* what) {
  if (rc != BSLAM_OK) throw std::runtime_error(std::string(what) + ": " + bslam_last_error());
}
// CameraImpl::Scaled (LV/camera.h:1696-1705) with PixelMapping4::ScaleParameters (:1086-1096)
bslam_camera4f Scaled(const PinholeCamera4f& c, float factor) {
  const float* p = c.parameters();
  bslam_camera4f s;
  s.fx = p[0] * factor; s.fy = p[1] * factor; s.cx = p[2] * factor; s.cy = p[3] * factor;
  s.width = static_cast<int>(factor * c.width() + 0.5f);
  s.height = static_cast<int>(factor * c.height() + 0.5f);
  return s;
}
// IsScaleNPoseEstimationConverged (BS/convergence_analysis.h:56-63)
bool IsScaleNPoseEstimationConverged(const float* x, float scaling_factor) {
  constexpr float translation_threshold = 1e-08f, rotation_threshold = 1e-08f;
  float n = 0;
  for (int i = 0; i < 6; ++i) { const float v = (i < 3) ? x[i] : x[i] * (translation_threshold / rotation_threshold); n += v * v; }
  return n < scaling_factor * scaling_factor * translation_threshold;
}

// The per-scale images of one side (base or tracked) of a buffers object as the library takes them; level 0 of the normals is the
// frame's own image.
struct LevelPods {
  std::vector<bslam_buffer2d> depth, normals, color;
};
LevelPods Pods(const PairwiseFrameTrackingBuffers& b, bool base, const DeviceBuffer<u16>& normals_l0) {
  LevelPods pods;
  for (int s = 0; s < b.num_scales; ++s) {
    pods.depth.push_back((base ? b.base_depth : b.tracked_depth)[s]->ToPod());
    pods.color.push_back((base ? b.base_color : b.tracked_color)[s]->ToPod());
    pods.normals.push_back(s ? (base ? b.base_normals : b.tracked_normals)[s]->ToPod() : normals_l0.ToPod());
  }
  return pods;
}
// gradient-magnitude images instead of brightness images when use_gradmag (BS/bad_slam.cc:859-869, 888-898)
void ColourCue(bslam_context* ctx, hipStream_t stream, bool use_gradmag, const DeviceBuffer<uchar4_t>& rgba, const bslam_buffer2d& out) {
  const bslam_buffer2d in = rgba.ToPod();
  if (use_gradmag) Check(bslam_compute_sobel_gradient_magnitude(ctx, stream, &in, &out), "bslam_compute_sobel_gradient_magnitude");
  else Check(bslam_compute_brightness_from_color(ctx, stream, &in, &out), "bslam_compute_brightness_from_color");
}
void Downsample(bslam_context* ctx, hipStream_t stream, const LevelPods& l, int s) {
  Check(bslam_downsample_images(ctx, stream, &l.depth[s - 1], &l.normals[s - 1], &l.color[s - 1], &l.depth[s], &l.normals[s], &l.color[s]), "bslam_downsample_images");
}
// The base frame's pyramid: colour cue, depth calibrated and colour brought into the depth image's geometry, then halved per scale
// (BS/bad_slam.cc:859-897, BS/pairwise_frame_tracking.cc:283-341).
void PrepareBase(bslam_context* ctx, hipStream_t stream, bool use_gradmag, const bslam_camera4f& color_cam, const bslam_camera4f& depth_cam,
                 const bslam_depth_params& dp, const DeviceBuffer<u16>& depth_u16, const DeviceBuffer<uchar4_t>& rgba, const bslam_buffer2d& cue,
                 const LevelPods& base) {
  const bslam_buffer2d d16 = depth_u16.ToPod();
  ColourCue(ctx, stream, use_gradmag, rgba, cue);
  Check(bslam_calibrate_depth_and_transform_color_to_depth(ctx, stream, &color_cam, &depth_cam, &dp, &d16, &cue, &base.depth[0], &base.color[0]),
        "bslam_calibrate_depth_and_transform_color_to_depth");
  for (size_t s = 1; s < base.depth.size(); ++s) Downsample(ctx, stream, base, static_cast<int>(s));
}
// A tracked frame's pyramid: colour cue, then level 0 (calibrated depth, normalised colour) or, without it, level 1 straight from
// the raw images (:303-323), then halved per scale.
void PrepareTracked(bslam_context* ctx, hipStream_t stream, bool use_gradmag, bool use_pyramid_level_0, bool downsample_color, const bslam_depth_params& dp,
                    const DeviceBuffer<u16>& depth_u16, const DeviceBuffer<u16>& normals_l0, const DeviceBuffer<uchar4_t>& rgba, const bslam_buffer2d& cue,
                    const LevelPods& tracked) {
  const bslam_buffer2d d16 = depth_u16.ToPod(), normals_in = normals_l0.ToPod();
  const int num_scales = static_cast<int>(tracked.depth.size());
  ColourCue(ctx, stream, use_gradmag, rgba, cue);
  if (use_pyramid_level_0) {
    Check(bslam_calibrate_depth(ctx, stream, &dp, &d16, &tracked.depth[0]), "bslam_calibrate_depth");
    Check(bslam_set_to_read_mode_normalized(ctx, stream, &cue, &tracked.color[0]), "bslam_set_to_read_mode_normalized");
  } else if (num_scales > 1) {
    Check(bslam_calibrate_and_downsample_images(ctx, stream, downsample_color, &dp, &d16, &normals_in, &cue, &tracked.depth[1], &tracked.normals[1],
                                                &tracked.color[1]),
          "bslam_calibrate_and_downsample_images");
  }
  for (int s = use_pyramid_level_0 ? 1 : 2; s < num_scales; ++s) Downsample(ctx, stream, tracked, s);
}
// The better of two estimates (BS/pairwise_frame_tracking.cc:428-489): the one with more than twice the residuals, else the cheaper.
bool BetterOf(u32 count_a, float cost_a, u32 count_b, float cost_b) {
  if (count_a > 2 * count_b) return true;
  if (count_b > 2 * count_a) return false;
  return cost_a < cost_b;
}
// Step damping at the two coarsest scales (:573-579).
float Damping(int scale, int num_scales) { return scale == num_scales - 1 ? 0.25f : scale == num_scales - 2 ? 0.5f : 1.f; }
constexpr int kMaxIterationsPerScale = 30;
}  // namespace

PairwiseFrameTrackingBuffers::PairwiseFrameTrackingBuffers(int depth_width, int depth_height, int color_width, int color_height, int num_scales_)
    : num_scales(num_scales_), base_depth(num_scales_), tracked_depth(num_scales_), base_normals(num_scales_), tracked_normals(num_scales_),
      base_color(num_scales_), tracked_color(num_scales_) {
  for (int scale = 0; scale < num_scales; ++scale) {   // BS/pairwise_frame_tracking.cc:38-80
    const int w = static_cast<int>(depth_width / std::pow(2, scale)), h = static_cast<int>(depth_height / std::pow(2, scale));
    base_depth[scale].reset(new DeviceBuffer<float>(h, w));
    tracked_depth[scale].reset(new DeviceBuffer<float>(h, w));
    base_color[scale].reset(new DeviceBuffer<u8>(h, w));   // the base colour is transformed into the depth image's geometry
    // The tracked colour keeps the colour camera's geometry, which the pose kernels sample with the scaled colour camera (the
    // reference sizes these by the depth image and leaves the other case as a TODO, BS/pairwise_frame_tracking.cc:301-302).
    tracked_color[scale].reset(new DeviceBuffer<u8>(static_cast<int>(color_height / std::pow(2, scale)), static_cast<int>(color_width / std::pow(2, scale))));
    if (scale >= 1) {
      base_normals[scale].reset(new DeviceBuffer<u16>(h, w));
      tracked_normals[scale].reset(new DeviceBuffer<u16>(h, w));
    }
  }
  base_gradmag.reset(new DeviceBuffer<u8>(color_height, color_width));
  tracked_gradmag.reset(new DeviceBuffer<u8>(color_height, color_width));
}

void TrackFramePairwise(bslam_context* ctx, hipStream_t stream, PairwiseFrameTrackingBuffers* buffers, const PinholeCamera4f& color_camera,
                        const PinholeCamera4f& depth_camera, const bslam_depth_params& dp, bool use_depth_residuals, bool use_descriptor_residuals,
                        const DeviceBuffer<u16>& tracked_depth_u16, const DeviceBuffer<u16>& tracked_normals_l0, const DeviceBuffer<uchar4_t>& tracked_color_rgba,
                        const DeviceBuffer<u16>& base_depth_u16, const DeviceBuffer<u16>& base_normals_l0, const DeviceBuffer<uchar4_t>& base_color_rgba,
                        bool test_different_initial_estimates, const SE3f& init1, const SE3f& init2, SE3f* out_base_T_frame, int* iterations_per_scale,
                        bool use_pyramid_level_0, bool use_gradmag) {
  if (!use_pyramid_level_0 && (depth_camera.width() != color_camera.width() || depth_camera.height() != color_camera.height()))
    throw std::invalid_argument("TrackFramePairwise: without pyramid level 0, depth and colour images must have the same size");   // :303-323 builds level 1 of both at once
  const int num_scales = buffers->num_scales;
  const LevelPods base = Pods(*buffers, true, base_normals_l0), tracked = Pods(*buffers, false, tracked_normals_l0);
  PrepareBase(ctx, stream, use_gradmag, color_camera.pod(), depth_camera.pod(), dp, base_depth_u16, base_color_rgba, buffers->base_gradmag->ToPod(), base);
  PrepareTracked(ctx, stream, use_gradmag, use_pyramid_level_0, depth_camera.width() == color_camera.width(), dp, tracked_depth_u16, tracked_normals_l0,
                 tracked_color_rgba, buffers->tracked_gradmag->ToPod(), tracked);
  // --- coarse to fine (:343-640)
  SE3f estimate = init1, chosen_initial = init1;
  for (int scale = num_scales - 1; scale >= (use_pyramid_level_0 ? 0 : 1); --scale) {   // :367
    const float scaling_factor = static_cast<float>(std::pow(2, scale));
    const bslam_camera4f tcc = Scaled(color_camera, 1.f / scaling_factor), tdc = Scaled(depth_camera, 1.f / scaling_factor);
    const float threshold_factor = scaling_factor;
    auto cost_of = [&](const SE3f& base_T_frame, u32* count, float* cost) {
      const bslam_mat3x4 M = base_T_frame.Inverse().Matrix3x4();
      Check((use_gradmag ? bslam_compute_cost_and_residual_count_from_images_gradmag : bslam_compute_cost_and_residual_count_from_images)(
                ctx, stream, use_depth_residuals, use_descriptor_residuals, &tcc, &tdc, dp.baseline_fx, threshold_factor, &tracked.depth[scale],
                &tracked.normals[scale], &tracked.color[scale], &M, &base.depth[scale], &base.normals[scale], &base.color[scale], count, cost),
            "bslam_compute_cost_and_residual_count_from_images");
    };
    if (scale != num_scales - 1 || test_different_initial_estimates) {   // :428-489
      const SE3f last = (scale != num_scales - 1) ? estimate : init1;
      const SE3f other = (scale != num_scales - 1) ? chosen_initial : init2;
      u32 count_last = 0, count_other = 0;
      float cost_last = 0, cost_other = 0;
      cost_of(last, &count_last, &cost_last);
      cost_of(other, &count_other, &cost_other);
      estimate = BetterOf(count_last, cost_last, count_other, cost_other) ? last : other;
      if (scale == num_scales - 1) chosen_initial = estimate;
    }
    int iteration;
    for (iteration = 0; iteration < kMaxIterationsPerScale; ++iteration) {
      const bslam_mat3x4 M = estimate.Inverse().Matrix3x4();
      float H[21], b[6], x[6];
      Check((use_gradmag ? bslam_accumulate_pose_coeffs_from_images_gradmag : bslam_accumulate_pose_coeffs_from_images)(
                ctx, stream, use_depth_residuals, use_descriptor_residuals, &tcc, &tdc, dp.baseline_fx, threshold_factor, &tracked.depth[scale],
                &tracked.normals[scale], &tracked.color[scale], &M, &base.depth[scale], &base.normals[scale], &base.color[scale], nullptr, H, b),
            "bslam_accumulate_pose_coeffs_from_images");
      SolveLDLTUpper(6, H, b, x);   // :561
      const float damping = Damping(scale, num_scales);
      float step[6];
      for (int i = 0; i < 6; ++i) step[i] = -damping * x[i];
      estimate = estimate * SE3f::Exp(step);
      if (IsScaleNPoseEstimationConverged(x, scaling_factor)) { ++iteration; break; }
    }
    if (iterations_per_scale) iterations_per_scale[scale] = iteration;
  }
  *out_base_T_frame = estimate;
}

void TrackFramesPairwiseBatched(bslam_context* ctx, hipStream_t stream, std::vector<std::unique_ptr<PairwiseFrameTrackingBuffers>>* buffers, int num_scales,
                                const PinholeCamera4f& color_camera, const PinholeCamera4f& depth_camera, const bslam_depth_params& dp,
                                bool use_depth_residuals, bool use_descriptor_residuals, const std::vector<TrackedFrameImages>& tracked,
                                const DeviceBuffer<u16>& base_depth_u16, const DeviceBuffer<u16>& base_normals_l0, const DeviceBuffer<uchar4_t>& base_color_rgba,
                                const std::vector<SE3f>& inits, std::vector<SE3f>* out_base_T_frame, std::vector<std::vector<int>>* iterations_per_scale) {
  const int pairs = static_cast<int>(tracked.size());
  if (pairs < 1 || pairs > BSLAM_MAX_PAIR_BATCH) throw std::invalid_argument("TrackFramesPairwiseBatched: 1 to BSLAM_MAX_PAIR_BATCH tracked frames");
  if (static_cast<int>(inits.size()) != pairs) throw std::invalid_argument("TrackFramesPairwiseBatched: one initial estimate per tracked frame");
  while (static_cast<int>(buffers->size()) < pairs)
    buffers->emplace_back(new PairwiseFrameTrackingBuffers(depth_camera.width(), depth_camera.height(), color_camera.width(), color_camera.height(), num_scales));
  for (int p = 0; p < pairs; ++p)
    if ((*buffers)[p]->num_scales != num_scales) throw std::invalid_argument("TrackFramesPairwiseBatched: buffers built for another scale count");
  // --- input preparation and pyramids, as TrackFramePairwise does them (base once, in entry 0; each tracked frame once)
  PairwiseFrameTrackingBuffers& b0 = *(*buffers)[0];
  const LevelPods base = Pods(b0, true, base_normals_l0);
  PrepareBase(ctx, stream, false, color_camera.pod(), depth_camera.pod(), dp, base_depth_u16, base_color_rgba, b0.base_gradmag->ToPod(), base);
  std::vector<LevelPods> tracked_pods;
  for (int p = 0; p < pairs; ++p) {
    tracked_pods.push_back(Pods(*(*buffers)[p], false, *tracked[p].normals));
    PrepareTracked(ctx, stream, false, true, false, dp, *tracked[p].depth, *tracked[p].normals, *tracked[p].color, (*buffers)[p]->tracked_gradmag->ToPod(),
                   tracked_pods[p]);
  }
  // --- coarse to fine in lockstep (TrackFramePairwise's loop per pair)
  std::vector<SE3f> estimate = inits;
  iterations_per_scale->assign(pairs, std::vector<int>(num_scales, 0));
  for (int scale = num_scales - 1; scale >= 0; --scale) {
    const float scaling_factor = static_cast<float>(std::pow(2, scale));
    const bslam_camera4f tcc = Scaled(color_camera, 1.f / scaling_factor), tdc = Scaled(depth_camera, 1.f / scaling_factor);
    const float threshold_factor = scaling_factor;
    if (scale != num_scales - 1) {   // last estimate vs the initial one (test_different_initial_estimates = false: chosen_initial = init)
      for (int p = 0; p < pairs; ++p) {
        u32 count[2] = {0, 0};
        float cost[2] = {0, 0};
        const SE3f cand[2] = {estimate[p], inits[p]};
        for (int i = 0; i < 2; ++i) {
          const bslam_mat3x4 M = cand[i].Inverse().Matrix3x4();
          Check(bslam_compute_cost_and_residual_count_from_images(ctx, stream, use_depth_residuals, use_descriptor_residuals, &tcc, &tdc, dp.baseline_fx,
                                                                  threshold_factor, &tracked_pods[p].depth[scale], &tracked_pods[p].normals[scale],
                                                                  &tracked_pods[p].color[scale], &M, &base.depth[scale], &base.normals[scale], &base.color[scale],
                                                                  &count[i], &cost[i]),
                "bslam_compute_cost_and_residual_count_from_images");
        }
        estimate[p] = cand[BetterOf(count[0], cost[0], count[1], cost[1]) ? 0 : 1];
      }
    }
    const float damping = Damping(scale, num_scales);
    std::vector<int> active(pairs);
    for (int p = 0; p < pairs; ++p) active[p] = p;
    while (!active.empty()) {
      const int n = static_cast<int>(active.size());
      std::vector<bslam_buffer2d> td(n), tn(n), tc(n);
      std::vector<bslam_mat3x4> M(n);
      for (int i = 0; i < n; ++i) {
        const int p = active[i];
        td[i] = tracked_pods[p].depth[scale]; tn[i] = tracked_pods[p].normals[scale]; tc[i] = tracked_pods[p].color[scale];
        M[i] = estimate[p].Inverse().Matrix3x4();
      }
      std::vector<float> H(21 * static_cast<size_t>(n)), b(6 * static_cast<size_t>(n));
      Check(bslam_accumulate_pose_coeffs_from_images_batched(ctx, stream, use_depth_residuals, use_descriptor_residuals, &tcc, &tdc, dp.baseline_fx,
                                                              threshold_factor, n, td.data(), tn.data(), tc.data(), M.data(), &base.depth[scale],
                                                              &base.normals[scale], &base.color[scale], nullptr, H.data(), b.data()),
            "bslam_accumulate_pose_coeffs_from_images_batched");
      std::vector<int> still;
      for (int i = 0; i < n; ++i) {
        const int p = active[i];
        float x[6], step[6];
        SolveLDLTUpper(6, &H[21 * static_cast<size_t>(i)], &b[6 * static_cast<size_t>(i)], x);
        for (int k = 0; k < 6; ++k) step[k] = -damping * x[k];
        estimate[p] = estimate[p] * SE3f::Exp(step);
        const int done = ++(*iterations_per_scale)[p][scale];
        if (!IsScaleNPoseEstimationConverged(x, scaling_factor) && done < kMaxIterationsPerScale) still.push_back(p);
      }
      active.swap(still);
    }
  }
  *out_base_T_frame = estimate;
}

}  // namespace bslam_host
