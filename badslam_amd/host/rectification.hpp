// rectification.hpp -- the once-per-sensor host side of the sensor rectification: the radtan camera model in double
// (forward model RadtanDistortion5::Project, LV/camera.h:615-631; its inverse a 2x2 Gauss-Newton iteration as
// LV/camera.h:673-700 describes it), the choice of the undistorted pinhole camera (rule of BS/undistortion.cc:33-98) and
// the unprojection map of the raw depth camera (BS/input_structure.cc:429-434).  The per-frame work is on the device:
// csrc/rectify_kernels.hpp.
//
// Conventions: bslam_radtan_camera is pixel-CENTRE (the centre of pixel (x, y) is at (x, y)), PinholeCamera4f is
// pixel-CORNER (at (x + 0.5, y + 0.5)).  DecideUndistortedCamera is where the half pixel is added.
#pragma once

#include <vector>

#include "direct_ba.hpp"

namespace bslam_host {

// Normalised undistorted point -> normalised distorted point.
void RadtanDistort(const bslam_radtan_camera& camera, double x, double y, double* distorted_x, double* distorted_y);

// The inverse: Gauss-Newton on the 2x2 system in double, at most 100 iterations, stopping once the squared residual
// is below 1e-10 (the update of that iteration is still applied, so the result is one step better than the test).
void RadtanUndistort(const bslam_radtan_camera& camera, double distorted_x, double distorted_y, double* x, double* y);

// The pinhole camera (same fx, fy) whose image is the undistorted view of `camera`.  The four border lines of the raw
// image are undistorted; avoid_invalid_pixels = true takes the tightest bounds (every pixel of the result sees the raw
// image), false the loosest (every raw pixel is seen).  The first pixel centre sits on the lower bound; the last one at
// or below the upper bound with the tightest bounds, size = int(max - min) + 1 per axis, and at or above it with the
// loosest, size = int(ceil(max - min)) + 1; cx_corner = cx + 0.5 - min.  (The reference takes int(max - min) in both
// cases: one column and row fewer than its own comment states, and with the loosest bounds it can cut the outermost raw
// pixels off.  With zero distortion the rule here returns the raw camera's size.)  The bounds are formed in double and
// rounded to fp32 once.
PinholeCamera4f DecideUndistortedCamera(const bslam_radtan_camera& camera, bool avoid_invalid_pixels);

// (x, y) of the unit-z ray through the centre of every raw pixel, row-major, 2 floats per pixel.
std::vector<float> MakeUnprojectionMap(const bslam_radtan_camera& camera);

// What BadSlam::SetSensorRectification takes: the raw sensor as it streams.
struct SensorRectification {
  bslam_radtan_camera color_camera;
  bslam_radtan_camera depth_camera;
  bslam_mat3x4 color_T_depth = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
  float depth_difference_threshold = 0.05f;   // metres; structure_depth_diff_threshold, BS/bad_slam_config.h:326
  float raw_depth_to_metres = 0.001f;         // the raw depth unit (Structure Core, Azure Kinect, RealSense: millimetres)
};

}  // namespace bslam_host
