// rectification.cpp -- see rectification.hpp.
#include "rectification.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>

namespace bslam_host {

namespace {

// distorted point and the Jacobian d(distorted) / d(x, y) (symmetric off-diagonal)
void DistortWithJacobian(const bslam_radtan_camera& c, double x, double y, double* dx, double* dy, double* j00, double* j01, double* j11) {
  const double k1 = c.k1, k2 = c.k2, k3 = c.k3, p1 = c.p1, p2 = c.p2;
  const double x2 = x * x, y2 = y * y, xy = x * y, r2 = x2 + y2;
  const double radial = k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2;
  *dx = x + x * radial + 2 * p1 * xy + p2 * (r2 + 2 * x2);
  *dy = y + y * radial + 2 * p2 * xy + p1 * (r2 + 2 * y2);
  const double dradial_dr2 = k1 + 2 * k2 * r2 + 3 * k3 * r2 * r2;   // d r2 / dx = 2 x
  *j00 = 1 + radial + 2 * x2 * dradial_dr2 + 2 * p1 * y + 6 * p2 * x;
  *j01 = 2 * xy * dradial_dr2 + 2 * p1 * x + 2 * p2 * y;
  *j11 = 1 + radial + 2 * y2 * dradial_dr2 + 6 * p1 * y + 2 * p2 * x;
}

void CheckCamera(const bslam_radtan_camera& c) {
  if (c.width < 2 || c.height < 2 || !(c.fx > 0) || !(c.fy > 0)) throw std::invalid_argument("radtan camera: size must be >= 2 x 2 and fx, fy > 0");
}

}  // namespace

void RadtanDistort(const bslam_radtan_camera& camera, double x, double y, double* distorted_x, double* distorted_y) {
  double j00, j01, j11;
  DistortWithJacobian(camera, x, y, distorted_x, distorted_y, &j00, &j01, &j11);
}

void RadtanUndistort(const bslam_radtan_camera& camera, double distorted_x, double distorted_y, double* x, double* y) {
  double cur_x = distorted_x, cur_y = distorted_y;
  for (int iteration = 0; iteration < 100; ++iteration) {
    double dx, dy, j00, j01, j11;
    DistortWithJacobian(camera, cur_x, cur_y, &dx, &dy, &j00, &j01, &j11);
    const double rx = dx - distorted_x, ry = dy - distorted_y;
    // J is square: the Gauss-Newton step (J^T J)^-1 J^T r is J^-1 r
    const double det = j00 * j11 - j01 * j01;
    if (det == 0 || !std::isfinite(det)) break;
    cur_x -= (j11 * rx - j01 * ry) / det;
    cur_y -= (j00 * ry - j01 * rx) / det;
    if (rx * rx + ry * ry < 1e-10) break;
  }
  *x = cur_x;
  *y = cur_y;
}

PinholeCamera4f DecideUndistortedCamera(const bslam_radtan_camera& camera, bool avoid_invalid_pixels) {
  CheckCamera(camera);
  const double inf = std::numeric_limits<double>::infinity();
  double min_x = avoid_invalid_pixels ? -inf : inf, min_y = min_x, max_x = -min_x, max_y = -min_x;
  // where the raw pixel centre (px, py) lands in an undistorted image with the same fx, fy, cx, cy (pixel-centre)
  auto undistorted_pixel = [&](int px, int py, double* ux, double* uy) {
    double nx, ny;
    RadtanUndistort(camera, (px - static_cast<double>(camera.cx)) / camera.fx, (py - static_cast<double>(camera.cy)) / camera.fy, &nx, &ny);
    *ux = camera.fx * nx + camera.cx;
    *uy = camera.fy * ny + camera.cy;
  };
  auto tighten_low = [&](double* bound, double v) { *bound = avoid_invalid_pixels ? std::max(*bound, v) : std::min(*bound, v); };
  auto tighten_high = [&](double* bound, double v) { *bound = avoid_invalid_pixels ? std::min(*bound, v) : std::max(*bound, v); };
  double ux, uy;
  for (int x = 0; x < camera.width; ++x) {
    undistorted_pixel(x, 0, &ux, &uy);                     // top line
    tighten_low(&min_y, uy);
    undistorted_pixel(x, camera.height - 1, &ux, &uy);     // bottom line
    tighten_high(&max_y, uy);
  }
  for (int y = 0; y < camera.height; ++y) {
    undistorted_pixel(0, y, &ux, &uy);                     // left line
    tighten_low(&min_x, ux);
    undistorted_pixel(camera.width - 1, y, &ux, &uy);      // right line
    tighten_high(&max_x, ux);
  }
  const float fmin_x = static_cast<float>(min_x), fmin_y = static_cast<float>(min_y), fmax_x = static_cast<float>(max_x), fmax_y = static_cast<float>(max_y);
  if (!(fmax_x - fmin_x >= 1) || !(fmax_y - fmin_y >= 1) || !(fmax_x - fmin_x < 65536) || !(fmax_y - fmin_y < 65536))
    throw std::invalid_argument("DecideUndistortedCamera: the distortion leaves no usable undistorted image");
  // tightest: the last pixel centre at or below the upper bound (truncate); loosest: at or above it (round up)
  const float span_x = avoid_invalid_pixels ? fmax_x - fmin_x : std::ceil(fmax_x - fmin_x), span_y = avoid_invalid_pixels ? fmax_y - fmin_y : std::ceil(fmax_y - fmin_y);
  const int width = static_cast<int>(span_x) + 1, height = static_cast<int>(span_y) + 1;
  const float parameters[4] = {camera.fx, camera.fy, camera.cx + 0.5f - fmin_x, camera.cy + 0.5f - fmin_y};
  return PinholeCamera4f(width, height, parameters);
}

std::vector<float> MakeUnprojectionMap(const bslam_radtan_camera& camera) {
  CheckCamera(camera);
  std::vector<float> map(static_cast<size_t>(camera.width) * camera.height * 2);
  for (int y = 0; y < camera.height; ++y)
    for (int x = 0; x < camera.width; ++x) {
      double nx, ny;
      RadtanUndistort(camera, (x - static_cast<double>(camera.cx)) / camera.fx, (y - static_cast<double>(camera.cy)) / camera.fy, &nx, &ny);
      float* entry = &map[2 * (static_cast<size_t>(y) * camera.width + x)];
      entry[0] = static_cast<float>(nx);
      entry[1] = static_cast<float>(ny);
    }
  return map;
}

}  // namespace bslam_host
