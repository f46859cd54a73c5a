// place_recognition.cpp -- see place_recognition.hpp.
#include "place_recognition.hpp"

#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>

namespace bslam_host {

#define HIP_OR_THROW(expr)                                                                         \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

namespace {

void CheckRc(int rc, const char* what) {
  if (rc != BSLAM_OK) throw std::runtime_error(std::string(what) + " failed: " + bslam_last_error());
}

u32 NextDraw(u32* s) {
  *s = *s * 1664525u + 1013904223u;
  return *s >> 16;
}

// Cyclic Jacobi eigen-decomposition of a symmetric 4x4 matrix; returns the eigenvector (4) of the largest eigenvalue.
void LargestEigenvector4(const double* A_in, double* v) {
  double A[16], V[16];
  for (int i = 0; i < 16; ++i) { A[i] = A_in[i]; V[i] = (i % 5 == 0) ? 1 : 0; }
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0;
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) off += A[4 * p + q] * A[4 * p + q];
    if (off < 1e-300) break;
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[4 * p + q];
        if (apq == 0) continue;
        const double theta = (A[4 * q + q] - A[4 * p + p]) / (2 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1));
        const double c = 1 / std::sqrt(t * t + 1), s = t * c;
        for (int k = 0; k < 4; ++k) {   // A <- A J
          const double akp = A[4 * k + p], akq = A[4 * k + q];
          A[4 * k + p] = c * akp - s * akq;
          A[4 * k + q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {   // A <- J^T A
          const double apk = A[4 * p + k], aqk = A[4 * q + k];
          A[4 * p + k] = c * apk - s * aqk;
          A[4 * q + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 4; ++k) {   // V <- V J
          const double vkp = V[4 * k + p], vkq = V[4 * k + q];
          V[4 * k + p] = c * vkp - s * vkq;
          V[4 * k + q] = s * vkp + c * vkq;
        }
      }
  }
  int best = 0;
  for (int i = 1; i < 4; ++i)
    if (A[5 * i] > A[5 * best]) best = i;
  for (int k = 0; k < 4; ++k) v[k] = V[4 * k + best];
}

struct Rigid { double R[9]; double t[3]; double q[4]; };   // p_old = R p_cur + t;  q = (x, y, z, w)

// Horn, "Closed-form solution of absolute orientation using unit quaternions" (1987), on the listed correspondences.
void AbsoluteOrientation(const double* p_cur, const double* p_old, const int* index, int count, Rigid* out) {
  double cc[3] = {0, 0, 0}, co[3] = {0, 0, 0};
  for (int i = 0; i < count; ++i)
    for (int a = 0; a < 3; ++a) { cc[a] += p_cur[3 * index[i] + a]; co[a] += p_old[3 * index[i] + a]; }
  for (int a = 0; a < 3; ++a) { cc[a] /= count; co[a] /= count; }
  double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // S[3 a + b] = sum of cur_a * old_b about the centroids
  for (int i = 0; i < count; ++i)
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) S[3 * a + b] += (p_cur[3 * index[i] + a] - cc[a]) * (p_old[3 * index[i] + b] - co[b]);
  const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
  const double N[16] = {Sxx + Syy + Szz, Syz - Szy,       Szx - Sxz,        Sxy - Syx,
                        Syz - Szy,       Sxx - Syy - Szz, Sxy + Syx,        Szx + Sxz,
                        Szx - Sxz,       Sxy + Syx,       -Sxx + Syy - Szz, Syz + Szy,
                        Sxy - Syx,       Szx + Sxz,       Syz + Szy,        -Sxx - Syy + Szz};
  double e[4];
  LargestEigenvector4(N, e);   // (w, x, y, z)
  double n = std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3]);
  if (!(n > 0)) { e[0] = 1; e[1] = e[2] = e[3] = 0; n = 1; }
  if (e[0] < 0) n = -n;
  const double w = e[0] / n, x = e[1] / n, y = e[2] / n, z = e[3] / n;
  out->q[0] = x; out->q[1] = y; out->q[2] = z; out->q[3] = w;
  double* R = out->R;
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w);     R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w);     R[7] = 2 * (y * z + x * w);     R[8] = 1 - 2 * (x * x + y * y);
  for (int a = 0; a < 3; ++a) out->t[a] = co[a] - ((R[3 * a] * cc[0] + R[3 * a + 1] * cc[1]) + R[3 * a + 2] * cc[2]);
}

int CountInliers(const Rigid& T, int n, const double* p_cur, const double* p_old, double threshold, uint8_t* mask) {
  int count = 0;
  for (int i = 0; i < n; ++i) {
    const double* p = p_cur + 3 * i;
    double d[3];
    for (int a = 0; a < 3; ++a) d[a] = (((T.R[3 * a] * p[0] + T.R[3 * a + 1] * p[1]) + T.R[3 * a + 2] * p[2]) + T.t[a]) - p_old[3 * i + a];
    const bool in = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) <= threshold;
    if (mask) mask[i] = in ? 1 : 0;
    count += in ? 1 : 0;
  }
  return count;
}

// sin^2 of the angle at point i0 of the triangle (i0, i1, i2) <= 1e-6, or a zero edge
bool Collinear(const double* p, int i0, int i1, int i2) {
  double a[3], b[3];
  for (int k = 0; k < 3; ++k) { a[k] = p[3 * i1 + k] - p[3 * i0 + k]; b[k] = p[3 * i2 + k] - p[3 * i0 + k]; }
  const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  const double cross2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
  const double scale = ((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]) * ((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
  return !(cross2 > 1e-6 * scale);
}

}  // namespace

uint32_t PlaceRansacSeed(int current_id, int matched_id) {
  return 0x0BAD51A4u ^ (static_cast<u32>(current_id) * 0x9E3779B1u) ^ (static_cast<u32>(matched_id) * 0x85EBCA6Bu);
}

void EstimateRelativePose(int current_id, int matched_id, int n, const double* p_cur, const double* p_old, int iterations, double inlier_threshold, int min_inliers,
                          RelativePoseEstimate* out) {
  *out = RelativePoseEstimate();
  out->inliers.assign(static_cast<size_t>(std::max(n, 0)), 0);
  if (n < 3) return;
  for (int i = 0; i < 3 * n; ++i)
    if (!std::isfinite(p_cur[i]) || !std::isfinite(p_old[i])) throw std::invalid_argument("EstimateRelativePose: non-finite point");
  u32 s = PlaceRansacSeed(current_id, matched_id);
  Rigid best;
  int best_count = -1;
  for (int it = 0; it < iterations; ++it) {
    int idx[3];
    for (int j = 0; j < 3; ++j) idx[j] = static_cast<int>(NextDraw(&s) % static_cast<u32>(n));
    if (idx[0] == idx[1] || idx[0] == idx[2] || idx[1] == idx[2]) continue;
    if (Collinear(p_cur, idx[0], idx[1], idx[2]) || Collinear(p_old, idx[0], idx[1], idx[2])) continue;
    Rigid T;
    AbsoluteOrientation(p_cur, p_old, idx, 3, &T);
    const int count = CountInliers(T, n, p_cur, p_old, inlier_threshold, nullptr);
    if (count > best_count) { best = T; best_count = count; }
  }
  if (best_count < 3) return;
  std::vector<uint8_t> mask(static_cast<size_t>(n));
  CountInliers(best, n, p_cur, p_old, inlier_threshold, mask.data());
  std::vector<int> index;
  for (int i = 0; i < n; ++i)
    if (mask[i]) index.push_back(i);
  Rigid refit;
  AbsoluteOrientation(p_cur, p_old, index.data(), static_cast<int>(index.size()), &refit);
  out->inlier_count = CountInliers(refit, n, p_cur, p_old, inlier_threshold, out->inliers.data());
  for (int a = 0; a < 4; ++a) out->q[a] = refit.q[a];
  for (int a = 0; a < 3; ++a) out->t[a] = refit.t[a];
  out->found = out->inlier_count >= min_inliers;
}

// ------------------------------------------------------------------------------------------------
// PlaceRecognizer
// ------------------------------------------------------------------------------------------------
PlaceRecognizer::PlaceRecognizer(bslam_context* ctx, int width, int height) : ctx_(ctx), width_(width), height_(height), cells_((width / 16) * (height / 16)) {
  if (cells_ <= 0) throw std::invalid_argument("PlaceRecognizer: the image holds no 16 x 16 cell");
}

PlaceRecognizer::~PlaceRecognizer() {
  for (void* p : {static_cast<void*>(database_), static_cast<void*>(match_), static_cast<void*>(count_)})
    if (p) { hipError_t e = hipFree(p); (void)e; }
}

void PlaceRecognizer::Reserve(hipStream_t stream, int slots) {
  if (slots <= capacity_) return;
  const int capacity = std::max(slots, std::max(16, 2 * capacity_));
  const size_t slot_bytes = static_cast<size_t>(9) * cells_ * sizeof(u32);
  u32* grown = nullptr;
  HIP_OR_THROW(hipMalloc(reinterpret_cast<void**>(&grown), slot_bytes * capacity));
  // a slot that was never written reads as empty (xy = 0xFFFFFFFF)
  hipError_t e = hipMemsetAsync(grown, 0xFF, slot_bytes * capacity, stream);
  if (e == hipSuccess && capacity_ > 0) e = hipMemcpyAsync(grown, database_, slot_bytes * capacity_, hipMemcpyDeviceToDevice, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) { hipError_t f = hipFree(grown); (void)f; throw std::runtime_error(std::string("PlaceRecognizer: growing the database: ") + hipGetErrorString(e)); }
  if (database_) HIP_OR_THROW(hipFree(database_));
  database_ = grown;
  capacity_ = capacity;
}

void PlaceRecognizer::Add(hipStream_t stream, const Keyframe& keyframe, int64_t score_threshold) {
  const int id = keyframe.id();
  if (id < 0) throw std::invalid_argument("PlaceRecognizer::Add: the keyframe has no id");
  const bslam_buffer2d color = keyframe.color_buffer().ToPod(), depth = keyframe.depth_buffer().ToPod();
  if (color.width != width_ || color.height != height_ || depth.width != width_ || depth.height != height_)
    throw std::invalid_argument("PlaceRecognizer::Add: colour and depth image must both have the size the recognizer was made for");
  Reserve(stream, id + 1);
  CheckRc(bslam_extract_keyframe_features(ctx_, stream, &color, &depth, score_threshold, Slot(id), Slot(id) + cells_), "bslam_extract_keyframe_features");
  if (static_cast<int>(added_.size()) <= id) added_.resize(static_cast<size_t>(id) + 1, false);
  added_[id] = true;
}

void PlaceRecognizer::Download(hipStream_t stream, int id, std::vector<u32>* xy, std::vector<u32>* desc) const {
  if (!Has(id)) throw std::invalid_argument("PlaceRecognizer::Download: keyframe " + std::to_string(id) + " has no features");
  xy->resize(static_cast<size_t>(cells_));
  desc->resize(static_cast<size_t>(8) * cells_);
  HIP_OR_THROW(hipMemcpyAsync(xy->data(), Slot(id), xy->size() * sizeof(u32), hipMemcpyDeviceToHost, stream));
  HIP_OR_THROW(hipMemcpyAsync(desc->data(), Slot(id) + cells_, desc->size() * sizeof(u32), hipMemcpyDeviceToHost, stream));
  HIP_OR_THROW(hipStreamSynchronize(stream));
}

void PlaceRecognizer::Match(hipStream_t stream, int query_id, int n_db, int max_distance, std::vector<int32_t>* match, std::vector<u32>* count) {
  if (!Has(query_id)) throw std::invalid_argument("PlaceRecognizer::Match: keyframe " + std::to_string(query_id) + " has no features");
  if (n_db < 0 || n_db > capacity_) throw std::invalid_argument("PlaceRecognizer::Match: n_db exceeds the database");
  match->assign(static_cast<size_t>(n_db) * cells_, -1);
  count->assign(static_cast<size_t>(n_db), 0);
  if (n_db == 0) return;
  if (n_db > match_capacity_) {
    const int capacity = std::max(n_db, 2 * match_capacity_);
    for (void* p : {static_cast<void*>(match_), static_cast<void*>(count_)})
      if (p) HIP_OR_THROW(hipFree(p));
    match_ = nullptr; count_ = nullptr; match_capacity_ = 0;
    HIP_OR_THROW(hipMalloc(reinterpret_cast<void**>(&match_), static_cast<size_t>(capacity) * cells_ * sizeof(int32_t)));
    HIP_OR_THROW(hipMalloc(reinterpret_cast<void**>(&count_), static_cast<size_t>(capacity) * sizeof(u32)));
    match_capacity_ = capacity;
  }
  CheckRc(bslam_match_features(ctx_, stream, Slot(query_id), Slot(query_id) + cells_, cells_, database_, n_db, max_distance, match_, count_), "bslam_match_features");
  HIP_OR_THROW(hipMemcpyAsync(match->data(), match_, match->size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  HIP_OR_THROW(hipMemcpyAsync(count->data(), count_, count->size() * sizeof(u32), hipMemcpyDeviceToHost, stream));
  HIP_OR_THROW(hipStreamSynchronize(stream));
}

int PlaceRecognizer::Query(hipStream_t stream, int current_id, int min_keyframe_gap, int min_matches, int max_distance,
                           const std::vector<std::shared_ptr<Keyframe>>& keyframes, int* match_count, std::vector<int32_t>* match_row) {
  *match_count = 0;
  match_row->clear();
  const int n_db = std::min(current_id - min_keyframe_gap + 1, capacity_);
  if (n_db <= 0) return -1;
  std::vector<int32_t> match;
  std::vector<u32> count;
  Match(stream, current_id, n_db, max_distance, &match, &count);
  int best = -1;
  for (int id = 0; id < n_db; ++id) {
    if (id >= static_cast<int>(keyframes.size()) || !keyframes[id] || !Has(id)) continue;   // deleted / merged, or never added
    if (static_cast<int>(count[id]) < min_matches) continue;
    if (best < 0 || count[id] > count[best]) best = id;   // strict: ties keep the lower id
  }
  if (best < 0) return -1;
  *match_count = static_cast<int>(count[best]);
  match_row->assign(match.begin() + static_cast<size_t>(best) * cells_, match.begin() + static_cast<size_t>(best + 1) * cells_);
  return best;
}

// ------------------------------------------------------------------------------------------------
// DirectBA: the place-recognition methods
// ------------------------------------------------------------------------------------------------
PlaceRecognizer& DirectBA::place_recognizer() {
  if (!place_recognizer_) place_recognizer_.reset(new PlaceRecognizer(ctx_, color_camera_.width(), color_camera_.height()));
  return *place_recognizer_;
}

void DirectBA::ResetPlaceRecognizer() { place_recognizer_.reset(); }

void DirectBA::ExtractKeyframeFeatures(hipStream_t stream, int keyframe_id, int64_t score_threshold, std::vector<u32>* xy, std::vector<u32>* desc) {
  const auto& kf = keyframes_.at(static_cast<size_t>(keyframe_id));
  if (!kf) throw std::invalid_argument("ExtractKeyframeFeatures: keyframe was deleted");
  PlaceRecognizer& pr = place_recognizer();
  pr.Add(stream, *kf, score_threshold);
  if (xy && desc) pr.Download(stream, keyframe_id, xy, desc);
}

void DirectBA::MatchKeyframeFeatures(hipStream_t stream, int query_id, const std::vector<int>& ids, int max_distance, std::vector<int32_t>* match,
                                     std::vector<u32>* count) {
  PlaceRecognizer& pr = place_recognizer();
  int n_db = 0;
  for (int id : ids) {
    if (!pr.Has(id)) throw std::invalid_argument("MatchKeyframeFeatures: keyframe " + std::to_string(id) + " has no features (ExtractKeyframeFeatures first)");
    n_db = std::max(n_db, id + 1);
  }
  std::vector<int32_t> all_match;
  std::vector<u32> all_count;
  pr.Match(stream, query_id, n_db, max_distance, &all_match, &all_count);
  const size_t cells = static_cast<size_t>(pr.cells());
  match->clear();
  count->clear();
  for (int id : ids) {
    match->insert(match->end(), all_match.begin() + id * cells, all_match.begin() + (id + 1) * cells);
    count->push_back(all_count[static_cast<size_t>(id)]);
  }
}

void DirectBA::RecognizePlace(hipStream_t stream, int current_id, const PlaceRecognitionOptions& options, int num_scales, PlaceRecognitionResult* result) {
  *result = PlaceRecognitionResult();
  result->keyframe_id = current_id;
  if (options.min_keyframe_gap < 1) throw std::invalid_argument("RecognizePlace: min_keyframe_gap must be >= 1");
  if (current_id < 0 || current_id >= static_cast<int>(keyframes_.size()) || !keyframes_[current_id]) throw std::invalid_argument("RecognizePlace: no such keyframe");
  PlaceRecognizer& pr = place_recognizer();
  for (int id = 0; id <= current_id; ++id)   // every keyframe enters the database once; normally only the new one is missing
    if (keyframes_[id] && !pr.Has(id)) pr.Add(stream, *keyframes_[id], options.score_threshold);
  std::vector<int32_t> match_row;
  const int candidate = pr.Query(stream, current_id, options.min_keyframe_gap, options.min_matches, options.max_distance, keyframes_, &result->match_count, &match_row);
  result->candidate_id = candidate;
  if (candidate < 0) return;

  // Points of the matched pixels (BS/loop_detector.cc:283-297): depth = raw * raw_to_float_depth without the cfactor
  // correction, unprojected at the pixel's centre (x + 0.5, y + 0.5) in the pixel-corner convention.
  std::vector<u32> xy_cur, xy_old, desc;
  pr.Download(stream, current_id, &xy_cur, &desc);
  pr.Download(stream, candidate, &xy_old, &desc);
  const int w = depth_camera_.width(), h = depth_camera_.height();
  std::vector<u16> depth_cur(static_cast<size_t>(w) * h), depth_old(depth_cur.size());
  keyframes_[current_id]->depth_buffer().Download(stream, depth_cur.data(), static_cast<size_t>(w) * sizeof(u16));
  keyframes_[candidate]->depth_buffer().Download(stream, depth_old.data(), static_cast<size_t>(w) * sizeof(u16));
  const float* cam = depth_camera_.parameters();
  const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], scale = raw_to_float_depth_;
  auto unproject = [&](u32 xy, const std::vector<u16>& depth, std::vector<double>* out) {
    const int x = static_cast<int>(xy & 0xffffu), y = static_cast<int>(xy >> 16);
    const double z = static_cast<double>(depth[static_cast<size_t>(y) * w + x]) * scale;
    out->push_back(((x + 0.5) - cx) / fx * z);
    out->push_back(((y + 0.5) - cy) / fy * z);
    out->push_back(z);
  };
  std::vector<double> p_cur, p_old;
  for (int q = 0; q < pr.cells(); ++q) {
    if (match_row[q] < 0) continue;
    unproject(xy_cur[q], depth_cur, &p_cur);
    unproject(xy_old[static_cast<size_t>(match_row[q])], depth_old, &p_old);
  }
  EstimateRelativePose(current_id, candidate, static_cast<int>(p_cur.size() / 3), p_cur.data(), p_old.data(), options.ransac_iterations,
                       options.ransac_inlier_threshold, options.ransac_min_inliers, &result->pose);
  if (!result->pose.found) return;
  SE3f old_T_cur;
  old_T_cur.qx = static_cast<float>(result->pose.q[0]); old_T_cur.qy = static_cast<float>(result->pose.q[1]);
  old_T_cur.qz = static_cast<float>(result->pose.q[2]); old_T_cur.qw = static_cast<float>(result->pose.q[3]);
  old_T_cur.tx = static_cast<float>(result->pose.t[0]); old_T_cur.ty = static_cast<float>(result->pose.t[1]); old_T_cur.tz = static_cast<float>(result->pose.t[2]);
  result->loop_attempted = true;
  CloseLoop(*this, stream, current_id, candidate, old_T_cur, num_scales, &result->loop);
}

}  // namespace bslam_host
