// place_recognition.hpp -- the front half of vis::LoopDetector::AddImage (BS/loop_detector.cc:98-127, 160-167, 274-360):
// recognise the place a new keyframe shows and estimate its pose relative to the recognised keyframe, which is what
// CloseLoop (host/loop_closure.hpp) starts from.  In place of FAST + BRIEF + DBoW2 + opengv:
//   features   one Harris corner with a 256-bit BRIEF descriptor per 16 x 16 cell (bslam_extract_keyframe_features)
//   matching   brute force against every older keyframe with a ratio test (bslam_match_features); the candidate is the
//              keyframe with the most accepted matches
//   start pose 3D-3D RANSAC on the matched pixels' depths, host code in double (EstimateRelativePose)
// DESIGN.md 8 "Place recognition" lists the rules and the deviations from the reference.
#pragma once

#include <cstdint>
#include <vector>

#include "direct_ba.hpp"
#include "loop_closure.hpp"

namespace bslam_host {

struct PlaceRecognitionOptions {
  int min_keyframe_gap = 10;                    // candidates have id <= current id - min_keyframe_gap
  int64_t score_threshold = 100000000000LL;     // corner score a feature must exceed (provisional: synthetic scenes only)
  int max_distance = 64;                        // largest accepted Hamming distance (provisional)
  int min_matches = 25;                         // accepted matches a candidate needs (provisional)
  int ransac_iterations = 500;                  // BS/loop_detector.cc:310-312
  double ransac_inlier_threshold = 0.06;        // metres
  int ransac_min_inliers = 10;
};

struct RelativePoseEstimate {
  bool found = false;
  double q[4] = {0, 0, 0, 1};   // old_T_cur: rotation as a unit quaternion (x, y, z, w), w >= 0
  double t[3] = {0, 0, 0};
  int inlier_count = 0;
  std::vector<uint8_t> inliers;   // per correspondence, after the refit
};

// 3D-3D RANSAC: p_cur / p_old hold n corresponding points (3 doubles each) in the frames of the current and the matched
// keyframe.  Hypotheses: `iterations` triples of indices from the generator s = s * 1664525 + 1013904223 (mod 2^32),
// index (s >> 16) % n, with s seeded by PlaceRansacSeed(current_id, matched_id); a triple with a repeated index, or whose
// points are collinear in either frame (sin^2 of the angle at the first point <= 1e-6), is skipped.  Model: Horn's
// closed-form absolute orientation.  Inlier: |R p_cur + t - p_old| <= inlier_threshold.  The hypothesis with the most
// inliers wins (the first among equals), is refitted on its inliers, the inliers are counted again, and the estimate is
// rejected below min_inliers.  Pure host code, no GPU; never produces NaN from finite input.
uint32_t PlaceRansacSeed(int current_id, int matched_id);
void EstimateRelativePose(int current_id, int matched_id, int n, const double* p_cur, const double* p_old, int iterations, double inlier_threshold, int min_inliers,
                          RelativePoseEstimate* out);

struct PlaceRecognitionResult {
  int keyframe_id = -1;
  int candidate_id = -1;      // -1: no keyframe reached min_matches
  int match_count = 0;        // accepted matches of the candidate
  RelativePoseEstimate pose;  // found = false without a candidate or when RANSAC rejects
  bool loop_attempted = false;   // CloseLoop ran (a candidate and a start pose exist)
  LoopClosureResult loop;
};

// The device database: one slot of 9 * cells words per keyframe id (xy[cells], then desc[cells][8]), grown geometrically.
class PlaceRecognizer {
 public:
  PlaceRecognizer(bslam_context* ctx, int width, int height);
  ~PlaceRecognizer();
  PlaceRecognizer(const PlaceRecognizer&) = delete;
  PlaceRecognizer& operator=(const PlaceRecognizer&) = delete;

  int cells() const { return cells_; }
  bool Has(int id) const { return id >= 0 && id < static_cast<int>(added_.size()) && added_[id]; }
  // Extracts the keyframe's features straight into slot keyframe.id() (again, if it was added before).
  void Add(hipStream_t stream, const Keyframe& keyframe, int64_t score_threshold);
  void Download(hipStream_t stream, int id, std::vector<u32>* xy, std::vector<u32>* desc) const;
  // One match launch of slot query_id against slots 0 ... n_db - 1: match[n_db][cells], count[n_db] on the host.
  void Match(hipStream_t stream, int query_id, int n_db, int max_distance, std::vector<int32_t>* match, std::vector<u32>* count);
  // The existing keyframe (keyframes[id] != null, features added) with id <= current_id - min_keyframe_gap that has the
  // most accepted matches, at least min_matches (ties: the lower id); -1 if there is none.  match_row: its row of `match`.
  int Query(hipStream_t stream, int current_id, int min_keyframe_gap, int min_matches, int max_distance, const std::vector<std::shared_ptr<Keyframe>>& keyframes,
            int* match_count, std::vector<int32_t>* match_row);

 private:
  u32* Slot(int id) const { return database_ + static_cast<size_t>(id) * 9 * cells_; }
  void Reserve(hipStream_t stream, int slots);

  bslam_context* ctx_;
  int width_, height_, cells_;
  u32* database_ = nullptr;
  int capacity_ = 0;
  int32_t* match_ = nullptr;   // device outputs of Match, grown with n_db
  u32* count_ = nullptr;
  int match_capacity_ = 0;
  std::vector<bool> added_;
};

}  // namespace bslam_host
