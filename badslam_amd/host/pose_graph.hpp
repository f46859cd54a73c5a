// pose_graph.hpp -- the keyframe pose graph of loop closure (BS/pose_graph_optimizer.cc) without g2o: vertices are
// rigid poses (g2o::VertexSE3), edges relative-pose measurements with identity information (g2o::EdgeSE3), solved by
// plain Gauss-Newton (g2o::OptimizationAlgorithmGaussNewton) with a block sparse Cholesky in vertex order.
// Double precision throughout; no GPU.
//
//   edge error   delta = meas^-1 * from^-1 * to,  e = [delta.t; q.xyz]   (q = delta's rotation, normalised, w >= 0)
//   vertex step  T <- T * fromVectorMQT(d),  d = [t; qx qy qz], qw = sqrt(1 - |q.xyz|^2) (identity rotation if negative)
//
// The Jacobians are central differences of that error in the update coordinates (the reference's EdgeSE3 has analytic
// ones; both vanish at the same stationary point, which is what the fixed iteration count converges to).
#pragma once

#include <cstddef>
#include <vector>

namespace bslam_host {

struct Pose3d {   // rotation (row-major) and translation: p_parent = R * p_child + t
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  double t[3] = {0, 0, 0};

  static Pose3d FromQuaternion(double qx, double qy, double qz, double qw, double tx, double ty, double tz);   // normalises q
  void ToQuaternion(double* qx, double* qy, double* qz, double* qw) const;   // Eigen's Quaternion(Matrix3), normalised, w >= 0
  Pose3d Inverse() const;
  Pose3d operator*(const Pose3d& o) const;
};

struct PoseGraphEdge {
  int from, to;       // vertex indices
  Pose3d from_T_to;   // measurement
};

struct PoseGraphResult {
  std::vector<double> chi2;     // sum of squared edge errors after each iteration
  double initial_chi2 = 0;
  size_t factor_blocks = 0;     // 6x6 blocks stored by the Cholesky factor (diagonal included)
};

// g2o::EdgeSE3::computeError
void PoseGraphEdgeError(const Pose3d& from, const Pose3d& to, const Pose3d& from_T_to, double* e6);
// g2o::internal::fromVectorMQT
Pose3d PoseFromVectorMQT(const double* d6);

// Optimises `poses` in place; vertex `fixed_vertex` is held constant (the gauge).  Throws std::invalid_argument on a
// bad edge index and std::runtime_error if the system is not positive definite (a vertex not connected to the gauge).
void OptimizePoseGraph(std::vector<Pose3d>* poses, const std::vector<PoseGraphEdge>& edges, int fixed_vertex, int iterations, PoseGraphResult* result);

// The graph of BS/pose_graph_optimizer.cc:48-113 over a keyframe list: vertex per non-deleted keyframe (exists[i]), an
// odometry edge between consecutive non-deleted keyframes measured from the current poses, plus the given loop edges
// (keyframe ids).  The gauge is the lowest-id existing keyframe (the reference fixes vertex 0, i.e. keyframe 0, and
// would fail if it was deleted).  Returns the gauge keyframe id, or -1 if no keyframe exists.
struct KeyframeLoopEdge {
  int from_id, to_id;
  Pose3d from_T_to;
};
int OptimizeKeyframePoseGraph(std::vector<Pose3d>* keyframe_global_T_frame, const std::vector<bool>& exists, const std::vector<KeyframeLoopEdge>& loop_edges,
                              int iterations, PoseGraphResult* result);

// AveragePose (BS/util.cc:110-129): rotation = SVD projection of the summed rotation matrices, translation = mean.
Pose3d AveragePose(const std::vector<Pose3d>& poses);

}  // namespace bslam_host
