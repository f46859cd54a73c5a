// pose_graph.cpp -- see pose_graph.hpp.
#include "pose_graph.hpp"

#include <algorithm>
#include <cmath>
#include <map>
#include <stdexcept>
#include <string>

namespace bslam_host {

namespace {
using Mat6 = double[36];

void Mat3Mul(const double* A, const double* B, double* C) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}

// Cyclic Jacobi eigen-decomposition of a symmetric 3x3 matrix: A = V diag(w) V^T (V column-major eigenvectors in columns).
void SymmetricEigen3(const double* A_in, double* w, double* V) {
  double A[9];
  std::copy(A_in, A_in + 9, A);
  for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) ? 1 : 0;
  for (int sweep = 0; sweep < 50; ++sweep) {
    const double off = A[1] * A[1] + A[2] * A[2] + A[5] * A[5];
    if (off < 1e-300) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        const double apq = A[3 * p + q];
        if (apq == 0) continue;
        const double theta = (A[3 * q + q] - A[3 * p + p]) / (2 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1));
        const double c = 1 / std::sqrt(t * t + 1), s = t * c;
        for (int k = 0; k < 3; ++k) {   // A <- A J
          const double akp = A[3 * k + p], akq = A[3 * k + q];
          A[3 * k + p] = c * akp - s * akq;
          A[3 * k + q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {   // A <- J^T A
          const double apk = A[3 * p + k], aqk = A[3 * q + k];
          A[3 * p + k] = c * apk - s * aqk;
          A[3 * q + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 3; ++k) {   // V <- V J
          const double vkp = V[3 * k + p], vkq = V[3 * k + q];
          V[3 * k + p] = c * vkp - s * vkq;
          V[3 * k + q] = s * vkp + c * vkq;
        }
      }
  }
  for (int i = 0; i < 3; ++i) w[i] = A[4 * i];
}

// In-place Cholesky of a symmetric positive definite 6x6 block (lower triangle, upper zeroed).
void Cholesky6(double* A) {
  for (int j = 0; j < 6; ++j) {
    double d = A[6 * j + j];
    for (int k = 0; k < j; ++k) d -= A[6 * j + k] * A[6 * j + k];
    if (!(d > 0)) throw std::runtime_error("OptimizePoseGraph: system is not positive definite (is every vertex connected to the gauge?)");
    d = std::sqrt(d);
    A[6 * j + j] = d;
    for (int i = j + 1; i < 6; ++i) {
      double v = A[6 * i + j];
      for (int k = 0; k < j; ++k) v -= A[6 * i + k] * A[6 * j + k];
      A[6 * i + j] = v / d;
    }
    for (int i = 0; i < j; ++i) A[6 * i + j] = 0;
  }
}
// X <- X * L^-T (X 6x6, L lower triangular)
void RightSolveLT(const double* L, double* X) {
  for (int r = 0; r < 6; ++r)
    for (int j = 0; j < 6; ++j) {
      double v = X[6 * r + j];
      for (int k = 0; k < j; ++k) v -= X[6 * r + k] * L[6 * j + k];
      X[6 * r + j] = v / L[6 * j + j];
    }
}
// C -= A * B^T
void SubABt(const double* A, const double* B, double* C) {
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) {
      double v = 0;
      for (int k = 0; k < 6; ++k) v += A[6 * r + k] * B[6 * c + k];
      C[6 * r + c] -= v;
    }
}

struct Block { double m[36]; };
}  // namespace

Pose3d Pose3d::FromQuaternion(double qx, double qy, double qz, double qw, double tx, double ty, double tz) {
  const double n = std::sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
  qx /= n; qy /= n; qz /= n; qw /= n;
  Pose3d T;
  T.R[0] = 1 - 2 * (qy * qy + qz * qz); T.R[1] = 2 * (qx * qy - qz * qw);     T.R[2] = 2 * (qx * qz + qy * qw);
  T.R[3] = 2 * (qx * qy + qz * qw);     T.R[4] = 1 - 2 * (qx * qx + qz * qz); T.R[5] = 2 * (qy * qz - qx * qw);
  T.R[6] = 2 * (qx * qz - qy * qw);     T.R[7] = 2 * (qy * qz + qx * qw);     T.R[8] = 1 - 2 * (qx * qx + qy * qy);
  T.t[0] = tx; T.t[1] = ty; T.t[2] = tz;
  return T;
}

void Pose3d::ToQuaternion(double* qx, double* qy, double* qz, double* qw) const {
  double q[3], w;
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0) {
    double s = std::sqrt(tr + 1.0);
    w = 0.5 * s;
    s = 0.5 / s;
    q[0] = (R[7] - R[5]) * s; q[1] = (R[2] - R[6]) * s; q[2] = (R[3] - R[1]) * s;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double s = std::sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
    q[i] = 0.5 * s;
    s = 0.5 / s;
    w = (R[3 * k + j] - R[3 * j + k]) * s;
    q[j] = (R[3 * j + i] + R[3 * i + j]) * s;
    q[k] = (R[3 * k + i] + R[3 * i + k]) * s;
  }
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + w * w);
  const double sgn = (w < 0) ? -1.0 : 1.0;
  *qx = sgn * q[0] / n; *qy = sgn * q[1] / n; *qz = sgn * q[2] / n; *qw = sgn * w / n;
}

Pose3d Pose3d::Inverse() const {
  Pose3d I;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) I.R[3 * r + c] = R[3 * c + r];
  for (int r = 0; r < 3; ++r) I.t[r] = -(I.R[3 * r] * t[0] + I.R[3 * r + 1] * t[1] + I.R[3 * r + 2] * t[2]);
  return I;
}

Pose3d Pose3d::operator*(const Pose3d& o) const {
  Pose3d P;
  Mat3Mul(R, o.R, P.R);
  for (int r = 0; r < 3; ++r) P.t[r] = R[3 * r] * o.t[0] + R[3 * r + 1] * o.t[1] + R[3 * r + 2] * o.t[2] + t[r];
  return P;
}

void PoseGraphEdgeError(const Pose3d& from, const Pose3d& to, const Pose3d& from_T_to, double* e) {
  const Pose3d delta = from_T_to.Inverse() * (from.Inverse() * to);
  double qw;
  delta.ToQuaternion(e + 3, e + 4, e + 5, &qw);
  e[0] = delta.t[0]; e[1] = delta.t[1]; e[2] = delta.t[2];
}

Pose3d PoseFromVectorMQT(const double* d) {
  const double w2 = 1 - (d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
  Pose3d T = (w2 < 0) ? Pose3d() : Pose3d::FromQuaternion(d[3], d[4], d[5], std::sqrt(w2), 0, 0, 0);
  T.t[0] = d[0]; T.t[1] = d[1]; T.t[2] = d[2];
  return T;
}

void OptimizePoseGraph(std::vector<Pose3d>* poses_, const std::vector<PoseGraphEdge>& edges, int fixed_vertex, int iterations, PoseGraphResult* result) {
  std::vector<Pose3d>& poses = *poses_;
  const int n = static_cast<int>(poses.size());
  if (fixed_vertex < 0 || fixed_vertex >= n) throw std::invalid_argument("OptimizePoseGraph: fixed vertex out of range");
  for (const PoseGraphEdge& e : edges)
    if (e.from < 0 || e.from >= n || e.to < 0 || e.to >= n || e.from == e.to) throw std::invalid_argument("OptimizePoseGraph: bad edge");
  // unknown index of each vertex (-1 = the gauge)
  std::vector<int> unknown(n, -1);
  int m = 0;
  for (int v = 0; v < n; ++v)
    if (v != fixed_vertex) unknown[v] = m++;
  auto chi2_of = [&]() {
    double s = 0;
    for (const PoseGraphEdge& e : edges) {
      double err[6];
      PoseGraphEdgeError(poses[e.from], poses[e.to], e.from_T_to, err);
      for (int i = 0; i < 6; ++i) s += err[i] * err[i];
    }
    return s;
  };
  PoseGraphResult res;
  res.initial_chi2 = chi2_of();
  constexpr double kStep = 1e-6;   // central-difference step in the update coordinates
  for (int it = 0; it < iterations; ++it) {
    // H = sum J^T J, g = sum J^T e in block form; diag[i] and lower[col][row] (row > col) hold the blocks of H
    std::vector<Block> diag(m);
    for (Block& b : diag) std::fill(b.m, b.m + 36, 0.0);
    std::vector<std::map<int, Block>> lower(m);
    std::vector<double> g(6 * static_cast<size_t>(m), 0.0);
    for (const PoseGraphEdge& e : edges) {
      double err[6], J[2][36];   // J[side][6 * row + col]
      PoseGraphEdgeError(poses[e.from], poses[e.to], e.from_T_to, err);
      const int vs[2] = {e.from, e.to};
      for (int side = 0; side < 2; ++side) {
        if (unknown[vs[side]] < 0) continue;
        for (int c = 0; c < 6; ++c) {
          double d[6] = {0, 0, 0, 0, 0, 0};
          double ep[6], em[6];
          d[c] = kStep;
          const Pose3d plus = poses[vs[side]] * PoseFromVectorMQT(d);
          d[c] = -kStep;
          const Pose3d minus = poses[vs[side]] * PoseFromVectorMQT(d);
          if (side == 0) { PoseGraphEdgeError(plus, poses[e.to], e.from_T_to, ep); PoseGraphEdgeError(minus, poses[e.to], e.from_T_to, em); }
          else { PoseGraphEdgeError(poses[e.from], plus, e.from_T_to, ep); PoseGraphEdgeError(poses[e.from], minus, e.from_T_to, em); }
          for (int r = 0; r < 6; ++r) J[side][6 * r + c] = (ep[r] - em[r]) / (2 * kStep);
        }
      }
      for (int a = 0; a < 2; ++a) {
        const int ua = unknown[vs[a]];
        if (ua < 0) continue;
        for (int r = 0; r < 6; ++r) {
          double v = 0;
          for (int k = 0; k < 6; ++k) v += J[a][6 * k + r] * err[k];
          g[6 * ua + r] += v;
        }
        for (int bside = 0; bside < 2; ++bside) {
          const int ub = unknown[vs[bside]];
          if (ub < 0 || ub > ua) continue;   // lower triangle: row ua >= col ub
          double* blk = (ub == ua) ? diag[ua].m : nullptr;
          if (!blk) {
            auto ins = lower[ub].emplace(ua, Block{});
            if (ins.second) std::fill(ins.first->second.m, ins.first->second.m + 36, 0.0);
            blk = ins.first->second.m;
          }
          for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) {
              double v = 0;
              for (int k = 0; k < 6; ++k) v += J[a][6 * k + r] * J[bside][6 * k + c];
              blk[6 * r + c] += v;
            }
        }
      }
    }
    // right-looking block Cholesky in vertex order: H = L L^T, fill lands in lower[k] for rows of a shared column
    size_t blocks = static_cast<size_t>(m);
    for (int j = 0; j < m; ++j) {
      Cholesky6(diag[j].m);
      for (auto& rb : lower[j]) RightSolveLT(diag[j].m, rb.second.m);   // L_ij = A_ij L_jj^-T
      for (auto it_i = lower[j].begin(); it_i != lower[j].end(); ++it_i) {
        const int i = it_i->first;
        SubABt(it_i->second.m, it_i->second.m, diag[i].m);
        for (auto it_k = lower[j].begin(); it_k != it_i; ++it_k) {   // k < i: A_ik -= L_ij L_kj^T, stored in column k
          auto ins = lower[it_k->first].emplace(i, Block{});
          if (ins.second) std::fill(ins.first->second.m, ins.first->second.m + 36, 0.0);
          SubABt(it_i->second.m, it_k->second.m, ins.first->second.m);
        }
      }
      blocks += lower[j].size();
    }
    res.factor_blocks = blocks;
    // L y = -g (forward), L^T x = y (backward)
    std::vector<double> x(6 * static_cast<size_t>(m));
    for (size_t i = 0; i < x.size(); ++i) x[i] = -g[i];
    for (int j = 0; j < m; ++j) {
      double* xj = &x[6 * static_cast<size_t>(j)];
      const double* L = diag[j].m;
      for (int r = 0; r < 6; ++r) {
        double v = xj[r];
        for (int k = 0; k < r; ++k) v -= L[6 * r + k] * xj[k];
        xj[r] = v / L[6 * r + r];
      }
      for (const auto& rb : lower[j]) {
        double* xi = &x[6 * static_cast<size_t>(rb.first)];
        for (int r = 0; r < 6; ++r)
          for (int k = 0; k < 6; ++k) xi[r] -= rb.second.m[6 * r + k] * xj[k];
      }
    }
    for (int j = m - 1; j >= 0; --j) {
      double* xj = &x[6 * static_cast<size_t>(j)];
      for (const auto& rb : lower[j]) {
        const double* xi = &x[6 * static_cast<size_t>(rb.first)];
        for (int r = 0; r < 6; ++r)
          for (int k = 0; k < 6; ++k) xj[r] -= rb.second.m[6 * k + r] * xi[k];
      }
      const double* L = diag[j].m;
      for (int r = 5; r >= 0; --r) {
        double v = xj[r];
        for (int k = r + 1; k < 6; ++k) v -= L[6 * k + r] * xj[k];
        xj[r] = v / L[6 * r + r];
      }
    }
    for (int v = 0; v < n; ++v)
      if (unknown[v] >= 0) poses[v] = poses[v] * PoseFromVectorMQT(&x[6 * static_cast<size_t>(unknown[v])]);
    res.chi2.push_back(chi2_of());
  }
  if (result) *result = res;
}

int OptimizeKeyframePoseGraph(std::vector<Pose3d>* keyframe_global_T_frame, const std::vector<bool>& exists, const std::vector<KeyframeLoopEdge>& loop_edges,
                              int iterations, PoseGraphResult* result) {
  std::vector<Pose3d>& kf = *keyframe_global_T_frame;
  if (exists.size() != kf.size()) throw std::invalid_argument("OptimizeKeyframePoseGraph: exists / poses size mismatch");
  std::vector<int> vertex_of(kf.size(), -1), id_of;
  for (size_t i = 0; i < kf.size(); ++i)
    if (exists[i]) { vertex_of[i] = static_cast<int>(id_of.size()); id_of.push_back(static_cast<int>(i)); }
  if (id_of.empty()) return -1;
  std::vector<Pose3d> poses;
  for (int id : id_of) poses.push_back(kf[id]);
  std::vector<PoseGraphEdge> edges;
  for (size_t v = 0; v + 1 < id_of.size(); ++v)   // odometry constraints from the current state (BS/pose_graph_optimizer.cc:80-99)
    edges.push_back(PoseGraphEdge{static_cast<int>(v), static_cast<int>(v + 1), poses[v].Inverse() * poses[v + 1]});
  for (const KeyframeLoopEdge& e : loop_edges) {
    if (e.from_id < 0 || e.to_id < 0 || e.from_id >= static_cast<int>(kf.size()) || e.to_id >= static_cast<int>(kf.size()) || vertex_of[e.from_id] < 0 ||
        vertex_of[e.to_id] < 0)
      throw std::invalid_argument("OptimizeKeyframePoseGraph: loop edge names a missing keyframe");
    edges.push_back(PoseGraphEdge{vertex_of[e.from_id], vertex_of[e.to_id], e.from_T_to});
  }
  OptimizePoseGraph(&poses, edges, 0, iterations, result);
  for (size_t v = 0; v < id_of.size(); ++v) kf[id_of[v]] = poses[v];
  return id_of[0];
}

Pose3d AveragePose(const std::vector<Pose3d>& poses) {
  if (poses.empty()) throw std::invalid_argument("AveragePose: no poses");
  double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, t[3] = {0, 0, 0};
  for (const Pose3d& p : poses) {
    for (int i = 0; i < 9; ++i) M[i] += p.R[i];
    for (int i = 0; i < 3; ++i) t[i] += p.t[i];
  }
  // U V^T of M = U S V^T is M (M^T M)^-1/2
  double MtM[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) MtM[3 * r + c] = M[r] * M[c] + M[3 + r] * M[3 + c] + M[6 + r] * M[6 + c];
  double w[3], V[9];
  SymmetricEigen3(MtM, w, V);
  double S[9];   // V diag(w^-1/2) V^T
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double v = 0;
      for (int k = 0; k < 3; ++k) v += V[3 * r + k] * V[3 * c + k] / std::sqrt(w[k]);
      S[3 * r + c] = v;
    }
  Pose3d out;
  Mat3Mul(M, S, out.R);
  for (int i = 0; i < 3; ++i) out.t[i] = t[i] / static_cast<double>(poses.size());
  return out;
}

}  // namespace bslam_host
