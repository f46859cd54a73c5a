"""Accuracy and completeness of a reconstructed surface against a ground-truth surface: the counterpart of ate.py for geometry.

Both figures are one primitive, the distance from each point of a set to the nearest triangle of a mesh within a search radius
(DirectBA.PointMeshDistance, bslam_point_mesh_distance on the GPU):

    accuracy       the reconstruction's vertices -> the ground truth      (how far is what was built from the truth)
    completeness   the ground truth's vertices   -> the reconstruction    (how much of the truth was built)

with, per threshold d, precision = the share of the reconstruction's vertices within d of the ground truth, recall = the share
of the ground truth's vertices within d of the reconstruction, and F-score = 2 P R / (P + R).  A point without a hit inside the
search radius fails every threshold.

Completeness is sampled at the ground truth's VERTICES.  A coarsely tessellated ground truth (a wall of two triangles) says
nothing about the surface between its corners: its owner has to subdivide it to the resolution the thresholds ask for.  No
surface sampler is part of this.  The ground truth has to be given in the frame of the reconstruction; align it first, for
example with the transform ate.align_rigid finds for the trajectory.  A ground truth without triangles is a point cloud (the form the
ETH3D SLAM scans come in): every point then is its own degenerate triangle.

distance_summary is pure NumPy; evaluate needs a DirectBA for the distance calls.
"""
import numpy as np


def _percentile(sorted_values, q):
    """Linear-interpolated percentile of an ascending array (NumPy's default method), nan when empty."""
    if len(sorted_values) == 0:
        return float("nan")
    return float(np.percentile(sorted_values, q))


def distance_summary(distance, thresholds):
    """Summary of the distances a PointMeshDistance call returned (+inf: no hit inside the search radius).
    Over the hits: mean, median, rmse, p90, p99 (nan without a hit).  Of ALL points: `within`, the share at a distance <= each
    threshold (a list in the order of `thresholds`), and `beyond`, the share without a hit.  count / hits: the numbers of points."""
    d = np.asarray(distance, np.float64).reshape(-1)
    hit = np.isfinite(d)
    h = np.sort(d[hit])
    n = len(d)
    nan = float("nan")
    return dict(count=int(n), hits=int(len(h)),
                mean=float(h.mean()) if len(h) else nan, median=_percentile(h, 50), rmse=float(np.sqrt(np.mean(h * h))) if len(h) else nan,
                p90=_percentile(h, 90), p99=_percentile(h, 99),
                thresholds=[float(t) for t in thresholds],
                within=[float(np.count_nonzero(h <= float(t)) / n) if n else nan for t in thresholds],
                beyond=float((n - len(h)) / n) if n else nan)


def f_scores(accuracy, completeness):
    """Per threshold: precision = accuracy's share within, recall = completeness's share within, F = 2 P R / (P + R) (0 when both
    are 0, nan when a side has no point)."""
    out = []
    for t, p, r in zip(accuracy["thresholds"], accuracy["within"], completeness["within"]):
        f = 0.0 if p + r == 0 else 2.0 * p * r / (p + r)
        out.append(dict(threshold=t, precision=p, recall=r, f_score=f))
    return out


def evaluate(ba, reconstruction, ground_truth, max_distance=0.1, thresholds=(0.01, 0.02, 0.05), cell_size=None):
    """reconstruction, ground_truth: mesh dicts (positions (V, 3), triangles (T, 3); DirectBA.ExtractMesh, LoadPLY) in one frame; the
    ground truth may be a point cloud (no or empty triangles).  -> dict of accuracy and completeness (distance_summary each),
    f_scores (a list per threshold), max_distance and the grids the two calls used.  Completeness is sampled at the ground truth's
    vertices: see the module's docstring."""
    acc = ba.PointMeshDistance(reconstruction["positions"], ground_truth, max_distance, cell_size)
    com = ba.PointMeshDistance(ground_truth["positions"], reconstruction, max_distance, cell_size)
    accuracy, completeness = distance_summary(acc["distance"], thresholds), distance_summary(com["distance"], thresholds)
    grid = lambda r: dict(cell_size=r["cell_size"], grid_cells=r["grid_cells"], grid_entries=r["grid_entries"])
    return dict(max_distance=float(max_distance), accuracy=accuracy, completeness=completeness, f_scores=f_scores(accuracy, completeness),
                accuracy_grid=grid(acc), completeness_grid=grid(com))


def format_summary(name, s):
    within = ", ".join(f"<= {t:g}: {100 * w:.1f} %" for t, w in zip(s["thresholds"], s["within"]))
    return (f"{name}: {s['hits']} of {s['count']} points hit; mean {s['mean']:.4f}, median {s['median']:.4f}, rmse {s['rmse']:.4f}, p90 {s['p90']:.4f}, "
            f"p99 {s['p99']:.4f}; {within}; beyond {100 * s['beyond']:.1f} %")
