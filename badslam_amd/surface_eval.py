"""Accuracy and completeness of a reconstructed surface against a ground-truth surface: the counterpart of ate.py for geometry.

Both figures are one primitive, the distance from each point of a set to the nearest triangle of a mesh within a search radius
(DirectBA.PointMeshDistance, bslam_point_mesh_distance on the GPU):

    accuracy       the reconstruction's vertices -> the ground truth      (how far is what was built from the truth)
    completeness   the ground truth's vertices   -> the reconstruction    (how much of the truth was built)

with, per threshold d, precision = the share of the reconstruction's vertices within d of the ground truth, recall = the share
of the ground truth's vertices within d of the reconstruction, and F-score = 2 P R / (P + R).  A point without a hit inside the
search radius fails every threshold.

By default both point sets are the meshes' VERTICES, and then the figures depend on how the meshes happen to be tessellated: a
wall of two triangles says nothing about the surface between its corners, and a scan meshed at 1 mm outweighs a plane next to it
by orders of magnitude.  evaluate(sample_density=...) measures at points drawn uniformly by area instead, as the published surface
benchmarks do (DirectBA.SampleMesh, bslam_sample_mesh on the GPU): accuracy from samples of the reconstruction, completeness from
samples of the ground truth, `sample_density` per square unit on each, the meshes themselves staying the targets.  A side
without triangles (a point cloud) cannot be sampled and keeps its vertices.

The ground truth has to be given in the frame of the reconstruction, or evaluate(register=True) has to bring the reconstruction into the ground truth's frame first (DirectBA.RegisterPoints, an iterative closest point that
needs a start within its search radius, for example the transform ate.align_rigid finds for the trajectory).  A ground truth without triangles is a point cloud (the form the
ETH3D SLAM scans come in): every point then is its own degenerate triangle.

evaluate(max_distance=None) measures without a search radius (DirectBA.NearestTriangle, bslam_nearest_triangle: a bounding-volume
hierarchy in place of the grid), and deviation() uses the same call to say how far a mesh operator moved a surface: mean, rmse and
maximum from a mesh to its reference and back, and the Hausdorff distance.

evaluate(visible_from=...) restricts completeness and recall to the part of the ground truth the sensor could have observed, as
the published surface benchmarks do: an RGB-D run never sees the back of a cupboard or the room next door, and recall over the
whole scan is dominated by such surface.  The completeness query points are tested against the ground-truth mesh from the given
keyframe poses (DirectBA.MeshVisibility, bslam_mesh_visibility: inside a view's image and depth range, facing it, and not occluded),
and only those seen from at least min_views views count.

distance_summary is pure NumPy; evaluate and deviation need a DirectBA for the distance calls.
"""
import numpy as np

VISIBILITY_MARGIN = 0.02      # the default margin of DirectBA.MeshVisibility


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


def _has_triangles(mesh):
    triangles = mesh.get("triangles")
    return triangles is not None and len(triangles) > 0


def evaluate(ba, reconstruction, ground_truth, max_distance=0.1, thresholds=(0.01, 0.02, 0.05), cell_size=None, register=False, initial=None,
             sample_density=None, sample_seed=0, visible_from=None):
    """reconstruction, ground_truth: mesh dicts (positions (V, 3), triangles (T, 3); DirectBA.ExtractMesh, LoadPLY) in one frame; the
    ground truth may be a point cloud (no or empty triangles).  -> dict of accuracy and completeness (distance_summary each),
    f_scores (a list per threshold), max_distance and the grids the two calls used.  Both are measured at the vertices unless
    sample_density is given: see the module's docstring.
    max_distance None: no search radius.  Both directions run through DirectBA.NearestTriangle (a bounding-volume hierarchy, no grid):
    every point hits, `beyond` is 0, the result has max_distance None and, in place of the grids, accuracy_tree and completeness_tree
    (leaves, height).  cell_size is not used then.
    sample_density: each side that has triangles is replaced as a query point set by DirectBA.SampleMesh(side, density=sample_density,
    seed=sample_seed); the result then also has `sampling`: density, seed, reconstruction_samples and ground_truth_samples (the
    numbers of samples; None for a side without triangles, which keeps its vertices).
    register: the ground truth is in another frame.  The reconstruction's vertices are registered to it first
    (DirectBA.RegisterPoints at max_distance from `initial`, a 4 x 4 ground_truth_T_reconstruction, default identity), the motion found
    is applied to a copy of the reconstruction's positions (in float64, then rounded to float32), and that copy is evaluated.  The
    result then also has `registration`: target_T_source (4 x 4 as nested lists), iterations, converged, reason, history, and
    `before`, the accuracy and completeness summaries under `initial` alone.  The registration itself runs on the reconstruction's
    vertices; the sampling arguments apply to the evaluations before and after it.
    visible_from: a dict of `poses` (global_T_camera of the views, as for DirectBA.MeshVisibility, in the reconstruction's frame)
    and optionally camera, min_depth, max_depth, margin (DirectBA.MeshVisibility's arguments and defaults) and min_views (1).  The
    completeness query points -- vertices or samples of the ground truth, the samples with their normals -- are tested against the
    ground-truth mesh, and `completeness` and the recall in f_scores are taken over the points seen from at least min_views views.
    The result then also has completeness_all, the summary over all points, and `visibility`: views, points, visible_points,
    visible_fraction, margin, min_views.  A ground truth without triangles is a ValueError.  With register=True the poses are moved
    by the motion in force (`initial` for `before`, the one found for the result) before the test.  Accuracy is untouched."""
    sampled = {} if sample_density is None else dict(sample_density=sample_density, sample_seed=sample_seed)
    if visible_from is not None:
        if "poses" not in visible_from or set(visible_from) - {"poses", "camera", "min_depth", "max_depth", "margin", "min_views"}:
            raise ValueError("evaluate: visible_from needs poses and may hold camera, min_depth, max_depth, margin and min_views")
        if not _has_triangles(ground_truth):
            raise ValueError("evaluate: visible_from needs a ground truth with triangles (occlusion is tested against its mesh)")
    if register and max_distance is None:
        raise ValueError("evaluate: register=True needs a finite max_distance (the registration's search radius)")
    if register:
        start = np.eye(4) if initial is None else np.asarray(initial, np.float64).reshape(4, 4)
        moved_views = lambda T: {} if visible_from is None else dict(visible_from=dict(visible_from, poses=transform_poses(visible_from["poses"], T)))
        before = evaluate(ba, dict(reconstruction, positions=transform_positions(reconstruction["positions"], start)), ground_truth, max_distance, thresholds, cell_size,
                          **sampled, **moved_views(start))
        found = ba.RegisterPoints(reconstruction["positions"], ground_truth, max_distance, initial=start, cell_size=cell_size)
        moved = dict(reconstruction, positions=transform_positions(reconstruction["positions"], found["target_T_source"]))
        result = evaluate(ba, moved, ground_truth, max_distance, thresholds, cell_size, **sampled, **moved_views(found["target_T_source"]))
        result["registration"] = dict(target_T_source=np.asarray(found["target_T_source"], np.float64).tolist(), iterations=found["iterations"],
                                      converged=found["converged"], reason=found["reason"], history=found["history"],
                                      before=dict(accuracy=before["accuracy"], completeness=before["completeness"]))
        return result
    queries, counts, query_normals = [], [], None
    for side in (reconstruction, ground_truth):
        if sample_density is not None and _has_triangles(side):
            samples = ba.SampleMesh(side, density=sample_density, seed=sample_seed)
            queries.append(samples["positions"])
            counts.append(int(len(queries[-1])))
            query_normals = samples.get("normals")   # of the last side, the ground truth, when it was sampled
        else:
            queries.append(side["positions"])
            counts.append(None)
            query_normals = None
    visible = None
    if visible_from is not None:
        options = {k: visible_from[k] for k in ("camera", "min_depth", "max_depth", "margin") if k in visible_from}
        min_views = int(visible_from.get("min_views", 1))
        seen = ba.MeshVisibility(queries[1], ground_truth, visible_from["poses"], normals=query_normals, **options)
        visible = np.asarray(seen["count"]) >= min_views
        points = int(len(visible))
        visibility = dict(views=int(len(visible_from["poses"])), points=points, visible_points=int(visible.sum()),
                          visible_fraction=float(visible.sum() / points) if points else float("nan"), margin=float(visible_from.get("margin", VISIBILITY_MARGIN)),
                          min_views=min_views)
    if max_distance is None:   # no radius: the tree, and every point of a side hits whatever the other side holds
        acc = ba.NearestTriangle(queries[0], ground_truth)
        com = ba.NearestTriangle(queries[1], reconstruction)
        accuracy, completeness = distance_summary(acc["distance"], thresholds), _completeness(com["distance"], thresholds, visible)
        tree = lambda r: dict(leaves=r["leaves"], height=r["height"])
        result = dict(max_distance=None, accuracy=accuracy, completeness=completeness, f_scores=f_scores(accuracy, completeness),
                      accuracy_tree=tree(acc), completeness_tree=tree(com))
    else:
        acc = ba.PointMeshDistance(queries[0], ground_truth, max_distance, cell_size)
        com = ba.PointMeshDistance(queries[1], reconstruction, max_distance, cell_size)
        accuracy, completeness = distance_summary(acc["distance"], thresholds), _completeness(com["distance"], thresholds, visible)
        grid = lambda r: dict(cell_size=r["cell_size"], grid_cells=r["grid_cells"], grid_entries=r["grid_entries"])
        result = dict(max_distance=float(max_distance), accuracy=accuracy, completeness=completeness, f_scores=f_scores(accuracy, completeness),
                      accuracy_grid=grid(acc), completeness_grid=grid(com))
    if sample_density is not None:
        result["sampling"] = dict(density=float(sample_density), seed=int(sample_seed), reconstruction_samples=counts[0], ground_truth_samples=counts[1])
    if visible is not None:
        result["completeness_all"] = distance_summary(com["distance"], thresholds)
        result["visibility"] = visibility
    return result


def _completeness(distance, thresholds, visible):
    """The summary of the completeness distances: of all points, or of those flagged visible."""
    return distance_summary(distance if visible is None else np.asarray(distance).reshape(-1)[visible], thresholds)


def transform_poses(poses, T):
    """global_T_camera poses (abi.SE3f or 4 x 4) moved by T (4 x 4, new_T_global): 4 x 4 float64 matrices."""
    from .direct_ba import pose_matrix
    T = np.asarray(T, np.float64).reshape(4, 4)
    return [T @ pose_matrix(pose) for pose in poses]


def _deviation_side(distance):
    d = np.asarray(distance, np.float64).reshape(-1)
    d = d[np.isfinite(d)]
    nan = float("nan")
    return dict(count=int(len(d)), mean=float(d.mean()) if len(d) else nan, rmse=float(np.sqrt(np.mean(d * d))) if len(d) else nan,
                max=float(d.max()) if len(d) else nan)


def deviation(ba, mesh, reference, sample_density=None, sample_seed=0):
    """How far a mesh operator (SimplifyMesh, DecimateMesh, SmoothMesh, FillHoles ...) moved a surface: the distances from `mesh` to
    `reference` and back, without a search radius (DirectBA.NearestTriangle), so that the points that moved most count in full.
    Measured at the vertices, or -- sample_density given -- at DirectBA.SampleMesh samples of each side that has triangles.
    -> dict of mesh_to_reference and reference_to_mesh (count, mean, rmse, max each), hausdorff (the larger of the two maxima) and,
    with sample_density, sampling: density, seed, mesh_samples and reference_samples (None for a side without triangles).  A side without a point, or a target without a valid triangle, gives nan."""
    queries, counts = [], []
    for side in (mesh, reference):
        if sample_density is not None and _has_triangles(side):
            queries.append(ba.SampleMesh(side, density=sample_density, seed=sample_seed)["positions"])
            counts.append(int(len(queries[-1])))
        else:
            queries.append(side["positions"])
            counts.append(None)
    forth = _deviation_side(ba.NearestTriangle(queries[0], reference)["distance"])
    back = _deviation_side(ba.NearestTriangle(queries[1], mesh)["distance"])
    result = dict(mesh_to_reference=forth, reference_to_mesh=back, hausdorff=float(np.fmax(forth["max"], back["max"])))
    if sample_density is not None:
        result["sampling"] = dict(density=float(sample_density), seed=int(sample_seed), mesh_samples=counts[0], reference_samples=counts[1])
    return result


def transform_positions(positions, T):
    """T (4 x 4) applied to positions (n, 3) in float64, rounded to float32."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    return np.ascontiguousarray(np.asarray(positions, np.float64).reshape(-1, 3) @ T[:3, :3].T + T[:3, 3], np.float32)


def format_summary(name, s):
    within = ", ".join(f"<= {t:g}: {100 * w:.1f} %" for t, w in zip(s["thresholds"], s["within"]))
    return (f"{name}: {s['hits']} of {s['count']} points hit; mean {s['mean']:.4f}, median {s['median']:.4f}, rmse {s['rmse']:.4f}, p90 {s['p90']:.4f}, "
            f"p99 {s['p99']:.4f}; {within}; beyond {100 * s['beyond']:.1f} %")
