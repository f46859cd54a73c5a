"""The point-to-mesh distance rule (include/badslam_hip.h "Surface evaluation") as tests/point_mesh_util.py restates it, against
an independent float64 closest-point-on-triangle (Ericson's region form) on the same fp32 inputs.  No GPU.

Measured with this restatement on the sphere (1 774 vertices, 3 544 triangles, voxel units), 680 points, R = 2:
  481 hits;  max |distance - float64| 2.37e-7 voxels (median 2.18e-8);  2.16e-7 with everything shifted by (1e4, -1e4, 1e4);
  every miss has a float64 distance above 2.006;  the 80 constructed points lie at a distance <= 1.36e-6 (the square root of a
  squared distance that is rounding error alone);  51 of them tie, with a multiplicity of up to 9 at vertices.
The bounds asserted are twice the measured maxima: the run is deterministic, the factor only covers another NumPy."""
import numpy as np
import pytest

from tests import point_mesh_util as pm

F = np.float32
R = 2.0
MEASURED_HITS = 481
MEASURED_MAX = 2.37e-7
MEASURED_MAX_SHIFTED = 2.16e-7
MEASURED_CONSTRUCTED = 1.36e-6
SHIFT = np.array([1e4, -1e4, 1e4], F)


@pytest.fixture(scope="module")
def sphere():
    """Mesh, points, the restatement's answer and the float64 distance matrix: computed once, never changed."""
    positions, triangles = pm.sphere_mesh()
    points = pm.sphere_points(positions, triangles)
    distance, triangle = pm.point_mesh_distance(points, positions, triangles, R)
    return positions, triangles, points, distance, triangle, pm.distances64(points, positions, triangles)


def test_sphere_and_points(sphere):
    positions, triangles, points, _, _, _ = sphere
    assert positions.shape == (1774, 3) and triangles.shape == (3544, 3) and points.shape == (680, 3)


def test_no_decision_depends_on_rounding(sphere):
    """A condition on the inputs: no point's float64 distance lies within 1e-3 relative of R."""
    d64 = sphere[5].min(axis=1)
    gap = np.abs(d64 - R).min() / R
    print(f"nearest float64 distance to R: {gap:.2e} relative")
    assert gap > 1e-3


def test_restatement_against_float64(sphere):
    positions, triangles, points, distance, triangle, all64 = sphere
    d64 = all64.min(axis=1)
    hit = np.isfinite(distance)
    assert np.array_equal(hit, d64 <= R) and (triangle[~hit] == pm.NO_TRIANGLE).all() and (triangle[hit] < len(triangles)).all()
    err = np.abs(distance[hit].astype(np.float64) - d64[hit])
    print(f"{int(hit.sum())} hits, max |difference| {err.max():.2e} voxels, median {np.median(err):.2e}; smallest miss {d64[~hit].min():.4f}")
    assert int(hit.sum()) == MEASURED_HITS
    assert err.max() <= 2 * MEASURED_MAX
    assert d64[~hit].min() > R * (1 + 1e-3)
    # the triangle named attains the float64 minimum, up to the same bound
    assert (np.abs(all64[np.arange(len(points)), np.where(hit, triangle, 0)][hit] - d64[hit]) <= 2 * MEASURED_MAX).all()
    constructed = distance[600:]
    print(f"the 80 constructed points: distance <= {constructed.max():.2e}")
    assert constructed.max() <= 2 * MEASURED_CONSTRUCTED


def test_shifted_by_1e4(sphere):
    """Everything 1e4 away from the origin, where the coordinates carry an ulp of 9.8e-4: the float64 reference sees the same rounded
    coordinates, so the difference stays that of the unshifted case."""
    positions, triangles, points, _, _, _ = sphere
    sp, sq = (positions + SHIFT).astype(F), (points + SHIFT).astype(F)
    distance, triangle = pm.point_mesh_distance(sq, sp, triangles, R)
    d64 = pm.distances64(sq, sp, triangles).min(axis=1)
    hit = np.isfinite(distance)
    assert np.array_equal(hit, d64 <= R)
    err = np.abs(distance[hit].astype(np.float64) - d64[hit])
    print(f"shifted: {int(hit.sum())} hits of {len(hit)}, max |difference| {err.max():.2e}")
    assert err.max() <= 2 * MEASURED_MAX_SHIFTED


def test_lowest_index_among_ties(sphere):
    """A condition on the inputs: at least 30 of the 80 constructed points (vertices, edge midpoints) are equally near to two or
    more triangles, so the lowest-index rule is exercised."""
    positions, triangles, points, distance, triangle, _ = sphere
    ties = 0
    most = 0
    for i in range(600, 680):
        p = np.broadcast_to(points[i], (len(triangles), 3))
        tri = positions[triangles.astype(np.int64)]
        d2 = pm.pair_d2(p, tri[:, 0], tri[:, 1], tri[:, 2])
        attain = np.flatnonzero(d2 == d2.min())
        assert triangle[i] == attain[0]
        ties += len(attain) >= 2
        most = max(most, len(attain))
    print(f"{ties} of 80 constructed points tie, multiplicity up to {most}")
    assert ties >= 30


def test_point_cloud_form():
    rng = np.random.default_rng(3)
    cloud = rng.uniform(-1, 1, (300, 3)).astype(F)
    points = rng.uniform(-1.2, 1.2, (200, 3)).astype(F)
    tri = np.repeat(np.arange(300, dtype=np.uint32)[:, None], 3, axis=1)
    distance, nearest = pm.point_mesh_distance(points, cloud, tri, 0.25)
    d = np.linalg.norm(points[:, None].astype(np.float64) - cloud[None].astype(np.float64), axis=2)
    hit = np.isfinite(distance)
    assert np.array_equal(hit, d.min(axis=1) <= 0.25) and 20 < hit.sum() < 200
    assert np.array_equal(nearest[hit], d.argmin(axis=1)[hit])
    assert np.abs(distance[hit] - d.min(axis=1)[hit]).max() <= 1e-6


def test_segment_form():
    positions = np.array([[0, 0, 0], [2, 0, 0]], F)
    tri = np.array([[0, 0, 1]], np.uint32)
    points = np.array([[1, 1, 0], [-1, 0, 0], [3, 0.5, 0], [0.5, 0, 0]], F)
    distance, which = pm.point_mesh_distance(points, positions, tri, 5.0)
    assert np.array_equal(distance, np.array([1.0, 1.0, np.sqrt(F(1.25)), 0.0], F)) and (which == 0).all()


def test_nan_vertex_nan_point_infinite_point_and_no_triangle():
    positions = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0]], F)
    tri = np.array([[0, 1, 3], [0, 1, 2]], np.uint32)
    points = np.array([[0.2, 0.2, 0.5], [np.nan, 0.2, 0.5], [np.inf, 0.2, 0.5], [0.2, -np.inf, 0.0]], F)
    distance, which = pm.point_mesh_distance(points, positions, tri, 1.0)
    assert distance[0] == F(0.5) and which[0] == 1                    # the triangle with the NaN vertex is nobody's candidate
    assert np.isinf(distance[1:]).all() and (which[1:] == pm.NO_TRIANGLE).all()
    distance, which = pm.point_mesh_distance(points, positions, np.zeros((0, 3), np.uint32), 1.0)
    assert np.isinf(distance).all() and (which == pm.NO_TRIANGLE).all()
    assert pm.grid_census(positions, tri, 1.0, 1.0) == (4 * 4 * 3, 48)
