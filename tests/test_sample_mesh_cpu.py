"""Surface sampling without a GPU: the restatement of tests/sample_mesh_util.py against what the rule promises -- points inside
their triangles, an unbiased count, uniformity by area, determinism -- the plumbing of surface_eval.evaluate(sample_density=...)
against a stub, and the reason for the feature: the recall of a coarse wall against a strip that covers 60 % of it.

Measured with the restatement (sphere: point_mesh_util.sphere_mesh(), 3 544 triangles, float64 area 1 174.65 voxel^2; seed 0):

    density   samples   sum of x    bound (4 sigma)   triangles without a sample
      0.5        569      587.3         87.3                2 975
      3        3 509    3 524.0         98.5                  571
     40       46 975   46 986.0         97.1                    0

    wall at 1e4, seeds 1, 2, 3:   N = 10 000 each;  chi-square over 10 x 10 cells 89.5, 89.2, 105.5;  recall at 1 cm 0.6061, 0.6108, 0.6149
    (analytic 0.60954)."""
import numpy as np
import pytest

from tests import point_mesh_util as pm
from tests import sample_mesh_util as su

F = np.float32


@pytest.fixture(scope="module")
def sphere():
    return pm.sphere_mesh()


@pytest.fixture(scope="module")
def sphere40(sphere):
    return su.sample_mesh(*sphere, 40.0, 0)


def barycentric64(points, positions, triangles, which):
    """(w1, w2, distance to the plane) in float64 of each point in its triangle's frame."""
    tri = np.asarray(positions, np.float64)[np.asarray(triangles, np.int64)[which.astype(np.int64)]]
    a, u, v = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    w = np.asarray(points, np.float64) - a
    rows = lambda p, q: np.einsum("ij,ij->i", p, q)
    uu, uv, vv, wu, wv = rows(u, u), rows(u, v), rows(v, v), rows(w, u), rows(w, v)
    det = uu * vv - uv * uv
    w1, w2 = (vv * wu - uv * wv) / det, (uu * wv - uv * wu) / det
    n = np.cross(u, v)
    return w1, w2, np.abs(rows(w, n)) / np.linalg.norm(n, axis=1)


def test_the_fixtures():
    positions, triangles = pm.sphere_mesh()
    assert len(triangles) == 3544 and abs(su.areas64(positions, triangles).sum() - 1174.65) < 0.01
    positions, triangles = su.wall()
    assert su.areas64(positions, triangles).tolist() == [0.5, 0.5]
    positions, triangles = su.strip()
    assert positions.shape == (31 * 51, 3) and triangles.shape == (3000, 3) and abs(su.areas64(positions, triangles).sum() - 0.6) < 1e-6
    assert positions[:, 0].max() == F(0.6) and positions[:, 1].max() == F(1.0) and (positions[:, 2] == F(0.003)).all()
    assert abs(su.ANALYTIC_RECALL - 0.60954) < 1e-5


def test_the_hash_is_the_stated_one():
    assert int(su.mix(0)) == 0
    x = 1
    for shift, mul in ((16, 0x7feb352d), (15, 0x846ca68b)):
        x ^= x >> shift
        x = (x * mul) & 0xFFFFFFFF
    x ^= x >> 16
    assert int(su.mix(1)) == x
    py_mix = lambda v: int(su.mix(np.uint32(v)))
    seed, s, t, j = 0xDEADBEEF, 2, 77, 5
    want = py_mix((py_mix(((seed + s * 0x9e3779b9) & 0xFFFFFFFF) ^ py_mix(t)) + j) & 0xFFFFFFFF)
    assert int(su.h(seed, s, np.array([t], np.uint32), np.array([j], np.uint32))[0]) == want
    assert int(su.u24(np.uint32(0xFFFFFFFF))) == (1 << 24) - 1


def test_points_lie_in_their_triangles(sphere, sphere40):
    positions, triangles = sphere
    points, normals, which = sphere40
    w1, w2, off_plane = barycentric64(points, positions, triangles, which)
    print(f"barycentric range [{min(w1.min(), w2.min()):.3e}, {(w1 + w2).max():.9f}], off the plane by at most {off_plane.max():.3e}")
    for w in (w1, w2, 1.0 - w1 - w2):
        assert w.min() >= -1e-6 and w.max() <= 1 + 1e-6
    assert off_plane.max() <= 1e-5
    tri = positions[triangles[which.astype(np.int64)].astype(np.int64)].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert np.abs(normals - n / np.linalg.norm(n, axis=1, keepdims=True)).max() < 1e-5
    assert (np.diff(which.astype(np.int64)) >= 0).all()                   # ordered by triangle


@pytest.mark.parametrize("density", [0.5, 3.0, 40.0])
def test_the_count_is_unbiased(sphere, density):
    positions, triangles = sphere
    count = su.counts(positions, triangles, density, 0)
    x = su.expected_counts(positions, triangles, density).astype(np.float64)
    bound = su.count_bound(x)
    print(f"density {density}: {count.sum()} samples for {x.sum():.1f}, bound {bound:.1f}; {(count == 0).sum()} triangles without a sample")
    assert abs(x.sum() - su.areas64(positions, triangles).sum() * density) < 1e-3 * x.sum()
    assert bound < 120 and abs(count.sum() - x.sum()) <= bound
    assert ((count == np.floor(x)) | (count == np.floor(x) + 1)).all()
    if density == 0.5:
        assert (count == 0).sum() > 2900                                  # the runs of empty triangles the search has to survive


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_wall_is_covered_uniformly(seed):
    positions, triangles = su.wall()
    points, _, which = su.sample_mesh(positions, triangles, 1e4, seed)
    N = len(points)
    assert abs(N - 10000) <= 4
    assert points.min() >= 0 and points.max() <= 1 and (points[:, 2] == 0).all()
    cell = np.minimum((points[:, :2].astype(np.float64) * 10).astype(np.int64), 9)
    histogram = np.bincount(cell[:, 0] * 10 + cell[:, 1], minlength=100)
    chi = float(((histogram - N / 100) ** 2 / (N / 100)).sum())
    print(f"seed {seed}: N {N}, chi-square {chi:.1f}")
    assert chi <= 148                                                     # the 99.9th percentile of 99 degrees of freedom
    assert abs((which == 0).sum() - N / 2) <= 2


def clipped_area(polygon, centre, signs):
    """Area of a planar convex polygon (float64 [k, 3]) inside the octant sign * (x - centre) >= 0 on every axis: Sutherland-Hodgman."""
    for axis in range(3):
        d = signs[axis] * (polygon[:, axis] - centre[axis])
        out = []
        for k in range(len(polygon)):
            p, q, dp, dq = polygon[k], polygon[(k + 1) % len(polygon)], d[k], d[(k + 1) % len(polygon)]
            if dp >= 0:
                out.append(p)
            if (dp >= 0) != (dq >= 0):
                out.append(p + (q - p) * (dp / (dp - dq)))
        if len(out) < 3:
            return 0.0
        polygon = np.array(out)
    return 0.5 * np.linalg.norm(sum(np.cross(polygon[k] - polygon[0], polygon[k + 1] - polygon[0]) for k in range(1, len(polygon) - 1)))


def test_the_sphere_is_covered_in_proportion_to_area(sphere, sphere40):
    """Per octant about the centre: the samples in it against the float64 area in it, triangles that straddle an octant's faces
    clipped."""
    positions, triangles = sphere
    points = sphere40[0]
    centre = np.array(pm.SPHERE_CENTRE)
    tri = positions.astype(np.float64)[triangles.astype(np.int64)]
    area = np.zeros(8)
    for octant in range(8):
        signs = np.array([1.0 if octant >> axis & 1 else -1.0 for axis in range(3)])
        inside = (signs * (tri - centre) >= 0).all(axis=2)                # [T, 3 vertices]
        whole = inside.all(axis=1)
        partly = ~whole & ((signs * (tri - centre)).max(axis=1) >= 0).all(axis=1)      # its box reaches into the octant
        area[octant] = su.areas64(positions, triangles)[whole].sum() + sum(clipped_area(t, centre, signs) for t in tri[partly])
    assert abs(area.sum() - su.areas64(positions, triangles).sum()) < 1e-9
    octant_of = ((points.astype(np.float64) - centre >= 0) @ np.array([1, 2, 4])).astype(np.int64)
    ratio = np.bincount(octant_of, minlength=8) / (area * 40.0)
    print("samples / (area * density) per octant:", np.round(ratio, 4))
    assert np.abs(ratio - 1).max() <= 0.01


def test_seeds_duplicates_and_degenerate_triangles(sphere):
    positions, triangles = sphere
    first, second, other = su.sample_mesh(positions, triangles, 3.0, 5), su.sample_mesh(positions, triangles, 3.0, 5), su.sample_mesh(positions, triangles, 3.0, 6)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(first, second))
    assert len(other[0]) != len(first[0]) or not np.array_equal(other[0], first[0])
    wall_positions, wall_triangles = su.wall()
    twice = np.concatenate([wall_triangles[:1], wall_triangles[:1]])
    points, _, which = su.sample_mesh(wall_positions, twice, 400.0, 9)
    a, b = points[which == 0], points[which == 1]
    assert len(a) >= 199 and len(b) >= 199 and not np.array_equal(a[:199], b[:199])
    bad = np.concatenate([wall_positions, [[np.nan, 0.5, 0.5]]]).astype(F)
    for triangle in ([1, 1, 1], [1, 1, 2], [0, 1, 4], [4, 4, 4]):
        assert su.counts(bad, np.array([triangle]), 1e6, 0).tolist() == [0]
    assert len(su.sample_mesh(wall_positions, np.zeros((0, 3), np.uint32), 10.0, 0)[0]) == 0
    assert su.counts(wall_positions, wall_triangles, 1e10, 0).sum() > su.MAX_SAMPLES
    assert su.counts(wall_positions * F(1e30), wall_triangles, 1.0, 0).tolist() == [1 << 32, 1 << 32]          # nn overflows: not finite counts as 2^32


def test_the_reflection_boundary_stays_inside():
    rng = np.random.default_rng(8)
    a, b, c = (rng.uniform(-3, 3, (1000, 3)).astype(F) for _ in range(3))
    i1 = rng.integers(0, su.ONE, 1000)
    for total in (su.ONE - 1, su.ONE, su.ONE + 1):                        # below, on (not reflected: on the edge bc) and above the diagonal
        i2 = np.clip(total - i1, 0, su.ONE - 1)
        keep = i1 + i2 == total
        points = su.place(a[keep], (b - a)[keep], (c - a)[keep], i1[keep], i2[keep])
        positions = np.stack([a[keep], b[keep], c[keep]], 1).reshape(-1, 3)
        w1, w2, off_plane = barycentric64(points, positions, np.arange(len(positions)).reshape(-1, 3), np.arange(keep.sum()))
        for w in (w1, w2, 1.0 - w1 - w2):
            assert w.min() >= -1e-6 and w.max() <= 1 + 1e-6
        if total == su.ONE:
            assert np.abs(1.0 - w1 - w2).max() <= 1e-6
    corner = su.place(a[:1], (b - a)[:1], (c - a)[:1], [0], [0])
    assert np.array_equal(corner, a[:1])


# ------------------------------------------------------------------------------------------------
# why sampling matters: the wall against a strip that covers 60 % of it
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_recall_of_the_wall_against_the_strip(seed):
    positions, triangles = su.wall()
    points, _, _ = su.sample_mesh(positions, triangles, su.EVAL_DENSITY, seed)
    recall = float((su.wall_to_strip_distance(points) <= su.RECALL_THRESHOLD).mean())
    print(f"seed {seed}: recall at 1 cm {recall:.4f} for {su.ANALYTIC_RECALL:.5f}")
    assert abs(recall - su.ANALYTIC_RECALL) <= 0.02                       # four binomial sigma at N = 10^4
    assert float((su.wall_to_strip_distance(positions) <= su.RECALL_THRESHOLD).mean()) == 0.5


def test_the_seed_of_the_gpu_test_keeps_clear_of_the_thresholds():
    positions, triangles = su.wall()
    points, _, _ = su.sample_mesh(positions, triangles, su.EVAL_DENSITY, su.EVAL_SEED)
    distance = su.wall_to_strip_distance(points)
    for threshold in su.EVAL_THRESHOLDS:
        assert np.abs(distance - threshold).min() > 1e-6


# ------------------------------------------------------------------------------------------------
# surface_eval.evaluate(sample_density=...)
# ------------------------------------------------------------------------------------------------
class StubBA:
    """Distances: |x| of each point.  Samples: the vertices shifted by 100 times the density, three copies.  Registration: a fixed motion."""

    def __init__(self):
        self.calls = []

    def PointMeshDistance(self, points, mesh, max_distance, cell_size=None):
        self.calls.append(("distance", np.array(points), mesh, max_distance, cell_size))
        return dict(distance=np.abs(np.asarray(points, F)[:, 0]), triangle=np.zeros(len(points), np.uint32), cell_size=1.0, grid_cells=1, grid_entries=1)

    def SampleMesh(self, mesh, density=None, spacing=None, seed=0):
        assert spacing is None
        self.calls.append(("sample", mesh, density, seed))
        return dict(positions=np.tile(np.asarray(mesh["positions"], F) + F(100 * density), (3, 1)))

    def RegisterPoints(self, points, mesh, max_distance, initial=None, cell_size=None):
        self.calls.append(("register", np.array(points), mesh, max_distance, np.array(initial), cell_size))
        return dict(target_T_source=np.eye(4), iterations=1, converged=True, reason="converged", history=[])


def test_evaluate_sampling_plumbing():
    from badslam_amd import surface_eval
    reconstruction = dict(positions=np.array([[0.01, 1, 2], [0.03, -1, 0.5], [0.2, 0, 0]], F), triangles=np.array([[0, 1, 2]], np.uint32))
    truth = dict(positions=np.array([[0.02, 0, 0], [0.04, 1, 1], [0.3, 1, 0]], F), triangles=np.array([[0, 1, 2]], np.uint32))
    cloud = dict(positions=truth["positions"])
    samples = lambda mesh, density: np.tile(mesh["positions"] + F(100 * density), (3, 1))
    stub = StubBA()
    plain = surface_eval.evaluate(stub, reconstruction, truth, 0.1, (0.02, 0.05))
    assert [c[0] for c in stub.calls] == ["distance", "distance"]
    assert sorted(plain) == ["accuracy", "accuracy_grid", "completeness", "completeness_grid", "f_scores", "max_distance"]
    assert np.array_equal(stub.calls[0][1], reconstruction["positions"]) and np.array_equal(stub.calls[1][1], truth["positions"])
    # both sides have triangles: both are sampled, the targets stay the meshes
    stub = StubBA()
    r = surface_eval.evaluate(stub, reconstruction, truth, 0.1, (0.02, 0.05), cell_size=0.3, sample_density=0.5, sample_seed=7)
    assert [c[0] for c in stub.calls] == ["sample", "sample", "distance", "distance"]
    assert stub.calls[0][1] is reconstruction and stub.calls[1][1] is truth and [c[2:] for c in stub.calls[:2]] == [(0.5, 7), (0.5, 7)]
    assert np.array_equal(stub.calls[2][1], samples(reconstruction, 0.5)) and stub.calls[2][2] is truth and stub.calls[2][3:] == (0.1, 0.3)
    assert np.array_equal(stub.calls[3][1], samples(truth, 0.5)) and stub.calls[3][2] is reconstruction
    assert r["sampling"] == dict(density=0.5, seed=7, reconstruction_samples=9, ground_truth_samples=9)
    assert {k: v for k, v in r.items() if k != "sampling"}.keys() == plain.keys()
    assert r["accuracy"] == surface_eval.distance_summary(np.abs(samples(reconstruction, 0.5)[:, 0]), (0.02, 0.05)) and r["accuracy"]["count"] == 9
    # a side without triangles keeps its vertices
    for other in (cloud, dict(cloud, triangles=np.zeros((0, 3), np.uint32))):
        stub = StubBA()
        r = surface_eval.evaluate(stub, reconstruction, other, 0.1, (0.02,), sample_density=2.0)
        assert [c[0] for c in stub.calls] == ["sample", "distance", "distance"] and stub.calls[0][1] is reconstruction and stub.calls[0][3] == 0
        assert np.array_equal(stub.calls[1][1], samples(reconstruction, 2.0)) and np.array_equal(stub.calls[2][1], other["positions"])
        assert r["sampling"] == dict(density=2.0, seed=0, reconstruction_samples=9, ground_truth_samples=None)
    # register: on the vertices; the evaluations before and after it are sampled
    stub = StubBA()
    r = surface_eval.evaluate(stub, reconstruction, truth, 0.1, (0.02,), register=True, sample_density=0.5, sample_seed=3)
    assert [c[0] for c in stub.calls] == ["sample", "sample", "distance", "distance", "register", "sample", "sample", "distance", "distance"]
    assert np.array_equal(stub.calls[4][1], reconstruction["positions"]) and all(c[2:] == (0.5, 3) for c in stub.calls if c[0] == "sample")
    assert r["sampling"]["seed"] == 3 and "registration" in r
    stub = StubBA()
    r = surface_eval.evaluate(stub, reconstruction, truth, 0.1, (0.02,), register=True)
    assert [c[0] for c in stub.calls] == ["distance", "distance", "register", "distance", "distance"] and "sampling" not in r


def test_python_entry_points_exist():
    import inspect

    from badslam_amd import abi, direct_ba
    assert "bslam_sample_mesh" in abi.SIGNATURES and len(abi.SIGNATURES["bslam_sample_mesh"][1]) == 13
    assert list(inspect.signature(direct_ba.DirectBA.SampleMesh).parameters) == ["self", "mesh", "density", "spacing", "seed"]
    for arguments in (dict(), dict(density=1.0, spacing=1.0)):
        with pytest.raises(ValueError):
            direct_ba.DirectBA.SampleMesh(None, dict(positions=np.zeros((0, 3), F)), **arguments)
    from tools import run_tum
    assert "surface_sample_spacing" in inspect.signature(run_tum.run).parameters
    assert run_tum.arg_parser().parse_args(["somewhere", "--surface-sample-spacing", "0.005"]).surface_sample_spacing == 0.005
