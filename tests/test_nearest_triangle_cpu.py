"""The nearest-triangle rule on the CPU (tests/nearest_triangle_util.py): what the GPU comparison rests on.  The restatement equals the
grid's rule where no clamp is active at a minimum, differs from it in last bits only where one is, stays as close to float64 as the
unclamped rule, and surface_eval.deviation reports what it should on meshes with a known answer."""
import numpy as np
import pytest

from badslam_amd import surface_eval
from tests import nearest_triangle_util as nt
from tests import point_mesh_util as pm

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def sphere():
    positions, triangles = pm.sphere_mesh()
    points = pm.sphere_points(positions, triangles)
    return positions, triangles, points, nt.nearest_triangle(points, positions, triangles)


@pytest.fixture(scope="module")
def plane():
    positions, triangles = nt.plane_mesh()
    points = nt.plane_points()
    return positions, triangles, points, nt.nearest_triangle(points, positions, triangles)


@pytest.mark.parametrize("R, hits", [(1.0, 265), (3.0, 678), (np.inf, 680)])
def test_sphere_equals_the_grid_rule_bit_for_bit(sphere, R, hits):
    positions, triangles, points, unbounded = sphere
    want_d, want_t = pm.point_mesh_distance(points, positions, triangles, R)
    got_d, got_t = unbounded if R == np.inf else nt.nearest_triangle(points, positions, triangles, R)
    assert int(np.isfinite(want_d).sum()) == hits
    assert np.array_equal(bits(got_d), bits(want_d)) and np.array_equal(got_t, want_t)


def test_sphere_radius_only_turns_hits_into_misses(sphere):
    positions, triangles, points, (d, t) = sphere
    got_d, got_t = nt.nearest_triangle(points, positions, triangles, 1.0)
    hit = d <= F(1.0)
    assert np.array_equal(bits(got_d[hit]), bits(d[hit])) and np.array_equal(got_t[hit], t[hit])
    assert np.isinf(got_d[~hit]).all() and (got_t[~hit] == nt.NO_TRIANGLE).all()


def test_plane_clamp_changes_last_bits_and_no_index(plane):
    positions, triangles, points, (d, t) = plane
    want_d, want_t = pm.point_mesh_distance(points, positions, triangles, np.inf)
    differ = bits(d) != bits(want_d)
    assert 0 < differ.sum() <= 20, "the clamp is meant to be active on this fixture, at a few points"
    assert (np.abs(bits(d).astype(np.int64) - bits(want_d).astype(np.int64)) <= 2).all()
    assert (d >= want_d).all(), "the clamp only raises"
    assert np.array_equal(t, want_t)


def test_sphere_against_float64(sphere):
    positions, triangles, points, (d, t) = sphere
    d64 = pm.distances64(points, positions, triangles)
    assert np.isfinite(d).all()
    assert np.abs(d - d64.min(axis=1)).max() < 1e-6                            # the bound of test_point_mesh_cpu.py
    assert np.abs(d64[np.arange(len(points)), t] - d64.min(axis=1)).max() < 1e-6   # the triangle named is a nearest one


def test_plane_against_float64(plane):
    positions, triangles, points, (d, t) = plane
    d64 = pm.distances64(points, positions, triangles).min(axis=1)
    relative = np.abs(d - d64) / d64
    print("plane: largest relative error against float64", relative.max())
    # measured 8.2e-8 on these inputs (the unclamped rule: 9.2e-8); a factor 2 over that.  Each value is a few fp32 roundings
    # (2^-24 = 6e-8 each) of well-conditioned sums, so the figure is of the size one expects.
    assert relative.max() < 1.7e-7


def test_misses():
    positions, triangles = nt.plane_mesh(3)
    points = np.array([[0.1, 0.1, 5], [np.nan, 0, 0], [0, np.inf, 0], [1e6, 0, 0]], F)
    d, t = nt.nearest_triangle(points, positions, triangles)
    assert np.isfinite(d[[0, 3]]).all() and np.isinf(d[[1, 2]]).all() and (t[[1, 2]] == nt.NO_TRIANGLE).all()
    bad = positions.copy()
    bad[:, 0] = np.nan
    d, t = nt.nearest_triangle(points, bad, triangles)
    assert np.isinf(d).all() and (t == nt.NO_TRIANGLE).all()


def test_check_tree_accepts_a_hand_made_tree_and_refuses_a_small_box():
    positions = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [6, 5, 5], [5, 6, 5], [np.nan, 0, 0]], F)
    triangles = np.array([[0, 1, 2], [3, 4, 5], [0, 1, 6]], np.uint32)
    tree = dict(leaves=2, parent=[nt.NO_NODE, 0, 0], children=[2, 1], leaf_triangle=[1, 0],
                boxes=np.array([[0, 0, 0, 6, 6, 5], [5, 5, 5, 6, 6, 5], [0, 0, 0, 1, 1, 0]], F))
    assert nt.check_tree(tree, positions, triangles) == 1
    tree["boxes"][0, 3] = 5.5
    with pytest.raises(AssertionError):
        nt.check_tree(tree, positions, triangles)


def test_deviation_of_a_shifted_square():
    square = dict(positions=np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F), triangles=np.array([[0, 1, 2], [0, 2, 3]], np.uint32))
    shifted = dict(square, positions=square["positions"] + np.array([0, 0, 0.25], F))
    got = surface_eval.deviation(nt.RestatementBA(), shifted, square)
    for side in ("mesh_to_reference", "reference_to_mesh"):
        assert got[side] == dict(count=4, mean=0.25, rmse=0.25, max=0.25)
    assert got["hausdorff"] == 0.25
    # one corner pulled away: the maximum and the Hausdorff distance follow it, one direction more than the other
    pulled = dict(square, positions=square["positions"].copy())
    pulled["positions"][2] = [1, 1, 0.5]
    got = surface_eval.deviation(nt.RestatementBA(), pulled, square)
    assert got["mesh_to_reference"]["max"] == 0.5 and got["hausdorff"] == 0.5
    assert got["mesh_to_reference"]["mean"] == 0.125
    assert 0 < got["reference_to_mesh"]["max"] < 0.5


def test_run_tum_plumbing(monkeypatch, tmp_path):
    """tools/run_tum.py --surface-max-distance inf and --mesh-deviation, with everything that needs a GPU stubbed."""
    import inspect
    import json

    from tools import run_tum
    assert "mesh_deviation" in inspect.signature(run_tum.run).parameters
    parsed = run_tum.arg_parser().parse_args(["somewhere", "--surface-max-distance", "inf", "--mesh-deviation"])
    assert parsed.surface_max_distance == np.inf and parsed.mesh_deviation and not run_tum.arg_parser().parse_args(["somewhere"]).mesh_deviation
    square = dict(positions=np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F), normals=np.tile(np.array([0, 0, 1], F), (4, 1)),
                  colors=np.zeros((4, 4), np.uint8), triangles=np.array([[0, 1, 2], [0, 2, 3]], np.uint32))

    class StubBA(nt.RestatementBA):
        def keyframe_count(self):
            return 0

        def surfels_size(self):
            return 0

        def SmoothMesh(self, mesh, **kwargs):
            return dict(mesh, positions=mesh["positions"] + np.array([0, 0, 0.25], F))

    class StubSlam:
        def __init__(self, *args, **kwargs):
            self._ba = StubBA()

        def ba(self):
            return self._ba

        def frame_poses(self):
            return []

    monkeypatch.setattr(run_tum.dba, "read_tum_dataset", lambda d, t: dict(frames=[], width=64, height=48, camera=(50.0, 50.0, 32.0, 24.0)))
    monkeypatch.setattr(run_tum.dba, "save_poses", lambda *a: None)
    monkeypatch.setattr(run_tum.dba, "SaveMeshAsPLY", lambda path, mesh: None)
    monkeypatch.setattr(run_tum.dba, "LoadPLY", lambda path: dict(positions=square["positions"] + np.array([0, 0, 3], F), triangles=square["triangles"]))
    monkeypatch.setattr(run_tum.bad_slam, "BadSlam", StubSlam)
    monkeypatch.setattr(run_tum, "fuse_and_mesh", lambda ba, path, *args: (square, (0.0, 0.0, 0.0), (1, 1, 1), None))
    report = tmp_path / "surface.json"
    r = run_tum.run(tmp_path, out=str(tmp_path / "poses.txt"), mesh_smooth_iterations=2, mesh_deviation=True, ground_truth_surface="truth.ply",
                    surface_max_distance=np.inf, surface_report=str(report))
    sf = r["surface"]
    assert sf["max_distance"] is None and sf["accuracy"]["beyond"] == 0 and sf["accuracy"]["mean"] == 2.75 and "accuracy_grid" not in sf
    assert sf["mesh_deviation"]["operators"] == ["smooth"] and sf["mesh_deviation"]["hausdorff"] == 0.25
    assert sf["mesh_deviation"]["mesh_to_reference"] == dict(count=4, mean=0.25, rmse=0.25, max=0.25)
    assert json.loads(report.read_text())["mesh_deviation"]["hausdorff"] == 0.25
    with pytest.raises(ValueError, match="finite"):
        run_tum.run(tmp_path, out=str(tmp_path / "poses.txt"), ground_truth_surface="truth.ply", surface_max_distance=np.inf, register_surface=True)
    with pytest.raises(ValueError):
        run_tum.run(tmp_path, out=str(tmp_path / "poses.txt"), ground_truth_surface="truth.ply", surface_max_distance=0.0)


def test_evaluate_without_a_radius_uses_the_tree():
    square = dict(positions=np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F), triangles=np.array([[0, 1, 2], [0, 2, 3]], np.uint32))
    far = dict(square, positions=square["positions"] + np.array([0, 0, 7], F))
    got = surface_eval.evaluate(nt.RestatementBA(), far, square, max_distance=None)
    assert got["max_distance"] is None and "accuracy_grid" not in got and "completeness_grid" not in got
    assert got["accuracy"]["beyond"] == 0 and got["completeness"]["beyond"] == 0 and got["accuracy"]["mean"] == 7.0
    assert got["accuracy_tree"]["leaves"] == 2
