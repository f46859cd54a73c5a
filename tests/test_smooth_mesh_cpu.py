"""The restatement of the smoothing rule (tests/smooth_mesh_util.py) on meshes whose answer is known by their shape -- a flat plane
does not move, a noisy plane gets flatter, a noisy sphere gets rounder and keeps its radius under Taubin's filter and shrinks under
Laplace's -- and the plumbing of tools/run_tum.py --mesh-smooth-* with everything that needs a GPU stubbed.  Properties, not recorded
bits; the GPU tests compare bslam_smooth_mesh with the restatement bit for bit.

Measured with this restatement on the 48 x 24 sphere with radial noise of sigma 0.02, 10 iterations of 0.5 | -0.53: the standard
deviation of the radii 0.019694 before, 0.007887 after (Laplace: 0.010512); the mean radius 0.999209 before, 1.001676 after
(Laplace: 0.957842); on the clean sphere the mean moves to 1.002304.  The largest angle between the geometric normal of the clean
sphere and the radial direction is 1.268 degrees."""
import inspect
import json
import pathlib

import numpy as np
import pytest

from tests import smooth_mesh_util as sm

F = np.float32
# twice the measured Taubin figures, the margin of the decimation tests: still far below 0.0197 (no smoothing) and 0.042 (Laplace)
SPHERE_STD_BOUND = 2 * 0.007887
SPHERE_MEAN_BOUND = 2 * 0.001676
# the measured 1.268 degrees, rounded up to the next hundredth.  (A facet of the 48 x 24 sphere spans 7.5 degrees, so 3.75 would hold
# for any weighting of a fan; the measured figure is what tells the area weighting from a uniform one or from a dropped fan member.)
SPHERE_NORMAL_DEGREES = 1.27


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def box(positions):
    return positions.min(axis=0), positions.max(axis=0)


# ------------------------------------------------------------------------------------------------
# 1. the rule
# ------------------------------------------------------------------------------------------------
def test_a_flat_plane_does_not_move():
    positions, triangles = sm.plane(17)
    out, normals = sm.smooth(positions, None, triangles, iterations=3, mode=0)
    assert np.array_equal(bits(out), bits(positions)), "the stencil is symmetric and the sums are exact"
    assert np.array_equal(normals, np.tile(F([0, 0, 1]), (289, 1))), "counter-clockwise seen from +z"
    out, normals = sm.smooth(positions, None, triangles[:, ::-1], iterations=3, mode=0)
    assert np.array_equal(bits(out), bits(positions)) and np.array_equal(normals, np.tile(F([0, 0, -1]), (289, 1)))


@pytest.fixture(scope="module")
def smoothed_planes():
    positions, triangles = sm.noisy_plane(17)
    return positions, {mode: sm.smooth(positions, None, triangles, iterations=10, mode=mode)[0] for mode in (0, 1, 2)}


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_a_noisy_plane_gets_flatter(smoothed_planes, mode):
    positions, out = smoothed_planes
    before, after = positions[:, 2].astype(np.float64).std(), out[mode][:, 2].astype(np.float64).std()
    print(f"mode {mode}: standard deviation of z {before:.6f} -> {after:.6f}")
    assert after < before


def test_the_boundary_modes_on_the_noisy_plane(smoothed_planes):
    positions, out = smoothed_planes
    rim = sm.rim_of(17)
    assert np.array_equal(bits(out[0][rim]), bits(positions[rim])), "fixed leaves every rim vertex bit for bit"
    assert (bits(out[1][rim]) != bits(positions[rim])).any(axis=1).all() and (bits(out[2][rim]) != bits(positions[rim])).any(axis=1).all()
    (lo, hi), (lo0, hi0), (lo2, hi2) = box(positions), box(out[0]), box(out[2])
    assert np.array_equal(lo0[:2], lo[:2]) and np.array_equal(hi0[:2], hi[:2]), "fixed keeps the box"
    assert (lo2[:2] > lo[:2]).all() and (hi2[:2] < hi[:2]).all(), "free shrinks it"
    # rim moves a boundary vertex by its two rim neighbours only: in one step a straight side stays on its line, but for the corners
    side = rim[positions[rim, 0] == F(0.25)][1:-1]
    step = sm.smooth(positions, None, sm.noisy_plane(17)[1], 1, 0.5, 0.0, 1)[0]
    assert np.array_equal(bits(step[side, 0]), bits(positions[side, 0])) and (bits(step[side, 2]) != bits(positions[side, 2])).all()


@pytest.fixture(scope="module")
def spheres():
    noisy, clean, normals, triangles, centre = sm.noisy_sphere()
    assert len(noisy) == 1106
    return dict(noisy=noisy, clean=clean, normals=normals, triangles=triangles, centre=centre,
                taubin=sm.smooth(noisy, None, triangles, iterations=10)[0], laplace=sm.smooth(noisy, None, triangles, iterations=10, mu=0.0)[0],
                clean_taubin=sm.smooth(clean, None, triangles, iterations=10)[0])


def test_taubin_makes_the_sphere_rounder_and_keeps_its_radius(spheres):
    r = {k: sm.radii(spheres[k], spheres["centre"]) for k in ("noisy", "taubin", "laplace", "clean_taubin")}
    for k, v in r.items():
        print(f"{k}: radius mean {v.mean():.6f}, standard deviation {v.std():.6f}")
    assert r["noisy"].std() > 0.019
    assert r["taubin"].std() <= SPHERE_STD_BOUND
    assert abs(r["taubin"].mean() - 1.0) <= SPHERE_MEAN_BOUND
    assert abs(r["clean_taubin"].mean() - 1.0) <= SPHERE_MEAN_BOUND
    assert r["laplace"].mean() < 1.0 - SPHERE_MEAN_BOUND, "mu = 0 shrinks"
    assert r["laplace"].std() < r["noisy"].std()


def test_no_iterations_and_the_normals_of_the_clean_sphere(spheres):
    clean, triangles, centre = spheres["clean"], spheres["triangles"], spheres["centre"]
    out, normals = sm.smooth(clean, None, triangles, iterations=0)
    assert np.array_equal(bits(out), bits(clean))
    out, _ = sm.smooth(spheres["noisy"], None, triangles, iterations=0, mode=2, want_normals=False)
    assert np.array_equal(bits(out), bits(spheres["noisy"])) and _ is None
    radial = clean.astype(np.float64) - centre
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    angle = np.degrees(np.arccos(np.clip((normals.astype(np.float64) * radial).sum(axis=1), -1.0, 1.0)))
    print(f"largest angle to the radial direction {angle.max():.4f} degrees")
    assert angle.max() <= SPHERE_NORMAL_DEGREES
    assert np.abs(np.linalg.norm(normals.astype(np.float64), axis=1) - 1.0).max() < 1e-6


def test_small_meshes():
    positions, triangles = sm.tetrahedron()
    live, uses, boundary = sm.topology(4, triangles)
    assert not boundary and set(uses.values()) == {2}
    for mode in (0, 1, 2):
        out, _ = sm.smooth(positions, None, triangles, iterations=1, mode=mode)
        assert (bits(out) != bits(positions)).any(axis=1).all(), "no boundary: every vertex moves"
    # a single triangle: all boundary
    positions, triangles = np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, 0.25]], F), np.array([[0, 1, 2]], np.uint32)
    assert sm.topology(3, triangles)[2] == {0, 1, 2}
    assert np.array_equal(bits(sm.smooth(positions, None, triangles, 3, mode=0)[0]), bits(positions))
    assert (bits(sm.smooth(positions, None, triangles, 3, mode=1)[0]) != bits(positions)).any()
    assert np.array_equal(bits(sm.smooth(positions, None, triangles, 1, 1.0, 0.0, 2)[0][0]), bits((positions[1].astype(np.float64) + positions[2]) / 2))


def test_three_wings():
    positions, triangles = sm.three_wings()
    live, uses, boundary = sm.topology(len(positions), triangles)
    assert len(live) == 6, "the triangles that repeat an index are ignored"
    assert uses[(0, 1)] == 3 and uses[(1, 0)] == 3, "the shared edge is interior"
    assert boundary == {0, 1, 2, 3, 4, 5, 6, 7} and uses[(0, 2)] == 1 and (2, 5) not in uses and (6, 6) not in uses
    assert sm.stencils(len(positions), triangles, 1)[0] == [2, 3, 4], "rim: without vertex 1, across the interior edge"
    assert sm.stencils(len(positions), triangles, 2)[0] == [1, 2, 3, 4] and sm.stencils(len(positions), triangles, 0)[0] == []
    assert sm.stencils(len(positions), triangles, 2)[8] == [] and sm.stencils(len(positions), triangles, 2)[9] == []
    normals = np.tile(F([0, 1, 0]), (len(positions), 1))
    for mode in (0, 1, 2):
        out, n = sm.smooth(positions, normals, triangles, 3, mode=mode)
        assert np.array_equal(bits(out[[8, 9]]), bits(positions[[8, 9]])), "isolated vertices stay"
        assert np.array_equal(n[[8, 9]], normals[[8, 9]]), "... and keep the input normal"
        same = sm.smooth(positions, normals, triangles[[0, 1, 2, 4, 5, 6]], 3, mode=mode)
        assert np.array_equal(bits(out), bits(same[0])) and np.array_equal(bits(n), bits(same[1])), "an ignored triangle changes nothing"


def test_a_fan_that_sums_to_no_area_takes_the_input_normal_or_zero():
    positions, triangles = sm.zero_fan()
    given = np.tile(F([0.6, 0, 0.8]), (len(positions), 1))
    _, n = sm.smooth(positions, given, triangles, 0)
    assert np.array_equal(n[[0, 5]], given[[0, 5]]) and np.array_equal(n[1], F([0, 0, 1])) and np.array_equal(n[3], F([0, 0, -1]))
    _, n = sm.smooth(positions, None, triangles, 0)
    assert not n[[0, 5]].any() and np.array_equal(n[1], F([0, 0, 1]))


def test_a_fan_of_valence_70():
    positions, triangles = sm.fan(70)
    S = sm.stencils(71, triangles, 0)
    assert S[0] == list(range(1, 71)) and S[1] == [], "the centre has 70 neighbours; the rim is boundary"
    out, n = sm.smooth(positions, None, triangles, 1, 1.0, 0.0, 0)
    assert np.allclose(out[0], positions[1:].astype(np.float64).mean(axis=0), atol=1e-7) and np.array_equal(bits(out[1:]), bits(positions[1:]))
    assert n[0, 2] > 0.9


@pytest.mark.parametrize("options", [dict(lambda_=0.0), dict(lambda_=-0.5), dict(lambda_=1.5), dict(lambda_=np.inf), dict(lambda_=np.nan), dict(mu=0.1), dict(mu=-1.5),
                                     dict(mu=-np.inf), dict(mu=np.nan), dict(mode=3), dict(iterations=65536)])
def test_refused_parameters(options):
    positions, triangles = sm.tetrahedron()
    with pytest.raises(sm.Refused):
        sm.smooth(positions, None, triangles, **options)


def test_refused_meshes_and_the_ends_of_the_ranges():
    positions, triangles = sm.tetrahedron()
    sm.smooth(positions, None, triangles, 1, 1.0, -1.0, 2)
    sm.smooth(positions, None, triangles, 65535 * 0, 1e-6, -0.0, 0)
    bad = triangles.copy()
    bad[1, 2] = 4
    with pytest.raises(sm.Refused, match="beyond"):
        sm.smooth(positions, None, bad, 1)
    for value in (np.nan, np.inf):
        broken = positions.copy()
        broken[2, 0] = value
        with pytest.raises(sm.Refused, match="not finite"):
            sm.smooth(broken, None, None, 0)
    out, n = sm.smooth(positions, None, None, 5)
    assert np.array_equal(bits(out), bits(positions)) and not n.any(), "a point cloud: positions copied, normals zero"
    out, n = sm.smooth(np.zeros((0, 3), F), None, None, 5)
    assert out.shape == (0, 3) and n.shape == (0, 3)


def test_the_abi_declares_the_calls():
    from badslam_amd import abi
    assert len(abi.SIGNATURES["bslam_smooth_mesh"][1]) == 13 and len(abi.SIGNATURES["bslam_smooth_stage_times"][1]) == 2
    header = (pathlib.Path(__file__).resolve().parents[1] / "include" / "badslam_hip.h").read_text()
    assert "int bslam_smooth_mesh(bslam_context* ctx, void* stream, uint32_t vertex_count, uint32_t triangle_count" in header
    assert "int bslam_smooth_stage_times(bslam_context* ctx, float* stage_ms5);" in header and "Mesh smoothing" in header


# ------------------------------------------------------------------------------------------------
# 2. tools/run_tum.py --mesh-smooth-*, with everything that needs a GPU stubbed
# ------------------------------------------------------------------------------------------------
def test_run_tum_plumbing(monkeypatch, tmp_path):
    from tests import decimate_mesh_util as du
    from tools import run_tum
    parameters = inspect.signature(run_tum.run).parameters
    assert parameters["mesh_smooth_iterations"].default == 0 and parameters["mesh_smooth_lambda"].default == 0.5 and parameters["mesh_smooth_mu"].default == -0.53
    assert parameters["mesh_smooth_boundary"].default == "fixed"
    a = run_tum.arg_parser().parse_args(["somewhere"])
    assert (a.mesh_smooth_iterations, a.mesh_smooth_lambda, a.mesh_smooth_mu, a.mesh_smooth_boundary) == (0, 0.5, -0.53, "fixed")
    a = run_tum.arg_parser().parse_args(["somewhere", "--mesh-smooth-iterations", "4", "--mesh-smooth-lambda", "0.3", "--mesh-smooth-mu", "-0.31", "--mesh-smooth-boundary", "rim"])
    assert (a.mesh_smooth_iterations, a.mesh_smooth_lambda, a.mesh_smooth_mu, a.mesh_smooth_boundary) == (4, 0.3, -0.31, "rim")
    with pytest.raises(SystemExit):
        run_tum.arg_parser().parse_args(["somewhere", "--mesh-smooth-boundary", "open"])

    positions, normals, tri = sm.uv_sphere(12, 6)
    extracted = dict(positions=positions, normals=normals, colors=np.zeros((len(positions), 4), np.uint8), triangles=tri)
    calls = []

    class StubBA:
        def keyframe_count(self):
            return 0

        def surfels_size(self):
            return 0

        def SmoothMesh(self, mesh, iterations=10, lambda_=0.5, mu=-0.53, boundary="fixed"):
            calls.append(("smooth", mesh, iterations, lambda_, mu, boundary))
            p, n = sm.smooth(mesh["positions"], mesh["normals"], mesh["triangles"], iterations, lambda_, mu, sm.MODES[boundary])
            return dict(positions=p, normals=n, colors=mesh["colors"], triangles=mesh["triangles"])

        def DecimateMesh(self, mesh, target_vertices=None, ratio=None, boundary_weight=1.0, max_cost=None, max_rounds=0):
            calls.append(("decimate", mesh, target_vertices, ratio))
            return du.decimate(mesh["positions"], mesh["normals"], mesh["colors"], mesh["triangles"], target_vertices)

    class StubSlam:
        def __init__(self, *args, **kwargs):
            self._ba = StubBA()

        def ba(self):
            return self._ba

        def frame_poses(self):
            return []

    def fuse_and_mesh(ba, path, *args):
        calls.append(("extract", path))
        return extracted, (0.0, 0.0, 0.0), (1, 1, 1), None

    def evaluate(ba, mesh, truth, *args, **kwargs):
        calls.append(("evaluate", mesh))
        return {"accuracy": {"count": len(mesh["positions"])}}

    monkeypatch.setattr(run_tum.dba, "read_tum_dataset", lambda d, t: dict(frames=[], width=64, height=48, camera=(50.0, 50.0, 32.0, 24.0)))
    monkeypatch.setattr(run_tum.dba, "save_poses", lambda *a: None)
    monkeypatch.setattr(run_tum.dba, "SaveMeshAsPLY", lambda path, mesh: calls.append(("save", path, mesh)))
    monkeypatch.setattr(run_tum.dba, "LoadPLY", lambda path: {"positions": positions})
    monkeypatch.setattr(run_tum.bad_slam, "BadSlam", StubSlam)
    monkeypatch.setattr(run_tum, "fuse_and_mesh", fuse_and_mesh)
    monkeypatch.setattr(run_tum.surface_eval, "evaluate", evaluate)

    # off by default: the extraction writes the file itself and nothing is smoothed
    r = run_tum.run(tmp_path, out=str(tmp_path / "poses.txt"), mesh="m.ply")
    assert calls == [("extract", "m.ply")] and "smoothing" not in r["mesh"]

    del calls[:]
    report = tmp_path / "surface.json"
    r = run_tum.run(tmp_path, out=str(tmp_path / "poses.txt"), mesh="m.ply", mesh_smooth_iterations=4, mesh_smooth_lambda=0.3, mesh_smooth_mu=-0.31,
                    mesh_smooth_boundary="rim", ground_truth_surface="truth.ply", surface_report=str(report))
    assert [c[0] for c in calls] == ["extract", "smooth", "save", "evaluate"]
    assert calls[0][1] is None, "the unsmoothed mesh must not be written"
    assert calls[1][1] is extracted and calls[1][2:] == (4, 0.3, -0.31, "rim")
    smoothed = calls[2][2]
    assert calls[2][1] == "m.ply" and calls[3][1] is smoothed, "the smoothed mesh is what is written and what is scored"
    assert (bits(smoothed["positions"]) != bits(positions)).any()
    want = {"iterations": 4, "lambda": 0.3, "mu": -0.31, "boundary": "rim"}
    assert r["mesh"]["smoothing"] == want and r["mesh"]["vertices"] == len(positions)
    assert json.loads(report.read_text())["mesh_smoothing"] == want

    # before the decimation, with the defaults, with no file
    del calls[:]
    r = run_tum.run(tmp_path, out=str(tmp_path / "poses.txt"), mesh_smooth_iterations=2, mesh_decimate_vertices=30, ground_truth_surface="truth.ply")
    assert [c[0] for c in calls] == ["extract", "smooth", "decimate", "evaluate"]
    assert calls[1][2:] == (2, 0.5, -0.53, "fixed") and (bits(calls[2][1]["positions"]) != bits(positions)).any(), "the smoothed mesh is what is decimated"
    assert r["surface"]["mesh_smoothing"] == {"iterations": 2, "lambda": 0.5, "mu": -0.53, "boundary": "fixed"} and "mesh" not in r
    assert r["surface"]["mesh_decimation"]["vertices"] == 30 and calls[3][1]["positions"].shape[0] == 30

    with pytest.raises(ValueError, match="mesh-smooth-iterations"):
        run_tum.run(tmp_path, mesh="m.ply", mesh_smooth_iterations=-1)
