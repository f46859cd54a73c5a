"""Surface registration without a GPU: the restatement of tests/registration_util.py against finite differences and a known
motion, and the plumbing of surface_eval.evaluate(register=True) against a stub.

Measured with the restated loop (float32 step, float64 loop) on the corner surface of registration_util -- 384 triangles, source
points moved by 2 cm and 1 degree about the corner, start at the identity, search radius 8 cm down to 1 cm, every default:

    PLANE, 600 points against the mesh:                             7 steps, error 5.4e-8 m and 1.5e-8 rad
    POINT, 300 points against the surface as a cloud at 1.25 cm:   25 steps, error 8.7e-3 m and 4.4e-3 rad

(error: the norms of the translation and rotation parts of log(result * truth^-1)).  Point to plane ends at the rounding of the
float32 points; point to point against a cloud cannot see a slide along a plane that is shorter than the cloud's spacing, and stops
within that spacing.  tests/test_gpu_registration.py holds DirectBA.RegisterPoints to four times these figures."""
import numpy as np
import pytest

from tests import registration_util as ru

F = np.float32
CPU_ERROR = {ru.PLANE: (5.4e-8, 1.5e-8), ru.POINT: (8.7e-3, 4.4e-3)}      # (metres, radians), from the runs of the docstring
POINT_MODE_POINTS = 300


@pytest.fixture(scope="module")
def corner():
    positions, triangles, _ = ru.corner_surface()
    truth = ru.known_displacement()
    return positions, triangles, ru.displaced(ru.corner_points(), truth), truth


def test_the_corner_surface():
    positions, triangles, inner = ru.corner_surface()
    assert len(triangles) == 384 and inner.sum() == 150
    normals = np.cross(positions[triangles[:, 1]] - positions[triangles[:, 0]], positions[triangles[:, 2]] - positions[triangles[:, 0]])
    assert (np.linalg.norm(normals, axis=1) > 0).all()
    patch = [normals[k * 128] / np.linalg.norm(normals[k * 128]) for k in range(3)]
    for a in range(3):                                                           # mutually oblique: neither parallel nor orthogonal
        assert 0.05 < abs(patch[a] @ patch[(a + 1) % 3]) < 0.95
    points = ru.corner_points()
    d, t = ru.correspondences(points, positions, triangles, ru.CORNER_R0, ru.CORNER_R0)
    assert d.max() < 1e-6 and inner[t].all()                                      # on the surface, away from the open sides
    truth = ru.known_displacement()
    assert np.allclose(ru.pose_error(truth, np.eye(4))[1], np.deg2rad(1.0))
    assert np.allclose(truth[:3, :3] @ truth[:3, :3].T, np.eye(3), atol=1e-15)
    assert np.abs(ru.displaced(points, truth).astype(np.float64) @ truth[:3, :3].T + truth[:3, 3] - points).max() < 1e-6


def test_exp_and_log():
    rng = np.random.default_rng(2)
    for scale in (1e-10, 1e-3, 0.5):
        delta = rng.standard_normal(6) * scale
        T = ru.se3_exp(delta)
        assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-14)
        t, w = ru.se3_log(T)
        assert np.allclose(np.concatenate([t, w]), delta, rtol=1e-9, atol=1e-18)
    x, share = ru.solve_ldlt(np.diag([4.0, 1.0, 2.0, 8.0, 3.0, 5.0]) + 0.1, np.arange(6.0))
    assert np.allclose((np.diag([4.0, 1.0, 2.0, 8.0, 3.0, 5.0]) + 0.1) @ x, np.arange(6.0)) and 0.9 < share <= 1.0
    H = np.ones((6, 6))
    assert ru.solve_ldlt(H, np.ones(6))[1] == 0.0                                 # rank 1


@pytest.mark.parametrize("mode", [ru.PLANE, ru.POINT], ids=["plane", "point"])
def test_row_jacobians_agree_with_central_differences(corner, mode):
    positions, triangles, source, truth = corner
    rng = np.random.default_rng(4)
    M = (ru.se3_exp(rng.standard_normal(6) * 0.01) @ truth)[:3].astype(F)
    s = ru.step(source[:40], M, positions, triangles, ru.CORNER_R0, ru.CORNER_R0, mode, np.inf)
    assert s["counts"][2] == 40
    p = s["moved"].astype(np.float64)
    tri = positions[triangles[s["triangle"].astype(np.int64)]].astype(np.float64)
    if mode == ru.PLANE:
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        directions = [n / np.linalg.norm(n, axis=1, keepdims=True)]
        anchor = tri[:, 0]
    else:
        directions = [np.tile(np.eye(3)[k], (40, 1)) for k in range(3)]
        anchor = p - s["v"].astype(np.float64)                                    # the closest point, held fixed
    h = 1e-6
    for m in directions:
        residual = lambda delta: np.einsum("ij,ij->i", m, p @ ru.se3_exp(delta)[:3, :3].T + ru.se3_exp(delta)[:3, 3] - anchor)
        numeric = np.stack([(residual(h * np.eye(6)[k]) - residual(-h * np.eye(6)[k])) / (2 * h) for k in range(6)], -1)
        J = ru.jacobian(s["moved"], m.astype(F)).astype(np.float64)
        assert np.abs(numeric - J).max() < 1e-6, np.abs(numeric - J).max()
        # and the residual the rows carry is the one differentiated
        r0 = residual(np.zeros(6))
        terms = s["terms"].reshape(40, -1, ru.TERMS)
        k = 0 if mode == ru.PLANE else int(np.argmax(m[0]))
        assert np.allclose(terms[:, k, 28], r0 * r0, rtol=1e-3, atol=1e-12)


def test_the_step_of_a_point_on_each_feature():
    """v is the offset from the closest point: against one triangle, a point over the face, beyond an edge and beyond a vertex."""
    positions = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    triangles = np.array([[0, 1, 2]], np.uint32)
    points = np.array([[0.25, 0.25, 0.3], [0.5, -0.2, 0.1], [-0.3, -0.4, 0.0], [5, 5, 5]], F)
    M = np.eye(4)[:3].astype(F)
    s = ru.step(points, M, positions, triangles, 1.0, 1.0, ru.POINT, np.inf)
    assert s["counts"] == (4, 3, 3, 0) and s["triangle"][3] == 0xFFFFFFFF and np.isinf(s["distance"][3])
    assert np.allclose(s["v"][:3], [[0, 0, 0.3], [0, -0.2, 0.1], [-0.3, -0.4, 0]], atol=1e-7)
    assert np.allclose(s["distance"][:3], np.linalg.norm(s["v"][:3], axis=1), rtol=1e-6)
    plane = ru.step(points, M, positions, triangles, 1.0, 1.0, ru.PLANE, 0.05)
    assert plane["counts"] == (4, 3, 3, 0)
    assert np.allclose(plane["a"][:3], [0.3, 0.1, 0.0], atol=1e-7)
    sums, _ = ru.sums64(plane["terms"])
    assert np.isclose(sums[27], 0.05 * (0.3 - 0.025) + 0.05 * (0.1 - 0.025))       # Huber: both residuals are beyond k
    cloud = ru.step(points, M, positions, np.array([[0, 0, 0], [1, 1, 1]], np.uint32), 1.0, 1.0, ru.PLANE, np.inf)
    assert cloud["counts"][2] == 0 and cloud["counts"][3] == cloud["counts"][1] > 0 and len(cloud["terms"]) == 0


@pytest.mark.parametrize("mode", [ru.PLANE, ru.POINT], ids=["plane", "point"])
def test_the_loop_recovers_a_known_displacement(corner, mode):
    positions, triangles, source, truth = corner
    if mode == ru.POINT:
        positions = ru.corner_cloud()
        assert 12000 < len(positions) < 13000
        triangles = np.repeat(np.arange(len(positions), dtype=np.uint32)[:, None], 3, axis=1)
        source = source[:POINT_MODE_POINTS]
    start = ru.pose_error(np.eye(4), truth)
    r = ru.register(source, positions, triangles, ru.CORNER_R0, mode=mode)
    error = ru.pose_error(r["target_T_source"], truth)
    print(f"mode {mode}: {r['iterations']} steps, {r['reason']}; error {error[0]:.3e} m, {error[1]:.3e} rad (start {start[0]:.3e} m, {start[1]:.3e} rad)")
    assert r["converged"] and r["reason"] == "converged" and r["iterations"] == len(r["history"])
    assert [h["radius"] for h in r["history"]][0] == ru.CORNER_R0 and r["history"][-1]["radius"] == ru.CORNER_R0 / 8
    # PLANE: the data are exact planes, so the last step -- below the loop's thresholds -- bounds what is left.  POINT: what a
    # cloud cannot see is a slide of less than its spacing, 1.25 cm, and the rotation that makes of it over the 0.5 m of the points
    bound = (ru.STEP_TRANSLATION, ru.STEP_ROTATION) if mode == ru.PLANE else (0.0125, 0.0125 / 0.5)
    assert error[0] <= bound[0] and error[1] <= bound[1]
    assert error[0] < start[0] and error[1] < start[1]


def test_a_flat_plane_is_singular_and_too_few_pairs_end_the_loop(corner):
    _, _, source, _ = corner
    positions, triangles, _ = ru.flat_plane()
    r = ru.register(source[:200], positions, triangles, ru.CORNER_R0)
    assert not r["converged"] and r["reason"] == "singular system" and np.isfinite(r["target_T_source"]).all()
    assert np.array_equal(r["target_T_source"], np.eye(4)) and r["iterations"] == 1
    far = np.eye(4)
    far[:3, 3] = 50.0
    r = ru.register(source[:200], positions, triangles, ru.CORNER_R0, initial=far)
    assert not r["converged"] and r["reason"] == "fewer than 6 pairs" and np.array_equal(r["target_T_source"], far)
    assert r["history"][0]["used"] == 0 and np.isnan(r["history"][0]["rmse"])


# ------------------------------------------------------------------------------------------------
# surface_eval.evaluate(register=...)
# ------------------------------------------------------------------------------------------------
class StubBA:
    """Distances: the x coordinate of each point.  Registration: a fixed motion."""

    def __init__(self, found):
        self.found, self.calls = found, []

    def PointMeshDistance(self, points, mesh, max_distance, cell_size=None):
        self.calls.append(("distance", np.array(points), mesh, max_distance, cell_size))
        return dict(distance=np.abs(np.asarray(points, F)[:, 0]), triangle=np.zeros(len(points), np.uint32), cell_size=1.0, grid_cells=1, grid_entries=1)

    def RegisterPoints(self, points, mesh, max_distance, initial=None, cell_size=None):
        self.calls.append(("register", np.array(points), mesh, max_distance, np.array(initial), cell_size))
        return dict(target_T_source=self.found, iterations=3, converged=True, reason="converged", history=[dict(radius=0.1, hits=2, used=2, cost=0.0, rmse=0.0,
                                                                                                                  step_translation=0.0, step_rotation=0.0)])


def test_evaluate_register_plumbing():
    from badslam_amd import surface_eval
    found = ru.se3_exp([0.01, -0.02, 0.03, 0.01, 0.02, -0.01])
    start = ru.se3_exp([0.5, 0, 0, 0, 0, 0.1])
    reconstruction = dict(positions=np.array([[0.01, 1, 2], [0.03, -1, 0.5], [0.2, 0, 0]], F), triangles=np.array([[0, 1, 2]], np.uint32), normals="kept")
    truth = dict(positions=np.array([[0.02, 0, 0], [0.04, 1, 1]], F))
    stub = StubBA(found)
    plain = surface_eval.evaluate(stub, reconstruction, truth, 0.1, (0.02, 0.05))
    assert [c[0] for c in stub.calls] == ["distance", "distance"] and "registration" not in plain
    assert sorted(plain) == ["accuracy", "accuracy_grid", "completeness", "completeness_grid", "f_scores", "max_distance"]
    stub = StubBA(found)
    r = surface_eval.evaluate(stub, reconstruction, truth, 0.1, (0.02, 0.05), cell_size=0.3, register=True, initial=start)
    assert [c[0] for c in stub.calls] == ["distance", "distance", "register", "distance", "distance"]
    register = stub.calls[2]
    assert np.array_equal(register[1], reconstruction["positions"]) and register[2] is truth and register[3] == 0.1 and np.array_equal(register[4], start) and register[5] == 0.3
    moved = lambda T: (reconstruction["positions"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F)
    assert np.array_equal(stub.calls[0][1], moved(start)) and np.array_equal(stub.calls[3][1], moved(found))
    assert stub.calls[4][2]["positions"].dtype == F and np.array_equal(stub.calls[4][2]["positions"], moved(found)) and stub.calls[4][2]["normals"] == "kept"
    assert np.array_equal(reconstruction["positions"], np.array([[0.01, 1, 2], [0.03, -1, 0.5], [0.2, 0, 0]], F))         # the caller's mesh is not touched
    reg = r["registration"]
    assert np.array_equal(np.array(reg["target_T_source"]), found) and reg["iterations"] == 3 and reg["converged"] and reg["reason"] == "converged" and len(reg["history"]) == 1
    assert reg["before"]["accuracy"] == surface_eval.distance_summary(np.abs(moved(start)[:, 0]), (0.02, 0.05))
    assert r["accuracy"] == surface_eval.distance_summary(np.abs(moved(found)[:, 0]), (0.02, 0.05))
    assert {k: v for k, v in r.items() if k != "registration"}.keys() == plain.keys()
    identity = StubBA(np.eye(4))
    surface_eval.evaluate(identity, reconstruction, truth, 0.1, (0.02,), register=True)
    assert np.array_equal(identity.calls[2][4], np.eye(4))


def test_python_entry_points_exist():
    from badslam_amd import abi, direct_ba
    assert callable(direct_ba.DirectBA.RegisterPoints)
    for name in ("bslam_registration_prepare", "bslam_registration_step"):
        assert name in abi.SIGNATURES
