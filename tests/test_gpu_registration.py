"""-m gpu: surface registration -- bslam_registration_prepare / bslam_registration_step (badslam_amd/csrc/registration_kernels.hpp)
against the restatement of tests/registration_util.py, then DirectBA.RegisterPoints, surface_eval.evaluate(register=True) and
tools/run_tum.py --register-surface.  Per-point outputs and counts are compared exactly; the sums with the float64 sums of the
restatement's float32 terms within the bound of the summation alone.  Every device array stands between guard words, outputs are
filled with a sentinel first.

Measured beforehand on the CPU (the restated loop of registration_util.register over all 24 070 vertices of the fused mesh, the
candidates of a point pruned with a k-d tree over the triangles' centres and then taken through the rule; the pruned search
equals the brute-force restatement bit for bit on the first 200 vertices) on the fused three-keyframe scene of
tests/test_gpu_surface_eval.py, the analytic planes moved by 1.5 cm and 0.5 degrees about the centre of the volume, search radius
0.1 m: accuracy median 3.487 mm without registration and 0.761 mm with the restated loop's transform (9 steps; 0.763 mm for the
planes where they were); completeness median 3.386 mm and 0.645 mm.  The loop leaves 5.8e-5 m and 2.6e-4 rad of the motion: the
reconstruction's own error, not the planes', decides where the minimum lies."""
import ctypes as C
import json

import numpy as np
import pytest

import badslam_amd
from tests import point_mesh_util as pm
from tests import registration_util as ru
from tests.test_gpu_fusion import SENTINEL, bits, stream_ptr
from tests.test_gpu_mesh_components import Guarded
from tests.test_gpu_surface_eval import fused            # noqa: F401  (the fixture: three keyframes fused at 2 cm, the mesh extracted)
from tests.test_registration_cpu import CPU_ERROR, POINT_MODE_POINTS

pytestmark = pytest.mark.gpu
F = np.float32
INVALID_ARGUMENT = -1
IDENTITY = np.eye(4)[:3].astype(F)
SPHERE_R0, SPHERE_CELL = 2.0, 1.0
# the fused scene, its planes moved by MOVED_BY: medians in metres from the CPU run of the docstring
MOVED_BY = (0.015, np.deg2rad(0.5))
CPU_UNREGISTERED_ACCURACY_MEDIAN = 3.487e-3
CPU_REGISTERED_ACCURACY_MEDIAN = 7.61e-4
CPU_REGISTERED_COMPLETENESS_MEDIAN = 6.45e-4


@pytest.fixture(scope="module")
def gpu():
    import torch
    from badslam_amd import build
    build.build()
    return torch, badslam_amd.lib(), badslam_amd.Context(0)


@pytest.fixture(scope="module")
def sphere():
    """The sphere of point_mesh_util and its 680 points, of which nine are NaN, infinite or far away."""
    positions, triangles = pm.sphere_mesh()
    points = pm.sphere_points(positions, triangles).copy()
    points[[0, 3, 40, 62, 64, 200, 256, 600, 679]] = np.array([[np.nan, 15, 15], [16, np.nan, 14], [np.inf, 15, 15], [16, -np.inf, 14], [1e6, 0, 0], [-1e30, 1e30, 0],
                                                              [3e38, 3e38, 3e38], [np.nan, np.nan, np.nan], [16, 15, -500]], F)
    return positions, triangles, np.ascontiguousarray(points, F)


def prepare(gpu, positions, triangles, R0, cell, budget=1 << 28):
    """-> (rc, cells, entries); the mesh arrays are freed before this returns."""
    torch, L, ctx = gpu
    positions, triangles = np.ascontiguousarray(positions, F).reshape(-1, 3), np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    pos, tri = Guarded(torch, positions.size, positions), Guarded(torch, triangles.size, triangles)
    cells, entries = C.c_uint64(SENTINEL), C.c_uint64(SENTINEL)
    rc = L.bslam_registration_prepare(ctx.handle, stream_ptr(torch), len(positions), pos.ptr, len(triangles), tri.ptr, float(R0), float(cell), budget, C.byref(cells),
                                      C.byref(entries))
    assert np.array_equal(pos.read(), bits(positions).reshape(-1)) and np.array_equal(tri.read(), triangles.reshape(-1))
    del pos, tri
    torch.cuda.empty_cache()
    return rc, cells.value, entries.value


def step(gpu, points, M, R, mode, huber, outputs=True):
    """-> (rc, distance, triangle, sums f32[32], counts u64[4]); asserts that the points and the guard words are untouched."""
    torch, L, ctx = gpu
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    N = len(points)
    pts = Guarded(torch, 3 * N, points)
    out_d, out_t = (Guarded(torch, N + 7), Guarded(torch, N + 7)) if outputs else (None, None)
    m = np.ascontiguousarray(M, F).reshape(12)
    sums, counts = np.full(32, 1.5e16, F), np.full(4, SENTINEL, np.uint64)
    rc = L.bslam_registration_step(ctx.handle, stream_ptr(torch), N, pts.ptr, m.ctypes.data_as(C.POINTER(C.c_float)), float(R), int(mode), float(huber),
                                   out_d.ptr if outputs else None, out_t.ptr if outputs else None, sums.ctypes.data_as(C.POINTER(C.c_float)),
                                   counts.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert np.array_equal(pts.read(), bits(points).reshape(-1)), "the points were written to"
    if not outputs:
        return rc, None, None, sums, counts
    d, t = out_d.read(), out_t.read()
    assert (d[N:] == SENTINEL).all() and (t[N:] == SENTINEL).all(), "written beyond N"
    return rc, d[:N].view(F), t[:N], sums, counts


def assert_points_equal(d, t, want, what=""):
    differ = (bits(d) != bits(want["distance"])) | (t != want["triangle"])
    assert not differ.any(), f"{what}: {int(differ.sum())} points differ, first at {np.flatnonzero(differ)[0]}"


def assert_sums_agree(sums, counts, want, N, mode, what=""):
    assert tuple(int(c) for c in counts) == want["counts"], (what, counts, want["counts"])
    total, magnitude = ru.sums64(want["terms"])
    bound = (ru.additions(N, mode) + 4) * 2.0 ** -24 * magnitude
    error = np.abs(sums[:ru.TERMS].astype(np.float64) - total)
    print(f"{what}: N {N}, D {ru.additions(N, mode)}, largest error / bound {np.max(error / np.maximum(bound, 1e-300)):.3f}")
    assert (error <= bound).all(), (what, np.flatnonzero(error > bound), error, bound)
    assert (bits(sums[ru.TERMS:]) == 0).all()


# ------------------------------------------------------------------------------------------------
# 1. identity and R = R0
# ------------------------------------------------------------------------------------------------
def test_identity_at_the_prepared_radius_equals_point_mesh_distance(gpu, sphere):
    from tests.test_gpu_point_mesh import call
    positions, triangles, points = sphere
    rc, cells, entries = prepare(gpu, positions, triangles, SPHERE_R0, SPHERE_CELL)
    badslam_amd.check(rc)
    assert (cells, entries) == pm.grid_census(positions, triangles, SPHERE_R0, SPHERE_CELL)
    want_all = pm.point_mesh_distance(points, positions, triangles, SPHERE_R0)
    assert np.isinf(want_all[0][[0, 3, 40, 62, 64, 200, 256, 600, 679]]).all() and 100 < np.isfinite(want_all[0]).sum()
    for N in (1, 63, 64, 65, 257, 680):
        rc, d, t, sums, counts = step(gpu, points[:N], IDENTITY, SPHERE_R0, ru.PLANE, np.inf)
        badslam_amd.check(rc)
        want = ru.step(points[:N], IDENTITY, positions, triangles, SPHERE_R0, SPHERE_R0, ru.PLANE, np.inf)
        assert np.array_equal(bits(want["distance"]), bits(want_all[0][:N])) and np.array_equal(want["triangle"], want_all[1][:N])
        assert_points_equal(d, t, want, f"N {N}")
        rc, pd, pt, _, _ = call(gpu, points[:N], positions, triangles, SPHERE_R0, SPHERE_CELL)
        badslam_amd.check(rc)
        assert np.array_equal(bits(d), bits(pd)) and np.array_equal(t, pt)
        assert_sums_agree(sums, counts, want, N, ru.PLANE, f"identity, N {N}")


# ------------------------------------------------------------------------------------------------
# 2. a generic transform with R < R0
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generic(sphere):
    positions, triangles, points = sphere
    centre = np.array(pm.SPHERE_CENTRE)
    T = ru.se3_exp([0, 0, 0, 0.04, -0.07, 0.05])
    T[:3, 3] = centre - T[:3, :3] @ centre + np.array([0.21, -0.13, 0.17])
    return T[:3].astype(F)


@pytest.mark.parametrize("huber", [0.4, np.inf], ids=["huber 0.4", "no huber"])
@pytest.mark.parametrize("mode", [ru.PLANE, ru.POINT], ids=["plane", "point"])
def test_a_generic_transform_below_the_prepared_radius(gpu, sphere, generic, mode, huber):
    positions, triangles, points = sphere
    R = 1.3
    badslam_amd.check(prepare(gpu, positions, triangles, SPHERE_R0, SPHERE_CELL)[0])
    want = ru.step(points, generic, positions, triangles, SPHERE_R0, R, mode, huber)
    n, hits, used, degenerate = want["counts"]
    assert n == 680 and 200 < hits < 660 and used == hits and degenerate == 0
    if np.isfinite(huber):
        assert 20 < (want["a"][want["used"]] > F(huber)).sum() < used - 20           # both branches of the weight
    wider = ru.step(points, generic, positions, triangles, SPHERE_R0, SPHERE_R0, mode, huber)
    assert wider["counts"][1] > hits                                               # R, not R0, decides the hits
    rc, d, t, sums, counts = step(gpu, points, generic, R, mode, huber)
    badslam_amd.check(rc)
    assert_points_equal(d, t, want)
    assert_sums_agree(sums, counts, want, 680, mode, f"mode {mode}, huber {huber}")
    rc2, d2, t2, sums2, counts2 = step(gpu, points, generic, R, mode, huber)
    assert rc2 == 0 and np.array_equal(bits(d), bits(d2)) and np.array_equal(t, t2) and np.array_equal(bits(sums), bits(sums2)) and np.array_equal(counts, counts2)
    rc3, _, _, sums3, counts3 = step(gpu, points, generic, R, mode, huber, outputs=False)   # without the optional outputs
    assert rc3 == 0 and np.array_equal(bits(sums), bits(sums3)) and np.array_equal(counts, counts3)


# ------------------------------------------------------------------------------------------------
# 3. degenerate and empty cases
# ------------------------------------------------------------------------------------------------
def test_degenerate_and_empty_cases(gpu, sphere, generic):
    from tests.test_gpu_point_mesh import call
    positions, triangles, points = sphere
    cloud = positions[::3]
    own = np.repeat(np.arange(len(cloud), dtype=np.uint32)[:, None], 3, axis=1)
    badslam_amd.check(prepare(gpu, cloud, own, SPHERE_R0, SPHERE_CELL)[0])
    want = ru.step(points, generic, cloud, own, SPHERE_R0, 1.3, ru.PLANE, 0.4)
    rc, d, t, sums, counts = step(gpu, points, generic, 1.3, ru.PLANE, 0.4)
    assert rc == 0 and want["counts"][1] > 100
    assert_points_equal(d, t, want, "cloud")
    assert tuple(int(c) for c in counts) == (680, want["counts"][1], 0, want["counts"][1]) and (bits(sums) == 0).all()
    want = ru.step(points, generic, cloud, own, SPHERE_R0, 1.3, ru.POINT, 0.4)       # the same cloud serves POINT mode
    rc, d, t, sums, counts = step(gpu, points, generic, 1.3, ru.POINT, 0.4)
    assert rc == 0
    assert_points_equal(d, t, want, "cloud, point mode")
    assert_sums_agree(sums, counts, want, 680, ru.POINT, "cloud, point mode")
    # every point a miss; no point at all
    away = generic.copy()
    away[:, 3] += 1000
    rc, d, t, sums, counts = step(gpu, points, away, 1.3, ru.POINT, 0.4)
    assert rc == 0 and np.isinf(d).all() and (d > 0).all() and (t == pm.NO_TRIANGLE).all() and tuple(int(c) for c in counts) == (680, 0, 0, 0) and (bits(sums) == 0).all()
    rc, d, t, sums, counts = step(gpu, np.zeros((0, 3), F), generic, 1.3, ru.POINT, 0.4)
    assert rc == 0 and tuple(int(c) for c in counts) == (0, 0, 0, 0) and (bits(sums) == 0).all()
    # a mesh without a triangle, and one without a valid triangle: prepared, every point misses
    for pos, tri in ((positions, np.zeros((0, 3), np.uint32)), (np.full((3, 3), np.nan, F), np.array([[0, 1, 2]], np.uint32))):
        assert prepare(gpu, pos, tri, SPHERE_R0, SPHERE_CELL) == (0, 0, 0)
        rc, d, t, sums, counts = step(gpu, points, generic, 1.3, ru.PLANE, 0.4)
        assert rc == 0 and np.isinf(d).all() and (t == pm.NO_TRIANGLE).all() and tuple(int(c) for c in counts) == (680, 0, 0, 0) and (bits(sums) == 0).all()
    # a distance call between prepare and step -- on another, larger mesh, so that its scratch grows -- changes neither result
    badslam_amd.check(prepare(gpu, positions[:900], triangles[(triangles < 900).all(axis=1)], SPHERE_R0, SPHERE_CELL)[0])
    part = triangles[(triangles < 900).all(axis=1)]
    assert len(part) > 500
    first = step(gpu, points, generic, 1.3, ru.PLANE, 0.4)
    rc, pd, pt, _, _ = call(gpu, np.concatenate([points, points, points]), positions, triangles, 0.6, 0.3)
    assert rc == 0
    want_between = pm.point_mesh_distance(np.concatenate([points, points, points]), positions, triangles, 0.6)
    assert np.array_equal(bits(pd), bits(want_between[0])) and np.array_equal(pt, want_between[1])
    second = step(gpu, points, generic, 1.3, ru.PLANE, 0.4)
    assert first[0] == second[0] == 0
    for a, b in zip(first[1:], second[1:]):
        assert np.array_equal(bits(a) if a.dtype == F else a, bits(b) if b.dtype == F else b)
    assert_points_equal(second[1], second[2], ru.step(points, generic, positions[:900], part, SPHERE_R0, 1.3, ru.PLANE, 0.4), "after a distance call")


def test_prepare_budget_and_bad_indices(gpu, sphere, generic):
    torch, L, ctx = gpu
    positions, triangles, points = sphere
    badslam_amd.check(prepare(gpu, positions, triangles, SPHERE_R0, SPHERE_CELL)[0])
    before = step(gpu, points, generic, 1.3, ru.PLANE, 0.4)
    cells, entries = pm.grid_census(positions, triangles, SPHERE_R0, SPHERE_CELL)
    rc, got_cells, got_entries = prepare(gpu, positions, triangles, SPHERE_R0, SPHERE_CELL, budget=entries - 1)
    message = L.bslam_last_error()
    assert rc == INVALID_ARGUMENT and (got_cells, got_entries) == (cells, entries) and str(entries).encode() in message and b"max_grid_entries" in message
    bad = triangles.copy()
    bad[1777, 2] = len(positions)
    assert prepare(gpu, positions, bad, SPHERE_R0, SPHERE_CELL)[0] == INVALID_ARGUMENT and b"beyond vertex_count" in L.bslam_last_error()
    for changes in (dict(R0=0.0), dict(R0=np.nan), dict(R0=np.inf), dict(cell=0.0), dict(cell=np.nan), dict(budget=0)):
        a = dict(dict(R0=SPHERE_R0, cell=SPHERE_CELL, budget=1 << 28), **changes)
        assert prepare(gpu, positions, triangles, a["R0"], a["cell"], a["budget"])[0] == INVALID_ARGUMENT, changes
    after = step(gpu, points, generic, 1.3, ru.PLANE, 0.4)                          # a refused prepare leaves the mesh that was there
    assert after[0] == 0 and np.array_equal(bits(before[1]), bits(after[1])) and np.array_equal(bits(before[3]), bits(after[3]))


# ------------------------------------------------------------------------------------------------
# 4. refusals
# ------------------------------------------------------------------------------------------------
def test_rejected_arguments(gpu, sphere, generic):
    torch, L, ctx = gpu
    positions, triangles, points = sphere
    N = len(points)
    fresh = badslam_amd.Context(0)                                                # nothing prepared on it
    badslam_amd.check(prepare(gpu, positions, triangles, SPHERE_R0, SPHERE_CELL)[0])
    pts, out_d, out_t = Guarded(torch, 3 * N, points), Guarded(torch, N), Guarded(torch, N)
    sums, counts = np.full(32, 1.5e16, F), np.full(4, SENTINEL, np.uint64)
    base = dict(ctx=ctx.handle, N=N, points=pts.address, M=generic.reshape(12).copy(), R=1.3, mode=ru.PLANE, huber=0.4, out_d=out_d.address, out_t=out_t.address,
                sums=sums.ctypes.data, counts=counts.ctypes.data)

    def run(**changes):
        a = dict(base, **changes)
        p = lambda v: None if v is None else C.c_void_p(v)
        m = None if a["M"] is None else np.ascontiguousarray(a["M"], F).ctypes.data_as(C.POINTER(C.c_float))
        f = lambda v: None if v is None else C.cast(C.c_void_p(v), C.POINTER(C.c_float))
        u = lambda v: None if v is None else C.cast(C.c_void_p(v), C.POINTER(C.c_uint64))
        return L.bslam_registration_step(a["ctx"], stream_ptr(torch), a["N"], p(a["points"]), m, a["R"], a["mode"], a["huber"], p(a["out_d"]), p(a["out_t"]), f(a["sums"]),
                                         u(a["counts"]))

    def matrix(index, value):
        m = base["M"].copy()
        m[index] = value
        return m

    cases = {"null context": dict(ctx=None), "null points": dict(points=None), "null sums": dict(sums=None), "null counts": dict(counts=None),
             "null matrix": dict(M=None), "no prepared mesh": dict(ctx=fresh.handle),
             "NaN in the matrix": dict(M=matrix(5, np.nan)), "inf in the matrix": dict(M=matrix(3, np.inf)), "-inf in the matrix": dict(M=matrix(11, -np.inf)),
             "R = 0": dict(R=0.0), "R < 0": dict(R=-1.0), "R = inf": dict(R=float("inf")), "R = NaN": dict(R=float("nan")),
             "R > R0": dict(R=float(np.nextafter(F(SPHERE_R0), F(np.inf)))),
             "huber = 0": dict(huber=0.0), "huber < 0": dict(huber=-0.5), "huber = NaN": dict(huber=float("nan")),
             "mode 2": dict(mode=2), "mode -1": dict(mode=-1), "more than 2^32 - 256 points": dict(N=0xFFFFFF01),
             "misaligned points": dict(points=base["points"] + 2), "the outputs are one": dict(out_t=base["out_d"]), "in place": dict(out_d=base["points"])}
    for name, changes in cases.items():
        rc = run(**changes)
        assert rc == INVALID_ARGUMENT, (name, rc, L.bslam_last_error())
        assert len(L.bslam_last_error()) > 0
    torch.cuda.synchronize()
    assert (out_d.read() == SENTINEL).all() and (out_t.read() == SENTINEL).all(), "a refused call wrote to an output"
    assert (sums == F(1.5e16)).all() and (counts == SENTINEL).all(), "a refused call wrote to a host output"
    assert np.array_equal(pts.read(), bits(points).reshape(-1))
    assert run() == 0 and run(R=SPHERE_R0) == 0 and run(huber=float("inf")) == 0 and run(out_d=None, out_t=None) == 0
    want = ru.step(points, generic, positions, triangles, SPHERE_R0, 1.3, ru.PLANE, 0.4)
    assert run() == 0
    assert_points_equal(out_d.read().view(F), out_t.read(), want)


# ------------------------------------------------------------------------------------------------
# 5. DirectBA.RegisterPoints
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [ru.PLANE, ru.POINT], ids=["plane", "point"])
def test_register_points_recovers_the_known_displacement(fused, mode):
    ba = fused[0]
    positions, triangles, _ = ru.corner_surface()
    truth = ru.known_displacement()
    source = ru.displaced(ru.corner_points(), truth)
    if mode == ru.PLANE:
        target = dict(positions=positions, triangles=triangles)
    else:
        target, source = dict(positions=ru.corner_cloud()), source[:POINT_MODE_POINTS]
    r = ba.RegisterPoints(source, target, ru.CORNER_R0)                            # the mode by the target's kind
    error = ru.pose_error(r["target_T_source"], truth)
    print(f"mode {mode}: {r['iterations']} steps, {r['reason']}; error {error[0]:.3e} m, {error[1]:.3e} rad; the CPU loop: {CPU_ERROR[mode]}")
    assert r["converged"] and r["reason"] == "converged" and r["iterations"] == len(r["history"]) > 3
    assert r["history"][0]["radius"] == F(ru.CORNER_R0) and r["history"][0]["hits"] == r["history"][0]["used"] == len(source)
    assert r["history"][-1]["step_translation"] < 1e-5 and r["cell_size"] == F(ru.CORNER_R0)
    assert error[0] <= 4 * CPU_ERROR[mode][0] and error[1] <= 4 * CPU_ERROR[mode][1]
    again = ba.RegisterPoints(source, target, ru.CORNER_R0, mode=mode)
    assert np.array_equal(again["target_T_source"], r["target_T_source"]) and again["history"] == r["history"]


def test_register_points_on_a_flat_plane_and_far_away(fused):
    ba = fused[0]
    positions, triangles, _ = ru.flat_plane()
    source = ru.displaced(ru.corner_points(), ru.known_displacement())[:200]
    r = ba.RegisterPoints(source, dict(positions=positions, triangles=triangles), ru.CORNER_R0)
    assert not r["converged"] and "singular" in r["reason"] and np.isfinite(r["target_T_source"]).all()
    assert np.allclose(r["target_T_source"][:3, :3] @ r["target_T_source"][:3, :3].T, np.eye(3), atol=1e-12) and np.array_equal(r["target_T_source"][3], [0, 0, 0, 1])
    far = np.eye(4)
    far[:3, 3] = 50.0
    r = ba.RegisterPoints(source, dict(positions=positions, triangles=triangles), ru.CORNER_R0, initial=far)
    assert not r["converged"] and r["reason"] == "fewer than 6 pairs" and np.array_equal(r["target_T_source"], far) and r["iterations"] == 1
    assert r["history"][0]["used"] == 0 and np.isnan(r["history"][0]["rmse"])
    with pytest.raises(Exception, match="max_grid_entries"):                       # a cell that was asked for is not changed
        ba.RegisterPoints(source, dict(positions=positions, triangles=triangles), ru.CORNER_R0, cell_size=0.01, max_grid_entries=10)
    r = ba.RegisterPoints(source, dict(positions=positions, triangles=triangles), ru.CORNER_R0, max_grid_entries=100)
    assert r["cell_size"] > F(ru.CORNER_R0) and r["grid_entries"] <= 100            # the cell doubled while over budget


# ------------------------------------------------------------------------------------------------
# 6. evaluate(register=True) on the fused scene
# ------------------------------------------------------------------------------------------------
def moved_planes(cam, scene):
    """The analytic planes of tests/test_gpu_surface_eval.py in a frame of their own: moved by MOVED_BY about the volume's centre."""
    from tests.test_gpu_mesh_components import VOLUME_DIMS, VOLUME_ORIGIN
    from tests.test_gpu_surface_eval import plane_ground_truth
    truth = plane_ground_truth(cam, scene)
    centre = np.array(VOLUME_ORIGIN) + 0.01 * np.array(VOLUME_DIMS)
    rng = np.random.default_rng(23)
    t, w = rng.standard_normal(3), rng.standard_normal(3)
    T = ru.se3_exp(np.concatenate([np.zeros(3), MOVED_BY[1] * w / np.linalg.norm(w)]))
    T[:3, 3] = centre - T[:3, :3] @ centre + MOVED_BY[0] * t / np.linalg.norm(t)
    moved = np.ascontiguousarray(truth["positions"].astype(np.float64) @ T[:3, :3].T + T[:3, 3], F)
    return dict(positions=moved, triangles=truth["triangles"]), T


def test_evaluate_with_registration_against_the_moved_planes(fused):
    from badslam_amd import surface_eval
    ba, mesh, scene, cam = fused
    truth, T = moved_planes(cam, scene)
    r = surface_eval.evaluate(ba, mesh, truth, 0.1, (0.01, 0.02, 0.05), register=True)
    reg = r["registration"]
    error = ru.pose_error(np.array(reg["target_T_source"]), T)
    print(f"{reg['iterations']} steps, {reg['reason']}; error {error[0]:.3e} m, {error[1]:.3e} rad; the CPU's accuracy medians: {CPU_UNREGISTERED_ACCURACY_MEDIAN} "
          f"before, {CPU_REGISTERED_ACCURACY_MEDIAN} after")
    print(surface_eval.format_summary("accuracy before", reg["before"]["accuracy"]))
    print(surface_eval.format_summary("accuracy", r["accuracy"]))
    print(surface_eval.format_summary("completeness before", reg["before"]["completeness"]))
    print(surface_eval.format_summary("completeness", r["completeness"]))
    assert r["accuracy"]["count"] == len(mesh["positions"]) and r["completeness"]["count"] == len(truth["positions"])
    assert r["accuracy"]["median"] <= 2 * CPU_REGISTERED_ACCURACY_MEDIAN
    assert r["completeness"]["median"] <= 2 * CPU_REGISTERED_COMPLETENESS_MEDIAN
    assert reg["before"]["accuracy"]["median"] > 2 * CPU_REGISTERED_ACCURACY_MEDIAN
    plain = surface_eval.evaluate(ba, mesh, truth, 0.1, (0.01, 0.02, 0.05))
    assert "registration" not in plain and plain["accuracy"] == reg["before"]["accuracy"] and plain["completeness"] == reg["before"]["completeness"]


# ------------------------------------------------------------------------------------------------
# 7. tools/run_tum.py --register-surface
# ------------------------------------------------------------------------------------------------
def test_run_tum_register_surface(tmp_path):
    """Five frames of the rendered sequence of tests/test_gpu_bad_slam.py; the ground truth is the run's own mesh (--mesh, 4 cm),
    written again moved by a known motion: the report carries the registration, which undoes the motion."""
    from badslam_amd import direct_ba as dba
    from badslam_amd import png
    from tests.test_gpu_bad_slam import render_sequence
    from tools import run_tum
    cam, raw_to_float, frames, gt = render_sequence(5, seed=5)
    source = tmp_path / "source"
    (source / "rgb").mkdir(parents=True)
    (source / "depth").mkdir()
    assoc = []
    for k, (depth, rgb) in enumerate(frames):
        ts = f"{200.0 + 0.1 * k:.6f}"
        png.write_png(source / "rgb" / f"{ts}.png", rgb)
        png.write_png(source / "depth" / f"{ts}.png", depth)
        assoc.append(f"{ts} rgb/{ts}.png {ts} depth/{ts}.png")
    (source / "associated.txt").write_text("\n".join(assoc) + "\n")
    (source / "calibration.txt").write_text(f"{cam.fx} {cam.fy} {cam.cx - 0.5} {cam.cy - 0.5}\n")
    mesh_path, truth_path, report_path = tmp_path / "mesh.ply", tmp_path / "truth.ply", tmp_path / "surface.json"
    options = dict(keyframe_interval=4, ba_iterations=2, max_depth=6.0, num_scales=4, max_surfel_count=400000, mesh_voxel_size=0.04, mesh_min_count=2, mesh_min_component=50)
    first = run_tum.run(source, mesh=mesh_path, **options)
    assert first["mesh"]["vertices"] > 1000 and "surface" not in first
    own = dba.LoadPLY(mesh_path)
    centre = own["positions"].astype(np.float64).mean(axis=0)
    T = ru.se3_exp([0, 0, 0, 0.004, -0.006, 0.005])
    T[:3, 3] = centre - T[:3, :3] @ centre + np.array([0.012, -0.008, 0.01])
    moved = np.ascontiguousarray(own["positions"].astype(np.float64) @ T[:3, :3].T + T[:3, 3], F)
    V = len(moved)
    dba.SaveMeshAsPLY(truth_path, dict(positions=moved, normals=np.zeros((V, 3), F), colors=np.full((V, 4), 255, np.uint8), triangles=own["triangles"]))
    r = run_tum.run(source, ground_truth_surface=truth_path, surface_report=report_path, register_surface=True, **options)
    report = json.loads(report_path.read_text())
    reg = report["registration"]
    error = ru.pose_error(np.array(reg["target_T_source"]), T)
    print(f"{reg['iterations']} steps, {reg['reason']}; error {error[0]:.3e} m, {error[1]:.3e} rad; accuracy median {reg['before']['accuracy']['median']:.5f} -> "
          f"{report['accuracy']['median']:.5f}")
    assert reg["target_T_source"] == r["surface"]["registration"]["target_T_source"] and reg["iterations"] == len(reg["history"]) > 0
    assert report["accuracy"]["count"] == first["mesh"]["vertices"]
    assert report["accuracy"]["median"] < 0.02                                     # half a voxel
    assert reg["before"]["accuracy"]["median"] > report["accuracy"]["median"]
    assert error[0] < 0.02
    a = run_tum.arg_parser().parse_args(["x"])
    assert a.register_surface is False
    assert (a.ground_truth_surface, a.surface_max_distance, a.surface_thresholds, a.surfel_mesh_distance, a.surface_report) == (None, 0.1, (0.01, 0.02, 0.05), False, None)
    assert run_tum.arg_parser().parse_args(["x", "--register-surface"]).register_surface is True
