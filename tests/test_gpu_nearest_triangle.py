"""-m gpu: bslam_nearest_triangle (badslam_amd/csrc/bvh_kernels.hpp) against the brute-force restatement of
tests/nearest_triangle_util.py.  Distance and triangle are compared bit for bit: the tree, the sort and the traversal may change no
result.  The tree itself is read back and checked, box by box.  Every device array stands between guard words, outputs are filled
with a sentinel first and have room beyond N."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from tests import nearest_triangle_util as nt
from tests import point_mesh_util as pm
from tests.test_gpu_fusion import SENTINEL, bits, stream_ptr
from tests.test_gpu_mesh_components import Guarded

pytestmark = pytest.mark.gpu
F = np.float32
INF = float("inf")
INVALID_ARGUMENT = -1   # BSLAM_ERR_INVALID_ARGUMENT
SPARE = 7               # output words beyond N


@pytest.fixture(scope="module")
def gpu():
    import torch
    from badslam_amd import build
    build.build()
    return torch, badslam_amd.lib(), badslam_amd.Context(0)


@pytest.fixture(scope="module")
def sphere():
    positions, triangles = pm.sphere_mesh()
    return positions, triangles, pm.sphere_points(positions, triangles)


@pytest.fixture(scope="module")
def plane():
    positions, triangles = nt.plane_mesh()
    return positions, triangles, nt.plane_points()


@pytest.fixture(scope="module")
def repeated():
    """One triangle 200 times, behind one and in front of two others: equal keys, a subtree split by the index alone."""
    positions = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [3, 3, 3], [4, 3, 3], [3, 4, 3], [-2, -2, 1], [-1, -2, 1], [-2, -1, 1], [0, 0, 2], [1, 0, 2], [0, 1, 2]], F)
    triangles = np.array([[3, 4, 5]] + [[0, 1, 2]] * 200 + [[6, 7, 8], [9, 10, 11]], np.uint32)
    points = np.ascontiguousarray(np.random.default_rng(11).uniform(-3, 5, (150, 3)), F)
    return positions, triangles, points


@pytest.fixture(scope="module")
def two_spheres(sphere):
    """Two copies of the sphere 1e4 units apart: the quantisation collapses each into a few cells.  Points near each and midway."""
    positions, triangles, points = sphere
    shift = np.array([1e4, 0, 0], F)
    both = np.concatenate([positions, (positions + shift).astype(F)])
    index = np.concatenate([triangles, triangles + np.uint32(len(positions))])
    middle = (np.array(pm.SPHERE_CENTRE, F) + F(0.5) * shift + np.random.default_rng(5).uniform(-40, 40, (20, 3))).astype(F)
    query = np.concatenate([points[::8], (points[3::8] + shift).astype(F), middle, (np.array(pm.SPHERE_CENTRE, F) + F(0.5) * shift)[None]])
    return np.ascontiguousarray(both, F), np.ascontiguousarray(index, np.uint32), np.ascontiguousarray(query, F)


_wanted = {}


def wanted(name, points, positions, triangles, R=INF):
    """The restatement's answer, computed once per (inputs, R) and never changed."""
    key = (name, float(R))
    if key not in _wanted:
        _wanted[key] = nt.nearest_triangle(points, positions, triangles, R)
    return _wanted[key]


def call(gpu, points, positions, triangles, R=INF, with_triangle=True):
    """-> (rc, distance [N], triangle [N] or None, leaves, height); asserts that the inputs, the guard words and the outputs beyond N
    are untouched."""
    torch, L, ctx = gpu
    points, positions = np.ascontiguousarray(points, F).reshape(-1, 3), np.ascontiguousarray(positions, F).reshape(-1, 3)
    triangles = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    N, V, T = len(points), len(positions), len(triangles)
    ins = [Guarded(torch, 3 * N, points), Guarded(torch, 3 * V, positions), Guarded(torch, 3 * T, triangles)]
    before = [b.read() for b in ins]
    out_d, out_t = Guarded(torch, N + SPARE), Guarded(torch, N + SPARE) if with_triangle else None
    leaves, height = C.c_uint32(SENTINEL), C.c_uint32(SENTINEL)
    rc = L.bslam_nearest_triangle(ctx.handle, stream_ptr(torch), N, ins[0].ptr, V, ins[1].ptr, T, ins[2].ptr, float(R), out_d.ptr,
                                  out_t.ptr if with_triangle else None, C.byref(leaves), C.byref(height))
    for b, was in zip(ins, before):
        assert np.array_equal(b.read(), was), "an input was written to"
    d, t = out_d.read(), out_t.read() if with_triangle else None
    assert (d[N:] == SENTINEL).all() and (t is None or (t[N:] == SENTINEL).all()), "written beyond N"
    return rc, d[:N], None if t is None else t[:N], leaves.value, height.value


def assert_equal(got_d, got_t, want, what=""):
    want_d, want_t = want
    got_d = got_d.view(F)
    differ = bits(got_d) != bits(want_d)
    assert not differ.any(), f"{what}: {int(differ.sum())} distances differ, first at {np.flatnonzero(differ)[0]}: {got_d[differ][0]!r} for {want_d[differ][0]!r}"
    if got_t is not None:
        differ = got_t != want_t
        assert not differ.any(), f"{what}: {int(differ.sum())} triangles differ, first at {np.flatnonzero(differ)[0]}: {got_t[differ][0]} for {want_t[differ][0]}"


def read_tree(gpu):
    """The tree of the last call, in the form nt.check_tree takes."""
    _, L, ctx = gpu
    leaves = C.c_uint32(SENTINEL)
    badslam_amd.check(L.bslam_debug_nearest_triangle_tree(ctx.handle, 0, None, None, None, None, C.byref(leaves)))
    n = leaves.value
    tree = dict(leaves=n, parent=np.full(max(2 * n - 1, 0), SENTINEL, np.uint32), children=np.full(max(2 * (n - 1), 0), SENTINEL, np.uint32),
                boxes=np.full((max(2 * n - 1, 0), 6), np.nan, F), leaf_triangle=np.full(n, SENTINEL, np.uint32))
    if n:
        badslam_amd.check(L.bslam_debug_nearest_triangle_tree(ctx.handle, n, tree["parent"].ctypes.data, tree["children"].ctypes.data, tree["boxes"].ctypes.data,
                                                              tree["leaf_triangle"].ctypes.data, C.byref(leaves)))
        assert leaves.value == n
    return tree


def run_case(gpu, name, points, positions, triangles, R=INF, tree=False):
    """The call against the restatement; with `tree`, the tree through the checker and the height the call reported."""
    rc, d, t, leaves, height = call(gpu, points, positions, triangles, R)
    badslam_amd.check(rc)
    want = wanted(name, points, positions, triangles, R)
    assert_equal(d, t, want, name)
    assert leaves == int(nt.triangle_boxes(positions, triangles)[0].sum())
    assert height <= nt.HEIGHT_BOUND
    if tree:
        assert nt.check_tree(read_tree(gpu), positions, triangles) == height
    return want


# ------------------------------------------------------------------------------------------------
# 1, 2, 12. the sphere and the plane, and their trees
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [INF, 1.0])
def test_sphere(gpu, sphere, R):
    positions, triangles, points = sphere
    want_d, _ = run_case(gpu, "sphere", points, positions, triangles, R, tree=R == INF)
    assert int(np.isfinite(want_d).sum()) == (680 if R == INF else 265)      # at R = 1 the misses are part of the comparison


def test_sphere_equals_the_grid_call(gpu, sphere):
    positions, triangles, points = sphere
    torch, L, ctx = gpu
    want = run_case(gpu, "sphere", points, positions, triangles, 3.0)
    N, V, T = len(points), len(positions), len(triangles)
    ins = [Guarded(torch, 3 * N, points), Guarded(torch, 3 * V, positions), Guarded(torch, 3 * T, triangles)]
    out_d, out_t = Guarded(torch, N), Guarded(torch, N)
    badslam_amd.check(L.bslam_point_mesh_distance(ctx.handle, stream_ptr(torch), N, ins[0].ptr, V, ins[1].ptr, T, ins[2].ptr, 3.0, 3.0, 1 << 28, out_d.ptr, out_t.ptr,
                                                  None, None))
    assert_equal(out_d.read(), out_t.read(), want, "the grid at R = 3")
    assert int(np.isfinite(want[0]).sum()) == 678


def test_plane(gpu, plane):
    positions, triangles, points = plane
    want_d, want_t = run_case(gpu, "plane", points, positions, triangles, tree=True)
    unclamped = pm.point_mesh_distance(points, positions, triangles, np.inf)[0]
    assert (bits(want_d) != bits(unclamped)).any(), "the clamp is meant to be active on this fixture"
    run_case(gpu, "plane", points, positions, triangles, 0.8)


# ------------------------------------------------------------------------------------------------
# 3, 4, 5, 6, 7. small and degenerate trees
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2])
def test_one_and_two_triangles(gpu, plane, T):
    positions, triangles, points = plane
    run_case(gpu, f"first {T}", points, positions, triangles[:T], tree=True)
    _, _, _, leaves, height = call(gpu, points[:5], positions, triangles[:T])
    assert (leaves, height) == (T, T - 1)                                      # no internal node, then one


def test_repeated_triangle(gpu, repeated):
    positions, triangles, points = repeated
    _, want_t = run_case(gpu, "repeated", points, positions, triangles, tree=True)
    assert not ((want_t >= 2) & (want_t <= 200)).any() and (want_t == 1).sum() > 20     # of the 200 copies, the lowest index


def test_point_cloud(gpu):
    rng = np.random.default_rng(23)
    positions = np.ascontiguousarray(rng.uniform(-2, 2, (500, 3)), F)
    triangles = np.repeat(np.arange(500, dtype=np.uint32)[:, None], 3, axis=1)
    points = np.ascontiguousarray(np.concatenate([rng.uniform(-3, 3, (200, 3)), positions[:10]]), F)
    want_d, want_t = run_case(gpu, "cloud", points, positions, triangles)
    assert (want_d[200:] == 0).all() and np.array_equal(want_t[200:], np.arange(10))
    run_case(gpu, "cloud", points, positions, triangles, 0.3)


def test_two_spheres_far_apart(gpu, two_spheres):
    positions, triangles, points = two_spheres
    want_d, want_t = run_case(gpu, "two spheres", points, positions, triangles, tree=True)
    T = len(triangles) // 2
    assert (want_t[:85] < T).all() and (want_t[85:170] >= T).all() and want_d[170:].min() > 4000


def test_ties_go_to_the_lowest_index(gpu):
    """Four triangles fanned around a centre, queried from the axis above it: all four are at the same distance."""
    positions = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], F)
    fan = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]], np.uint32)
    points = np.array([[0, 0, 1], [0, 0, -2.5], [0, 0, 0]], F)
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):
        triangles = fan[order]
        want_d, want_t = run_case(gpu, f"fan {order}", points, positions, triangles)
        values = nt.pair_values(points, positions, triangles)
        assert (values == values[:, :1]).all(), "the fixture is meant to tie"
        assert (want_t == 0).all() and np.array_equal(want_d, np.array([1, 2.5, 0], F))


# ------------------------------------------------------------------------------------------------
# 8, 9, 10. what is not valid
# ------------------------------------------------------------------------------------------------
def test_invalid_triangles_are_never_returned(gpu, sphere):
    positions, triangles, points = sphere
    positions, triangles = positions.copy(), triangles[:100].copy()
    V = len(positions)
    positions = np.concatenate([positions, np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf]], F)])
    bad = [3, 17, 40, 41, 99]
    triangles[bad, [0, 1, 2, 0, 1]] = [V, V + 1, V + 2, V + 1, V]
    want_d, want_t = run_case(gpu, "five invalid", points[:200], positions, triangles, tree=True)
    assert np.isfinite(want_d).all() and not np.isin(want_t, bad).any()
    # a point in the plane of an invalid triangle's finite corners still goes elsewhere
    triangles[:, 0] = V
    rc, d, t, leaves, height = call(gpu, points[:200], positions, triangles)
    badslam_amd.check(rc)
    assert (leaves, height) == (0, 0) and np.isinf(d.view(F)).all() and (t == nt.NO_TRIANGLE).all()
    assert read_tree(gpu)["leaves"] == 0


def test_invalid_and_distant_points(gpu, sphere):
    positions, triangles, _ = sphere
    points = np.array([[np.nan, 15, 15], [16, np.nan, 14], [16, 15, np.nan], [np.inf, 15, 15], [16, -np.inf, 14], [np.nan, np.nan, np.nan],
                       [1e6, 0, 0], [-3e5, 7e5, 1e6], [16, 15, 14], [3e38, -3e38, 3e38]], F)
    want_d, want_t = run_case(gpu, "special points", points, positions, triangles)
    assert np.isinf(want_d[:6]).all() and (want_t[:6] == nt.NO_TRIANGLE).all()
    assert np.isfinite(want_d[6:9]).all() and want_d[6] > 9e5                  # a point at 1e6 still hits without a radius
    run_case(gpu, "special points", points, positions, triangles, 50.0)


def test_arguments(gpu, sphere):
    positions, triangles, points = sphere
    beyond = triangles[:50].copy()
    beyond[31, 2] = len(positions)
    rc, d, t, _, _ = call(gpu, points[:9], positions, beyond)
    assert rc == INVALID_ARGUMENT and b"beyond vertex_count" in gpu[1].bslam_last_error()
    assert (d == SENTINEL).all() and (t == SENTINEL).all(), "outputs touched by a refused call"
    for R in (0.0, -1.0, float("nan"), -INF):
        assert call(gpu, points[:9], positions, triangles, R)[0] == INVALID_ARGUMENT
    rc, d, t, leaves, _ = call(gpu, points[:0], positions, triangles)
    assert rc == 0 and leaves == len(triangles)
    rc, d, t, leaves, height = call(gpu, points[:9], positions, triangles[:0])
    assert rc == 0 and (leaves, height) == (0, 0) and np.isinf(d.view(F)).all() and (t == nt.NO_TRIANGLE).all()
    rc, d, t, _, _ = call(gpu, points[:9], positions, triangles, with_triangle=False)
    assert rc == 0 and t is None
    assert_equal(d, None, (wanted("sphere", points, positions, triangles)[0][:9], None))


# ------------------------------------------------------------------------------------------------
# 11. the order of the triangles, and of execution
# ------------------------------------------------------------------------------------------------
def test_triangle_order_and_repeat(gpu, sphere):
    positions, triangles, points = sphere
    want_d, want_t = wanted("sphere", points, positions, triangles)
    permutation = np.random.default_rng(41).permutation(len(triangles))
    rc, d, t, _, _ = call(gpu, points, positions, triangles[permutation])
    badslam_amd.check(rc)
    assert np.array_equal(d, bits(want_d))
    values = nt.pair_values(points, positions, triangles)
    unique = (values == values.min(axis=1, keepdims=True)).sum(axis=1) == 1
    assert unique.sum() > 500
    assert np.array_equal(permutation[t[unique]], want_t[unique])
    again = call(gpu, points, positions, triangles[permutation])
    assert np.array_equal(again[1], d) and np.array_equal(again[2], t)


# ------------------------------------------------------------------------------------------------
# 13. above the kernels
# ------------------------------------------------------------------------------------------------
def test_direct_ba_and_surface_eval(sphere):
    from badslam_amd import abi, surface_eval
    from badslam_amd.direct_ba import DirectBA
    positions, triangles, points = sphere
    cam = abi.Camera4f(131.25, 131.25, 80.0, 60.0, 160, 120)
    ba = DirectBA(1000, 1.0 / 5000.0, 40.0, 4, 0.8, 1, 1, 1, cam, cam, 0, True, False)   # no keyframe: the mesh calls need none
    mesh = dict(positions=positions, triangles=triangles)
    got = ba.NearestTriangle(points, mesh)
    assert_equal(got["distance"], got["triangle"], wanted("sphere", points, positions, triangles), "DirectBA.NearestTriangle")
    assert got["leaves"] == len(triangles) and 0 < got["height"] <= nt.HEIGHT_BOUND
    got = ba.NearestTriangle(points, mesh, max_distance=1.0)
    assert_equal(got["distance"], got["triangle"], wanted("sphere", points, positions, triangles, 1.0), "DirectBA.NearestTriangle at R = 1")
    cloud = ba.NearestTriangle(points[:50], dict(positions=positions[:300]))
    as_triangles = np.repeat(np.arange(300, dtype=np.uint32)[:, None], 3, axis=1)
    assert_equal(cloud["distance"], cloud["triangle"], nt.nearest_triangle(points[:50], positions[:300], as_triangles), "a point cloud")
    # the sphere against a copy scaled by 1.05 about its centre: the surfaces are 0.05 radii apart, up to the tessellation
    grown = dict(positions=nt.scaled_about(positions, pm.SPHERE_CENTRE, 1.05), triangles=triangles)
    forth = nt.nearest_triangle(grown["positions"], positions, triangles)[0].astype(np.float64)
    back = nt.nearest_triangle(positions, grown["positions"], triangles)[0].astype(np.float64)
    gap = 0.05 * pm.SPHERE_RADIUS
    tessellation = max(np.abs(forth - gap).max(), np.abs(back - gap).max())
    assert tessellation < 0.5 * gap, "the fixture is meant to be finely tessellated"
    result = surface_eval.evaluate(ba, grown, mesh, max_distance=None, thresholds=(0.25, 0.5, 1.0))
    assert result["max_distance"] is None and "accuracy_grid" not in result
    assert result["accuracy"]["beyond"] == 0 and result["completeness"]["beyond"] == 0
    assert result["accuracy"]["hits"] == len(positions) and result["accuracy"]["within"][2] == 1.0
    assert result["accuracy"]["mean"] == pytest.approx(forth.mean(), rel=1e-12) and result["completeness"]["mean"] == pytest.approx(back.mean(), rel=1e-12)
    dev = surface_eval.deviation(ba, grown, mesh)
    assert dev["mesh_to_reference"]["max"] == forth.max() and dev["reference_to_mesh"]["max"] == back.max()
    assert abs(dev["mesh_to_reference"]["max"] - gap) <= tessellation and abs(dev["reference_to_mesh"]["max"] - gap) <= tessellation
    assert dev["hausdorff"] == max(forth.max(), back.max())
    assert dev["mesh_to_reference"]["mean"] == pytest.approx(forth.mean(), rel=1e-12) and dev["mesh_to_reference"]["rmse"] == pytest.approx(np.sqrt((forth ** 2).mean()), rel=1e-12)
    sampled = surface_eval.deviation(ba, grown, mesh, sample_density=2.0, sample_seed=3)
    assert sampled["sampling"]["mesh_samples"] == sampled["mesh_to_reference"]["count"] > 1000 and np.isfinite(sampled["hausdorff"])
    ba.close()
