"""-m gpu: bslam_point_mesh_distance (badslam_amd/csrc/distance_kernels.hpp) against the brute-force restatement of
tests/point_mesh_util.py.  Distance and triangle are compared bit for bit: the grid, the sort and the LDS tiles may change no
result.  Every device array stands between guard words, outputs are filled with a sentinel first and have room beyond N."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from tests import point_mesh_util as pm
from tests.test_gpu_fusion import SENTINEL, bits, stream_ptr
from tests.test_gpu_mesh_components import Guarded

pytestmark = pytest.mark.gpu
F = np.float32
INVALID_ARGUMENT = -1   # BSLAM_ERR_INVALID_ARGUMENT
SPARE = 7               # output words beyond N
SHIFT = np.array([1e4, -1e4, 1e4], F)


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
def extended(sphere):
    """The sphere with a 40 x 40 quad of two large triangles below it, five duplicated triangles, triangles of the forms (i, i, i)
    and (i, i, j) and one with a NaN vertex; the points with NaN and infinite ones, points far outside the grid, points on and one
    ulp outside the dilated bounds (of R = 2), 300 copies of one point and a point alone in its cell."""
    positions, triangles, points = sphere
    V = len(positions)
    quad = np.array([[-4, -5, 1], [36, -5, 1], [36, 35, 1], [-4, 35, 1], [np.nan, 3, 3], [40, 40, 30]], F)
    more = np.array([[V, V + 1, V + 2], [V, V + 2, V + 3], [7, 7, 7], [V + 5, V + 5, V + 5], [9, 9, 300], [V + 5, V + 5, 100], [V + 4, 0, 1], [2, V + 4, V + 4]], np.uint32)
    mesh_positions = np.concatenate([positions, quad])
    mesh_triangles = np.concatenate([triangles[:1000], triangles[200:205], triangles[1000:], more, triangles[3000:3001]])
    R = F(2.0)
    lo, hi = F(-4) - R, F(40) + R
    below, above = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
    special = np.array([[np.nan, 15, 15], [16, np.nan, 14], [16, 15, np.nan], [np.inf, 15, 15], [16, -np.inf, 14], [np.nan, np.nan, np.nan],
                        [1e6, 0, 0], [-1e30, 1e30, 0], [16, 15, -500], [3e38, 3e38, 3e38],
                        [lo, 15, 1.5], [below, 15, 1.5], [hi, 39, 29], [above, 39, 29], [10, 10, F(1) + R], [10, 10, np.nextafter(F(1) + R, F(np.inf))],
                        [10, 10, F(1) - R], [10, 10, np.nextafter(F(1) - R, F(-np.inf))], [-3, -4, 1.2], [41, 41, 31]], F)
    mesh_points = np.concatenate([points, special, np.repeat(points[5:6], 300, axis=0), points[600:620]])
    return np.ascontiguousarray(mesh_positions, F), np.ascontiguousarray(mesh_triangles, np.uint32), np.ascontiguousarray(mesh_points, F)


_wanted = {}


def wanted(name, points, positions, triangles, R):
    """The restatement's answer, computed once per (inputs, R) and never changed."""
    key = (name, float(R))
    if key not in _wanted:
        _wanted[key] = pm.point_mesh_distance(points, positions, triangles, R)
    return _wanted[key]


def call(gpu, points, positions, triangles, R, cell, budget=1 << 28, with_triangle=True):
    """-> (rc, distance [N], triangle [N] or None, cells, entries); asserts that the inputs, the guard words and the outputs beyond N
    are untouched."""
    torch, L, ctx = gpu
    points, positions = np.ascontiguousarray(points, F).reshape(-1, 3), np.ascontiguousarray(positions, F).reshape(-1, 3)
    triangles = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    N, V, T = len(points), len(positions), len(triangles)
    ins = [Guarded(torch, 3 * N, points), Guarded(torch, 3 * V, positions), Guarded(torch, 3 * T, triangles)]
    before = [b.read() for b in ins]
    out_d, out_t = Guarded(torch, N + SPARE), Guarded(torch, N + SPARE) if with_triangle else None
    cells, entries = C.c_uint64(SENTINEL), C.c_uint64(SENTINEL)
    rc = L.bslam_point_mesh_distance(ctx.handle, stream_ptr(torch), N, ins[0].ptr, V, ins[1].ptr, T, ins[2].ptr, float(R), float(cell), budget, out_d.ptr,
                                     out_t.ptr if with_triangle else None, C.byref(cells), C.byref(entries))
    for b, was in zip(ins, before):
        assert np.array_equal(b.read(), was), "an input was written to"
    d, t = out_d.read(), out_t.read() if with_triangle else None
    assert (d[N:] == SENTINEL).all() and (t is None or (t[N:] == SENTINEL).all()), "written beyond N"
    return rc, d[:N].view(F), None if t is None else t[:N], cells.value, entries.value


def assert_equal(got_d, got_t, want, what=""):
    want_d, want_t = want
    differ = bits(got_d) != bits(want_d)
    assert not differ.any(), f"{what}: {int(differ.sum())} distances differ, first at {np.flatnonzero(differ)[0]}: {got_d[differ][0]!r} for {want_d[differ][0]!r}"
    if got_t is not None:
        differ = got_t != want_t
        assert not differ.any(), f"{what}: {int(differ.sum())} triangles differ, first at {np.flatnonzero(differ)[0]}: {got_t[differ][0]} for {want_t[differ][0]}"


# ------------------------------------------------------------------------------------------------
# 1. the case matrix
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifted", [False, True], ids=["at the origin", "shifted by 1e4"])
@pytest.mark.parametrize("cell", ["R / 2", "R", "3.7 R", "1000"])
@pytest.mark.parametrize("R", [2.0, 0.6])
def test_sphere(gpu, sphere, R, cell, shifted):
    positions, triangles, points = sphere
    if shifted:
        positions, points = (positions + SHIFT).astype(F), (points + SHIFT).astype(F)
    want = wanted("sphere shifted" if shifted else "sphere", points, positions, triangles, R)
    assert 100 < np.isfinite(want[0]).sum() < 600
    cell_size = {"R / 2": F(R) / F(2), "R": F(R), "3.7 R": F(3.7) * F(R), "1000": F(1000)}[cell]
    rc, d, t, cells, entries = call(gpu, points, positions, triangles, R, cell_size)
    badslam_amd.check(rc)
    assert_equal(d, t, want, f"R {R} cell {cell}")
    assert (cells, entries) == pm.grid_census(positions, triangles, R, cell_size)
    if cell == "1000":
        assert (cells, entries) == (1, len(triangles))              # one list, longer than any LDS tile


@pytest.mark.parametrize("cell", ["R / 2", "R", "1000"])
@pytest.mark.parametrize("R", [2.0, 0.6])
def test_extended_mesh_and_points(gpu, extended, R, cell):
    positions, triangles, points = extended
    want = wanted("extended", points, positions, triangles, R)
    assert np.isinf(want[0][680:690]).all()                         # NaN, infinite and far points miss
    cell_size = {"R / 2": F(R) / F(2), "R": F(R), "1000": F(1000)}[cell]
    rc, d, t, cells, entries = call(gpu, points, positions, triangles, R, cell_size)
    badslam_amd.check(rc)
    assert_equal(d, t, want, f"R {R} cell {cell}")
    assert (cells, entries) == pm.grid_census(positions, triangles, R, cell_size)
    if R == 2.0:
        # on the dilated bounds: a candidate exists; one ulp outside: outside the grid.  Exactly R above and below the quad: a hit
        # at distance R; one ulp further: a miss
        assert d[694] == F(2.0) and d[696] == F(2.0) and np.isinf(d[[691, 693, 695, 697]]).all()
        assert (t[680 + 20:680 + 320] == t[5]).all() and bits(d[700:1000]).max() == bits(d[700:1000]).min() == bits(d[5:6])[0]


def test_duplicates_and_degenerate_triangles_take_the_lowest_index(gpu, extended):
    positions, triangles, points = extended
    V = 1774
    want_d, want_t = wanted("extended", points, positions, triangles, 2.0)
    rc, d, t, _, _ = call(gpu, points, positions, triangles, 2.0, 2.0)
    badslam_amd.check(rc)
    assert_equal(d, t, (want_d, want_t))
    tri = triangles.astype(np.int64)
    assert (np.bincount(t[t != pm.NO_TRIANGLE], minlength=len(tri))[1000:1005] == 0).all()       # a duplicate never wins over its original
    point_like = np.flatnonzero((tri[:, 0] == tri[:, 1]) & (tri[:, 1] == tri[:, 2]))
    assert len(point_like) == 2 and t[699] == point_like[1] and d[699] == np.sqrt(F(3.0))      # (41, 41, 31) is nearest to the lone vertex (40, 40, 30)
    nan_triangles = np.flatnonzero((tri == V + 4).any(axis=1))
    assert len(nan_triangles) == 2 and not np.isin(t, nan_triangles).any()


def test_point_cloud_form(gpu):
    rng = np.random.default_rng(3)
    cloud = rng.uniform(-1, 1, (3000, 3)).astype(F)
    points = rng.uniform(-1.2, 1.2, (1500, 3)).astype(F)
    tri = np.repeat(np.arange(len(cloud), dtype=np.uint32)[:, None], 3, axis=1)
    want = pm.point_mesh_distance(points, cloud, tri, 0.1)
    assert 300 < np.isfinite(want[0]).sum() < 1400
    for cell in (0.05, 0.1, 0.3):
        rc, d, t, _, _ = call(gpu, points, cloud, tri, 0.1, cell)
        badslam_amd.check(rc)
        assert_equal(d, t, want, f"cell {cell}")


# ------------------------------------------------------------------------------------------------
# 2. the call
# ------------------------------------------------------------------------------------------------
def test_without_out_triangle_and_two_calls_agree(gpu, sphere):
    positions, triangles, points = sphere
    want = wanted("sphere", points, positions, triangles, 2.0)
    rc, d, t, _, _ = call(gpu, points, positions, triangles, 2.0, 1.0, with_triangle=False)
    badslam_amd.check(rc)
    assert t is None
    assert_equal(d, None, want)
    first, second = call(gpu, points, positions, triangles, 2.0, 1.0), call(gpu, points, positions, triangles, 2.0, 1.0)
    assert first[0] == second[0] == 0 and np.array_equal(bits(first[1]), bits(second[1])) and np.array_equal(first[2], second[2])


def test_empty_inputs(gpu, sphere):
    positions, triangles, points = sphere
    none3, no_triangles = np.zeros((0, 3), F), np.zeros((0, 3), np.uint32)
    rc, d, t, cells, entries = call(gpu, none3, positions, triangles, 2.0, 2.0)                   # N = 0
    assert rc == 0 and len(d) == 0 and (cells, entries) == pm.grid_census(positions, triangles, 2.0, 2.0)
    for pos in (positions, none3):                                                                # T = 0, and V = 0 with it
        rc, d, t, cells, entries = call(gpu, points, pos, no_triangles, 2.0, 2.0)
        assert rc == 0 and np.isinf(d).all() and (d > 0).all() and (t == pm.NO_TRIANGLE).all() and (cells, entries) == (0, 0)
    rc, d, t, cells, entries = call(gpu, none3, none3, no_triangles, 2.0, 2.0)
    assert rc == 0
    # no valid triangle at all
    rc, d, t, cells, entries = call(gpu, points, np.full((3, 3), np.nan, F), np.array([[0, 1, 2]], np.uint32), 2.0, 2.0)
    assert rc == 0 and np.isinf(d).all() and (t == pm.NO_TRIANGLE).all() and (cells, entries) == (0, 0)


def test_budget(gpu, sphere):
    torch, L, ctx = gpu
    positions, triangles, points = sphere
    cells, entries = pm.grid_census(positions, triangles, 2.0, 1.0)
    rc, d, t, got_cells, got_entries = call(gpu, points, positions, triangles, 2.0, 1.0, budget=entries)
    assert rc == 0 and (got_cells, got_entries) == (cells, entries)
    rc, d, t, got_cells, got_entries = call(gpu, points, positions, triangles, 2.0, 1.0, budget=entries - 1)
    message = L.bslam_last_error()
    assert rc == INVALID_ARGUMENT and str(entries).encode() in message and str(cells).encode() in message, message
    assert (got_cells, got_entries) == (cells, entries)
    assert (bits(d) == SENTINEL).all() and (t == SENTINEL).all(), "a refused call wrote to an output"
    # a few huge triangles under a tiny cell: refused by the cap on the cells, before anything is built
    big = np.array([[0, 0, 0], [1e4, 0, 0], [0, 1e4, 1e4]], F)
    rc, d, t, _, _ = call(gpu, points, big, np.array([[0, 1, 2]], np.uint32), 0.01, 0.01)
    assert rc == INVALID_ARGUMENT and b"cells" in L.bslam_last_error() and (bits(d) == SENTINEL).all()
    rc, d, t, _, _ = call(gpu, points, positions, triangles, 2.0, 1.0)                            # the context is fine afterwards
    assert rc == 0
    assert_equal(d, t, wanted("sphere", points, positions, triangles, 2.0))


@pytest.mark.parametrize("bad", ["V", "0xFFFFFFFF"])
def test_an_index_beyond_the_vertices_is_refused(gpu, sphere, bad):
    torch, L, ctx = gpu
    positions, triangles, points = sphere
    tri = triangles.copy()
    tri[1777, 2] = len(positions) if bad == "V" else 0xFFFFFFFF
    rc, d, t, _, _ = call(gpu, points, positions, tri, 2.0, 2.0)
    assert rc == INVALID_ARGUMENT and b"beyond vertex_count" in L.bslam_last_error()
    assert (bits(d) == SENTINEL).all() and (t == SENTINEL).all()
    rc, d, t, _, _ = call(gpu, points, np.zeros((0, 3), F), tri[:1], 2.0, 2.0)                    # no vertex at all: every index is beyond
    assert rc == INVALID_ARGUMENT


def test_rejected_arguments(gpu, sphere):
    torch, L, ctx = gpu
    positions, triangles, points = sphere
    N, V, T = len(points), len(positions), len(triangles)
    b = dict(points=Guarded(torch, 3 * N, points), positions=Guarded(torch, 3 * V, positions), indices=Guarded(torch, 3 * T, triangles),
             out_distance=Guarded(torch, N), out_triangle=Guarded(torch, N))
    cells, entries = C.c_uint64(SENTINEL), C.c_uint64(SENTINEL)
    base = dict(ctx=ctx.handle, R=2.0, cell=1.0, budget=1 << 28, **{k: v.address for k, v in b.items()})

    def run(**changes):
        a = dict(base, **changes)
        p = lambda v: None if v is None else C.c_void_p(v)
        return L.bslam_point_mesh_distance(a["ctx"], stream_ptr(torch), N, p(a["points"]), V, p(a["positions"]), T, p(a["indices"]), a["R"], a["cell"], a["budget"],
                                           p(a["out_distance"]), p(a["out_triangle"]), C.byref(cells), C.byref(entries))

    a = base
    cases = {"null context": dict(ctx=None), "null points": dict(points=None), "null positions": dict(positions=None), "null indices": dict(indices=None),
             "null out_distance": dict(out_distance=None), "misaligned points": dict(points=a["points"] + 2), "misaligned positions": dict(positions=a["positions"] + 1),
             "misaligned indices": dict(indices=a["indices"] + 2), "misaligned out_distance": dict(out_distance=a["out_distance"] + 2),
             "misaligned out_triangle": dict(out_triangle=a["out_triangle"] + 3), "in place: points": dict(out_distance=a["points"]),
             "out_distance inside positions": dict(out_distance=a["positions"] + 12 * V - 4), "out_triangle inside indices": dict(out_triangle=a["indices"] + 8),
             "the outputs overlap": dict(out_triangle=a["out_distance"] + 4 * N - 4), "the outputs are one": dict(out_triangle=a["out_distance"]),
             "R = 0": dict(R=0.0), "R < 0": dict(R=-1.0), "R = inf": dict(R=float("inf")), "R = NaN": dict(R=float("nan")),
             "cell = 0": dict(cell=0.0), "cell < 0": dict(cell=-0.5), "cell = inf": dict(cell=float("inf")), "cell = NaN": dict(cell=float("nan")),
             "no budget": dict(budget=0)}
    for name, changes in cases.items():
        rc = run(**changes)
        assert rc == INVALID_ARGUMENT, (name, rc, L.bslam_last_error())
    torch.cuda.synchronize()
    assert (b["out_distance"].read() == SENTINEL).all() and (b["out_triangle"].read() == SENTINEL).all(), "a refused call wrote to an output"
    assert np.array_equal(b["points"].read(), bits(points).reshape(-1))
    assert run() == 0
    assert_equal(b["out_distance"].read().view(F), b["out_triangle"].read(), wanted("sphere", points, positions, triangles, 2.0))
    assert run(points=a["positions"]) in (0, INVALID_ARGUMENT) and run(out_triangle=None) == 0   # two inputs may share memory: only outputs are exclusive


def test_profiling_counts_offered_and_evaluated_pairs(gpu, sphere):
    torch, L, ctx = gpu
    positions, triangles, points = sphere
    tested, culled = C.c_uint64(), C.c_uint64()
    valid, lo, hi = pm.dilated_boxes(positions, triangles, 2.0)
    candidates = int(((points[:, None, :] >= lo[None]) & (points[:, None, :] <= hi[None])).all(-1).sum())
    try:
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
        badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))     # reset
        rc, d, t, _, _ = call(gpu, points, positions, triangles, 2.0, 2.0)
        badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))
        offered, evaluated = tested.value, tested.value - culled.value
        rc0, d0, t0, _, _ = call(gpu, points, positions, np.zeros((0, 3), np.uint32), 2.0, 2.0)
        badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))
    finally:
        L.bslam_profile_enable(ctx.handle, 0)
    assert rc == 0 and rc0 == 0
    assert_equal(d, t, wanted("sphere", points, positions, triangles, 2.0))
    print(f"{offered} pairs offered, {evaluated} evaluated, of {len(points) * len(triangles)}")
    assert offered >= evaluated > 0 and evaluated == candidates and offered < len(points) * len(triangles)
    assert (tested.value, culled.value) == (0, 0)


def test_scratch_carving_at_its_boundaries():
    """The mesh calls and this one carve their scratch out of slabs that only grow.  On one fresh context: bslam_mesh_components and
    bslam_filter_mesh (min_vertices 2) on strips with isolated vertices of (V, T) around the padding to 64 elements, from the largest
    to the smallest and back up, then this call on 7 triangles, 9 vertices and 13, then 5 points in a grid of 54 cells (54, 55,
    the 174 entries, 13 and 5: no multiple of four) -- so a slab reserved for a larger call is carved for a smaller one and grown
    again.  Every output equals the restatements of tests/mesh_components_util.py and tests/point_mesh_util.py exactly."""
    import torch
    from tests import mesh_components_util as mu
    from tests.test_gpu_mesh_components import assert_components_equal, assert_filtered_equal, gpu_components, gpu_filter
    gpu = (torch, badslam_amd.lib(), badslam_amd.Context(0))
    rng = np.random.default_rng(41)
    shapes = [(129, 127), (65, 1), (64, 62), (63, 61), (1, 0)]
    for V, T in shapes + shapes[-2::-1]:
        i = np.arange(T, dtype=np.uint32)
        triangles = np.stack([i, i + 1, i + 2], -1).reshape(T, 3)          # a strip on the first T + 2 vertices; the rest is isolated
        positions, normals = rng.normal(size=(V, 3)).astype(F), rng.normal(size=(V, 3)).astype(F)
        colors = rng.integers(0, 256, (V, 4), dtype=np.uint8)
        want = mu.components(V, triangles)
        assert want[2] == (V - T - 1 if T else V)
        got = gpu_components(gpu, V, triangles)
        assert_components_equal(got, want)
        assert_filtered_equal(gpu_filter(gpu, positions, normals, colors, triangles, got[1], 2), want[1], 2, positions, normals, colors, triangles)
    i = np.arange(9)
    positions = np.stack([0.5 * i, (i % 2) * 1.0, 0.1 * i], -1).astype(F)
    triangles = np.stack([i[:7], i[:7] + 1, i[:7] + 2], -1).astype(np.uint32)
    points = (rng.uniform(-0.5, 1.5, (13, 3)) * np.array([3.0, 1.0, 0.8])).astype(F)
    assert pm.grid_census(positions, triangles, 0.6, 0.9) == (54, 174)
    for N in (13, 5):
        want = pm.point_mesh_distance(points[:N], positions, triangles, 0.6)
        assert np.isfinite(want[0]).any() and np.isinf(want[0]).any()
        rc, d, t, cells, entries = call(gpu, points[:N], positions, triangles, 0.6, 0.9)
        assert (rc, cells, entries) == (0, 54, 174)
        assert_equal(d, t, want, f"{N} points")
