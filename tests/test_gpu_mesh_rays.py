"""-m gpu: bslam_mesh_rays (badslam_amd/csrc/ray_kernels.hpp) against the brute-force restatement of tests/mesh_rays_util.py.  t, triangle,
uv, front and the any-hit flag are compared bit for bit: the tree, the sort and the traversal may change no result.  Every device
array stands between guard words, outputs are filled with a sentinel first and have room beyond N."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from tests import mesh_rays_util as mr
from tests.test_gpu_fusion import SENTINEL, bits, stream_ptr
from tests.test_gpu_mesh_components import Guarded
from tests.test_gpu_nearest_triangle import read_tree

pytestmark = pytest.mark.gpu
F = np.float32
INVALID_ARGUMENT = -1   # BSLAM_ERR_INVALID_ARGUMENT
SPARE = 7               # output entries beyond N


@pytest.fixture(scope="module")
def gpu():
    import torch
    from badslam_amd import build
    build.build()
    return torch, badslam_amd.lib(), badslam_amd.Context(0)


@pytest.fixture(scope="module")
def sphere():
    """The icosphere of 1 280 triangles and about 1 000 rays: from inside, from outside at it, and past it."""
    positions, triangles = mr.icosphere()
    rng = np.random.default_rng(7)
    centre = positions.mean(axis=0)
    inside = centre + rng.uniform(-0.6, 0.6, (340, 3))
    outward = rng.standard_normal((660, 3))
    outside = centre + outward / np.linalg.norm(outward, axis=1, keepdims=True) * rng.uniform(2.0, 6.0, (660, 1))
    aim = np.concatenate([rng.standard_normal((340, 3)), centre + rng.uniform(-0.9, 0.9, (330, 3)) - outside[:330], rng.standard_normal((330, 3))])
    origins = np.ascontiguousarray(np.concatenate([inside, outside]), F)
    return positions, triangles, origins, np.ascontiguousarray(aim * rng.uniform(0.2, 4.0, (1000, 1)), F)


@pytest.fixture(scope="module")
def plane():
    """The 9 x 9 axis-aligned plane at z = 1.3 (boxes of zero thickness) and rays of every awkward kind."""
    positions, triangles = mr.plane_mesh()
    rng = np.random.default_rng(13)
    step, z = F(0.37), F(1.3)
    o, d = [], []
    for axis in range(3):                                                      # along each axis, both ways, off and in the plane
        for sign in (1.0, -1.0):
            e = np.zeros(3)
            e[axis] = sign
            for _ in range(12):
                o.append(rng.uniform(-0.5, 3.5, 3) * [1, 1, 0] + [0, 0, rng.choice([0.0, 1.3, 3.0])])
                d.append(e * rng.uniform(0.5, 2.0))
    for _ in range(200):                                                       # random angles
        o.append(rng.uniform(-1, 4, 3))
        d.append(rng.standard_normal(3))
    for _ in range(60):                                                        # origins on the plane: t = 0
        o.append([rng.uniform(0, 2.9), rng.uniform(0, 2.9), 1.3])
        d.append(rng.standard_normal(3))
    for _ in range(60):                                                        # origins exactly on box planes x = i step, y = j step
        o.append([float(step * F(rng.integers(0, 9))), float(step * F(rng.integers(0, 9))), rng.uniform(-1, 3)])
        d.append(rng.standard_normal(3))
    for _ in range(60):                                                        # one zero component
        v = rng.standard_normal(3)
        v[rng.integers(0, 2)] = 0.0
        o.append(rng.uniform(0, 3, 3) * [1, 1, 0])
        d.append(v)
    for _ in range(40):                                                        # two zero components, through the grid's own lines
        o.append([float(step * F(rng.integers(0, 9))), rng.uniform(0, 2.9), rng.uniform(-1, 3)])
        d.append([0.0, 0.0, rng.choice([-1.5, 0.7])])
    o, d = np.array(o), np.array(d)
    o[:, 2] = np.where(o[:, 2] == 1.3, z, o[:, 2])
    return positions, triangles, np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)


@pytest.fixture(scope="module")
def copies():
    """One triangle 4 096 times between two others, in shuffled order: a deep tree of equal codes."""
    positions = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1], [0, 0, -1], [1, 0, -1], [0, 1, -1]], F)
    triangles = np.array([[3, 4, 5]] + [[0, 1, 2]] * 4096 + [[6, 7, 8]], np.uint32)
    rng = np.random.default_rng(29)
    triangles = triangles[rng.permutation(len(triangles))]
    origins = np.ascontiguousarray(np.concatenate([rng.uniform(-0.2, 1.0, (48, 2)), np.full((48, 1), 0.5)], 1), F)
    directions = np.ascontiguousarray(np.concatenate([rng.uniform(-0.1, 0.1, (48, 2)), np.full((48, 1), -1.0)], 1), F)
    return positions, triangles, origins, directions


_wanted = {}


def wanted(name, origins, directions, t_range, positions, triangles):
    """The restatement's closest hit, computed once per name and never changed."""
    if name not in _wanted:
        _wanted[name] = mr.closest_hit(origins, directions, t_range, positions, triangles)
    return _wanted[name]


def words_of(count, itemsize):
    return (count * itemsize + 3) // 4


def call(gpu, origins, directions, t_range, positions, triangles, mode=0, outputs=("t", "triangle", "uv", "front"), stream=None):
    """-> (rc, dict of the outputs asked for, leaves, height); asserts that the inputs, the guard words and the outputs beyond N are
    untouched."""
    torch, L, ctx = gpu
    origins, directions = np.ascontiguousarray(origins, F).reshape(-1, 3), np.ascontiguousarray(directions, F).reshape(-1, 3)
    positions, triangles = np.ascontiguousarray(positions, F).reshape(-1, 3), np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    N, V, T = len(origins), len(positions), len(triangles)
    ins = [Guarded(torch, 3 * N, origins), Guarded(torch, 3 * N, directions), Guarded(torch, 3 * V, positions), Guarded(torch, 3 * T, triangles)]
    if t_range is not None:
        ins.append(Guarded(torch, 2 * N, np.ascontiguousarray(t_range, F)))
    before = [b.read() for b in ins]
    shape = dict(t=(4, 1), triangle=(4, 1), uv=(4, 2), front=(1, 1), hit=(1, 1))
    outs = {k: Guarded(torch, words_of((N + SPARE) * shape[k][1], shape[k][0])) for k in outputs}
    ptr = lambda k: outs[k].ptr if k in outs else None
    leaves, height = C.c_uint32(SENTINEL), C.c_uint32(SENTINEL)
    rc = L.bslam_mesh_rays(ctx.handle, stream_ptr(torch) if stream is None else C.c_void_p(stream.cuda_stream), N, ins[0].ptr, ins[1].ptr,
                           ins[4].ptr if t_range is not None else None, V, ins[2].ptr, T, ins[3].ptr, mode, ptr("t"), ptr("triangle"), ptr("uv"), ptr("front"), ptr("hit"),
                           C.byref(leaves), C.byref(height))
    for b, was in zip(ins, before):
        assert np.array_equal(b.read(), was), "an input was written to"
    got = {}
    for k, g in outs.items():
        raw = g.read()
        if shape[k][0] == 1:
            raw = raw.view(np.uint8)
            assert (raw[N:N + SPARE] == 0x5A).all(), f"{k} written beyond N"
            got[k] = raw[:N].copy()
        else:
            assert (raw[N * shape[k][1]:] == SENTINEL).all(), f"{k} written beyond N"
            got[k] = raw[:N * shape[k][1]].copy()
    return rc, got, leaves.value, height.value


def assert_equal(got, want, what):
    for key in got:
        if key in ("t", "uv"):
            g, w = got[key], bits(np.ascontiguousarray(want[key], F)).reshape(-1)
        else:
            g, w = got[key], np.asarray(want[key]).reshape(-1)
        differ = g != w
        assert not differ.any(), f"{what}: {int(differ.sum())} of {key} differ, first at {np.flatnonzero(differ)[0]}: {g[differ][0]!r} for {w[differ][0]!r}"


def run_case(gpu, name, origins, directions, t_range, positions, triangles, tree=False):
    """Closest hit and any hit against the restatement; with `tree`, the tree the call leaves through the checker."""
    want = wanted(name, origins, directions, t_range, positions, triangles)
    rc, got, leaves, height = call(gpu, origins, directions, t_range, positions, triangles)
    badslam_amd.check(rc)
    assert_equal(got, want, name)
    assert leaves == int(mr.triangle_boxes(positions, triangles)[0].sum())
    if tree:
        assert mr.check_tree(read_tree(gpu), positions, triangles) == height
    rc, got, _, _ = call(gpu, origins, directions, t_range, positions, triangles, mode=1, outputs=("hit",))
    badslam_amd.check(rc)
    assert np.array_equal(got["hit"], np.isfinite(want["t"]).astype(np.uint8)), f"{name}: any hit is not isfinite(t) of the closest hit"
    return want


# ------------------------------------------------------------------------------------------------
# bit equality
# ------------------------------------------------------------------------------------------------
def test_sphere(gpu, sphere):
    positions, triangles, origins, directions = sphere
    want = run_case(gpu, "sphere", origins, directions, None, positions, triangles, tree=True)
    hit = np.isfinite(want["t"])
    assert hit[:670].all() and (~hit[670:]).sum() > 100 and want["front"][340:670].all() and not want["front"][:340].any()


def test_plane(gpu, plane):
    positions, triangles, origins, directions = plane
    want = run_case(gpu, "plane", origins, directions, None, positions, triangles, tree=True)
    hit = np.isfinite(want["t"])
    assert 100 < hit.sum() < len(hit) - 100
    assert (want["t"][hit] == 0).sum() >= 10, "origins on the plane are meant to hit at t = 0"
    assert not hit[:48].any(), "a ray along x or y never meets the plane, and one inside it is parallel to every triangle"


def test_shuffled_meshes(gpu, sphere, plane):
    for name, (positions, triangles, origins, directions) in (("sphere", sphere), ("plane", plane)):
        want = wanted(name, origins, directions, None, positions, triangles)
        permutation = np.random.default_rng(41).permutation(len(triangles))
        rc, got, _, _ = call(gpu, origins, directions, None, positions, triangles[permutation])
        badslam_amd.check(rc)
        assert np.array_equal(got["t"], bits(want["t"])), f"{name}: t depends on the order of the triangles"
        pairs = mr.pair_hits(origins, directions, None, positions, triangles)["t"]
        unique = np.isfinite(want["t"]) & ((pairs == want["t"][:, None]).sum(axis=1) == 1)
        assert unique.sum() > 100
        assert np.array_equal(permutation[got["triangle"][unique]], want["triangle"][unique])
        assert_equal(got, mr.closest_hit(origins, directions, None, positions, triangles[permutation]), name + " shuffled")


def test_the_lowest_of_4096_copies_wins(gpu, copies):
    positions, triangles, origins, directions = copies
    want = run_case(gpu, "copies", origins, directions, None, positions, triangles, tree=True)
    first = int(np.flatnonzero((triangles == [0, 1, 2]).all(axis=1))[0])
    on_copy = np.isfinite(want["t"]) & (want["t"] == F(0.5))
    assert on_copy.sum() > 10 and (want["triangle"][on_copy] == first).all()


def test_small_trees_and_empty_inputs(gpu, plane):
    positions, triangles, origins, directions = plane
    run_case(gpu, "one triangle", origins, directions, None, positions, triangles[:1], tree=True)
    rc, got, leaves, height = call(gpu, origins[:9], directions[:9], None, positions, triangles[:0])
    assert rc == 0 and (leaves, height) == (0, 0)
    assert np.isinf(got["t"].view(F)).all() and (got["triangle"] == mr.NO_TRIANGLE).all() and (got["uv"] == 0).all() and (got["front"] == 0).all()
    rc, got, leaves, _ = call(gpu, origins[:0], directions[:0], None, positions, triangles)
    assert rc == 0 and leaves == len(triangles)
    rc, got, _, _ = call(gpu, origins[:9], directions[:9], None, positions, triangles[:0], mode=1, outputs=("hit",))
    assert rc == 0 and (got["hit"] == 0).all()


def test_invalid_triangles_and_rays(gpu, sphere):
    positions, triangles, origins, directions = sphere
    V = len(positions)
    positions = np.concatenate([positions, np.array([[np.nan, 1, 1], [1, np.inf, 1]], F)])
    triangles = triangles.copy()
    bad = [3, 170, 400, 1279]
    triangles[bad, [0, 1, 2, 0]] = [V, V + 1, V, V + 1]
    o, d = origins[:200].copy(), directions[:200].copy()
    t_range = np.tile(np.array([0, np.inf], F), (200, 1))
    o[0, 1] = np.nan
    d[1, 2] = np.nan
    o[2, 0] = np.inf
    d[3, 1] = -np.inf
    d[4] = 0
    t_range[5] = [2.0, 1.0]
    t_range[6] = [np.nan, 1.0]
    t_range[7] = [0.0, np.nan]
    t_range[8] = [-np.inf, np.inf]
    want = run_case(gpu, "invalid", o, d, t_range, positions, triangles, tree=True)
    assert np.isinf(want["t"][:8]).all() and np.isfinite(want["t"][8:]).all() and not np.isin(want["triangle"], bad).any()


def test_t_range_cuts_off_the_first_hit(gpu, sphere):
    positions, triangles, origins, directions = sphere
    first = wanted("sphere", origins, directions, None, positions, triangles)
    rows = np.arange(340, 670)                                                 # from outside at the sphere: a second hit behind the first
    t_range = np.stack([np.nextafter(first["t"][rows], F(np.inf)), np.full(len(rows), np.inf, F)], -1).astype(F)
    want = run_case(gpu, "behind the first hit", origins[rows], directions[rows], t_range, positions, triangles)
    assert np.isfinite(want["t"]).all() and (want["t"] > first["t"][rows]).all() and not want["front"].any()
    short = np.stack([np.zeros(len(rows), F), np.nextafter(first["t"][rows], F(0))], -1).astype(F)
    want = run_case(gpu, "short of the first hit", origins[rows], directions[rows], short, positions, triangles)
    assert np.isinf(want["t"]).all()


# ------------------------------------------------------------------------------------------------
# watertightness
# ------------------------------------------------------------------------------------------------
def test_no_ray_gets_out_of_the_sphere(gpu, sphere):
    """From the centre and from 20 points outside, rays through every vertex, every edge midpoint and the points at 1/3 and 2/3 of
    every edge.  The GPU runs all 21 x 6 402 of them; the restatement those from the centre and every 60th of the others."""
    positions, triangles, _, _ = sphere
    targets = mr.edge_points(positions, triangles)
    n = len(targets)
    centre = positions.mean(axis=0).astype(F)
    rng = np.random.default_rng(3)
    outward = rng.standard_normal((20, 3))
    outside = (centre + outward / np.linalg.norm(outward, axis=1, keepdims=True) * rng.uniform(2.0, 5.0, (20, 1))).astype(F)
    origins = np.ascontiguousarray(np.concatenate([np.broadcast_to(p, targets.shape) for p in [centre] + list(outside)]), F)
    directions = (np.tile(targets, (21, 1)) - origins).astype(F)
    rc, got, _, _ = call(gpu, origins, directions, None, positions, triangles)
    badslam_amd.check(rc)
    t = got["t"].view(F)
    assert np.isfinite(t[:n]).all(), "a ray from the centre through a vertex or an edge point got out"
    # from outside a ray through a point of the surface meets the sphere at that point or before it -- unless the point lies on the
    # silhouette, where the rounding of the direction may carry the ray past the edge (float64 agrees): it then meets the next face
    # within a fraction of a triangle's size, or nothing at all, and every miss grazes
    out, missed = t[n:], ~np.isfinite(t[n:])
    assert (out[~missed] <= F(1.01)).all() and (out[~missed] > F(1.0001)).mean() < 0.001 and missed.mean() < 0.03
    normal = (np.tile(targets, (20, 1)) - centre)[missed].astype(np.float64)
    along = directions[n:][missed].astype(np.float64)
    cosine = np.abs((normal * along).sum(axis=1)) / (np.linalg.norm(normal, axis=1) * np.linalg.norm(along, axis=1))
    assert (cosine < 0.1).all(), "a ray from outside that does not graze the sphere met nothing"
    rows = np.concatenate([np.arange(n), np.arange(n, 21 * n, 60)])
    want = wanted("through edges", origins[rows], directions[rows], None, positions, triangles)
    assert np.isfinite(want["t"][:n]).all(), "the restatement lets a ray from the centre out"
    assert_equal({k: v.reshape(21 * n, -1)[rows].reshape(-1) for k, v in got.items()}, want, "through edges")


def test_no_ray_gets_through_the_plane(gpu, plane):
    positions, triangles, _, _ = plane
    targets = mr.edge_points(positions, triangles)[:len(positions) + (len(mr.edge_points(positions, triangles)) - len(positions)) // 3]   # vertices and midpoints
    origins = np.ascontiguousarray(targets * np.array([1, 1, 0], F) + np.array([0, 0, -0.7], F), F)
    directions = np.tile(np.array([0, 0, 1.9], F), (len(targets), 1))
    want = run_case(gpu, "through the grid", origins, directions, None, positions, triangles)
    assert np.isfinite(want["t"]).all(), "a perpendicular ray through a grid vertex or an edge midpoint got through"


# ------------------------------------------------------------------------------------------------
# the traversal, the order of execution, the arguments
# ------------------------------------------------------------------------------------------------
def test_any_hit_fetches_no_more_than_closest_hit(gpu, sphere):
    positions, triangles, origins, directions = sphere
    _, L, ctx = gpu
    counts = {}
    badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
    try:
        tested, culled = C.c_uint64(), C.c_uint64()
        badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))     # reads and clears
        for mode, outputs in ((0, ("t",)), (1, ("hit",))):
            badslam_amd.check(call(gpu, origins, directions, None, positions, triangles, mode=mode, outputs=outputs)[0])
            badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))
            counts[mode] = (tested.value, tested.value - culled.value)
    finally:
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 0))
    print(f"nodes, triangles per ray: closest {counts[0][0] / 1000:.1f}, {counts[0][1] / 1000:.1f}; any {counts[1][0] / 1000:.1f}, {counts[1][1] / 1000:.1f}")
    assert 0 < counts[1][0] <= counts[0][0] and 0 < counts[1][1] <= counts[0][1]
    assert counts[0][0] < 1000 * 200, "the closest hit looks at a small part of the 1 279 nodes"


def test_two_calls_and_a_second_stream_agree(gpu, sphere):
    positions, triangles, origins, directions = sphere
    torch = gpu[0]
    want = wanted("sphere", origins, directions, None, positions, triangles)
    for stream in (None, None, torch.cuda.Stream()):
        rc, got, _, _ = call(gpu, origins, directions, None, positions, triangles, stream=stream)
        badslam_amd.check(rc)
        assert_equal(got, want, "again")


def test_arguments(gpu, sphere):
    positions, triangles, origins, directions = sphere
    L = gpu[1]
    o, d = origins[:9], directions[:9]

    def refused(message, **kw):
        rc, got, _, _ = call(gpu, o, d, kw.pop("t_range", None), positions, kw.pop("triangles", triangles), **kw)
        assert rc == INVALID_ARGUMENT and message in L.bslam_last_error(), (rc, L.bslam_last_error())
        for key, g in got.items():
            assert (g == (0x5A if g.dtype == np.uint8 else SENTINEL)).all(), f"{key} touched by a refused call"

    beyond = triangles[:50].copy()
    beyond[31, 2] = len(positions)
    refused(b"beyond vertex_count", triangles=beyond)
    refused(b"out_t is null", outputs=("triangle",))
    refused(b"out_hit belongs to mode 1", outputs=("t", "hit"))
    refused(b"out_hit is null", mode=1, outputs=())
    refused(b"returns out_hit alone", mode=1, outputs=("hit", "t"))
    refused(b"returns out_hit alone", mode=1, outputs=("hit", "front"))
    refused(b"mode must be", mode=2)
    rc, got, _, _ = call(gpu, o, d, None, positions, triangles, outputs=("t",))
    assert rc == 0
    assert_equal(got, dict(t=wanted("sphere", origins, directions, None, positions, triangles)["t"][:9]), "t alone")


def test_direct_ba_returns_the_same_bits(sphere):
    from badslam_amd import abi
    from badslam_amd.direct_ba import DirectBA
    positions, triangles, origins, directions = sphere
    cam = abi.Camera4f(131.25, 131.25, 80.0, 60.0, 160, 120)
    ba = DirectBA(1000, 1.0 / 5000.0, 40.0, 4, 0.8, 1, 1, 1, cam, cam, 0, True, False)   # no keyframe: the mesh calls need none
    mesh = dict(positions=positions, triangles=triangles)
    want = wanted("sphere", origins, directions, None, positions, triangles)
    got = ba.RayCastMesh(origins, directions, mesh)
    assert got["leaves"] == len(triangles) and 0 < got["height"] <= 62
    assert_equal(dict(t=bits(got["t"]), triangle=got["triangle"], uv=bits(got["uv"]).reshape(-1), front=got["front"].astype(np.uint8)), want, "DirectBA.RayCastMesh")
    assert np.array_equal(ba.RayCastMesh(origins, directions, mesh, any_hit=True)["hit"], np.isfinite(want["t"]))
    rows = np.arange(340, 670)
    behind = ba.RayCastMesh(origins[rows], directions[rows], mesh, t_min=np.nextafter(want["t"][rows], F(np.inf)))
    assert np.isfinite(behind["t"]).all() and (behind["t"] > want["t"][rows]).all()
    assert not ba.RayCastMesh(origins[rows], directions[rows], mesh, t_max=0.01, any_hit=True)["hit"].any()
    ba.close()
