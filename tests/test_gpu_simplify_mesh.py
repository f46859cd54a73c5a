"""-m gpu: bslam_simplify_mesh (badslam_amd/csrc/simplify_kernels.hpp) against the brute-force restatement of
tests/simplify_mesh_util.py -- counts, positions, colours, indices and vertex_cluster bit for bit, normals within 1e-6 (the
tolerance of the extracted normals in tests/test_gpu_fusion.py): the sort, the head flags and the scans may change no result -- and
the layers above it: DirectBA.SimplifyMesh and tools/run_tum.py --mesh-simplify-cell.  Every device array stands between guard
words; outputs have room for V vertices and T triangles, are filled with a sentinel first, and must be untouched at and beyond the
returned counts."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from tests import simplify_mesh_util as su
from tests.test_gpu_fusion import SENTINEL, bits, stream_ptr
from tests.test_gpu_mesh_components import Guarded

pytestmark = pytest.mark.gpu
F = np.float32
INVALID_ARGUMENT = -1   # BSLAM_ERR_INVALID_ARGUMENT
NORMAL_TOLERANCE = 1e-6


@pytest.fixture(scope="module")
def gpu():
    import torch
    from badslam_amd import build
    build.build()
    return torch, badslam_amd.lib(), badslam_amd.Context(0)


class Case:
    """A mesh on the device between guard words, and sentinel-filled outputs with room for V vertices and T triangles."""

    def __init__(self, torch, positions, normals=None, colors=None, triangles=None, with_cluster=True):
        self.positions = np.ascontiguousarray(positions, F).reshape(-1, 3)
        self.normals = None if normals is None else np.ascontiguousarray(normals, F).reshape(-1, 3)
        self.colors = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
        self.triangles = np.zeros((0, 3), np.uint32) if triangles is None else np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
        V, T = self.V, self.T = len(self.positions), len(self.triangles)
        opt = lambda present, words, content=None: Guarded(torch, words, content) if present else None
        self.inputs = dict(positions=Guarded(torch, 3 * V, self.positions), normals=opt(normals is not None, 3 * V, self.normals),
                           colors=opt(colors is not None, V, self.colors), indices=Guarded(torch, 3 * T, self.triangles))
        self.outputs = dict(out_positions=Guarded(torch, 3 * V), out_normals=opt(normals is not None, 3 * V), out_colors=opt(colors is not None, V),
                            out_indices=Guarded(torch, 3 * T), vertex_cluster=opt(with_cluster, V))
        self.before = {k: b.read() for k, b in self.inputs.items() if b is not None}

    def assert_inputs_untouched(self):
        for k, was in self.before.items():
            assert np.array_equal(self.inputs[k].read(), was), f"{k} was written to"

    def assert_outputs_untouched(self):
        for k, b in self.outputs.items():
            assert b is None or (b.read() == SENTINEL).all(), f"a refused call wrote to {k}"


def raw(gpu, case, origin, cell, ctx=None, counts=None):
    """The call itself -> (return code, out_vertex_count, out_triangle_count)."""
    torch, L, default_ctx = gpu
    p = lambda b: None if b is None else b.ptr
    v, t = counts or (C.c_uint32(SENTINEL), C.c_uint32(SENTINEL))
    o = (C.c_float * 3)(*[float(x) for x in origin])
    i, out = case.inputs, case.outputs
    rc = L.bslam_simplify_mesh((ctx or default_ctx).handle, stream_ptr(torch), case.V, case.T, p(i["positions"]), p(i["normals"]), p(i["colors"]), p(i["indices"]), o,
                               float(cell), p(out["out_positions"]), p(out["out_normals"]), p(out["out_colors"]), p(out["out_indices"]), p(out["vertex_cluster"]),
                               C.byref(v), C.byref(t))
    return rc, v.value, t.value


def simplify(gpu, positions, normals, colors, triangles, origin, cell, with_cluster=True, ctx=None):
    """bslam_simplify_mesh of host arrays -> the dict of su.simplify (vertex_cluster None when not asked for); asserts that the
    inputs, the guard words and the outputs at and beyond the counts are untouched."""
    torch, L, _ = gpu
    case = Case(torch, positions, normals, colors, triangles, with_cluster)
    rc, V2, T2 = raw(gpu, case, origin, cell, ctx)
    badslam_amd.check(rc)
    case.assert_inputs_untouched()
    assert V2 <= case.V and T2 <= case.T
    o = {k: None if b is None else b.read() for k, b in case.outputs.items()}
    for k, per, n in (("out_positions", 3, V2), ("out_normals", 3, V2), ("out_colors", 1, V2), ("out_indices", 3, T2)):
        assert o[k] is None or (o[k][per * n:] == SENTINEL).all(), f"{k} was written at or beyond the returned count"
    return dict(positions=o["out_positions"][:3 * V2].view(F).reshape(V2, 3), normals=None if o["out_normals"] is None else o["out_normals"][:3 * V2].view(F).reshape(V2, 3),
                colors=None if o["out_colors"] is None else o["out_colors"][:V2].view(np.uint8).reshape(V2, 4), triangles=o["out_indices"][:3 * T2].reshape(T2, 3),
                vertex_cluster=o["vertex_cluster"])


def assert_equal(got, want, what=""):
    assert len(got["positions"]) == len(want["positions"]), f"{what}: {len(got['positions'])} vertices for {len(want['positions'])}"
    assert len(got["triangles"]) == len(want["triangles"]), f"{what}: {len(got['triangles'])} triangles for {len(want['triangles'])}"
    for k in ("positions", "colors", "triangles", "vertex_cluster"):
        g, w = got[k], want[k]
        assert (g is None) == (w is None) or k == "vertex_cluster", f"{what}: {k} present in one only"
        if g is None:
            continue
        differ = bits(g) != bits(w) if g.dtype == F else g != w
        assert not differ.any(), f"{what}: {int(differ.sum())} {k} differ, first at {np.argwhere(differ)[0]}: {g[differ][0]!r} for {w[differ][0]!r}"
    assert (got["normals"] is None) == (want["normals"] is None)
    if got["normals"] is not None and len(got["normals"]):
        error = np.abs(got["normals"].astype(np.float64) - want["normals"].astype(np.float64)).max()
        assert error <= NORMAL_TOLERANCE, f"{what}: normals differ by {error:.3e}"


def check(gpu, positions, normals, colors, triangles, origin, cell, what="", **kwargs):
    want = su.simplify(positions, normals, colors, triangles, origin, cell)
    got = simplify(gpu, positions, normals, colors, triangles, origin, cell, **kwargs)
    assert_equal(got, want, what)
    return got, want


def random_mesh(V, cell, origin, seed):
    """V random vertices in the unit box above `origin` with normals and colours, a tenth of the coordinates exactly on multiples of
    the cell from the origin, a -0.0f when the origin is 0, and about 2 V triangles: random ones, input-degenerate ones (i0 == i1), and
    -- where the restatement finds a cluster of two -- triangles that collapse to two clusters and to one."""
    rng = np.random.default_rng(seed)
    origin = np.asarray(origin, F)
    positions = (origin + rng.uniform(0, 1, (V, 3))).astype(F)
    positions = np.maximum(positions, origin)
    on_face = rng.random((V, 3)) < 0.1
    k = rng.integers(0, int(1.0 / cell), (V, 3)).astype(F)
    positions[on_face] = (origin[None, :] + k * F(cell)).astype(F)[on_face]
    positions = np.maximum(positions, origin)                    # origin + k * cell never rounds below the origin, but say so
    if not origin.any():
        positions[V // 2, 1] = F(-0.0)
    normals = rng.standard_normal((V, 3)).astype(F)
    colors = rng.integers(0, 256, (V, 4), dtype=np.uint8)
    tri = rng.integers(0, V, (2 * V, 3)).astype(np.uint32)
    tri[::7, 1] = tri[::7, 0]                                    # degenerate on input
    cluster = su.simplify(positions, None, None, None, origin, cell)["vertex_cluster"]
    sizes = np.bincount(cluster)
    if sizes.max() >= 2:
        a, b = np.flatnonzero(cluster == np.argmax(sizes))[:2]
        other = int(np.flatnonzero(cluster != cluster[a])[0]) if (cluster != cluster[a]).any() else a
        extra = [[a, b, other], [other, a, b], [a, b, a], [b, a, b]]       # two clusters, twice; one cluster, twice
        if sizes.max() >= 3:
            extra.append(np.flatnonzero(cluster == np.argmax(sizes))[:3])  # three vertices, one cluster
        tri = np.concatenate([tri, np.array(extra, np.uint32)])
    return positions, normals, colors, tri


# ------------------------------------------------------------------------------------------------
# 1. bit for bit with the restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell, origin", [(0.03, (-0.013, -0.007, 0.0)), (0.0625, (0.0, 0.0, 0.0))])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 257, 1025, 5000])
def test_random_meshes(gpu, V, cell, origin):
    positions, normals, colors, tri = random_mesh(V, cell, origin, seed=V)
    got, want = check(gpu, positions, normals, colors, tri, origin, cell, f"V {V} cell {cell}")
    if V >= 1025:
        mapped = want["vertex_cluster"][tri.astype(np.int64)]
        distinct = np.array([len(set(row)) for row in mapped.tolist()])
        assert (distinct == 1).any() and (distinct == 2).any() and (distinct == 3).any(), "the case lost a kind of triangle"
        assert 0 < len(want["triangles"]) < len(tri) and 1 < len(want["positions"]) < V


def test_a_cluster_of_700_among_singletons(gpu):
    """The segment spans three blocks of the cluster pass and its members are spread over the vertex ids; 700 x 255 overflows a
    16-bit colour sum, and the mean of 700 equal colours has to come out as that colour."""
    rng = np.random.default_rng(700)
    V = 1000
    positions = np.zeros((V, 3), F)
    members = np.sort(rng.permutation(V)[:700])
    single = np.setdiff1d(np.arange(V), members)
    positions[members] = (np.array([5.0, 3.0, 2.0]) + rng.uniform(0, 1, (700, 3))).astype(F)       # cell (5, 3, 2) at cell size 1
    positions[single] = np.stack([rng.uniform(0, 1, 300) + 10 + np.arange(300), rng.uniform(0, 4, 300), rng.uniform(0, 4, 300)], axis=1).astype(F)
    normals = rng.standard_normal((V, 3)).astype(F)
    colors = rng.integers(0, 256, (V, 4), dtype=np.uint8)
    colors[members] = 255
    tri = rng.integers(0, V, (2 * V, 3)).astype(np.uint32)
    got, want = check(gpu, positions, normals, colors, tri, np.zeros(3, F), 1.0, "cluster of 700")
    assert np.bincount(want["vertex_cluster"]).max() == 700 and len(want["positions"]) == 301
    big = want["vertex_cluster"][members[0]]
    assert (got["colors"][big] == 255).all()


def test_every_vertex_its_own_cluster_and_one_cluster_in_total(gpu):
    rng = np.random.default_rng(11)
    V = 300
    positions = (rng.uniform(0, 1, (V, 3)) * 0.5 + rng.permutation(V)[:, None] * np.array([1.0, 0.0, 0.0]) + rng.integers(0, 3, (V, 3)) * np.array([0.0, 1.0, 1.0])).astype(F)
    normals = rng.standard_normal((V, 3)).astype(F)
    colors = rng.integers(0, 256, (V, 4), dtype=np.uint8)
    tri = rng.integers(0, V, (2 * V, 3)).astype(np.uint32)
    got, want = check(gpu, positions, normals, colors, tri, np.zeros(3, F), 1.0, "singletons")
    assert len(want["positions"]) == V
    assert np.array_equal(bits(got["positions"][got["vertex_cluster"]]), bits(positions)), "a cluster of one changed its position bits"
    got, want = check(gpu, positions, normals, colors, tri, np.zeros(3, F), 1000.0, "one cluster")
    assert len(want["positions"]) == 1 and len(want["triangles"]) == 0 and (got["vertex_cluster"] == 0).all()


def test_key_packing(gpu):
    """Cell 0 and cell 2^21 - 1 on each axis in turn: the top bit of every field of the key, and the (z, y, x) order."""
    top = 2097151.5
    positions = np.array([[0.5, 0.5, top], [0.5, top, 0.5], [top, 0.5, 0.5], [0.5, 0.5, 0.5], [top, top, top], [top, 0.25, 0.75]], F)
    tri = np.array([[0, 1, 2], [3, 4, 0], [2, 5, 1], [5, 2, 2]], np.uint32)
    got, want = check(gpu, positions, None, None, tri, np.zeros(3, F), 1.0, "key packing")
    assert np.array_equal(want["vertex_cluster"], [3, 2, 1, 0, 4, 1]) and np.array_equal(want["triangles"], [[3, 2, 1], [0, 4, 3]])


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_the_cell_2_to_the_21_is_refused(gpu, axis):
    torch, L, ctx = gpu
    positions = np.full((70, 3), 0.5, F)
    positions[66, axis] = 2097152.5
    case = Case(torch, positions, triangles=[[0, 1, 2]])
    rc, _, _ = raw(gpu, case, (0, 0, 0), 1.0)
    assert rc == INVALID_ARGUMENT and b"bslam_simplify_mesh: a vertex is not finite or lies outside the grid" in L.bslam_last_error()
    case.assert_inputs_untouched()


@pytest.mark.parametrize("with_cluster", [False, True])
@pytest.mark.parametrize("with_normals, with_colors", [(False, False), (True, False), (False, True), (True, True)])
def test_pointer_variants(gpu, with_normals, with_colors, with_cluster):
    positions, normals, colors, tri = random_mesh(700, 0.0625, (0, 0, 0), seed=5)
    check(gpu, positions, normals if with_normals else None, colors if with_colors else None, tri, (0, 0, 0), 0.0625, with_cluster=with_cluster)


def test_point_clouds_and_empty_meshes(gpu):
    torch, L, ctx = gpu
    positions, normals, colors, _ = random_mesh(700, 0.0625, (0, 0, 0), seed=6)
    got, want = check(gpu, positions, normals, colors, None, (0, 0, 0), 0.0625, "T = 0")
    assert len(got["triangles"]) == 0 and 1 < len(got["positions"]) < 700
    got = simplify(gpu, np.zeros((0, 3), F), None, None, None, (0, 0, 0), 1.0)
    assert len(got["positions"]) == 0 and len(got["triangles"]) == 0
    case = Case(torch, np.zeros((0, 3), F), triangles=[[0, 0, 0]])                   # V = 0: every index is beyond
    rc, v, t = raw(gpu, case, (0, 0, 0), 1.0)
    assert rc == INVALID_ARGUMENT and b"bslam_simplify_mesh: a triangle names a vertex beyond vertex_count" in L.bslam_last_error()
    assert (v, t) == (SENTINEL, SENTINEL)
    case.assert_outputs_untouched()


def test_degenerate_normals(gpu):
    positions = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [1.5, 0.5, 0.5], [1.6, 0.5, 0.5], [2.5, 0.5, 0.5], [2.6, 0.5, 0.5], [3.5, 0.5, 0.5]], F)
    normals = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, np.inf, 0], [0, 0, 1], [0, 1, 0], [0, 0, 0]], F)
    got, want = check(gpu, positions, normals, None, None, (0, 0, 0), 1.0, "degenerate normals")
    assert np.array_equal(bits(got["normals"][[0, 1, 3]]), bits(np.zeros((3, 3), F))), "a zero sum, a non-finite member and a zero normal give (0, 0, 0)"
    assert np.abs(got["normals"][2] - np.array([0, 1, 1]) / np.sqrt(2.0)).max() <= NORMAL_TOLERANCE


def test_two_calls_agree(gpu):
    positions, normals, colors, tri = random_mesh(5000, 0.0625, (0, 0, 0), seed=8)
    a = simplify(gpu, positions, normals, colors, tri, (0, 0, 0), 0.0625)
    b = simplify(gpu, positions, normals, colors, tri, (0, 0, 0), 0.0625)
    for k in a:
        assert np.array_equal(bits(a[k]) if a[k].dtype == F else a[k], bits(b[k]) if b[k].dtype == F else b[k]), k


def test_stage_times_with_profiling_on(gpu):
    """Profiling changes no result, and a profiled call leaves five stage times.  A context of its own: the switch is the context's."""
    from tests import decimate_mesh_util as du
    torch, L, _ = gpu
    ctx = badslam_amd.Context(0)
    positions, tri = du.noisy_plane(9, seed=9)
    normals, colors = du.attributes(81, 9)
    assert len(positions) == 81 and len(tri) == 128
    runs = []
    try:
        for on in (0, 1, 0):
            badslam_amd.check(L.bslam_profile_enable(ctx.handle, on))
            runs.append(simplify(gpu, positions, normals, colors, tri, (0, 0, 0), 2.0, ctx=ctx))
            if on:
                ms = (C.c_float * 5)(*[-1.0] * 5)
                badslam_amd.check(L.bslam_simplify_stage_times(ctx.handle, ms))
                ms = np.array(ms[:], np.float64)
                assert np.isfinite(ms).all() and (ms >= 0).all() and (ms > 0).any(), ms
    finally:
        L.bslam_profile_enable(ctx.handle, 0)
    assert 1 < len(runs[0]["positions"]) < 81
    for other in runs[1:]:
        for k in runs[0]:
            assert np.array_equal(bits(runs[0][k]) if runs[0][k].dtype == F else runs[0][k], bits(other[k]) if other[k].dtype == F else other[k]), k


def test_a_second_call_with_a_larger_mesh_grows_the_slab(gpu):
    """A context of its own, so that its first simplification is the small one."""
    ctx = badslam_amd.Context(0)
    for V in (64, 5000, 65):
        positions, normals, colors, tri = random_mesh(V, 0.0625, (0, 0, 0), seed=V)
        want = su.simplify(positions, normals, colors, tri, (0, 0, 0), 0.0625)
        assert_equal(simplify(gpu, positions, normals, colors, tri, (0, 0, 0), 0.0625, ctx=ctx), want, f"V {V}")


# ------------------------------------------------------------------------------------------------
# 2. refusals: by the return code, without a fault and without a write
# ------------------------------------------------------------------------------------------------
def test_rejected_arguments(gpu):
    torch, L, ctx = gpu
    positions, normals, colors, tri = random_mesh(300, 0.0625, (0, 0, 0), seed=9)
    want = su.simplify(positions, normals, colors, tri, (0, 0, 0), 0.0625)
    case = Case(torch, positions, normals, colors, tri)
    V, T = case.V, case.T
    vc, tc = C.c_uint32(SENTINEL), C.c_uint32(SENTINEL)
    base = dict(ctx=ctx.handle, origin=(0.0, 0.0, 0.0), cell=0.0625, vcount=C.byref(vc), tcount=C.byref(tc))
    base.update({k: b.address for k, b in case.inputs.items()})
    base.update({k: b.address for k, b in case.outputs.items()})

    def run(**changes):
        a = dict(base, **changes)
        p = lambda v: None if v is None else C.c_void_p(v)
        o = None if a["origin"] is None else (C.c_float * 3)(*a["origin"])
        return L.bslam_simplify_mesh(a["ctx"], stream_ptr(torch), V, T, p(a["positions"]), p(a["normals"]), p(a["colors"]), p(a["indices"]), o, a["cell"],
                                     p(a["out_positions"]), p(a["out_normals"]), p(a["out_colors"]), p(a["out_indices"]), p(a["vertex_cluster"]), a["vcount"], a["tcount"])

    a = base
    inf, nan = float("inf"), float("nan")
    cases = {"null context": dict(ctx=None), "null out_vertex_count": dict(vcount=None), "null out_triangle_count": dict(tcount=None), "null origin": dict(origin=None),
             "null positions": dict(positions=None), "null indices": dict(indices=None), "null out_positions": dict(out_positions=None),
             "null out_indices": dict(out_indices=None),
             "misaligned positions": dict(positions=a["positions"] + 2), "misaligned normals": dict(normals=a["normals"] + 1), "misaligned colors": dict(colors=a["colors"] + 2),
             "misaligned indices": dict(indices=a["indices"] + 1), "misaligned out_positions": dict(out_positions=a["out_positions"] + 2),
             "misaligned out_normals": dict(out_normals=a["out_normals"] + 3), "misaligned out_colors": dict(out_colors=a["out_colors"] + 1),
             "misaligned out_indices": dict(out_indices=a["out_indices"] + 2), "misaligned vertex_cluster": dict(vertex_cluster=a["vertex_cluster"] + 2),
             "in place: positions": dict(out_positions=a["positions"]), "in place: indices": dict(out_indices=a["indices"]),
             "out_normals inside positions": dict(out_normals=a["positions"] + 12 * V - 4), "vertex_cluster inside colors": dict(vertex_cluster=a["colors"] + 4 * V - 4),
             "two outputs overlap": dict(out_normals=a["out_positions"] + 12 * V - 4), "two outputs are one": dict(vertex_cluster=a["out_colors"]),
             "cell_size = 0": dict(cell=0.0), "cell_size < 0": dict(cell=-0.0625), "cell_size = inf": dict(cell=inf), "cell_size = NaN": dict(cell=nan),
             "origin inf": dict(origin=(0.0, inf, 0.0)), "origin -inf": dict(origin=(-inf, 0.0, 0.0)), "origin NaN": dict(origin=(0.0, 0.0, nan)),
             "normals without out_normals": dict(out_normals=None), "out_normals without normals": dict(normals=None),
             "colors without out_colors": dict(out_colors=None), "out_colors without colors": dict(colors=None)}
    for name, changes in cases.items():
        rc = run(**changes)
        assert rc == INVALID_ARGUMENT, (name, rc, L.bslam_last_error())
    torch.cuda.synchronize()
    case.assert_outputs_untouched()
    case.assert_inputs_untouched()
    assert (vc.value, tc.value) == (SENTINEL, SENTINEL)
    assert run() == 0 and (vc.value, tc.value) == (len(want["positions"]), len(want["triangles"]))
    o = {k: b.read() for k, b in case.outputs.items()}
    V2, T2 = vc.value, tc.value
    assert_equal(dict(positions=o["out_positions"][:3 * V2].view(F).reshape(V2, 3), normals=o["out_normals"][:3 * V2].view(F).reshape(V2, 3),
                      colors=o["out_colors"][:V2].view(np.uint8).reshape(V2, 4), triangles=o["out_indices"][:3 * T2].reshape(T2, 3), vertex_cluster=o["vertex_cluster"]), want)


@pytest.mark.parametrize("bad", ["V", "0xFFFFFFFF"])
def test_an_index_beyond_the_vertices_is_refused(gpu, bad):
    torch, L, ctx = gpu
    positions, normals, colors, tri = random_mesh(1025, 0.0625, (0, 0, 0), seed=10)
    broken = tri.copy()
    broken[1500, 1] = len(positions) if bad == "V" else 0xFFFFFFFF
    case = Case(torch, positions, normals, colors, broken)
    rc, v, t = raw(gpu, case, (0, 0, 0), 0.0625)
    assert rc == INVALID_ARGUMENT and b"bslam_simplify_mesh: a triangle names a vertex beyond vertex_count" in L.bslam_last_error()
    assert (v, t) == (SENTINEL, SENTINEL)
    case.assert_inputs_untouched()
    check(gpu, positions, normals, colors, tri, (0, 0, 0), 0.0625, "the context is fine afterwards")


@pytest.mark.parametrize("value, origin", [(np.nan, 0.0), (np.inf, 0.0), (-np.inf, 0.0), (0.49, 0.5), (-1e-30, 0.0), (3e6, 0.0), (3e38, -3e38)])
def test_an_invalid_vertex_is_refused(gpu, value, origin):
    """Not finite, below the origin, beyond 2^21 cells, and a difference that overflows: each raises the device error bit."""
    torch, L, ctx = gpu
    positions, normals, colors, tri = random_mesh(1025, 1.0, (0.5, 0.5, 0.5), seed=12)
    positions[777, 1] = value
    case = Case(torch, positions, normals, colors, tri)
    rc, v, t = raw(gpu, case, (origin, origin, origin), 1.0)
    assert rc == INVALID_ARGUMENT and b"bslam_simplify_mesh: a vertex is not finite or lies outside the grid" in L.bslam_last_error()
    assert (v, t) == (SENTINEL, SENTINEL)
    case.assert_inputs_untouched()
    with pytest.raises(su.Refused):
        su.simplify(positions, normals, colors, tri, np.full(3, origin, F), 1.0)


# ------------------------------------------------------------------------------------------------
# 3. through DirectBA
# ------------------------------------------------------------------------------------------------
VOXEL = 0.02


@pytest.fixture(scope="module")
def extracted():
    """(DirectBA, the extracted mesh) of the three 160 x 120 keyframes of tests/scenes.py that tests/test_gpu_fusion.py fuses at 2 cm."""
    from badslam_amd.direct_ba import DirectBA
    from tests import bso, scenes
    from tools import run_tum
    cam = bso.make_camera(131.25, 131.25, 80.0, 60.0, 160, 120)
    scene = scenes.synthetic_scene(3, width=160, height=120, cell=2, camera=cam)
    ba = DirectBA(scene.max_surfels, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, 0.8, 1, 1, 1, scene.color_camera, scene.depth_camera, 0, True, False)
    for kf in scene.keyframes:
        ba.AddKeyframe(kf.id, max(kf.min_depth, 1e-3), max(kf.max_depth, 1e-2), kf.depth, kf.normals, kf.radius, kf.color, kf.global_T_frame)
    for kf in scene.keyframes:
        ba.CreateSurfelsForKeyframe(False, kf.id)
    lo, hi = ba.ModelBounds()
    origin, dims = run_tum.mesh_volume(lo, hi, VOXEL, 4 * VOXEL)
    ba.FuseKeyframes(origin, VOXEL, dims, 4 * VOXEL)
    yield ba, ba.ExtractMesh(1)
    ba.close()


@pytest.mark.parametrize("voxels", [2, 4])
def test_direct_ba_simplify_mesh(extracted, voxels):
    ba, mesh = extracted
    cell = voxels * VOXEL
    V, T = len(mesh["positions"]), len(mesh["triangles"])
    assert V > 10000 and T > 10000
    got = ba.SimplifyMesh(mesh, cell)
    assert set(got) == set(mesh) | {"vertex_cluster"}
    origin = mesh["positions"].min(axis=0)
    want = su.simplify(mesh["positions"], mesh["normals"], mesh["colors"], mesh["triangles"], origin, cell)
    assert_equal(got, want, f"{voxels} voxels")
    print(f"{V} vertices, {T} triangles at {voxels} voxels -> {len(got['positions'])}, {len(got['triangles'])}")
    assert 0 < len(got["positions"]) < V and 0 < len(got["triangles"]) < T
    # an explicit origin is taken as given
    assert_equal(ba.SimplifyMesh(mesh, cell, origin=origin - F(0.37)), su.simplify(mesh["positions"], mesh["normals"], mesh["colors"], mesh["triangles"], origin - F(0.37), cell))
    # no input vertex is farther from the simplified surface than the diagonal of a cell, plus the rounding slack of the cell formula
    slack = 4 * float(np.spacing(F(np.abs(mesh["positions"]).max())))
    bound = np.sqrt(3.0) * cell + slack
    distance = ba.PointMeshDistance(mesh["positions"], got, 2 * bound)["distance"]
    print(f"farthest input vertex from the simplified mesh: {distance.max() / cell:.4f} cells (bound {bound / cell:.4f})")
    assert np.isfinite(distance).all() and distance.max() <= bound
    labels, sizes = ba.MeshComponents(got)
    assert len(labels) == len(got["positions"]) and sizes.min() >= 1 and (labels <= np.arange(len(labels))).all()


def test_direct_ba_accepts_ply_dicts_and_clouds(extracted):
    ba, mesh = extracted
    cell = 4 * VOXEL
    origin = mesh["positions"].min(axis=0)
    rgb = np.ascontiguousarray(mesh["colors"][:, :3])
    padded = np.concatenate([rgb, np.full((len(rgb), 1), 255, np.uint8)], axis=1)
    want = su.simplify(mesh["positions"], None, padded, None, origin, cell)
    got = ba.SimplifyMesh(dict(positions=mesh["positions"], normals=None, colors=rgb), cell)     # a LoadPLY cloud without normals
    assert got["normals"] is None and got["colors"].shape == (len(want["positions"]), 3) and got["triangles"].shape == (0, 3)
    assert np.array_equal(got["colors"], want["colors"][:, :3]) and np.array_equal(bits(got["positions"]), bits(want["positions"]))
    assert np.array_equal(got["vertex_cluster"], want["vertex_cluster"])
    with pytest.raises(Exception, match="not finite or lies outside the grid"):
        ba.SimplifyMesh(mesh, cell, origin=origin + F(0.01))


# ------------------------------------------------------------------------------------------------
# 4. tools/run_tum.py --mesh-simplify-cell
# ------------------------------------------------------------------------------------------------
def test_run_tum_mesh_simplify_cell(tmp_path):
    """Five frames of the rendered sequence of tests/test_gpu_bad_slam.py with --mesh and --mesh-simplify-cell 0.08: the file parses and
    holds SimplifyMesh(ExtractMesh) of the run."""
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
    mesh_path = tmp_path / "mesh.ply"
    again = {}

    def inspect(slam, result):
        again["extracted"] = slam.ba().ExtractMesh(2, min_component_vertices=50)
        again["simplified"] = slam.ba().SimplifyMesh(again["extracted"], 0.08)

    r = run_tum.run(source, mesh=mesh_path, mesh_simplify_cell=0.08, keyframe_interval=4, ba_iterations=2, max_depth=6.0, num_scales=4, max_surfel_count=400000,
                    mesh_voxel_size=0.04, mesh_min_count=2, mesh_min_component=50, inspect=inspect)
    extracted_mesh, simplified = again["extracted"], again["simplified"]
    sp = r["mesh"]["simplification"]
    print(f"{sp['vertices_before']} vertices, {sp['triangles_before']} triangles -> {sp['vertices']}, {sp['triangles']}")
    assert sp == {"cell": 0.08, "vertices_before": len(extracted_mesh["positions"]), "triangles_before": len(extracted_mesh["triangles"]),
                  "vertices": len(simplified["positions"]), "triangles": len(simplified["triangles"])}
    assert 0 < sp["vertices"] < sp["vertices_before"] and 0 < sp["triangles"] < sp["triangles_before"] and sp["vertices_before"] > 1000
    assert r["mesh"]["vertices"] == sp["vertices"] and r["mesh"]["triangles"] == sp["triangles"]
    own = dba.LoadPLY(mesh_path)
    assert np.array_equal(bits(own["positions"]), bits(simplified["positions"])) and np.array_equal(own["triangles"], simplified["triangles"])
    assert np.array_equal(bits(own["normals"]), bits(simplified["normals"])) and np.array_equal(own["colors"], simplified["colors"][:, :3])
    want = su.simplify(extracted_mesh["positions"], extracted_mesh["normals"], extracted_mesh["colors"], extracted_mesh["triangles"],
                       extracted_mesh["positions"].min(axis=0), 0.08)
    assert_equal(simplified, want, "run_tum")
