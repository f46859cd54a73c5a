"""-m gpu: bslam_decimate_mesh (badslam_amd/csrc/decimate_kernels.hpp) against the brute-force restatement of
tests/decimate_mesh_util.py -- counts, rounds, positions, colours, indices and vertex_map bit for bit, normals within 1e-6 (the
midpoint normal takes a square root): the sorts, the head flags, the scans and the atomic minima may change no result -- and
DirectBA.DecimateMesh above it.  Every device array stands between guard words; outputs have room for V vertices and T triangles,
are filled with a sentinel first, and must be untouched at and beyond the returned counts."""
import ctypes as C
import math

import numpy as np
import pytest

import badslam_amd
from tests import decimate_mesh_util as du
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

    def __init__(self, torch, positions, normals=None, colors=None, triangles=None, with_map=True):
        self.positions = np.ascontiguousarray(positions, F).reshape(-1, 3)
        self.normals = None if normals is None else np.ascontiguousarray(normals, F).reshape(-1, 3)
        self.colors = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
        self.triangles = np.zeros((0, 3), np.uint32) if triangles is None else np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
        V, T = self.V, self.T = len(self.positions), len(self.triangles)
        opt = lambda present, words, content=None: Guarded(torch, words, content) if present else None
        self.inputs = dict(positions=Guarded(torch, 3 * V, self.positions), normals=opt(normals is not None, 3 * V, self.normals),
                           colors=opt(colors is not None, V, self.colors), indices=Guarded(torch, 3 * T, self.triangles))
        self.outputs = dict(out_positions=Guarded(torch, 3 * V), out_normals=opt(normals is not None, 3 * V), out_colors=opt(colors is not None, V),
                            out_indices=Guarded(torch, 3 * T), vertex_map=opt(with_map, V))
        self.before = {k: b.read() for k, b in self.inputs.items() if b is not None}

    def assert_inputs_untouched(self):
        for k, was in self.before.items():
            assert np.array_equal(self.inputs[k].read(), was), f"{k} was written to"

    def assert_outputs_untouched(self):
        for k, b in self.outputs.items():
            assert b is None or (b.read() == SENTINEL).all(), f"a refused call wrote to {k}"


def raw(gpu, case, target, boundary_weight=1.0, max_cost=math.inf, max_rounds=0, ctx=None):
    """The call itself -> (return code, out_vertex_count, out_triangle_count, out_rounds)."""
    torch, L, default_ctx = gpu
    p = lambda b: None if b is None else b.ptr
    v, t, r = C.c_uint32(SENTINEL), C.c_uint32(SENTINEL), C.c_uint32(SENTINEL)
    i, out = case.inputs, case.outputs
    rc = L.bslam_decimate_mesh((ctx or default_ctx).handle, stream_ptr(torch), case.V, case.T, p(i["positions"]), p(i["normals"]), p(i["colors"]), p(i["indices"]),
                               int(target), float(boundary_weight), float(max_cost), int(max_rounds), p(out["out_positions"]), p(out["out_normals"]), p(out["out_colors"]),
                               p(out["out_indices"]), p(out["vertex_map"]), C.byref(v), C.byref(t), C.byref(r))
    return rc, v.value, t.value, r.value


def results(case, V2, T2, rounds):
    """The outputs of a call as the dict of du.decimate; asserts that nothing at or beyond the counts was written."""
    assert V2 <= case.V and T2 <= case.T
    o = {k: None if b is None else b.read() for k, b in case.outputs.items()}
    for k, per, n in (("out_positions", 3, V2), ("out_normals", 3, V2), ("out_colors", 1, V2), ("out_indices", 3, T2)):
        assert o[k] is None or (o[k][per * n:] == SENTINEL).all(), f"{k} was written at or beyond the returned count"
    return dict(positions=o["out_positions"][:3 * V2].view(F).reshape(V2, 3), normals=None if o["out_normals"] is None else o["out_normals"][:3 * V2].view(F).reshape(V2, 3),
                colors=None if o["out_colors"] is None else o["out_colors"][:V2].view(np.uint8).reshape(V2, 4), triangles=o["out_indices"][:3 * T2].reshape(T2, 3),
                vertex_map=o["vertex_map"], rounds=rounds)


def decimate(gpu, positions, normals, colors, triangles, target, with_map=True, ctx=None, **options):
    torch, L, _ = gpu
    case = Case(torch, positions, normals, colors, triangles, with_map)
    rc, V2, T2, rounds = raw(gpu, case, target, ctx=ctx, **options)
    badslam_amd.check(rc)
    case.assert_inputs_untouched()
    return results(case, V2, T2, rounds)


def assert_equal(got, want, what=""):
    assert len(got["positions"]) == len(want["positions"]), f"{what}: {len(got['positions'])} vertices for {len(want['positions'])}"
    assert len(got["triangles"]) == len(want["triangles"]), f"{what}: {len(got['triangles'])} triangles for {len(want['triangles'])}"
    assert got["rounds"] == want["rounds"], f"{what}: {got['rounds']} rounds for {want['rounds']}"
    for k in ("positions", "colors", "triangles", "vertex_map"):
        g, w = got[k], want[k]
        assert (g is None) == (w is None) or k == "vertex_map", f"{what}: {k} present in one only"
        if g is None:
            continue
        differ = bits(g) != bits(w) if g.dtype == F else g != w
        assert not differ.any(), f"{what}: {int(differ.sum())} {k} differ, first at {np.argwhere(differ)[0]}: {g[differ][0]!r} for {w[differ][0]!r}"
    assert (got["normals"] is None) == (want["normals"] is None)
    if got["normals"] is not None and len(got["normals"]):
        error = np.abs(got["normals"].astype(np.float64) - want["normals"].astype(np.float64)).max()
        assert error <= NORMAL_TOLERANCE, f"{what}: normals differ by {error:.3e}"


def check(gpu, positions, normals, colors, triangles, target, what="", with_map=True, ctx=None, **options):
    want = du.decimate(positions, normals, colors, triangles, target, **options)
    got = decimate(gpu, positions, normals, colors, triangles, target, with_map=with_map, ctx=ctx, **options)
    assert_equal(got, want, what)
    return got, want


def dressed(mesh, seed=0):
    """(positions, normals, colours, triangles) of a (positions, triangles) mesh with random unit normals and colours."""
    positions, triangles = mesh
    normals, colors = du.attributes(len(positions), seed)
    return positions, normals, colors, triangles


# ------------------------------------------------------------------------------------------------
# 1. bit for bit with the restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 5, 8, 9, 17])
def test_noisy_planes_at_half(gpu, n):
    """4, 9, 25, 64, 81 and 289 vertices; 6 to 1 536 slots, so from a part of a wave to several blocks."""
    positions, normals, colors, triangles = dressed(du.noisy_plane(n, seed=n), seed=n)
    got, want = check(gpu, positions, normals, colors, triangles, math.ceil(0.5 * n * n), f"plane({n})")
    if n >= 5:
        assert len(want["positions"]) == math.ceil(0.5 * n * n) and want["rounds"] > 1


def test_an_octahedron_and_a_tetrahedron(gpu):
    got, want = check(gpu, *dressed(du.octahedron()), 0, "octahedron")
    assert len(want["positions"]) == 4 and len(want["triangles"]) == 4, "an octahedron collapses to a tetrahedron and stops"
    got, want = check(gpu, *dressed(du.tetrahedron()), 0, "tetrahedron")
    assert len(want["positions"]) == 4 and len(want["triangles"]) == 4 and want["rounds"] == 1


def test_a_fan_of_valence_70(gpu):
    """The walk around vertex 0 is longer than a wave."""
    got, want = check(gpu, *dressed(du.fan(70)), 30, "fan")
    assert len(want["positions"]) < 71


def test_the_sphere_for_four_rounds(gpu):
    positions, normals, triangles = du.uv_sphere(48, 24)
    _, colors = du.attributes(len(positions), 3)
    got, want = check(gpu, positions, normals, colors, triangles, 300, "sphere", max_rounds=4)
    assert want["rounds"] == 4 and 300 < len(want["positions"]) < len(positions)
    uses, directed = du.edge_counts(got["triangles"])
    assert (uses == 2).all() and (directed == 1).all()


def test_the_roof_to_60_vertices(gpu):
    got, want = check(gpu, *dressed(du.roof()), 60, "roof")
    assert len(got["positions"]) == 60
    assert np.abs(got["positions"][:, 2].astype(np.float64) - du.roof_height(got["positions"][:, 0])).max() <= 1e-6


def test_three_triangles_on_an_edge_degenerate_triangles_and_isolated_vertices(gpu):
    positions, normals, colors, triangles = dressed(du.three_wings())
    got, want = check(gpu, positions, normals, colors, triangles, 0, "three wings, one round", max_rounds=1)
    assert got["vertex_map"][0] != got["vertex_map"][1] and len(got["positions"]) < len(positions), "the edge with three triangles collapsed"
    got, want = check(gpu, positions, normals, colors, triangles, 0, "three wings")
    kept = got["positions"][got["vertex_map"][[8, 9]]]
    assert np.array_equal(bits(kept), bits(positions[[8, 9]])), "an isolated vertex moved"
    got, want = check(gpu, positions, normals, colors, triangles, len(positions), "three wings, identity")
    assert want["rounds"] == 0 and len(want["triangles"]) == 6


@pytest.mark.parametrize("with_map", [False, True])
@pytest.mark.parametrize("with_normals, with_colors", [(False, False), (True, False), (False, True), (True, True)])
def test_pointer_variants(gpu, with_normals, with_colors, with_map):
    positions, normals, colors, triangles = dressed(du.noisy_plane(8, seed=4), seed=4)
    check(gpu, positions, normals if with_normals else None, colors if with_colors else None, triangles, 30, with_map=with_map)


def test_targets_and_empty_meshes(gpu):
    torch, L, ctx = gpu
    positions, normals, colors, triangles = dressed(du.noisy_plane(9, seed=6), seed=6)
    got, want = check(gpu, positions, normals, colors, triangles, 81, "target = V")
    assert want["rounds"] == 0 and np.array_equal(bits(got["positions"]), bits(positions)) and np.array_equal(got["triangles"], triangles)
    assert np.array_equal(got["vertex_map"], np.arange(81)) and np.array_equal(got["colors"], colors) and np.array_equal(bits(got["normals"]), bits(normals))
    check(gpu, positions, normals, colors, triangles, 1000, "target > V")
    got, want = check(gpu, positions, normals, colors, triangles, 0, "target 0")
    assert 0 < len(want["positions"]) < 20
    got, want = check(gpu, positions, normals, colors, None, 10, "T = 0")
    assert len(got["positions"]) == 81 and want["rounds"] == 1
    got = decimate(gpu, np.zeros((0, 3), F), None, None, None, 0)
    assert len(got["positions"]) == 0 and len(got["triangles"]) == 0 and got["rounds"] == 0
    case = Case(torch, np.zeros((0, 3), F), triangles=[[0, 1, 2]])                   # V = 0: every index is beyond
    rc, v, t, r = raw(gpu, case, 0)
    assert rc == INVALID_ARGUMENT and b"bslam_decimate_mesh: a triangle names a vertex beyond vertex_count" in L.bslam_last_error()
    assert (v, t, r) == (SENTINEL, SENTINEL, SENTINEL)
    case.assert_outputs_untouched()


@pytest.mark.parametrize("options", [dict(boundary_weight=0.0), dict(boundary_weight=100.0), dict(max_cost=0.0), dict(max_cost=1e-3), dict(max_rounds=1),
                                     dict(max_rounds=3, boundary_weight=0.5, max_cost=0.5)])
def test_parameters(gpu, options):
    positions, normals, colors, triangles = dressed(du.noisy_plane(9, seed=7), seed=7)
    got, want = check(gpu, positions, normals, colors, triangles, 20, str(options), **options)
    if options == dict(max_cost=0.0):
        assert len(want["positions"]) == 81, "a noisy plane has no edge of cost 0"
    got, want = check(gpu, *dressed(du.roof()), 100, f"roof {options}", **options)
    if "max_rounds" not in options:
        assert len(want["positions"]) == 100, "the roof has edges of cost 0 to spare"


def test_two_calls_agree(gpu):
    positions, normals, colors, triangles = dressed(du.noisy_plane(17, seed=8), seed=8)
    a = decimate(gpu, positions, normals, colors, triangles, 60)
    b = decimate(gpu, positions, normals, colors, triangles, 60)
    assert a["rounds"] == b["rounds"] and len(a["positions"]) == 60
    for k in ("positions", "normals", "colors", "triangles", "vertex_map"):
        assert np.array_equal(bits(a[k]) if a[k].dtype == F else a[k], bits(b[k]) if b[k].dtype == F else b[k]), k


def test_stage_times_with_profiling_on(gpu):
    """Profiling changes no result, a profiled call leaves seven stage sums, and every call resets them at entry.  A context of its
    own: the switch is the context's."""
    torch, L, _ = gpu
    ctx = badslam_amd.Context(0)
    positions, normals, colors, triangles = dressed(du.noisy_plane(9, seed=9), seed=9)
    assert len(positions) == 81 and len(triangles) == 128

    def stage_times():
        ms = (C.c_float * 7)(*[-1.0] * 7)
        badslam_amd.check(L.bslam_decimate_stage_times(ctx.handle, ms))
        return np.array(ms[:], np.float64)

    runs = []
    try:
        for on in (0, 1, 0):
            badslam_amd.check(L.bslam_profile_enable(ctx.handle, on))
            runs.append(decimate(gpu, positions, normals, colors, triangles, 41, ctx=ctx))
            if on:
                ms = stage_times()
                assert np.isfinite(ms).all() and (ms >= 0).all() and (ms > 0).any(), ms
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
        decimate(gpu, np.zeros((0, 3), F), None, None, None, 0, ctx=ctx)
        assert (stage_times() == 0).all(), "the empty mesh did not reset the stage times"
    finally:
        L.bslam_profile_enable(ctx.handle, 0)
    assert len(runs[0]["positions"]) == 41 and runs[0]["rounds"] > 1
    for other in runs[1:]:
        assert other["rounds"] == runs[0]["rounds"]
        for k in ("positions", "normals", "colors", "triangles", "vertex_map"):
            assert np.array_equal(bits(runs[0][k]) if runs[0][k].dtype == F else runs[0][k], bits(other[k]) if other[k].dtype == F else other[k]), k


def test_a_second_call_with_a_larger_mesh_grows_the_slab(gpu):
    """A context of its own, so that its first decimation is the small one."""
    ctx = badslam_amd.Context(0)
    for n in (5, 17, 6):
        positions, normals, colors, triangles = dressed(du.noisy_plane(n, seed=n), seed=n)
        check(gpu, positions, normals, colors, triangles, n * n // 2, f"plane({n})", ctx=ctx)


# ------------------------------------------------------------------------------------------------
# 2. refusals: by the return code, without a fault and without a write
# ------------------------------------------------------------------------------------------------
def test_rejected_arguments(gpu):
    torch, L, ctx = gpu
    positions, normals, colors, triangles = dressed(du.noisy_plane(9, seed=9), seed=9)
    want = du.decimate(positions, normals, colors, triangles, 40)
    case = Case(torch, positions, normals, colors, triangles)
    V, T = case.V, case.T
    vc, tc, rc_ = C.c_uint32(SENTINEL), C.c_uint32(SENTINEL), C.c_uint32(SENTINEL)
    base = dict(ctx=ctx.handle, target=40, weight=1.0, cost=math.inf, vcount=C.byref(vc), tcount=C.byref(tc), rounds=C.byref(rc_))
    base.update({k: b.address for k, b in case.inputs.items()})
    base.update({k: b.address for k, b in case.outputs.items()})

    def run(**changes):
        a = dict(base, **changes)
        p = lambda v: None if v is None else C.c_void_p(v)
        return L.bslam_decimate_mesh(a["ctx"], stream_ptr(torch), V, T, p(a["positions"]), p(a["normals"]), p(a["colors"]), p(a["indices"]), a["target"], a["weight"],
                                     a["cost"], 0, p(a["out_positions"]), p(a["out_normals"]), p(a["out_colors"]), p(a["out_indices"]), p(a["vertex_map"]), a["vcount"],
                                     a["tcount"], a["rounds"])

    a = base
    inf, nan = math.inf, math.nan
    cases = {"null context": dict(ctx=None), "null out_vertex_count": dict(vcount=None), "null out_triangle_count": dict(tcount=None), "null out_rounds": dict(rounds=None),
             "null positions": dict(positions=None), "null indices": dict(indices=None), "null out_positions": dict(out_positions=None),
             "null out_indices": dict(out_indices=None),
             "misaligned positions": dict(positions=a["positions"] + 2), "misaligned normals": dict(normals=a["normals"] + 1), "misaligned colors": dict(colors=a["colors"] + 2),
             "misaligned indices": dict(indices=a["indices"] + 1), "misaligned out_positions": dict(out_positions=a["out_positions"] + 2),
             "misaligned out_normals": dict(out_normals=a["out_normals"] + 3), "misaligned out_colors": dict(out_colors=a["out_colors"] + 1),
             "misaligned out_indices": dict(out_indices=a["out_indices"] + 2), "misaligned vertex_map": dict(vertex_map=a["vertex_map"] + 2),
             "in place: positions": dict(out_positions=a["positions"]), "in place: indices": dict(out_indices=a["indices"]),
             "out_normals inside positions": dict(out_normals=a["positions"] + 12 * V - 4), "vertex_map inside colors": dict(vertex_map=a["colors"] + 4 * V - 4),
             "two outputs overlap": dict(out_normals=a["out_positions"] + 12 * V - 4), "two outputs are one": dict(vertex_map=a["out_colors"]),
             "boundary_weight < 0": dict(weight=-1.0), "boundary_weight = inf": dict(weight=inf), "boundary_weight = NaN": dict(weight=nan),
             "max_cost < 0": dict(cost=-1e-6), "max_cost = NaN": dict(cost=nan), "max_cost = -inf": dict(cost=-inf),
             "normals without out_normals": dict(out_normals=None), "out_normals without normals": dict(normals=None),
             "colors without out_colors": dict(out_colors=None), "out_colors without colors": dict(colors=None)}
    for name, changes in cases.items():
        rc = run(**changes)
        assert rc == INVALID_ARGUMENT, (name, rc, L.bslam_last_error())
    torch.cuda.synchronize()
    case.assert_outputs_untouched()
    case.assert_inputs_untouched()
    assert (vc.value, tc.value, rc_.value) == (SENTINEL, SENTINEL, SENTINEL)
    assert run() == 0 and (vc.value, tc.value, rc_.value) == (len(want["positions"]), len(want["triangles"]), want["rounds"])
    assert_equal(results(case, vc.value, tc.value, rc_.value), want)


@pytest.mark.parametrize("bad", ["V", "0xFFFFFFFF"])
def test_an_index_beyond_the_vertices_is_refused(gpu, bad):
    torch, L, ctx = gpu
    positions, normals, colors, triangles = dressed(du.noisy_plane(17, seed=10), seed=10)
    broken = triangles.copy()
    broken[300, 1] = len(positions) if bad == "V" else 0xFFFFFFFF
    case = Case(torch, positions, normals, colors, broken)
    for target in (100, 1000):                                                       # with rounds and without
        rc, v, t, r = raw(gpu, case, target)
        assert rc == INVALID_ARGUMENT and b"bslam_decimate_mesh: a triangle names a vertex beyond vertex_count" in L.bslam_last_error()
        assert (v, t, r) == (SENTINEL, SENTINEL, SENTINEL)
    case.assert_inputs_untouched()
    case.assert_outputs_untouched()
    with pytest.raises(du.Refused):
        du.decimate(positions, normals, colors, broken, 100)
    check(gpu, positions, normals, colors, triangles, 250, "the context is fine afterwards")


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_a_position_that_is_not_finite_is_refused(gpu, value):
    torch, L, ctx = gpu
    positions, normals, colors, triangles = dressed(du.noisy_plane(17, seed=12), seed=12)
    positions[200, 1] = value
    case = Case(torch, positions, normals, colors, triangles)
    for target in (100, 1000):
        rc, v, t, r = raw(gpu, case, target)
        assert rc == INVALID_ARGUMENT and b"bslam_decimate_mesh: a vertex is not finite" in L.bslam_last_error()
        assert (v, t, r) == (SENTINEL, SENTINEL, SENTINEL)
    case.assert_inputs_untouched()
    case.assert_outputs_untouched()
    with pytest.raises(du.Refused):
        du.decimate(positions, normals, colors, triangles, 100)


# ------------------------------------------------------------------------------------------------
# 3. through DirectBA
# ------------------------------------------------------------------------------------------------
from tests.test_gpu_simplify_mesh import extracted   # noqa: E402,F401  the three-keyframe mesh of tests/test_gpu_fusion.py, fused at 2 cm


def test_direct_ba_decimate_mesh(extracted):   # noqa: F811
    ba, mesh = extracted
    V, T = len(mesh["positions"]), len(mesh["triangles"])
    assert V > 10000 and T > 10000
    got = ba.DecimateMesh(mesh, ratio=0.25, max_rounds=2)
    assert set(got) == set(mesh) | {"vertex_map", "rounds"}
    want = du.decimate(mesh["positions"], mesh["normals"], mesh["colors"], mesh["triangles"], math.ceil(0.25 * V), max_rounds=2)
    assert_equal(got, want, "ratio 0.25, two rounds")
    print(f"{V} vertices, {T} triangles in two rounds -> {len(got['positions'])}, {len(got['triangles'])}")
    assert got["rounds"] == 2 and 0 < len(got["positions"]) < V and 0 < len(got["triangles"]) < T
    labels, sizes = ba.MeshComponents(got)
    assert len(labels) == len(got["positions"]) and sizes.min() >= 1 and (labels <= np.arange(len(labels))).all()
    # to the end: the target is met exactly, and a LoadPLY dict (three colour channels, no normals) is taken as it is
    rgb = np.ascontiguousarray(mesh["colors"][:, :3])
    small = ba.DecimateMesh(dict(positions=mesh["positions"], normals=None, colors=rgb, triangles=mesh["triangles"]), target_vertices=V // 4)
    assert len(small["positions"]) == V // 4 and small["normals"] is None and small["colors"].shape == (V // 4, 3)
    print(f"to {V // 4} vertices in {small['rounds']} rounds, {len(small['triangles'])} triangles")
    with pytest.raises(ValueError, match="exactly one"):
        ba.DecimateMesh(mesh)
    with pytest.raises(ValueError, match="exactly one"):
        ba.DecimateMesh(mesh, target_vertices=10, ratio=0.5)
    with pytest.raises(Exception, match="max_cost"):
        ba.DecimateMesh(mesh, ratio=0.5, max_cost=-1.0)
