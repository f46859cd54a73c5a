"""-m gpu: bslam_smooth_mesh (badslam_amd/csrc/smooth_kernels.hpp) against the restatement of tests/smooth_mesh_util.py -- positions bit
for bit, normals within 1e-6 (the normal takes a square root; the decimation tolerance): the sorts, the head flags and the scan may
change no result -- and DirectBA.SmoothMesh / MeshNormals above it.  Every device array stands between guard words; outputs are
filled with a sentinel first and must still hold it after a refused call."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from tests import decimate_mesh_util as du
from tests import smooth_mesh_util as mu_
from tests.test_gpu_fusion import SENTINEL, bits, stream_ptr
from tests.test_gpu_mesh_components import Guarded

pytestmark = pytest.mark.gpu
F = np.float32
INVALID_ARGUMENT = -1   # BSLAM_ERR_INVALID_ARGUMENT
NORMAL_TOLERANCE = 1e-6
MODES = (0, 1, 2)


@pytest.fixture(scope="module")
def gpu():
    import torch
    from badslam_amd import build
    build.build()
    return torch, badslam_amd.lib(), badslam_amd.Context(0)


class Case:
    """A mesh on the device between guard words, and sentinel-filled outputs with room for V vertices."""

    def __init__(self, torch, positions, normals=None, triangles=None, with_out_normals=True):
        self.positions = np.ascontiguousarray(positions, F).reshape(-1, 3)
        self.normals = None if normals is None else np.ascontiguousarray(normals, F).reshape(-1, 3)
        self.triangles = np.zeros((0, 3), np.uint32) if triangles is None else np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
        V, T = self.V, self.T = len(self.positions), len(self.triangles)
        self.inputs = dict(positions=Guarded(torch, 3 * V, self.positions), normals=None if normals is None else Guarded(torch, 3 * V, self.normals),
                           indices=Guarded(torch, 3 * T, self.triangles))
        self.outputs = dict(out_positions=Guarded(torch, 3 * V), out_normals=Guarded(torch, 3 * V) if with_out_normals else None)
        self.before = {k: b.read() for k, b in self.inputs.items() if b is not None}

    def assert_inputs_untouched(self):
        for k, was in self.before.items():
            assert np.array_equal(self.inputs[k].read(), was), f"{k} was written to"

    def assert_outputs_untouched(self):
        for k, b in self.outputs.items():
            assert b is None or (b.read() == SENTINEL).all(), f"a refused call wrote to {k}"


def raw(gpu, case, iterations=10, lambda_=0.5, mu=-0.53, mode=0, ctx=None):
    torch, L, default_ctx = gpu
    p = lambda b: None if b is None else b.ptr
    i, out = case.inputs, case.outputs
    return L.bslam_smooth_mesh((ctx or default_ctx).handle, stream_ptr(torch), case.V, case.T, p(i["positions"]), p(i["normals"]), p(i["indices"]), int(iterations),
                               float(lambda_), float(mu), int(mode), p(out["out_positions"]), p(out["out_normals"]))


def results(case):
    o = {k: None if b is None else b.read().view(F).reshape(case.V, 3) for k, b in case.outputs.items()}
    return o["out_positions"], o["out_normals"]


def smooth(gpu, positions, normals, triangles, with_out_normals=True, ctx=None, **options):
    torch, L, _ = gpu
    case = Case(torch, positions, normals, triangles, with_out_normals)
    badslam_amd.check(raw(gpu, case, ctx=ctx, **options))
    case.assert_inputs_untouched()
    return results(case)


def assert_equal(got, want, what=""):
    (gp, gn), (wp, wn) = got, want
    assert gp.shape == wp.shape, what
    differ = bits(gp) != bits(wp)
    assert not differ.any(), f"{what}: {int(differ.sum())} position coordinates differ, first at {np.argwhere(differ)[0]}: {gp[differ][0]!r} for {wp[differ][0]!r}"
    assert (gn is None) == (wn is None), what
    if gn is not None and len(gn):
        error = np.abs(gn.astype(np.float64) - wn.astype(np.float64)).max()
        assert error <= NORMAL_TOLERANCE, f"{what}: normals differ by {error:.3e}"


def check(gpu, positions, normals, triangles, what="", with_out_normals=True, ctx=None, **options):
    want = mu_.smooth(positions, normals, triangles, want_normals=with_out_normals, **options)
    got = smooth(gpu, positions, normals, triangles, with_out_normals=with_out_normals, ctx=ctx, **options)
    assert_equal(got, want, f"{what} {options}")
    return got, want


def unit_normals(V, seed=0):
    return du.attributes(V, seed)[0]


# ------------------------------------------------------------------------------------------------
# 1. bit for bit with the restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(2, 18))
def test_noisy_planes(gpu, n):
    """4 to 289 vertices, so one lane up to more than one block of 256, with counts that are no multiple of 64; every mode with 0, 1
    and 3 iterations, and mu = 0 once."""
    positions, triangles = mu_.noisy_plane(n, seed=n)
    normals = unit_normals(n * n, n)
    for mode in MODES:
        for iterations in (0, 1, 3):
            got, want = check(gpu, positions, normals, triangles, f"plane({n})", iterations=iterations, mode=mode)
            if iterations == 0:
                assert np.array_equal(bits(got[0]), bits(positions))
    check(gpu, positions, normals, triangles, f"plane({n})", iterations=2, mu=0.0, mode=n % 3)


def test_a_tetrahedron_an_octahedron_and_a_single_triangle(gpu):
    for name, (positions, triangles) in (("tetrahedron", mu_.tetrahedron()), ("octahedron", mu_.octahedron())):
        for mode in MODES:
            got, want = check(gpu, positions, None, triangles, name, iterations=2, mode=mode)
            assert (bits(got[0]) != bits(positions)).any(axis=1).all(), "a closed mesh has no boundary: every vertex moves"
    positions, triangles = np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, 0.25]], F), np.array([[0, 1, 2]], np.uint32)
    for mode in MODES:
        got, want = check(gpu, positions, None, triangles, "one triangle", iterations=2, mode=mode)
        assert np.array_equal(bits(got[0]), bits(positions)) == (mode == 0)


def test_a_fan_of_valence_70(gpu):
    """The list of vertex 0 is longer than a wave."""
    positions, triangles = mu_.fan(70)
    for mode in MODES:
        got, want = check(gpu, positions, None, triangles, "fan", iterations=3, mode=mode)
    assert (bits(got[0][0]) != bits(positions[0])).any()


def test_the_noisy_sphere_for_three_iterations(gpu):
    positions, clean, normals, triangles, centre = mu_.noisy_sphere()
    got, want = check(gpu, positions, normals, triangles, "sphere", iterations=3)
    assert mu_.radii(got[0], centre).std() < mu_.radii(positions, centre).std()
    check(gpu, positions, normals, triangles, "sphere", iterations=3, mu=0.0, lambda_=1.0)


def test_three_triangles_on_an_edge_degenerate_triangles_and_isolated_vertices(gpu):
    positions, triangles = mu_.three_wings()
    normals = unit_normals(len(positions), 2)
    for mode in MODES:
        got, want = check(gpu, positions, normals, triangles, "three wings", iterations=3, mode=mode)
        assert np.array_equal(bits(got[0][[8, 9]]), bits(positions[[8, 9]])), "an isolated vertex moved"
        assert np.array_equal(bits(got[1][[8, 9]]), bits(normals[[8, 9]])), "an isolated vertex keeps the input normal"
    positions, triangles = mu_.zero_fan()
    normals = unit_normals(len(positions), 3)
    got, want = check(gpu, positions, normals, triangles, "zero fan", iterations=0)
    assert np.array_equal(bits(got[1][[0, 5]]), bits(normals[[0, 5]]))
    got, want = check(gpu, positions, None, triangles, "zero fan without normals", iterations=0)
    assert not got[1][[0, 5]].any()


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("with_out_normals", [False, True])
def test_pointer_variants(gpu, with_normals, with_out_normals):
    positions, triangles = mu_.noisy_plane(8, seed=4)
    normals = unit_normals(64, 4) if with_normals else None
    got, want = check(gpu, positions, normals, triangles, with_out_normals=with_out_normals, iterations=2, mode=1)
    assert (got[1] is None) == (not with_out_normals)


def test_point_clouds_and_the_empty_mesh(gpu):
    torch, L, ctx = gpu
    positions, _ = mu_.noisy_plane(9, seed=6)
    normals = unit_normals(81, 6)
    got, want = check(gpu, positions, normals, None, "T = 0", iterations=3, mode=2)
    assert np.array_equal(bits(got[0]), bits(positions)) and np.array_equal(bits(got[1]), bits(normals))
    got, want = check(gpu, positions, None, None, "T = 0 without normals", iterations=3)
    assert np.array_equal(bits(got[0]), bits(positions)) and not got[1].any()
    got = smooth(gpu, np.zeros((0, 3), F), None, None)
    assert got[0].shape == (0, 3)
    case = Case(torch, np.zeros((0, 3), F), triangles=[[0, 1, 2]])                   # V = 0: every index is beyond
    assert raw(gpu, case) == INVALID_ARGUMENT and b"bslam_smooth_mesh: a triangle names a vertex beyond vertex_count" in L.bslam_last_error()


def test_two_calls_agree(gpu):
    positions, triangles = mu_.noisy_plane(17, seed=8)
    a = smooth(gpu, positions, None, triangles, iterations=5, mode=1)
    b = smooth(gpu, positions, None, triangles, iterations=5, mode=1)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


def test_stage_times_with_profiling_on(gpu):
    """Profiling changes no result, a profiled call leaves five stage times, and every call resets them at entry.  A context of its
    own: the switch is the context's."""
    torch, L, _ = gpu
    ctx = badslam_amd.Context(0)
    positions, triangles = mu_.noisy_plane(9, seed=9)
    normals = unit_normals(81, 9)
    assert len(positions) == 81 and len(triangles) == 128

    def stage_times():
        ms = (C.c_float * 5)(*[-1.0] * 5)
        badslam_amd.check(L.bslam_smooth_stage_times(ctx.handle, ms))
        return np.array(ms[:], np.float64)

    runs = []
    try:
        for on in (0, 1, 0):
            badslam_amd.check(L.bslam_profile_enable(ctx.handle, on))
            runs.append(smooth(gpu, positions, normals, triangles, ctx=ctx, iterations=2))
            if on:
                ms = stage_times()
                assert np.isfinite(ms).all() and (ms >= 0).all() and (ms > 0).any(), ms
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
        smooth(gpu, np.zeros((0, 3), F), None, None, ctx=ctx, iterations=2)
        assert (stage_times() == 0).all(), "the empty mesh did not reset the stage times"
    finally:
        L.bslam_profile_enable(ctx.handle, 0)
    assert (bits(runs[0][0]) != bits(positions)).any()
    for other in runs[1:]:
        assert np.array_equal(bits(runs[0][0]), bits(other[0])) and np.array_equal(bits(runs[0][1]), bits(other[1]))


def test_small_large_small_on_one_context(gpu):
    """A context of its own, so that its first smoothing is the small one and the slab grows."""
    ctx = badslam_amd.Context(0)
    for n in (5, 17, 6):
        positions, triangles = mu_.noisy_plane(n, seed=n)
        check(gpu, positions, None, triangles, f"plane({n})", ctx=ctx, iterations=2, mode=2)


# ------------------------------------------------------------------------------------------------
# 2. refusals: by the return code, without a fault and without a write
# ------------------------------------------------------------------------------------------------
def test_rejected_arguments(gpu):
    torch, L, ctx = gpu
    positions, triangles = mu_.noisy_plane(9, seed=9)
    normals = unit_normals(81, 9)
    want = mu_.smooth(positions, normals, triangles, iterations=2)
    case = Case(torch, positions, normals, triangles)
    V, T = case.V, case.T
    base = dict(ctx=ctx.handle, iterations=2, lambda_=0.5, mu=-0.53, mode=0)
    base.update({k: b.address for k, b in case.inputs.items()})
    base.update({k: b.address for k, b in case.outputs.items()})

    def run(**changes):
        a = dict(base, **changes)
        p = lambda v: None if v is None else C.c_void_p(v)
        return L.bslam_smooth_mesh(a["ctx"], stream_ptr(torch), V, T, p(a["positions"]), p(a["normals"]), p(a["indices"]), a["iterations"], a["lambda_"], a["mu"], a["mode"],
                                   p(a["out_positions"]), p(a["out_normals"]))

    a = base
    inf, nan = float("inf"), float("nan")
    cases = {"null context": dict(ctx=None), "null positions": dict(positions=None), "null indices": dict(indices=None), "null out_positions": dict(out_positions=None),
             "lambda = 0": dict(lambda_=0.0), "lambda < 0": dict(lambda_=-0.5), "lambda > 1": dict(lambda_=1.5), "lambda = inf": dict(lambda_=inf), "lambda = NaN": dict(lambda_=nan),
             "mu > 0": dict(mu=0.1), "mu < -1": dict(mu=-1.5), "mu = -inf": dict(mu=-inf), "mu = NaN": dict(mu=nan),
             "boundary_mode 3": dict(mode=3), "boundary_mode 2^32 - 1": dict(mode=0xFFFFFFFF), "65536 iterations": dict(iterations=65536),
             "misaligned positions": dict(positions=a["positions"] + 2), "misaligned normals": dict(normals=a["normals"] + 1), "misaligned indices": dict(indices=a["indices"] + 1),
             "misaligned out_positions": dict(out_positions=a["out_positions"] + 2), "misaligned out_normals": dict(out_normals=a["out_normals"] + 3),
             "in place: positions": dict(out_positions=a["positions"]), "in place: normals": dict(out_normals=a["normals"]),
             "out_normals inside positions": dict(out_normals=a["positions"] + 12 * V - 4), "out_positions inside indices": dict(out_positions=a["indices"] + 12 * T - 4),
             "two outputs overlap": dict(out_normals=a["out_positions"] + 12 * V - 4), "two outputs are one": dict(out_normals=a["out_positions"])}
    for name, changes in cases.items():
        rc = run(**changes)
        assert rc == INVALID_ARGUMENT, (name, rc, L.bslam_last_error())
    torch.cuda.synchronize()
    case.assert_outputs_untouched()
    case.assert_inputs_untouched()
    for name in ("lambda = 0", "mu > 0", "boundary_mode 3", "65536 iterations"):
        options = {k: v for k, v in cases[name].items()}
        with pytest.raises(mu_.Refused):
            mu_.check_parameters(options.get("iterations", 2), options.get("lambda_", 0.5), options.get("mu", -0.53), options.get("mode", 0))
    assert run() == 0
    assert_equal(results(case), want)
    assert run(lambda_=1.0, mu=-1.0, mode=2, iterations=1) == 0 and run(mu=-0.0) == 0, "the ends of the ranges are legal"


def test_too_many_vertices_or_adjacency_entries_are_refused_before_anything_is_read(gpu):
    torch, L, ctx = gpu
    positions, triangles = mu_.noisy_plane(3)
    case = Case(torch, positions, None, triangles)
    i, out = case.inputs, case.outputs
    for V, T in ((0xFFFFFF01, 1), (9, 0xFFFFFF00 // 6 + 1)):
        rc = L.bslam_smooth_mesh(ctx.handle, stream_ptr(torch), V, T, i["positions"].ptr, None, i["indices"].ptr, 1, 0.5, -0.53, 0, out["out_positions"].ptr, None)
        assert rc == INVALID_ARGUMENT and b"2^32 - 256" in L.bslam_last_error()
    case.assert_outputs_untouched()


@pytest.mark.parametrize("bad", ["V", "0xFFFFFFFF"])
def test_an_index_beyond_the_vertices_is_refused(gpu, bad):
    torch, L, ctx = gpu
    positions, triangles = mu_.noisy_plane(17, seed=10)
    broken = triangles.copy()
    broken[300, 1] = len(positions) if bad == "V" else 0xFFFFFFFF
    case = Case(torch, positions, None, broken)
    for iterations in (0, 2):
        assert raw(gpu, case, iterations=iterations) == INVALID_ARGUMENT
        assert b"bslam_smooth_mesh: a triangle names a vertex beyond vertex_count" in L.bslam_last_error()
    case.assert_inputs_untouched()
    case.assert_outputs_untouched()
    with pytest.raises(mu_.Refused):
        mu_.smooth(positions, None, broken, iterations=1)
    check(gpu, positions, None, triangles, "the context is fine afterwards", iterations=1)


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_a_position_that_is_not_finite_is_refused(gpu, value):
    torch, L, ctx = gpu
    positions, triangles = mu_.noisy_plane(17, seed=12)
    positions[200, 1] = value
    for tri in (triangles, None):                                                    # a point cloud is checked too
        case = Case(torch, positions, None, tri)
        for iterations in (0, 2):
            assert raw(gpu, case, iterations=iterations) == INVALID_ARGUMENT and b"bslam_smooth_mesh: a vertex is not finite" in L.bslam_last_error()
        case.assert_inputs_untouched()
        case.assert_outputs_untouched()
    with pytest.raises(mu_.Refused):
        mu_.smooth(positions, None, triangles, iterations=1)


# ------------------------------------------------------------------------------------------------
# 3. through DirectBA
# ------------------------------------------------------------------------------------------------
from tests.test_gpu_simplify_mesh import extracted   # noqa: E402,F401  the three-keyframe mesh of tests/test_gpu_fusion.py, fused at 2 cm


def test_direct_ba_smooth_mesh(extracted):   # noqa: F811
    ba, mesh = extracted
    V, T = len(mesh["positions"]), len(mesh["triangles"])
    assert V > 10000 and T > 10000
    got = ba.SmoothMesh(mesh, iterations=2)
    assert set(got) == set(mesh)
    want = mu_.smooth(mesh["positions"], mesh["normals"], mesh["triangles"], iterations=2)
    assert_equal((got["positions"], got["normals"]), want, "two iterations")
    assert np.array_equal(got["colors"], mesh["colors"]) and np.array_equal(got["triangles"], mesh["triangles"])
    moved = (bits(got["positions"]) != bits(mesh["positions"])).any(axis=1)
    cosine = (got["normals"].astype(np.float64) * mesh["normals"]).sum(axis=1)
    print(f"{V} vertices, {T} triangles: {int(moved.sum())} moved; geometric against volume normals: median cosine {np.median(cosine):.4f}")
    # both are normals of one surface, the volume's from its gradient and these from facets of 2 cm: a median within 8 degrees
    # (measured: 0.9994) is wrong as soon as a part of the mesh is turned over
    assert moved.sum() > V // 2 and np.median(cosine) > 0.99, "the geometric normals point the way the volume's do"
    # the same on the mesh ExtractMesh left on the device: no upload, and no input normals to fall back on
    on_device = ba.SmoothExtractedMesh(iterations=2)
    smoothed = [tuple(float(x) for x in p) for p in want[0]]
    assert_equal(on_device, (want[0], mu_.vertex_normals(smoothed, None, V, mesh["triangles"])), "the device mesh")
    # SmoothMesh, then DecimateMesh, then MeshComponents
    small = ba.DecimateMesh(got, ratio=0.25, max_rounds=2)
    assert 0 < len(small["positions"]) < V
    labels, sizes = ba.MeshComponents(small)
    assert len(labels) == len(small["positions"]) and sizes.min() >= 1
    # MeshNormals of a DecimateMesh output, here without input normals and with three colour channels
    bare = dict(positions=small["positions"], normals=None, colors=np.ascontiguousarray(small["colors"][:, :3]), triangles=small["triangles"])
    normals = ba.MeshNormals(bare)
    want = mu_.smooth(bare["positions"], None, bare["triangles"], iterations=0)
    assert_equal((normals["positions"], normals["normals"]), want, "MeshNormals")
    assert np.array_equal(bits(normals["positions"]), bits(small["positions"])) and normals["colors"].shape == (len(small["positions"]), 3)
    other = ba.SmoothMesh(mesh, iterations=1, lambda_=0.4, mu=0.0, boundary="rim")
    assert_equal((other["positions"], other["normals"]), mu_.smooth(mesh["positions"], mesh["normals"], mesh["triangles"], 1, 0.4, 0.0, mu_.MODES["rim"]), "rim")
    with pytest.raises(ValueError, match="boundary"):
        ba.SmoothMesh(mesh, boundary="open")
    with pytest.raises(Exception, match="lambda"):
        ba.SmoothMesh(mesh, lambda_=0.0)
