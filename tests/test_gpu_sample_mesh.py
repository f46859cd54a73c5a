"""-m gpu: bslam_sample_mesh (badslam_amd/csrc/sampling_kernels.hpp) against the brute-force restatement of
tests/sample_mesh_util.py -- the number of samples, positions, normals and triangle ids, bit for bit: the scan and the searches may
change no result -- and the layers above it: DirectBA.SampleMesh, surface_eval.evaluate(sample_density=...), tools/run_tum.py
--surface-sample-spacing.  Every device array stands between guard words, outputs are filled with a sentinel first and have room
beyond N.

The reason for the feature, measured by test_evaluate_on_the_wall_and_the_strip: a wall of two triangles as the ground truth and a
strip that covers 60 % of it as the reconstruction have the recall 0.5 at 1 cm when measured at the wall's four vertices, and 0.6061
at 10 000 samples of it (analytic 0.60954)."""
import ctypes as C
import json

import numpy as np
import pytest

import badslam_amd
from tests import point_mesh_util as pm
from tests import sample_mesh_util as su
from tests.test_gpu_fusion import SENTINEL, bits, stream_ptr
from tests.test_gpu_mesh_components import Guarded

pytestmark = pytest.mark.gpu
F = np.float32
INVALID_ARGUMENT = -1   # BSLAM_ERR_INVALID_ARGUMENT
SPARE = 7               # output room beyond N, in samples


@pytest.fixture(scope="module")
def gpu():
    import torch
    from badslam_amd import build
    build.build()
    return torch, badslam_amd.lib(), badslam_amd.Context(0)


@pytest.fixture(scope="module")
def sphere():
    return pm.sphere_mesh()


@pytest.fixture(scope="module")
def ba():
    from badslam_amd.direct_ba import DirectBA
    from tests.test_gpu_surface_eval import make_scene
    cam, scene = make_scene()
    ba = DirectBA(scene.max_surfels, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, 0.8, 1, 1, 1, scene.color_camera, scene.depth_camera, 0, True, False)
    yield ba
    ba.close()


_wanted = {}


def wanted(name, positions, triangles, density, seed):
    """The restatement's answer, computed once per (inputs, density, seed) and never changed."""
    key = (name, float(density), int(seed))
    if key not in _wanted:
        _wanted[key] = su.sample_mesh(positions, triangles, density, seed)
    return _wanted[key]


class Mesh:
    """A mesh on the device between guard words."""

    def __init__(self, torch, positions, triangles):
        self.positions, self.triangles = np.ascontiguousarray(positions, F).reshape(-1, 3), np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
        self.V, self.T = len(self.positions), len(self.triangles)
        self.buffers = [Guarded(torch, 3 * self.V, self.positions), Guarded(torch, 3 * self.T, self.triangles)]
        self.before = [b.read() for b in self.buffers]

    def assert_untouched(self):
        for b, was in zip(self.buffers, self.before):
            assert np.array_equal(b.read(), was), "an input was written to"


def raw(gpu, mesh, density, seed, capacity, out_points, out_normals, out_triangles, count):
    torch, L, ctx = gpu
    p = lambda b: None if b is None else b.ptr
    return L.bslam_sample_mesh(ctx.handle, stream_ptr(torch), mesh.V, mesh.buffers[0].ptr, mesh.T, mesh.buffers[1].ptr, float(density), int(seed), int(capacity),
                               p(out_points), p(out_normals), p(out_triangles), C.byref(count))


def count_only(gpu, mesh, density, seed):
    count = C.c_uint64(SENTINEL)
    rc = raw(gpu, mesh, density, seed, 0, None, None, None, count)
    return rc, count.value


def call(gpu, positions, triangles, density, seed, with_normals=True, with_triangles=True):
    """The two calls -> (points [N, 3], normals [N, 3] or None, triangle [N] or None); asserts that the inputs, the guard words and
    the outputs beyond N are untouched."""
    torch, L, ctx = gpu
    mesh = Mesh(torch, positions, triangles)
    rc, N = count_only(gpu, mesh, density, seed)
    badslam_amd.check(rc)
    room = N + SPARE
    out_p, out_n, out_t = Guarded(torch, 3 * room), Guarded(torch, 3 * room) if with_normals else None, Guarded(torch, room) if with_triangles else None
    count = C.c_uint64(SENTINEL)
    badslam_amd.check(raw(gpu, mesh, density, seed, N, out_p, out_n, out_t, count))
    assert count.value == N
    mesh.assert_untouched()
    p, n, t = out_p.read(), None if out_n is None else out_n.read(), None if out_t is None else out_t.read()
    assert (p[3 * N:] == SENTINEL).all() and (n is None or (n[3 * N:] == SENTINEL).all()) and (t is None or (t[N:] == SENTINEL).all()), "written beyond N"
    return p[:3 * N].view(F).reshape(N, 3), None if n is None else n[:3 * N].view(F).reshape(N, 3), None if t is None else t[:N]


def assert_equal(got, want, what=""):
    names = ("positions", "normals", "triangles")
    assert len(got[0]) == len(want[0]), f"{what}: {len(got[0])} samples for {len(want[0])}"
    for name, g, w in zip(names, got, want):
        if g is None:
            continue
        differ = bits(g) != bits(w) if g.dtype == F else g != w
        assert not differ.any(), f"{what}: {int(differ.sum())} {name} differ, first at {np.argwhere(differ)[0]}: {g[differ][0]!r} for {w[differ][0]!r}"


def wall_case(N):
    """(density, seed) at which the restatement draws exactly N samples from the wall: each triangle has x = density / 2."""
    positions, triangles = su.wall()
    density = 1e-9 if N == 0 else float(N)
    seed = next(s for s in range(256) if su.counts(positions, triangles, density, s).sum() == N)
    return density, seed


# ------------------------------------------------------------------------------------------------
# 1. bit for bit with the restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 257])
def test_wall_with_few_samples(gpu, N):
    positions, triangles = su.wall()
    density, seed = wall_case(N)
    want = wanted("wall", positions, triangles, density, seed)
    assert len(want[0]) == N
    assert_equal(call(gpu, positions, triangles, density, seed), want, f"N {N}")


def test_wall_where_whole_waves_share_a_triangle(gpu):
    positions, triangles = su.wall()
    want = wanted("wall", positions, triangles, su.EVAL_DENSITY, su.EVAL_SEED)
    first = int((want[2] == 0).sum())
    assert len(want[0]) == 10000 and first % 64 != 0                    # one wave straddles the two triangles
    assert_equal(call(gpu, positions, triangles, su.EVAL_DENSITY, su.EVAL_SEED), want)


@pytest.mark.parametrize("density", [0.5, 3.0, 40.0])
def test_sphere(gpu, sphere, density):
    positions, triangles = sphere
    want = wanted("sphere", positions, triangles, density, 0)
    assert len(want[0]) == {0.5: 569, 3.0: 3509, 40.0: 46975}[density]     # tests/test_sample_mesh_cpu.py
    assert_equal(call(gpu, positions, triangles, density, 0), want, f"density {density}")


@pytest.fixture(scope="module")
def mixed(sphere):
    """Every third triangle of the sphere's first 900, among them five duplicated ones, triangles of the forms (i, i, i) and (i, i, j),
    triangles with a NaN and an infinite vertex, two large triangles, and degenerate ones at both ends."""
    positions, triangles = sphere
    V = len(positions)
    extra = np.array([[-4, -5, 1], [36, -5, 1], [36, 35, 1], [-4, 35, 1], [np.nan, 3, 3], [np.inf, 1, 1]], F)
    more = np.array([[V, V + 1, V + 2], [V, V + 2, V + 3], [7, 7, 7], [9, 9, 300], [V + 4, 0, 1], [2, V + 5, 3], [5, 6, 5]], np.uint32)
    return (np.ascontiguousarray(np.concatenate([positions, extra]), F),
            np.ascontiguousarray(np.concatenate([more[2:4], triangles[:900:3], triangles[30:45:3], more, triangles[900:1000], more[2:]]), np.uint32))


@pytest.mark.parametrize("density", [0.7, 6.0])
def test_degenerate_non_finite_and_duplicated_triangles(gpu, mixed, density):
    positions, triangles = mixed
    want = wanted("mixed", positions, triangles, density, 11)
    got = call(gpu, positions, triangles, density, 11)
    assert_equal(got, want, f"density {density}")
    count = np.bincount(got[2], minlength=len(triangles))
    tri = triangles.astype(np.int64)
    nothing = (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2]) | ~np.isfinite(positions[tri]).all(axis=(1, 2))
    assert nothing.sum() == 12 and (count[nothing] == 0).all() and count[~nothing].sum() == len(got[0]) > 1000 * density
    if density == 6.0:                                                    # a duplicate gets samples of its own
        original, copy = got[0][got[2] == 2 + 10], got[0][got[2] == 2 + 300]
        assert np.array_equal(triangles[12], triangles[302]) and len(original) and len(copy) and not np.array_equal(original[:1], copy[:1])


def test_empty_meshes(gpu, sphere):
    torch, L, ctx = gpu
    positions, triangles = sphere
    none3, no_triangles = np.zeros((0, 3), F), np.zeros((0, 3), np.uint32)
    for pos in (positions, none3):                                        # T = 0, and V = 0 with it
        got = call(gpu, pos, no_triangles, 5.0, 1)
        assert len(got[0]) == 0
    rc, N = count_only(gpu, Mesh(torch, none3, triangles[:4]), 5.0, 1)    # no vertex at all: every index is beyond
    assert rc == INVALID_ARGUMENT and b"beyond vertex_count" in L.bslam_last_error() and N == SENTINEL
    got = call(gpu, np.full((3, 3), np.nan, F), np.array([[0, 1, 2]], np.uint32), 5.0, 1)
    assert len(got[0]) == 0


def test_without_the_optional_outputs(gpu, sphere):
    positions, triangles = sphere
    want = wanted("sphere", positions, triangles, 3.0, 0)
    got = call(gpu, positions, triangles, 3.0, 0, with_normals=False, with_triangles=False)
    assert got[1] is None and got[2] is None
    assert_equal(got, want)
    assert_equal(call(gpu, positions, triangles, 3.0, 0, with_normals=False), want)


# ------------------------------------------------------------------------------------------------
# 2. capacity and determinism
# ------------------------------------------------------------------------------------------------
def test_capacity_and_two_calls(gpu, sphere):
    torch, L, ctx = gpu
    positions, triangles = sphere
    want = wanted("sphere", positions, triangles, 3.0, 0)
    N = len(want[0])
    mesh = Mesh(torch, positions, triangles)
    outs = [Guarded(torch, 3 * (N + SPARE)), Guarded(torch, 3 * (N + SPARE)), Guarded(torch, N + SPARE)]
    untouched = lambda: all((b.read() == SENTINEL).all() for b in outs)
    count = C.c_uint64(SENTINEL)
    assert raw(gpu, mesh, 3.0, 0, N + SPARE, None, outs[1], outs[2], count) == 0 and count.value == N and untouched()      # no out_points: the count alone
    for capacity in (0, N - 1):
        count = C.c_uint64(SENTINEL)
        assert raw(gpu, mesh, 3.0, 0, capacity, *outs, count) == 0 and count.value == N and untouched()
    first = call(gpu, positions, triangles, 3.0, 0)
    second = call(gpu, positions, triangles, 3.0, 0)
    assert_equal(first, want)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, second))
    other = call(gpu, positions, triangles, 3.0, 1)
    assert len(other[0]) != N or not np.array_equal(other[0], first[0])
    count = C.c_uint64(SENTINEL)
    assert raw(gpu, mesh, 3.0, 0, N + 3, *outs, count) == 0 and count.value == N                # more room than needed
    assert_equal((outs[0].read()[:3 * N].view(F).reshape(N, 3), outs[1].read()[:3 * N].view(F).reshape(N, 3), outs[2].read()[:N]), want)
    assert (outs[0].read()[3 * N:] == SENTINEL).all() and (outs[2].read()[N:] == SENTINEL).all()
    mesh.assert_untouched()


# ------------------------------------------------------------------------------------------------
# 3. refusals
# ------------------------------------------------------------------------------------------------
def test_rejected_arguments(gpu, sphere):
    torch, L, ctx = gpu
    positions, triangles = sphere
    want = wanted("sphere", positions, triangles, 3.0, 0)
    N, V, T = len(want[0]), len(positions), len(triangles)
    b = dict(positions=Guarded(torch, 3 * V, positions), indices=Guarded(torch, 3 * T, triangles), out_points=Guarded(torch, 3 * N), out_normals=Guarded(torch, 3 * N),
             out_triangles=Guarded(torch, N))
    count = C.c_uint64(SENTINEL)
    base = dict(ctx=ctx.handle, density=3.0, count=C.byref(count), **{k: v.address for k, v in b.items()})

    def run(**changes):
        a = dict(base, **changes)
        p = lambda v: None if v is None else C.c_void_p(v)
        return L.bslam_sample_mesh(a["ctx"], stream_ptr(torch), V, p(a["positions"]), T, p(a["indices"]), a["density"], 0, N, p(a["out_points"]), p(a["out_normals"]),
                                   p(a["out_triangles"]), a["count"])

    a = base
    cases = {"null context": dict(ctx=None), "null sample_count": dict(count=None), "null positions": dict(positions=None), "null indices": dict(indices=None),
             "misaligned positions": dict(positions=a["positions"] + 1), "misaligned indices": dict(indices=a["indices"] + 2),
             "misaligned out_points": dict(out_points=a["out_points"] + 2), "misaligned out_normals": dict(out_normals=a["out_normals"] + 1),
             "misaligned out_triangles": dict(out_triangles=a["out_triangles"] + 3), "in place: positions": dict(out_points=a["positions"]),
             "out_normals inside positions": dict(out_normals=a["positions"] + 12 * V - 4), "out_triangles inside indices": dict(out_triangles=a["indices"] + 8),
             "the outputs overlap": dict(out_normals=a["out_points"] + 12 * N - 4), "two outputs are one": dict(out_triangles=a["out_normals"]),
             "density = 0": dict(density=0.0), "density < 0": dict(density=-1.0), "density = inf": dict(density=float("inf")), "density = NaN": dict(density=float("nan"))}
    for name, changes in cases.items():
        rc = run(**changes)
        assert rc == INVALID_ARGUMENT, (name, rc, L.bslam_last_error())
    torch.cuda.synchronize()
    assert all((b[k].read() == SENTINEL).all() for k in ("out_points", "out_normals", "out_triangles")), "a refused call wrote to an output"
    assert count.value == SENTINEL
    assert np.array_equal(b["positions"].read(), bits(positions).reshape(-1))
    assert run() == 0 and count.value == N
    assert_equal((b["out_points"].read().view(F).reshape(N, 3), b["out_normals"].read().view(F).reshape(N, 3), b["out_triangles"].read()), want)


@pytest.mark.parametrize("bad", ["V", "0xFFFFFFFF"])
def test_an_index_beyond_the_vertices_is_refused_behind_the_count_pass(gpu, sphere, bad):
    torch, L, ctx = gpu
    positions, triangles = sphere
    tri = triangles.copy()
    tri[1777, 2] = len(positions) if bad == "V" else 0xFFFFFFFF
    mesh = Mesh(torch, positions, tri)
    outs = [Guarded(torch, 3 * 4000), Guarded(torch, 3 * 4000), Guarded(torch, 4000)]
    count = C.c_uint64(SENTINEL)
    assert raw(gpu, mesh, 3.0, 0, 4000, *outs, count) == INVALID_ARGUMENT and b"bslam_sample_mesh: a triangle names a vertex beyond vertex_count" in L.bslam_last_error()
    assert all((b.read() == SENTINEL).all() for b in outs) and count.value == SENTINEL
    mesh.assert_untouched()
    assert_equal(call(gpu, positions, triangles, 3.0, 0), wanted("sphere", positions, triangles, 3.0, 0))       # the context is fine afterwards


def test_more_samples_than_a_launch_holds_are_refused(gpu, ba):
    torch, L, ctx = gpu
    positions, triangles = su.wall()
    total = int(su.counts(positions, triangles, 1e10, 0).sum())
    assert total == 1 << 33 and total > su.MAX_SAMPLES
    mesh = Mesh(torch, positions, triangles)
    outs = [Guarded(torch, 3 * 64), Guarded(torch, 3 * 64), Guarded(torch, 64)]
    count = C.c_uint64(SENTINEL)
    rc = raw(gpu, mesh, 1e10, 0, 64, *outs, count)
    message = L.bslam_last_error()
    assert rc == INVALID_ARGUMENT and str(total).encode() in message and b"density" in message, message
    assert count.value == total and all((b.read() == SENTINEL).all() for b in outs)
    with pytest.raises(Exception, match=str(total)):                      # the object stops at the count call: nothing is allocated for the samples
        ba.SampleMesh(dict(positions=positions, triangles=triangles), density=1e10)
    # just below the limit the count call goes through (and nothing is written without room)
    below = su.MAX_SAMPLES // 2 - 1000.0
    want = int(su.counts(positions, triangles, 2 * below, 0).sum())
    count = C.c_uint64(SENTINEL)
    assert raw(gpu, mesh, 2 * below, 0, 64, *outs, count) == 0 and count.value == want <= su.MAX_SAMPLES and all((b.read() == SENTINEL).all() for b in outs)


def test_a_distance_call_in_between_disturbs_nothing(gpu, sphere):
    from tests.test_gpu_point_mesh import call as distance_call
    positions, triangles = sphere
    points = pm.sphere_points(positions, triangles)
    want = wanted("sphere", positions, triangles, 40.0, 0)
    assert_equal(call(gpu, positions, triangles, 40.0, 0), want)
    rc, d, t, _, _ = distance_call(gpu, points, positions, triangles, 2.0, 1.0)
    assert rc == 0
    assert_equal(call(gpu, positions, triangles, 40.0, 0), want)
    rc, d2, t2, _, _ = distance_call(gpu, points, positions, triangles, 2.0, 1.0)
    assert rc == 0 and np.array_equal(bits(d), bits(d2)) and np.array_equal(t, t2)


# ------------------------------------------------------------------------------------------------
# 4. DirectBA.SampleMesh
# ------------------------------------------------------------------------------------------------
def test_direct_ba_sample_mesh(gpu, ba, sphere):
    positions, triangles = sphere
    mesh = dict(positions=positions, triangles=triangles)
    got = ba.SampleMesh(mesh, density=3.0)
    assert got["positions"].dtype == F and got["normals"].dtype == F and got["triangle"].dtype == np.uint32 and got["positions"].shape == (3509, 3)
    assert_equal((got["positions"], got["normals"], got["triangle"]), call(gpu, positions, triangles, 3.0, 0))
    by_spacing, by_density = ba.SampleMesh(mesh, spacing=0.25, seed=4), ba.SampleMesh(mesh, density=16.0, seed=4)
    assert all(np.array_equal(bits(by_spacing[k]), bits(by_density[k])) for k in ("positions", "normals", "triangle"))
    assert_equal((by_density["positions"], by_density["normals"], by_density["triangle"]), wanted("sphere", positions, triangles, 16.0, 4))
    for arguments in (dict(), dict(density=1.0, spacing=1.0)):
        with pytest.raises(ValueError):
            ba.SampleMesh(mesh, **arguments)
    for cloud in (dict(positions=positions), dict(positions=positions, triangles=np.zeros((0, 3), np.uint32))):
        assert ba.SampleMesh(cloud, density=3.0)["positions"].shape == (0, 3)
    with pytest.raises(Exception, match="beyond vertex_count"):
        ba.SampleMesh(dict(positions=positions[:100], triangles=triangles), density=3.0)


# ------------------------------------------------------------------------------------------------
# 5. surface_eval.evaluate(sample_density=...): the wall as the ground truth, the strip as the reconstruction
# ------------------------------------------------------------------------------------------------
def test_evaluate_on_the_wall_and_the_strip(ba):
    from badslam_amd import surface_eval
    wall_positions, wall_triangles = su.wall()
    strip_positions, strip_triangles = su.strip()
    wall, strip = dict(positions=wall_positions, triangles=wall_triangles), dict(positions=strip_positions, triangles=strip_triangles)
    samples = ba.SampleMesh(wall, density=su.EVAL_DENSITY, seed=su.EVAL_SEED)
    want = wanted("wall", wall_positions, wall_triangles, su.EVAL_DENSITY, su.EVAL_SEED)
    assert_equal((samples["positions"], samples["normals"], samples["triangle"]), want)
    closed_form = su.wall_to_strip_distance(want[0])
    distance = ba.PointMeshDistance(samples["positions"], strip, 0.5)["distance"]
    print(f"largest difference to the closed form {np.abs(distance - closed_form).max():.3e}")
    assert np.abs(distance - closed_form).max() <= 1e-6
    r = surface_eval.evaluate(ba, strip, wall, 0.5, su.EVAL_THRESHOLDS, sample_density=su.EVAL_DENSITY, sample_seed=su.EVAL_SEED)
    strip_samples = int(su.counts(strip_positions, strip_triangles, su.EVAL_DENSITY, su.EVAL_SEED).sum())
    assert r["sampling"] == dict(density=su.EVAL_DENSITY, seed=su.EVAL_SEED, reconstruction_samples=strip_samples, ground_truth_samples=10000)
    assert r["completeness"]["count"] == 10000 and r["accuracy"]["count"] == strip_samples
    recall = [float((closed_form <= t).mean()) for t in su.EVAL_THRESHOLDS]     # no sample lies on a threshold: tests/test_sample_mesh_cpu.py
    assert [row["recall"] for row in r["f_scores"]] == recall and abs(recall[0] - su.ANALYTIC_RECALL) <= 0.02
    assert [row["precision"] for row in r["f_scores"]] == [1.0, 1.0, 1.0]
    plain = surface_eval.evaluate(ba, strip, wall, 0.5, su.EVAL_THRESHOLDS)
    print(f"recall at 1 cm: {plain['f_scores'][0]['recall']} at the wall's vertices, {recall[0]:.4f} at {r['completeness']['count']} samples; analytic {su.ANALYTIC_RECALL:.5f}")
    assert "sampling" not in plain and plain["f_scores"][0]["recall"] == 0.5 and plain["f_scores"][0]["precision"] == 1.0


# ------------------------------------------------------------------------------------------------
# 6. tools/run_tum.py --surface-sample-spacing
# ------------------------------------------------------------------------------------------------
def test_run_tum_surface_sample_spacing(tmp_path):
    """Five frames of the rendered sequence of tests/test_gpu_bad_slam.py, the mesh (--mesh, 4 cm) evaluated against itself at
    samples 2 cm apart: the report carries the sampling, and both numbers of samples are what the area asks for."""
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
    mesh_path, report_path = tmp_path / "mesh.ply", tmp_path / "surface.json"
    spacing = 0.02
    # the mesh is written before the ground truth is read: the run is evaluated against its own mesh
    r = run_tum.run(source, mesh=mesh_path, ground_truth_surface=mesh_path, surface_report=report_path, surface_sample_spacing=spacing, keyframe_interval=4,
                    ba_iterations=2, max_depth=6.0, num_scales=4, max_surfel_count=400000, mesh_voxel_size=0.04, mesh_min_count=2, mesh_min_component=50)
    report = json.loads(report_path.read_text())
    own = dba.LoadPLY(mesh_path)
    density = 1.0 / spacing ** 2
    x = su.areas64(own["positions"], own["triangles"]) * density
    bound = su.count_bound(x)
    sampling = report["sampling"]
    print(f"{r['mesh']['triangles']} triangles of {x.sum() / density:.3f} m^2: {sampling['reconstruction_samples']} and {sampling['ground_truth_samples']} samples for "
          f"{x.sum():.1f} +- {bound:.1f}")
    assert sampling == r["surface"]["sampling"] and sampling["density"] == density and sampling["seed"] == 0
    assert r["mesh"]["triangles"] > 1000 and x.sum() > 1000
    for n in (sampling["reconstruction_samples"], sampling["ground_truth_samples"]):
        assert abs(n - x.sum()) <= bound
    assert report["accuracy"]["count"] == sampling["reconstruction_samples"] and report["completeness"]["count"] == sampling["ground_truth_samples"]
    assert report["accuracy"]["median"] < 1e-6 and report["f_scores"][0]["f_score"] == 1.0           # a mesh against itself
    a = run_tum.arg_parser().parse_args(["x"])
    assert a.surface_sample_spacing is None
    assert run_tum.arg_parser().parse_args(["x", "--surface-sample-spacing", "0.005"]).surface_sample_spacing == 0.005
