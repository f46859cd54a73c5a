"""-m gpu: bslam_orient_mesh (badslam_amd/csrc/orient_kernels.hpp) against the breadth-first restatement of tests/orient_mesh_util.py --
out_indices, flipped, patch_of_triangle and every word of the report bit for bit: neither the sort nor which thread won which swap of
the parity union-find may change a result -- and the layers above: DirectBA.OrientMesh and tools/run_tum.py --mesh-orient.  Every
device array stands between guard words; outputs are filled with a sentinel first, and a refused call leaves them at it.  The shapes are
the smallest at which the kernels can go wrong: the sphere with two holes (3346 triangles, 10038 slots: several workgroups and scan
tiles), bands of 2048 triangles with shuffled ids (parent chains as long as the band, a conflict that only the seam that closes the
ring reveals), and 704 loose pieces (waves whose 64 lanes hold 64 roots)."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi
from tests import mesh_repair_util as ru
from tests import orient_mesh_util as ou
from tests.test_gpu_fusion import SENTINEL, bits, stream_ptr
from tests.test_gpu_mesh_components import Guarded
from tests.test_gpu_mesh_repair import topology
from tests.test_gpu_simplify_mesh import extracted   # noqa: F401  (the fixture: a DirectBA and its extracted mesh)

pytestmark = pytest.mark.gpu
F = np.float32
INVALID_ARGUMENT = -1   # BSLAM_ERR_INVALID_ARGUMENT
MODE = abi.ORIENT_MODES
SMALL = ["sphere 0, 30 % flipped", "sphere 0, 70 % flipped", "quad with one of two flipped", "cube inside out", "cube with 5 flipped", "sphere 2, all flipped",
         "sphere 2, all flipped, negated normals", "sphere 2, zero normals", "Moebius band of 16", "Moebius band of 16, half flipped", "ring of 16", "book", "concat of the parts"]
LARGE = ["sphere 2, half flipped, shuffled", "ring of 2048, half flipped, shuffled", "Moebius band of 2048, half flipped, shuffled", "confetti", "concat, shuffled"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    from badslam_amd import build
    build.build()
    return torch, badslam_amd.lib(), badslam_amd.Context(0)


def mixed(mesh, share, seed, shuffled=True):
    """`mesh` with a seeded share of its triangles flipped and, with `shuffled`, its triangle ids permuted."""
    p, n, t = mesh
    t = ou.flip(t, ou.seeded_mask(len(t), share, seed))
    return p, n, ou.shuffle(t, seed + 100)[0] if shuffled else t


@pytest.fixture(scope="module")
def meshes():
    """name -> (positions, normals, triangles)."""
    s0, s2, (cp, cn, ct), (mp, mn, mt) = ou.sphere(0), ou.sphere(2), ou.cube(), ou.strip(16, twist=True)
    every = lambda t: np.ones(len(t), bool)
    quad = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], F), np.tile(np.array([0, 0, 1], F), (4, 1)), np.array([[0, 1, 2], [1, 2, 3]], np.uint32))
    out = {"sphere 0, 30 % flipped": mixed(s0, 0.3, 1, shuffled=False), "sphere 0, 70 % flipped": mixed(s0, 0.7, 2, shuffled=False), "quad with one of two flipped": quad,
           "cube inside out": (cp, cn, ou.flip(ct, every(ct))), "cube with 5 flipped": mixed((cp, cn, ct), 5 / 12, 3, shuffled=False),
           "sphere 2, all flipped": (s2[0], s2[1], ou.flip(s2[2], every(s2[2]))), "sphere 2, all flipped, negated normals": (s2[0], -s2[1], ou.flip(s2[2], every(s2[2]))),
           "sphere 2, zero normals": (s2[0], np.zeros_like(s2[1]), s2[2]), "Moebius band of 16": (mp, mn, mt), "Moebius band of 16, half flipped": mixed((mp, mn, mt), 0.5, 4, shuffled=False),
           "ring of 16": ou.strip(16, twist=False), "book": ou.book()}
    out["concat of the parts"] = ou.concat(*[out[k] for k in ("sphere 0, 30 % flipped", "Moebius band of 16, half flipped", "cube inside out", "book")], ou.confetti(5, 4, seed=6),
                                           out["sphere 2, all flipped"])
    out["sphere 2, half flipped, shuffled"] = mixed(s2, 0.5, 7)
    out["ring of 2048, half flipped, shuffled"] = mixed(ou.strip(2048, twist=False), 0.5, 8)
    out["Moebius band of 2048, half flipped, shuffled"] = mixed(ou.strip(2048, twist=True), 0.5, 9)
    out["confetti"] = ou.confetti(640, 64, seed=10)
    out["sphere 0"], out["sphere 2"] = s0, s2
    out["concat, shuffled"] = mixed(ou.concat(out["sphere 0, 30 % flipped"], out["Moebius band of 16, half flipped"], out["cube inside out"], ou.book(), out["confetti"]), 0.0, 11)
    return out


@pytest.fixture(scope="module")
def expected(meshes):
    """(name, mode) -> the restatement's result, computed once."""
    cache = {}

    def get(name, mode):
        if (name, mode) not in cache:
            cache[name, mode] = ou.orient(*meshes[name], mode)
        return cache[name, mode]
    return get


def p_(b):
    return None if b is None else b.ptr


class Call:
    """One bslam_orient_mesh call on host arrays: inputs and sentinel-filled outputs between guard words."""

    def __init__(self, gpu, positions, normals, triangles, with_flipped=True, with_patches=True):
        self.torch, self.L, self.ctx = gpu
        torch = self.torch
        self.positions, self.normals, _, self.triangles = ru._arrays(positions, normals, None, triangles)
        V, T = self.V, self.T = len(self.positions), len(self.triangles)
        self.dev = dict(positions=Guarded(torch, 3 * V, self.positions), normals=None if self.normals is None else Guarded(torch, 3 * V, self.normals),
                        indices=Guarded(torch, 3 * T, self.triangles))
        self.before = {k: b.read() for k, b in self.dev.items() if b is not None}
        self.out = dict(out_indices=Guarded(torch, 3 * T), flipped=Guarded(torch, (T + 3) // 4) if with_flipped else None, patch_of_triangle=Guarded(torch, T) if with_patches else None)
        self.report = abi.OrientReport()
        self.report.patches = 77

    def run(self, mode, ctx=None, stream=None, **changes):
        """-> the return code; changes: argument name -> address (None: null), report=None for a null report, normals=None."""
        a = {k: None if b is None else b.address for k, b in {**self.dev, **self.out}.items()}
        if MODE.get(mode, mode) != 1:
            a["normals"] = None
        report = changes.pop("report", C.byref(self.report))
        a.update(changes)
        p = lambda v: None if v is None else C.c_void_p(v)
        handle = changes.get("handle", (ctx or self.ctx).handle)
        return self.L.bslam_orient_mesh(handle, stream or stream_ptr(self.torch), self.V, self.T, p(a["positions"]), p(a["normals"]), p(a["indices"]), MODE.get(mode, mode),
                                        p(a["out_indices"]), p(a["flipped"]), p(a["patch_of_triangle"]), report)

    def result(self):
        """The outputs; asserts that the inputs are as they were and that nothing beyond the last triangle's flag was written."""
        for k, was in self.before.items():
            assert np.array_equal(self.dev[k].read(), was), f"{k} was written to"
        got = dict(triangles=self.out["out_indices"].read().reshape(self.T, 3), report={k: int(getattr(self.report, k)) for k in ou.REPORT_FIELDS})
        if self.out["flipped"] is not None:
            flags = self.out["flipped"].read().view(np.uint8)
            assert (flags[self.T:] == 0x5A).all(), "flipped was written beyond the last triangle"
            got["flipped"] = flags[:self.T].copy()
        if self.out["patch_of_triangle"] is not None:
            got["patch_of_triangle"] = self.out["patch_of_triangle"].read()
        return got

    def assert_untouched(self):
        self.torch.cuda.synchronize()
        for k, b in self.out.items():
            assert b is None or (b.read() == SENTINEL).all(), f"a refused call wrote to {k}"
        for k, was in self.before.items():
            assert np.array_equal(self.dev[k].read(), was), f"{k} was written to"
        assert self.report.patches == 77 and self.report.seams == 0, "a refused call wrote the report"


def orient(gpu, mesh, mode, **kwargs):
    call = Call(gpu, *mesh, **{k: kwargs.pop(k) for k in ("with_flipped", "with_patches") if k in kwargs})
    badslam_amd.check(call.run(mode, **kwargs))
    return call.result()


def assert_equal(got, want, what):
    assert got["report"] == want["report"], f"{what}: {got['report']} for {want['report']}"
    for k in ("triangles", "flipped", "patch_of_triangle"):
        if k not in got:
            continue
        differ = np.asarray(got[k]) != np.asarray(want[k]).reshape(np.asarray(got[k]).shape)
        assert not differ.any(), f"{what}: {int(differ.sum())} {k} differ, first at {np.argwhere(differ)[0]}: {got[k][differ][0]!r} for {np.asarray(want[k]).reshape(got[k].shape)[differ][0]!r}"


# ------------------------------------------------------------------------------------------------
# 1. bit for bit with the restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ou.MODES)
@pytest.mark.parametrize("name", SMALL + LARGE)
def test_orient(gpu, meshes, expected, name, mode):
    want = expected(name, mode)
    got = orient(gpu, meshes[name], mode)
    assert_equal(got, want, f"{name}, {mode}")
    r = got["report"]
    if name.startswith("Moebius"):
        assert np.array_equal(got["triangles"], meshes[name][2]) and (r["nonorientable_patches"], r["flipped_triangles"]) == (1, 0)
        assert r["disagreeing_seams_after"] == r["disagreeing_seams_before"] > 0
    if name == "confetti":
        assert (r["patches"], r["seams"], r["nonorientable_patches"]) == (704, 64, 0)
    if name == "concat, shuffled":
        assert (r["patches"], r["nonorientable_patches"], r["closed_patches"]) == (1 + 1 + 1 + 3 + 704, 1, 2)
    if name.startswith("sphere 0"):
        assert np.array_equal(got["triangles"], meshes["sphere 0"][2]) == (mode != "majority" or "30" in name)
    # the census of the device agrees, and orienting the output on the device flips nothing
    inconsistent = topology(gpu, len(meshes[name][0]), got["triangles"], per_slot=False)[0]["inconsistent_edges"]
    assert inconsistent == r["disagreeing_seams_after"] and (inconsistent == 0) == (r["nonorientable_patches"] == 0)
    again = orient(gpu, (meshes[name][0], meshes[name][1], got["triangles"]), mode)
    assert again["report"]["flipped_triangles"] == 0 and np.array_equal(again["triangles"], got["triangles"]) and np.array_equal(again["patch_of_triangle"], got["patch_of_triangle"])


def test_the_report_of_a_concatenation_is_the_sum_of_the_parts(gpu, meshes):
    names = ("sphere 0, 30 % flipped", "Moebius band of 16, half flipped", "cube inside out", "book", "confetti")
    whole = orient(gpu, ou.concat(*[meshes[k] for k in names]), "volume")
    base, vertices, total = 0, 0, dict.fromkeys(ou.REPORT_FIELDS, 0)
    for k in names:
        part = orient(gpu, meshes[k], "volume")
        rows = slice(base, base + len(part["triangles"]))
        assert np.array_equal(whole["patch_of_triangle"][rows], part["patch_of_triangle"] + base), k
        assert np.array_equal(whole["flipped"][rows], part["flipped"]) and np.array_equal(whole["triangles"][rows], part["triangles"] + vertices), k
        total = {f: total[f] + part["report"][f] for f in total}
        base, vertices = base + len(part["triangles"]), vertices + len(meshes[k][0])
    assert whole["report"] == total


@pytest.mark.parametrize("mode", ou.MODES)
def test_two_calls_and_a_second_stream_agree(gpu, meshes, mode):
    torch = gpu[0]
    mesh = meshes["Moebius band of 2048, half flipped, shuffled"] if mode == "majority" else meshes["concat, shuffled"]
    first, second = orient(gpu, mesh, mode), orient(gpu, mesh, mode)
    side = torch.cuda.Stream()
    call = Call(gpu, *mesh)
    torch.cuda.synchronize()
    badslam_amd.check(call.run(mode, stream=C.c_void_p(side.cuda_stream)))
    third = call.result()
    for other in (second, third):
        assert other["report"] == first["report"]
        for k in ("triangles", "flipped", "patch_of_triangle"):
            assert np.array_equal(other[k], first[k]), k


@pytest.mark.parametrize("without", ["flipped", "patch_of_triangle", "both"])
def test_optional_outputs(gpu, meshes, expected, without):
    name = "sphere 2, half flipped, shuffled"
    got = orient(gpu, meshes[name], "normals", with_flipped=without == "patch_of_triangle", with_patches=without == "flipped")
    assert ("flipped" in got, "patch_of_triangle" in got) == (without == "patch_of_triangle", without == "flipped")
    assert_equal(got, expected(name, "normals"), f"without {without}")


@pytest.mark.parametrize("mode", ou.MODES)
def test_empty_meshes(gpu, mode):
    for V in (0, 7):
        got = orient(gpu, (np.ones((V, 3), F), np.ones((V, 3), F), np.zeros((0, 3), np.uint32)), mode)
        assert not any(got["report"].values()) and len(got["triangles"]) == 0


def test_a_flat_mesh_falls_back(gpu):
    """Every vertex in one point: the extent is zero, no volume is added, the majority decides."""
    mesh = (np.full((4, 3), 2.5, F), None, np.array([[0, 1, 2], [1, 2, 3], [0, 3, 1], [0, 2, 3]], np.uint32))
    got = orient(gpu, mesh, "volume")
    assert_equal(got, ou.orient(*mesh, "volume"), "flat")
    assert got["report"]["fallback_patches"] == 1 and got["report"]["closed_patches"] == 1


def test_stage_times_with_profiling_on(gpu, meshes, expected):
    """Profiling changes no result, and a profiled call leaves the times of its seven stages.  A context of its own: the switch is the context's."""
    torch, L, _ = gpu
    ctx = badslam_amd.Context(0)
    name = "sphere 2, half flipped, shuffled"
    try:
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
        assert_equal(orient(gpu, meshes[name], "volume", ctx=ctx), expected(name, "volume"), "profiled")
        ms = (C.c_float * 8)(*[-1.0] * 8)
        badslam_amd.check(L.bslam_repair_stage_times(ctx.handle, ms))
        ms = np.array(ms[:], np.float64)
        assert np.isfinite(ms).all() and (ms[:7] > 0).all() and ms[7] == 0, ms
    finally:
        L.bslam_profile_enable(ctx.handle, 0)


# ------------------------------------------------------------------------------------------------
# 2. refusals: by the return code, without a fault and without a write
# ------------------------------------------------------------------------------------------------
def test_rejected_arguments(gpu, meshes):
    L = gpu[1]
    call = Call(gpu, *meshes["sphere 2, half flipped, shuffled"])
    a = {k: b.address for k, b in {**call.dev, **call.out}.items()}
    T = call.T
    cases = {"null context": dict(handle=None), "null report": dict(report=None), "null positions": dict(positions=None), "null indices": dict(indices=None),
             "null out_indices": dict(out_indices=None), "misaligned positions": dict(positions=a["positions"] + 2), "misaligned indices": dict(indices=a["indices"] + 1),
             "misaligned out_indices": dict(out_indices=a["out_indices"] + 2), "misaligned flipped": dict(flipped=a["flipped"] + 1),
             "misaligned patch_of_triangle": dict(patch_of_triangle=a["patch_of_triangle"] + 2), "in place": dict(out_indices=a["indices"]),
             "out_indices inside positions": dict(out_indices=a["positions"]), "flipped inside out_indices": dict(flipped=a["out_indices"] + 12 * T - 4),
             "patch_of_triangle inside indices": dict(patch_of_triangle=a["indices"] + 12 * T - 4), "flipped inside patch_of_triangle": dict(flipped=a["patch_of_triangle"] + 4 * T - 4)}
    for name, changes in cases.items():
        rc = call.run("majority", **changes)
        assert rc == INVALID_ARGUMENT, (name, rc, L.bslam_last_error())
    for mode in (3, -1, 255):
        assert call.run(mode) == INVALID_ARGUMENT and b"mode must be" in L.bslam_last_error(), mode
    assert call.run("normals", normals=None) == INVALID_ARGUMENT and b"needs normals" in L.bslam_last_error()
    assert call.run("normals", out_indices=a["normals"]) == INVALID_ARGUMENT, "out_indices inside the normals of mode 1"
    call.assert_untouched()
    assert call.run("majority") == 0 and call.report.patches == 1
    # the normals are not looked at in the other modes: they may be anything, also the place of an output
    other = Call(gpu, *meshes["cube inside out"])
    assert other.run("volume", normals=other.out["out_indices"].address) == 0 and other.result()["report"]["flipped_triangles"] == 12


@pytest.mark.parametrize("what", ["index = V", "index = 0xFFFFFFFF", "NaN position", "infinite position", "repeated index"])
def test_device_refusals_leave_the_outputs_untouched(gpu, meshes, expected, what):
    L = gpu[1]
    name = "sphere 2, half flipped, shuffled"
    p, n, t = meshes[name]
    p, t = p.copy(), t.copy()
    if what.startswith("index"):
        t[1500, 1] = len(p) if what == "index = V" else 0xFFFFFFFF
        message = b"a triangle names a vertex beyond vertex_count"
    elif what == "repeated index":
        t[1500, 2] = t[1500, 0]
        message = b"a triangle repeats an index"
    else:
        p[777, 1] = np.nan if what == "NaN position" else -np.inf
        message = b"a vertex is not finite"
    for mode in ou.MODES:
        call = Call(gpu, p, n, t)
        rc = call.run(mode)
        assert rc == INVALID_ARGUMENT and b"bslam_orient_mesh: " + message in L.bslam_last_error(), (mode, rc, L.bslam_last_error())
        call.assert_untouched()
    assert_equal(orient(gpu, meshes[name], "volume"), expected(name, "volume"), "the context is fine afterwards")


# ------------------------------------------------------------------------------------------------
# 3. through DirectBA
# ------------------------------------------------------------------------------------------------
def as_dict(mesh, colors=None):
    p, n, t = mesh
    return dict(positions=p, normals=n, colors=colors, triangles=t)


@pytest.mark.parametrize("mode", ou.MODES)
def test_direct_ba_orient_mesh(extracted, meshes, expected, mode):   # noqa: F811
    ba, _ = extracted
    name = "concat, shuffled"
    mesh = meshes[name]
    colors = np.random.default_rng(5).integers(0, 256, (len(mesh[0]), 3), dtype=np.uint8)
    got = ba.OrientMesh(as_dict(mesh, colors), mode=mode, report=True)
    assert set(got) == {"positions", "normals", "colors", "triangles", "flipped", "patch_of_triangle", "report"} and got["flipped"].dtype == bool
    assert_equal(dict(got, flipped=got["flipped"].astype(np.uint8)), expected(name, mode), f"OrientMesh, {mode}")
    assert np.array_equal(bits(got["positions"]), bits(mesh[0])) and np.array_equal(bits(got["normals"]), bits(mesh[1])) and np.array_equal(got["colors"], colors)
    assert "report" not in ba.OrientMesh(as_dict(mesh), mode=mode)


def test_direct_ba_recomputed_normals_and_refusals(extracted, meshes):   # noqa: F811
    ba, _ = extracted
    mesh = as_dict(meshes["sphere 2, all flipped"])
    got = ba.OrientMesh(mesh, mode="normals", recompute_normals=True)
    assert np.array_equal(got["triangles"], meshes["sphere 2"][2])
    want = ba.MeshNormals(dict(mesh, triangles=got["triangles"]))["normals"]
    assert np.array_equal(bits(got["normals"]), bits(want)) and not np.array_equal(bits(got["normals"]), bits(mesh["normals"]))
    assert (np.einsum("ij,ij->i", got["normals"], mesh["normals"]) > 0).mean() > 0.99, "the recomputed normals point where the input's do"
    bare = dict(positions=mesh["positions"], triangles=mesh["triangles"])
    assert ba.OrientMesh(bare, mode="volume")["normals"] is None
    with pytest.raises(ValueError, match="normals"):
        ba.OrientMesh(bare, mode="normals")
    with pytest.raises(ValueError, match="mode"):
        ba.OrientMesh(mesh, mode="outward")
    broken = mesh["triangles"].copy()
    broken[5, 2] = broken[5, 0]
    with pytest.raises(Exception, match="repeats an index"):
        ba.OrientMesh(dict(mesh, triangles=broken))
    empty = ba.OrientMesh(dict(positions=np.zeros((0, 3), F), triangles=np.zeros((0, 3), np.uint32)), report=True)
    assert len(empty["triangles"]) == 0 and not any(empty["report"].values())


@pytest.mark.parametrize("name", ["cube", "sphere 0"])
def test_weld_flip_orient_render(extracted, meshes, name):   # noqa: F811
    """A soup is welded, a seeded half of its triangles is flipped: with back faces culled the view has holes; oriented by volume it is
    the view of the clean mesh, bit for bit."""
    ba, _ = extracted
    p, n, t = ou.cube() if name == "cube" else meshes["sphere 0"]
    p = p * F(1.0 / float((p.max(axis=0) - p.min(axis=0)).max()))   # an extent of one: the depth image is 16 bits at 5000 per metre
    clean = ba.CleanMesh(dict(zip(("positions", "normals", "colors", "triangles"), ru.soup(p, n, None, t))))
    assert len(clean["positions"]) == len(p) and len(clean["triangles"]) == len(t)
    flipped = dict(clean, triangles=ou.flip(clean["triangles"], ou.seeded_mask(len(t), 0.5, 12)))
    centre, extent = p.mean(axis=0), float((p.max(axis=0) - p.min(axis=0)).max())
    pose = abi.SE3f((C.c_float * 4)(0, 0, 0, 1), (C.c_float * 3)(float(centre[0]), float(centre[1]), float(centre[2]) - 3.0 * extent))
    cam = abi.Camera4f(60.0, 60.0, 30.5, 22.5, 61, 45)
    view = lambda m: ba.RenderMesh(m, pose, camera=cam, min_depth=0.05, max_depth=10.0 * extent, cull_backfaces=True, views=("depth",))["depth"]
    want = view(clean)
    assert (want != 0).sum() > 100 and not np.array_equal(view(flipped), want)
    assert ba.MeshTopology(flipped)["inconsistent_edges"] > 0
    got = ba.OrientMesh(flipped, mode="volume", report=True)
    assert np.array_equal(got["triangles"], clean["triangles"]) and got["report"]["disagreeing_seams_after"] == 0
    assert view(got).tobytes() == want.tobytes()
    assert ba.MeshTopology(got)["inconsistent_edges"] == 0


# ------------------------------------------------------------------------------------------------
# 4. tools/run_tum.py --mesh-orient
# ------------------------------------------------------------------------------------------------
def test_run_tum_mesh_orient(tmp_path):
    """Five frames of the rendered sequence of tests/test_gpu_bad_slam.py with --mesh, --mesh-orient volume and --surface-report: the
    report holds the counts, they are the restatement's of the extracted mesh, and the file is the oriented mesh."""
    import json

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
    common = dict(keyframe_interval=4, ba_iterations=2, max_depth=6.0, num_scales=4, max_surfel_count=400000, mesh_voxel_size=0.04, mesh_min_count=2, mesh_min_component=50)
    seen = {}

    def inspect(slam, result):
        seen["extracted"] = slam.ba().ExtractMesh(2, min_component_vertices=50)

    mesh_path, report_path = tmp_path / "mesh.ply", tmp_path / "report.json"
    r = run_tum.run(source, mesh=mesh_path, mesh_orient="volume", surface_report=report_path, inspect=inspect, **common)
    report = json.loads(report_path.read_text())
    mo = report["mesh_orientation"]
    assert set(mo) == set(ou.REPORT_FIELDS) | {"mode"} and mo["mode"] == "volume" and r["mesh"]["orientation"] == mo
    m = seen["extracted"]
    want = ou.orient(m["positions"], m["normals"], m["triangles"], "volume")
    assert {k: mo[k] for k in ou.REPORT_FIELDS} == want["report"]
    own = dba.LoadPLY(mesh_path)
    assert np.array_equal(own["triangles"], want["triangles"]) and np.array_equal(bits(own["positions"]), bits(m["positions"]))
    print(f"orientation: {mo}, topology: {report['mesh_topology']}")
    assert mo["patches"] >= 1 and report["mesh_topology"]["inconsistent_edges"] == mo["disagreeing_seams_after"]
    with pytest.raises(ValueError, match="--mesh-orient"):
        run_tum.run(source, mesh=mesh_path, mesh_orient="outward", **common)
