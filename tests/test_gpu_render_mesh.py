"""-m gpu: the mesh views (bslam_render_mesh, badslam_amd/csrc/render_mesh_kernels.hpp; DirectBA.RenderMesh; tools/run_tum.py
--render-source mesh) against the NumPy float32 restatement of tests/render_mesh_util.py: depth, index and colour bit for bit, the
normal view at 1e-6.  Never against the kernel's own output, except where a test is about two calls agreeing.  Through the C ABI
the output images are pitched wider than their content and filled with sentinels; triangle counts are no multiple of 64."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi
from tests import render_mesh_util as mu
from tests import render_util as ru
from tests.test_gpu_render import VIEWS, device_view, fetch_view, stream_ptr, untouched

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT = -1   # BSLAM_ERR_INVALID_ARGUMENT
MIN_DEPTH, MAX_DEPTH, SCALE = 0.5, 4.0, 5000.0


@pytest.fixture(scope="module")
def gpu():
    import torch
    from badslam_amd import build
    build.build()
    return torch, badslam_amd.lib(), badslam_amd.Context(0)


# ------------------------------------------------------------------------------------------------
# device plumbing
# ------------------------------------------------------------------------------------------------
class Call:
    """A mesh on the device and four sentinel-filled pitched output images; run() is one bslam_render_mesh, every argument of which
    can be replaced by name."""

    def __init__(self, gpu, mesh, T, cam, ctx=None):
        self.torch, self.L, own = gpu
        self.ctx = ctx or own
        self.cam, self.M = cam, ru.mat3x4(T)
        up = lambda a: self.torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.positions, self.triangles = up(mesh["positions"]), up(np.ascontiguousarray(mesh["triangles"], np.uint32).view(np.int32))
        self.normals = up(mesh["normals"]) if mesh.get("normals") is not None else None
        self.colors = up(mesh["colors"]) if mesh.get("colors") is not None else None
        self.V, self.T = len(mesh["positions"]), len(mesh["triangles"])
        self.images = {name: device_view(self.torch, name, cam) for name in VIEWS}

    def run(self, wanted=VIEWS, with_normals=True, with_colors=True, **replace):
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        a = dict(ctx=self.ctx.handle, stream=stream_ptr(self.torch), camera_T_global=C.byref(self.M), camera=C.byref(self.cam), vertex_count=self.V,
                 positions=ptr(self.positions), normals=ptr(self.normals) if with_normals else None, colors=ptr(self.colors) if with_colors else None, triangle_count=self.T,
                 indices=ptr(self.triangles), min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, cull_backfaces=1, metres_to_depth=SCALE)
        for name in VIEWS:
            a["out_" + name] = C.byref(self.images[name][1]) if name in wanted else None
        assert set(replace) <= set(a), set(replace) - set(a)
        a.update(replace)
        rc = self.L.bslam_render_mesh(*a.values())
        self.torch.cuda.synchronize()
        return rc

    def fetch(self, wanted=VIEWS):
        """{view: image} of the wanted views; asserts that padding and unwanted images keep their sentinel."""
        out = {}
        for name in VIEWS:
            image, padding = fetch_view(name, self.images[name][0], self.cam)
            assert untouched(name, padding), f"{name}: padding written"
            if name in wanted:
                out[name] = image
            else:
                assert untouched(name, self.images[name][0].cpu().numpy()), f"{name}: written although not asked for"
        return out

    def all_untouched(self):
        return all(untouched(name, self.images[name][0].cpu().numpy()) for name in VIEWS)


def gpu_views(gpu, mesh, T, cam, wanted=VIEWS, ctx=None, **arguments):
    call = Call(gpu, mesh, T, cam, ctx)
    badslam_amd.check(call.run(wanted, **arguments))
    return call.fetch(wanted)


def assert_equal_to_restatement(got, want, label=""):
    for name in ("depth", "index", "color"):
        if name in got:
            differ = got[name] != want[name]
            assert not differ.any(), f"{label}{name}: {int(differ.sum())} values differ, first at {np.argwhere(differ)[0]}: {got[name][differ][:4]} != {want[name][differ][:4]}"
    if "normal" in got:
        assert np.abs(got["normal"].astype(np.float64) - want["normal"]).max() <= 1e-6, f"{label}normal"


def view_pose(seed):
    """camera_T_global, (3, 4) float32, and its float64 inverse."""
    rng = np.random.default_rng(seed)
    T = np.hstack([ru.rotation(rng.normal(size=3), 0.3), rng.uniform(-0.5, 0.5, (3, 1))]).astype(np.float32)
    return T, ru.invert(T)


def to_global(mesh, G):
    """A mesh built in the camera's frame, moved into the global frame."""
    out = dict(mesh)
    out["positions"] = (mesh["positions"].astype(np.float64) @ G[:, :3].T + G[:, 3]).astype(np.float32)
    if mesh.get("normals") is not None:
        out["normals"] = (mesh["normals"].astype(np.float64) @ G[:, :3].T).astype(np.float32)
    return out


def restate(mesh, T, cam, cull_backfaces=1, **drop):
    mesh = {k: v for k, v in mesh.items() if k not in drop}
    return mu.render32(mesh, T, cam, MIN_DEPTH, MAX_DEPTH, cull_backfaces, SCALE)


# ------------------------------------------------------------------------------------------------
# a. the mesh of ExtractMesh, seen from a keyframe
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused_ba():
    """Three 160 x 120 keyframes of tests/scenes.py fused at 5 cm through the public interface, and the extracted mesh."""
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
    voxel, truncation = 0.05, 0.2
    origin, dims = run_tum.mesh_volume(*ba.ModelBounds(), voxel, truncation)
    ba.FuseKeyframes(origin, voxel, dims, truncation)
    mesh = ba.ExtractMesh(1)
    print(f"extracted mesh: {len(mesh['positions'])} vertices, {len(mesh['triangles'])} triangles")
    yield ba, scene, mesh
    ba.close()


def small_camera(ba):
    """The depth camera scaled to 61 x 45, a size that is no multiple of anything."""
    fx, fy, cx, cy = [float(v) for v in ba.intrinsics()[1]]
    return abi.Camera4f(fx * 61 / 160, fy * 45 / 120, cx * 61 / 160, cy * 45 / 120, 61, 45)


def test_extracted_mesh_from_a_keyframe_and_the_facing_sign(gpu, fused_ba):
    ba, scene, mesh = fused_ba
    count = len(mesh["triangles"])
    assert 1000 < count < 20000 and count % 64 != 0
    cam = small_camera(ba)
    T = ba.RenderMesh(mesh, ba.keyframe_pose(0), camera=cam, views=("depth",))["camera_T_global"]      # the matrix the host hands the kernels for keyframe 0
    got = gpu_views(gpu, mesh, T, cam, max_depth=6.0, metres_to_depth=1.0 / scene.raw_to_float_depth)
    want = mu.render32(mesh, T, cam, MIN_DEPTH, 6.0, 1, 1.0 / scene.raw_to_float_depth)
    assert_equal_to_restatement(got, want)
    share = (got["index"] != mu.NO_INDEX).mean()
    print(f"{count} triangles, {share:.3f} of the pixels drawn with back faces culled")
    assert share > 0.5, "front-facing is A < 0: seen from a keyframe most of an extracted mesh faces the camera"


# ------------------------------------------------------------------------------------------------
# b. the cooperative path
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cooperative():
    mesh, cam = mu.cooperative_scene()
    T, G = view_pose(3)
    mesh = to_global(mesh, G)
    return mesh, T, cam, restate(mesh, T, cam)


def test_one_large_triangle_among_small_ones(gpu, cooperative):
    mesh, T, cam, want = cooperative
    assert (want["index"] == 37).mean() > 0.4 and len(np.unique(want["index"])) > 60
    below, above = want["index"][want["index"] < 37], want["index"][(want["index"] > 37) & (want["index"] != mu.NO_INDEX)]
    assert len(below) and (above < 64).any() and (above >= 64).any()
    first = gpu_views(gpu, mesh, T, cam)
    assert_equal_to_restatement(first, want)
    again = gpu_views(gpu, mesh, T, cam)
    for name in VIEWS:
        assert first[name].tobytes() == again[name].tobytes(), name


def test_reversed_triangle_order(gpu, cooperative):
    mesh, T, cam, want = cooperative
    count = len(mesh["triangles"])
    reverse = dict(mesh, triangles=np.ascontiguousarray(mesh["triangles"][::-1]))
    got = gpu_views(gpu, reverse, T, cam)
    assert np.array_equal(got["depth"], want["depth"]) and np.array_equal(got["color"], want["color"])
    drawn = want["index"] != mu.NO_INDEX
    assert np.array_equal(got["index"][drawn], count - 1 - want["index"][drawn]) and (got["index"][~drawn] == mu.NO_INDEX).all()


INT_MAX = (1 << 31) - 1


@pytest.mark.parametrize("tuning", [(0, INT_MAX, 1, 1), (0, 1024, 1, 0), (0, 0, 1, 1), (16, 200, 0, 0), (1 << 20, 0, 0, 0), (64, 256, 1, 1)])
def test_tuning_changes_no_bit(gpu, cooperative, tuning):
    """(small_box, wave_box, project_once, resolve_reads_projected): every box by its wave; the small ones by their wave and the large
    one through the queue; every box through the queue; thresholds in between; every box by its lane; the defaults with the vertex
    pass.  All give the bits of the restatement."""
    mesh, T, cam, want = cooperative
    ctx = badslam_amd.Context(0)
    badslam_amd.check(gpu[1].bslam_set_render_mesh_tuning(ctx.handle, *tuning))
    assert_equal_to_restatement(gpu_views(gpu, mesh, T, cam, ctx=ctx), want)
    assert gpu[1].bslam_set_render_mesh_tuning(ctx.handle, 64, 1024, 0, 1) == INVALID_ARGUMENT and gpu[1].bslam_set_render_mesh_tuning(ctx.handle, -1, 1024, 1, 1) == INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------
# c. what is dropped
# ------------------------------------------------------------------------------------------------
def test_edge_cases_in_one_mesh(gpu):
    mesh, cam, case = mu.edge_case_scene(MIN_DEPTH, MAX_DEPTH)
    T, G = view_pose(8)
    mesh = to_global(mesh, G)
    want = restate(mesh, T, cam)
    dropped = [case[name] for name in mu.EDGE_CASES if name != "cut by the border"]
    assert not np.isin(want["index"], dropped).any() and (want["index"] == case["cut by the border"]).sum() > 50
    got = gpu_views(gpu, mesh, T, cam)
    assert_equal_to_restatement(got, want)
    assert not np.isin(got["index"], dropped).any()
    assert_equal_to_restatement(gpu_views(gpu, mesh, T, cam, cull_backfaces=0), restate(mesh, T, cam, 0), "unculled ")


# ------------------------------------------------------------------------------------------------
# d. ties
# ------------------------------------------------------------------------------------------------
def test_exact_centres_and_coincident_triangles(gpu):
    mesh, cam = mu.exact_centre_mesh()
    want = restate(mesh, mu.IDENTITY, cam)
    got = gpu_views(gpu, mesh, mu.IDENTITY, cam, wanted=("depth", "index", "color"))
    assert_equal_to_restatement(got, want)
    assert got["index"][8, 8] == 0 and got["index"][5, 5] == 0 and got["index"][5, 11] == 0 and got["index"][11, 11] == 1 and got["index"][11, 5] == 2
    for reverse_second in (False, True):
        mesh, cam = mu.coincident_pair(reverse_second)
        for cull in (1, 0):
            got = gpu_views(gpu, mesh, mu.IDENTITY, cam, wanted=("depth", "index", "color"), cull_backfaces=cull)
            assert_equal_to_restatement(got, restate(mesh, mu.IDENTITY, cam, cull))
            drawn = got["index"] != mu.NO_INDEX
            assert drawn.sum() > 200 and (got["index"][drawn] == 0).all()


# ------------------------------------------------------------------------------------------------
# e. attributes and outputs
# ------------------------------------------------------------------------------------------------
def test_face_normals_and_single_outputs(gpu, cooperative):
    mesh, T, cam, want = cooperative
    flat = gpu_views(gpu, mesh, T, cam, with_normals=False)
    want_flat = restate(mesh, T, cam, normals=None)
    assert_equal_to_restatement(flat, want_flat)
    assert np.abs(want_flat["normal"] - want["normal"]).max() > 0.1
    # no colours: every view but the colour view; the colour view is refused
    plain = gpu_views(gpu, mesh, T, cam, wanted=("depth", "index", "normal"), with_colors=False)
    assert_equal_to_restatement(plain, want)
    call = Call(gpu, mesh, T, cam)
    assert call.run(with_colors=False) == INVALID_ARGUMENT and call.all_untouched()
    everything = gpu_views(gpu, mesh, T, cam)
    for name in VIEWS:
        alone = gpu_views(gpu, mesh, T, cam, wanted=(name,))
        assert alone[name].tobytes() == everything[name].tobytes(), name


def test_empty_meshes_give_empty_views(gpu, cooperative):
    mesh, T, cam, _ = cooperative
    for empty in (dict(mesh, triangles=np.zeros((0, 3), np.uint32)),
                  dict(positions=np.zeros((0, 3), np.float32), normals=np.zeros((0, 3), np.float32), colors=np.zeros((0, 4), np.uint8), triangles=np.zeros((0, 3), np.uint32))):
        got = gpu_views(gpu, empty, T, cam, wanted=("depth", "index", "normal"))
        assert (got["depth"] == 0).all() and (got["index"] == mu.NO_INDEX).all() and (got["normal"] == 0).all()


# ------------------------------------------------------------------------------------------------
# f. refusals
# ------------------------------------------------------------------------------------------------
def test_rejected_arguments(gpu, cooperative):
    mesh, T, cam, _ = cooperative
    call = Call(gpu, mesh, T, cam)
    buffer = lambda name: call.images[name][1]
    camera = lambda **change: C.byref(abi.Camera4f(*[change.get(k, getattr(cam, k)) for k in ("fx", "fy", "cx", "cy", "width", "height")]))

    def shifted(name, address=0, pitch=0):
        b = buffer(name)
        return C.byref(abi.Buffer2D(b.address + address, b.height, b.width, b.pitch + pitch))

    over_positions = abi.Buffer2D(call.positions.data_ptr(), cam.height, cam.width, buffer("depth").pitch)
    refused = [dict(ctx=None), dict(camera_T_global=None), dict(camera=None), dict(positions=None), dict(indices=None),
               dict(out_depth=None, out_index=None, out_color=None, out_normal=None),
               dict(colors=None),
               dict(min_depth=0.0), dict(min_depth=-1.0), dict(min_depth=float("nan")), dict(max_depth=float("inf")), dict(max_depth=float("nan")),
               dict(metres_to_depth=0.0), dict(metres_to_depth=float("inf")), dict(metres_to_depth=float("nan")), dict(min_depth=2.0, max_depth=1.0),
               dict(cull_backfaces=2),
               dict(camera=camera(width=0)), dict(camera=camera(height=-3)), dict(camera=camera(fx=0.0)), dict(camera=camera(fy=float("nan"))),
               dict(camera=camera(width=1 << 16, height=1 << 15)), dict(camera=camera(width=cam.width + 1)),
               dict(positions=C.c_void_p(call.positions.data_ptr() + 2)), dict(normals=C.c_void_p(call.normals.data_ptr() + 1)),
               dict(colors=C.c_void_p(call.colors.data_ptr() + 2)), dict(indices=C.c_void_p(call.triangles.data_ptr() + 3)),
               dict(out_depth=shifted("depth", address=1)), dict(out_index=shifted("index", pitch=2)), dict(out_color=shifted("color", address=2)),
               dict(out_normal=shifted("normal", pitch=2)),
               dict(out_color=C.byref(buffer("index"))), dict(out_depth=C.byref(over_positions))]
    for replace in refused:
        assert call.run(**replace) == INVALID_ARGUMENT, sorted(replace)
        assert call.all_untouched(), sorted(replace)
        assert badslam_amd.lib().bslam_last_error()
    badslam_amd.check(call.run())        # and the call itself is fine
    assert not call.all_untouched()


@pytest.mark.parametrize("bad", ["V", "0xFFFFFFFF"])
def test_an_index_beyond_the_vertices(gpu, cooperative, bad):
    """A valid value that is out of range: the kernel tests it before it dereferences.  The call reports it; the padding stays."""
    mesh, T, cam, _ = cooperative
    triangles = mesh["triangles"].copy()
    triangles[100, 1] = len(mesh["positions"]) if bad == "V" else 0xFFFFFFFF
    call = Call(gpu, dict(mesh, triangles=triangles), T, cam)
    assert call.run() == INVALID_ARGUMENT
    assert b"beyond vertex_count" in badslam_amd.lib().bslam_last_error()
    call.fetch()
    no_vertices = Call(gpu, dict(mesh, triangles=triangles), T, cam)
    assert no_vertices.run(vertex_count=0) == INVALID_ARGUMENT
    views = no_vertices.fetch()
    assert (views["depth"] == 0).all() and (views["index"] == mu.NO_INDEX).all()


# ------------------------------------------------------------------------------------------------
# g. through DirectBA
# ------------------------------------------------------------------------------------------------
def test_render_mesh_through_direct_ba(gpu, fused_ba, tmp_path):
    from badslam_amd import direct_ba as dba
    ba, scene, mesh = fused_ba
    cam = small_camera(ba)
    pose = ba.keyframe_pose(1)
    m2d = float(np.float32(1.0) / np.float32(scene.raw_to_float_depth))
    decimated = ba.DecimateMesh(mesh, ratio=0.5)
    dba.SaveMeshAsPLY(str(tmp_path / "mesh.ply"), mesh)
    loaded = dba.LoadPLY(str(tmp_path / "mesh.ply"))
    assert loaded["colors"].shape[1] == 3
    for name, m in (("extracted", mesh), ("decimated", decimated), ("loaded", loaded)):
        got = ba.RenderMesh(m, pose, camera=cam, min_depth=MIN_DEPTH, max_depth=6.0, views=VIEWS)
        assert set(got) == set(VIEWS) | {"camera_T_global"}
        assert got["depth"].shape == (45, 61) and got["index"].shape == (45, 61) and got["color"].shape == (45, 61, 4) and got["normal"].shape == (45, 61, 3)
        colors = m["colors"] if m["colors"].shape[1] == 4 else np.concatenate([m["colors"], np.full((len(m["colors"]), 1), 255, np.uint8)], 1)
        raw = gpu_views(gpu, mu.mesh_dict(m["positions"], m["triangles"], m["normals"], colors), got["camera_T_global"], cam, max_depth=6.0, metres_to_depth=m2d)
        for view in VIEWS:
            assert got[view].dtype == raw[view].dtype and got[view].tobytes() == raw[view].tobytes(), (name, view)
        assert (got["depth"] != 0).mean() > 0.5, name
    assert set(ba.RenderMesh(mesh, pose)) == {"depth", "color", "camera_T_global"} and ba.RenderMesh(mesh, pose)["depth"].shape == (120, 160)
    bare = dict(positions=mesh["positions"], triangles=mesh["triangles"])
    with pytest.raises(ValueError, match="colour"):
        ba.RenderMesh(bare, pose)
    with pytest.raises(ValueError, match="views"):
        ba.RenderMesh(mesh, pose, views=("depth", "radius"))
    flat = ba.RenderMesh(bare, pose, camera=cam, views=("depth", "normal"))
    assert (flat["depth"] != 0).mean() > 0.5 and np.abs(np.linalg.norm(flat["normal"][flat["depth"] != 0], axis=-1) - 1).max() < 1e-5


# ------------------------------------------------------------------------------------------------
# h. the tool
# ------------------------------------------------------------------------------------------------
def test_run_tum_renders_the_mesh_it_writes(tmp_path):
    """tools/run_tum.py --render-dir ... --render-source mesh --mesh ... on five frames of the rendered sequence of
    tests/test_gpu_bad_slam.py: the views are RenderMesh of the PLY that was written, and a rendered depth image agrees with the
    keyframe's own at the median within the voxel size, the resolution of the surface."""
    from badslam_amd import direct_ba as dba
    from badslam_amd import png
    from tests import fusion_util as fu
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
    seen = {}
    voxel = 0.04

    def inspect(slam, result):
        kf = result["rendered"][0][0]
        seen["view"] = slam.ba().RenderMesh(dba.LoadPLY(result["mesh"]["path"]), slam.ba().keyframe_pose(kf), max_depth=6.0)
        seen["raw"] = slam.ba().keyframe_images(kf, cam.height, cam.width)[0]

    out = tmp_path / "views"
    with pytest.raises(ValueError, match="--mesh"):
        run_tum.run(source, render_dir=out, render_source="mesh")
    r = run_tum.run(source, keyframe_interval=4, ba_iterations=2, max_depth=6.0, num_scales=4, max_surfel_count=400000, render_dir=out, render_source="mesh",
                    mesh=str(tmp_path / "model.ply"), mesh_voxel_size=voxel, mesh_min_count=2, mesh_min_component=16, inspect=inspect)
    assert r["keyframes"] == 2 and len(r["rendered"]) == 2 and r["mesh"]["triangles"] > 1000
    ds = dba.read_tum_dataset(str(out), "groundtruth.txt")
    assert len(ds["frames"]) == 2 and (ds["width"], ds["height"]) == (cam.width, cam.height)
    for frame in ds["frames"]:
        assert (dba.read_png(frame["depth_path"]) > 0).sum() > 1000
    depth = dba.read_png(ds["frames"][0]["depth_path"])
    rgb = dba.read_png(ds["frames"][0]["rgb_path"])
    assert np.array_equal(depth, seen["view"]["depth"]) and np.array_equal(rgb, seen["view"]["color"][:, :, :3])
    raw = seen["raw"].astype(np.int64)
    both = (raw > 0) & (raw < fu.INVALID_DEPTH_BIT) & (depth > 0)
    error = np.abs(depth.astype(np.int64) - raw)[both]
    print(f"{int(both.sum())} pixels with both depths, |difference| median {np.median(error):.1f} raw units; a voxel is {voxel / raw_to_float:.0f}")
    assert both.sum() > 1000 and np.median(error) <= voxel / raw_to_float
    assert run_tum.arg_parser().parse_args(["dir"]).render_source == "surfels"
    assert run_tum.arg_parser().parse_args(["dir", "--render-source", "mesh"]).render_source == "mesh"
