"""-m gpu: surface views of a fused volume (bslam_volume_views_aux_bytes, bslam_prepare_volume_views, bslam_raycast_volume,
badslam_amd/csrc/raycast_kernels.hpp; DirectBA.RenderVolume; tools/run_tum.py --render-source volume) against the brute-force
NumPy float32 restatement of tests/raycast_util.py: depth and colour bit for bit, normals at 1e-6.  Never against the kernels'
own output, except where a test is about two calls agreeing.  Images are 61 x 45 (no multiple of the 8 x 8 tile, more than one
workgroup) with sentinel-padded pitches; the volume buffers are pitched wider than their content and no cell count is a multiple
of the 64-cell word or the 8-cell block."""
import ctypes as C
import itertools

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi
from tests import fusion_util as fu
from tests import raycast_util as ru
from tests.test_gpu_fusion import DIMS, ORIGIN, SENTINEL, VOXEL, Scene, bits, pitched, stream_ptr, volume_struct

pytestmark = pytest.mark.gpu
F = np.float32
INVALID_ARGUMENT = -1   # BSLAM_ERR_INVALID_ARGUMENT
W, H = 61, 45
CAMERA = abi.Camera4f(58.0, 57.0, 30.8, 22.3, W, H)
S_ORIGIN, S_VOXEL = (0.3, -1.7, 2.9), 0.013         # where the sphere field (voxel units) is put
M2D = 5000.0


@pytest.fixture(scope="module")
def gpu():
    import torch
    from badslam_amd import build
    build.build()
    return torch, badslam_amd.lib(), badslam_amd.Context(0)


def rotation(rotvec):
    return fu.pose_matrices(rotvec, np.zeros(3))[1].reshape(3, 3).astype(np.float64)       # global_R_frame


def sphere_pose(position, rotvec=(0, 0, 0), origin=S_ORIGIN):
    """global_T_camera (3, 4) f32 of a camera at `position` (voxel units of the sphere field)."""
    t = np.asarray(origin, np.float64) + S_VOXEL * np.asarray(position, np.float64)
    return np.concatenate([rotation(np.asarray(rotvec, np.float64)), t[:, None]], 1).astype(F)


def sphere_counts(shape):
    """Observation counts with samples seen 0, 1 and 3 times: the surface differs between min_count 1 and 3."""
    count = np.full(shape, 3, np.uint32)
    count[:, :, :13] = 1
    count[10:16, 12:18, 20:] = 0
    return count


@pytest.fixture(scope="module")
def sphere():
    return fu.sphere_field()


@pytest.fixture(scope="module")
def fused():
    """The restatement's volume of test_gpu_fusion's scene (37 x 29 x 23, colour), computed once."""
    scene = Scene()
    return scene, scene.fuse(0.0)


# ------------------------------------------------------------------------------------------------
# device plumbing
# ------------------------------------------------------------------------------------------------
class DeviceVolume:
    """Host volumes [nz, ny, nx] in pitched device buffers and an aux buffer prepared for min_count."""

    def __init__(self, gpu, tsdf, count, color, origin, voxel, min_count, prepare=True):
        torch, L, ctx = gpu
        nz, ny, nx = tsdf.shape
        self.vol = volume_struct((nx, ny, nz), origin, voxel)
        self.tsdf = pitched(torch, np.ascontiguousarray(tsdf, F).reshape(nz * ny, nx).view(np.int32), 5)
        self.count = pitched(torch, np.ascontiguousarray(count, np.uint32).reshape(nz * ny, nx).view(np.int32), 3)
        self.color = None if color is None else pitched(torch, np.ascontiguousarray(color, np.uint8).reshape(nz * ny, nx * 4).view(np.int32), 7)
        need = C.c_size_t()
        badslam_amd.check(L.bslam_volume_views_aux_bytes(C.byref(self.vol), C.byref(need)))
        self.aux_bytes = need.value
        self.aux = torch.full((self.aux_bytes + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        if prepare:
            self.prepare(gpu, min_count)

    def prepare(self, gpu, min_count):
        torch, L, ctx = gpu
        badslam_amd.check(L.bslam_prepare_volume_views(ctx.handle, stream_ptr(torch), C.byref(self.vol), C.byref(self.tsdf[1]), C.byref(self.count[1]), min_count,
                                                       C.c_void_p(self.aux.data_ptr()), self.aux_bytes))
        torch.cuda.synchronize()
        assert bool((self.aux[self.aux_bytes:] == 0x5A).all()), "written beyond the aux bytes"


def view_buffers(torch):
    """Sentinel-filled pitched depth, colour and normal images: name -> (tensor, Buffer2D, content width in elements)."""
    out = {"depth": pitched(torch, np.full((H, W), 0x5A5A, np.int16), 3) + (W,), "color": pitched(torch, np.full((H, W), SENTINEL, np.int32), 5) + (W,)}
    t, b = pitched(torch, np.full((H, 3 * W), SENTINEL, np.int32), 2)
    out["normal"] = (t, abi.Buffer2D(b.address, H, W, b.pitch), 3 * W)
    return out


def gpu_raycast(gpu, dev, pose, min_depth, max_depth, step, views=("depth", "color", "normal"), with_color=True, camera=CAMERA):
    """bslam_raycast_volume into fresh sentinel-filled images -> dict of the views asked for; asserts that padding and the images
    not asked for stay untouched."""
    torch, L, ctx = gpu
    out = view_buffers(torch)
    G = abi.Mat3x4((C.c_float * 12)(*np.asarray(pose, F).reshape(12)))
    ref = lambda name: C.byref(out[name][1]) if name in views else None
    badslam_amd.check(L.bslam_raycast_volume(ctx.handle, stream_ptr(torch), C.byref(dev.vol), C.byref(dev.tsdf[1]),
                                             C.byref(dev.color[1]) if with_color and dev.color is not None else None, C.c_void_p(dev.aux.data_ptr()), C.byref(G),
                                             C.byref(camera), min_depth, max_depth, step, M2D, ref("depth"), ref("color"), ref("normal")))
    torch.cuda.synchronize()
    got = {}
    for name, (t, _, width) in out.items():
        host = t.cpu().numpy()
        sentinel = 0x5A5A if name == "depth" else SENTINEL
        assert (host[:, width:] == sentinel).all(), f"{name}: padding written"
        if name not in views:
            assert (host == sentinel).all(), f"{name}: written although not asked for"
            continue
        content = np.ascontiguousarray(host[:, :width])
        got[name] = {"depth": lambda c: c.view(np.uint16), "color": lambda c: c.view(np.uint8).reshape(H, W, 4), "normal": lambda c: c.view(F).reshape(H, W, 3)}[name](content)
    return got


def assert_views_equal(got, want, label=""):
    for name, g in got.items():
        w = want[name]
        if name == "normal":
            worst = np.abs(g.astype(np.float64) - w).max()
            assert worst <= 1e-6, f"{label} normal: off by {worst}"
        else:
            differ = g != w
            assert not differ.any(), f"{label} {name}: {int(differ.sum())} values differ, first at {np.argwhere(differ)[0]}, got {g[differ][0]}, want {w[differ][0]}"


def restate(tsdf, count, color, origin, voxel, min_count, pose, min_depth, max_depth, step, camera=CAMERA):
    return ru.raycast(ru.Volume(tsdf, count, color, origin, voxel, min_count), pose, camera, min_depth, max_depth, step, M2D)


FRONT = dict(position=(16, 15, -25), lo=20 * S_VOXEL, hi=60 * S_VOXEL)


# ------------------------------------------------------------------------------------------------
# 1. the sphere
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_count", [1, 3])
@pytest.mark.parametrize("step", [0.5, 1.0, 2.3])
def test_sphere(gpu, sphere, step, min_count):
    count = sphere_counts(sphere.shape)
    pose = sphere_pose(FRONT["position"])
    want = restate(sphere, count, None, S_ORIGIN, S_VOXEL, min_count, pose, FRONT["lo"], FRONT["hi"], step * S_VOXEL)
    hits = int(want["hit"].sum())
    print(f"step {step}, min_count {min_count}: N {want['samples']}, {hits} hits")
    assert 300 < hits < W * H and (min_count == 1) == (hits > 600)     # min_count 3 loses the third of the surface seen once
    dev = DeviceVolume(gpu, sphere, count, None, S_ORIGIN, S_VOXEL, min_count)
    got = gpu_raycast(gpu, dev, pose, FRONT["lo"], FRONT["hi"], step * S_VOXEL)
    assert_views_equal(got, want)
    assert not got["color"].any()                                       # no colour volume


def test_holed_sphere(gpu, sphere):
    count = fu.holed_sphere_count(sphere.shape)
    pose = sphere_pose(FRONT["position"])
    want = restate(sphere, count, None, S_ORIGIN, S_VOXEL, 1, pose, FRONT["lo"], FRONT["hi"], S_VOXEL)
    full = restate(sphere, np.ones(sphere.shape, np.uint32), None, S_ORIGIN, S_VOXEL, 1, pose, FRONT["lo"], FRONT["hi"], S_VOXEL)
    assert 0 < want["hit"].sum() < full["hit"].sum()
    assert_views_equal(gpu_raycast(gpu, DeviceVolume(gpu, sphere, count, None, S_ORIGIN, S_VOXEL, 1), pose, FRONT["lo"], FRONT["hi"], S_VOXEL), want)


POSES = {
    # name: (position in voxel units, rotation vector, min depth, max depth in voxels, hits expected)
    "tilted": ((20, 10, -22), (0.2, -0.3, 0.1), 15, 70, "some"),
    "inside the volume": ((3, 3, 3), (-0.68, 0.747, 0), 0.5, 40, "some"),      # in the box's corner, looking at the sphere's centre
    "inside the sphere": ((16.3, 15.1, 14.2), (0, 0, 0), 0.5, 40, "none"),
    "facing away": ((16, 15, -25), (0, np.pi, 0), 20, 60, "none"),
    "a corner of the box": ((46, 40, -25), (0, 0, 0), 20, 70, "any"),
    "beginning inside the surface": ((16, 15, -25), (0, 0, 0), 32, 60, "some"),
}


@pytest.mark.parametrize("name", list(POSES))
def test_sphere_from_other_poses(gpu, sphere, name):
    position, rotvec, lo, hi, expected = POSES[name]
    count = np.ones(sphere.shape, np.uint32)
    pose = sphere_pose(position, rotvec)
    want = restate(sphere, count, None, S_ORIGIN, S_VOXEL, 1, pose, lo * S_VOXEL, hi * S_VOXEL, S_VOXEL)
    hits = int(want["hit"].sum())
    print(f"{name}: {hits} hits")
    assert {"some": hits > 50, "none": hits == 0, "any": True}[expected]
    if name == "beginning inside the surface":
        front = restate(sphere, count, None, S_ORIGIN, S_VOXEL, 1, pose, FRONT["lo"], FRONT["hi"], S_VOXEL)
        assert (front["hit"] & ~want["hit"]).sum() > 50                 # the rays through the middle begin inside and are empty
    got = gpu_raycast(gpu, DeviceVolume(gpu, sphere, count, None, S_ORIGIN, S_VOXEL, 1), pose, lo * S_VOXEL, hi * S_VOXEL, S_VOXEL)
    assert_views_equal(got, want, name)


def test_volume_far_from_the_origin(gpu, sphere):
    """An origin of 100 m: the coordinates lose seven bits, the clip of the walked range must still hold every in-range sample."""
    origin = (100.3, -101.7, 102.9)
    count = np.ones(sphere.shape, np.uint32)
    for position, rotvec in (((16, 15, -25), (0, 0, 0)), ((20, 10, -22), (0.2, -0.3, 0.1))):
        pose = sphere_pose(position, rotvec, origin)
        want = restate(sphere, count, None, origin, S_VOXEL, 1, pose, 15 * S_VOXEL, 70 * S_VOXEL, S_VOXEL)
        assert want["hit"].sum() > 300
        assert_views_equal(gpu_raycast(gpu, DeviceVolume(gpu, sphere, count, None, origin, S_VOXEL, 1), pose, 15 * S_VOXEL, 70 * S_VOXEL, S_VOXEL), want)


# ------------------------------------------------------------------------------------------------
# 2. the fused volume, with colour
# ------------------------------------------------------------------------------------------------
def keyframe_pose(kf):
    M = kf.T.reshape(3, 4).astype(np.float64)
    return np.concatenate([M[:, :3].T, (-M[:, :3].T @ M[:, 3])[:, None]], 1).astype(F)


@pytest.mark.parametrize("min_count", [1, 3])
def test_fused_volume(gpu, fused, min_count):
    scene, (tsdf, count, color) = fused
    pose = keyframe_pose(scene.keyframes[0])
    want = restate(tsdf, count, color, ORIGIN, VOXEL, min_count, pose, 0.5, 3.0, VOXEL)
    hits = int(want["hit"].sum())
    print(f"min_count {min_count}: {hits} hits, {(want['color'][..., 3] == 255).sum()} with colour")
    assert hits > (200 if min_count == 1 else 30) and (want["color"][..., 3] == 255).sum() > 30
    dev = DeviceVolume(gpu, tsdf, count, color, ORIGIN, VOXEL, min_count)
    assert_views_equal(gpu_raycast(gpu, dev, pose, 0.5, 3.0, VOXEL), want)
    # without the colour volume the colour view is written, and empty
    got = gpu_raycast(gpu, dev, pose, 0.5, 3.0, VOXEL, with_color=False)
    assert not got["color"].any()
    assert_views_equal({k: got[k] for k in ("depth", "normal")}, want)


def test_aux_buffer_decides_min_count_and_two_calls_agree(gpu, fused):
    scene, (tsdf, count, color) = fused
    pose = keyframe_pose(scene.keyframes[0])
    want = {m: restate(tsdf, count, color, ORIGIN, VOXEL, m, pose, 0.5, 3.0, VOXEL) for m in (1, 3)}
    assert (want[1]["depth"] != want[3]["depth"]).any()
    dev = DeviceVolume(gpu, tsdf, count, color, ORIGIN, VOXEL, 3)
    first, second = gpu_raycast(gpu, dev, pose, 0.5, 3.0, VOXEL), gpu_raycast(gpu, dev, pose, 0.5, 3.0, VOXEL)
    for name in first:
        assert np.array_equal(bits(first[name]) if name == "normal" else first[name], bits(second[name]) if name == "normal" else second[name])
    assert_views_equal(first, want[3])
    dev.prepare(gpu, 1)                                                  # the same buffer, prepared again
    assert_views_equal(gpu_raycast(gpu, dev, pose, 0.5, 3.0, VOXEL), want[1])


def test_every_subset_of_the_outputs(gpu, fused):
    scene, (tsdf, count, color) = fused
    pose = keyframe_pose(scene.keyframes[1])
    want = restate(tsdf, count, color, ORIGIN, VOXEL, 1, pose, 0.5, 3.0, VOXEL)
    assert want["hit"].sum() > 200
    dev = DeviceVolume(gpu, tsdf, count, color, ORIGIN, VOXEL, 1)
    for n in (1, 2, 3):
        for views in itertools.combinations(("depth", "color", "normal"), n):
            got = gpu_raycast(gpu, dev, pose, 0.5, 3.0, VOXEL, views=views)       # asserts the others stay untouched
            assert set(got) == set(views)
            assert_views_equal(got, want, "+".join(views))


def test_block_test_changes_no_bit_and_skips_samples(gpu, sphere, fused):
    torch, L, ctx = gpu
    scene, (tsdf, count, color) = fused
    cases = [(DeviceVolume(gpu, sphere, sphere_counts(sphere.shape), None, S_ORIGIN, S_VOXEL, 1), sphere_pose(FRONT["position"]), FRONT["lo"], FRONT["hi"], S_VOXEL,
              restate(sphere, sphere_counts(sphere.shape), None, S_ORIGIN, S_VOXEL, 1, sphere_pose(FRONT["position"]), FRONT["lo"], FRONT["hi"], S_VOXEL)),
             (DeviceVolume(gpu, tsdf, count, color, ORIGIN, VOXEL, 1), keyframe_pose(scene.keyframes[0]), 0.5, 3.0, VOXEL,
              restate(tsdf, count, color, ORIGIN, VOXEL, 1, keyframe_pose(scene.keyframes[0]), 0.5, 3.0, VOXEL))]
    for dev, pose, lo, hi, step, want in cases:
        stats = {}
        try:
            for on in (1, 0):
                badslam_amd.check(L.bslam_set_culling(ctx.handle, on))
                badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
                tested, culled = C.c_uint64(), C.c_uint64()
                badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))     # reset
                got = gpu_raycast(gpu, dev, pose, lo, hi, step)
                badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))
                badslam_amd.check(L.bslam_profile_enable(ctx.handle, 0))
                assert_views_equal(got, want, f"block test {on}")
                stats[on] = (tested.value, culled.value)
        finally:
            L.bslam_set_culling(ctx.handle, 1)
            L.bslam_profile_enable(ctx.handle, 0)
        print("in-range samples, skipped:", stats)
        assert stats[0][0] == stats[1][0] > 0                           # the rays end at the same samples either way
        assert stats[0][1] == 0 and 0 < stats[1][1] < stats[1][0]


# ------------------------------------------------------------------------------------------------
# 3. rejected arguments
# ------------------------------------------------------------------------------------------------
def test_rejected_arguments(gpu, sphere):
    torch, L, ctx = gpu
    count = np.ones(sphere.shape, np.uint32)
    color = np.zeros(sphere.shape + (4,), np.uint8)
    dev = DeviceVolume(gpu, sphere, count, color, S_ORIGIN, S_VOXEL, 1)
    nz, ny, nx = sphere.shape
    out = view_buffers(torch)
    G = abi.Mat3x4((C.c_float * 12)(*sphere_pose(FRONT["position"]).reshape(12)))
    ref = lambda v: None if v is None else C.byref(v)

    def buffer(b, **changes):
        c = abi.Buffer2D(b.address, b.height, b.width, b.pitch)
        for k, v in changes.items():
            setattr(c, k, v)
        return c

    volume = lambda dims=(nx, ny, nz), voxel=S_VOXEL: volume_struct(dims, S_ORIGIN, voxel)
    base = dict(ctx=ctx.handle, volume=dev.vol, tsdf=dev.tsdf[1], color=dev.color[1], aux=dev.aux.data_ptr(), G=G, camera=CAMERA, lo=FRONT["lo"], hi=FRONT["hi"],
                step=S_VOXEL, m2d=M2D, depth=out["depth"][1], colour=out["color"][1], normal=out["normal"][1])

    def cast(**changes):
        a = dict(base, **changes)
        return L.bslam_raycast_volume(a["ctx"], stream_ptr(torch), ref(a["volume"]), ref(a["tsdf"]), ref(a["color"]), C.c_void_p(a["aux"]) if a["aux"] else None,
                                      ref(a["G"]), ref(a["camera"]), a["lo"], a["hi"], a["step"], a["m2d"], ref(a["depth"]), ref(a["colour"]), ref(a["normal"]))

    inf, nan = float("inf"), float("nan")
    cases = {
        "null context": dict(ctx=None), "null volume": dict(volume=None), "null tsdf": dict(tsdf=None), "null aux": dict(aux=None), "null pose": dict(G=None),
        "null camera": dict(camera=None), "no output": dict(depth=None, colour=None, normal=None),
        "step 0": dict(step=0.0), "step < 0": dict(step=-0.01), "step inf": dict(step=inf), "step nan": dict(step=nan),
        "min_depth 0": dict(lo=0.0), "min_depth nan": dict(lo=nan), "max_depth inf": dict(hi=inf), "max_depth nan": dict(hi=nan),
        "min_depth = max_depth": dict(lo=0.5, hi=0.5), "min_depth > max_depth": dict(lo=0.8, hi=0.5),
        "metres_to_depth 0": dict(m2d=0.0), "metres_to_depth nan": dict(m2d=nan),
        "65537 samples": dict(lo=1.0, hi=1.0 + 65536 * 2.0 ** -10, step=2.0 ** -10), "far too many samples": dict(lo=0.05, hi=50.0, step=1e-9),
        "voxel size 0": dict(volume=volume(voxel=0.0)), "voxel size inf": dict(volume=volume(voxel=inf)), "nx 1": dict(volume=volume((1, ny, nz))),
        "volume of another shape": dict(volume=volume((nx, ny, nz + 1))), "more than 2^30 samples": dict(volume=volume((2048, 1024, 1024))),
        "tsdf pitch misaligned": dict(tsdf=buffer(dev.tsdf[1], pitch=dev.tsdf[1].pitch + 2)), "colour pitch too small": dict(color=buffer(dev.color[1], pitch=4 * nx - 4)),
        "aux misaligned": dict(aux=dev.aux.data_ptr() + 4),
        "camera without pixels": dict(camera=abi.Camera4f(58.0, 57.0, 30.8, 22.3, 0, H)), "focal length 0": dict(camera=abi.Camera4f(0.0, 57.0, 30.8, 22.3, W, H)),
        "depth view of another size": dict(depth=buffer(out["depth"][1], width=W - 1)), "depth view misaligned": dict(depth=buffer(out["depth"][1], address=out["depth"][1].address + 1)),
        "normal pitch too small": dict(normal=buffer(out["normal"][1], pitch=12 * W - 4)), "colour view misaligned": dict(colour=buffer(out["color"][1], pitch=out["color"][1].pitch + 2)),
        "two views overlap": dict(colour=buffer(out["normal"][1], pitch=out["normal"][1].pitch)), "a view overlaps the tsdf volume": dict(colour=buffer(dev.tsdf[1], height=H, width=W, pitch=4 * W)),
        "a view overlaps the aux buffer": dict(depth=abi.Buffer2D(dev.aux.data_ptr(), H, W, 2 * W)),
    }
    for name, changes in cases.items():
        rc = cast(**changes)
        assert rc == INVALID_ARGUMENT, (name, rc, L.bslam_last_error())
    assert cast(lo=1.0, hi=1.0 + 65535 * 2.0 ** -10, step=2.0 ** -10) == 0            # exactly 65536 samples are fine
    assert cast() == 0 and cast(color=None) == 0 and cast(colour=None, normal=None) == 0
    torch.cuda.synchronize()

    need = C.c_size_t(7)
    for name, (v, b) in {"null volume": (None, need), "null size": (dev.vol, None), "nz 1": (volume((nx, ny, 1)), need), "voxel size nan": (volume(voxel=nan), need)}.items():
        rc = L.bslam_volume_views_aux_bytes(ref(v), ref(b))
        assert rc == INVALID_ARGUMENT, (name, rc, L.bslam_last_error())
    assert L.bslam_volume_views_aux_bytes(C.byref(dev.vol), C.byref(need)) == 0 and need.value == dev.aux_bytes
    # one bit per cell in 64-bit words along x, after the flag bytes padded to 256
    assert need.value == 256 * -(-(1 * 4 * 4) // 256) + 8 * 1 * (ny - 1) * (nz - 1)

    pbase = dict(ctx=ctx.handle, volume=dev.vol, tsdf=dev.tsdf[1], count=dev.count[1], min_count=1, aux=dev.aux.data_ptr(), bytes=dev.aux_bytes)

    def prepare(**changes):
        a = dict(pbase, **changes)
        return L.bslam_prepare_volume_views(a["ctx"], stream_ptr(torch), ref(a["volume"]), ref(a["tsdf"]), ref(a["count"]), a["min_count"],
                                            C.c_void_p(a["aux"]) if a["aux"] else None, a["bytes"])

    for name, changes in {"null context": dict(ctx=None), "null volume": dict(volume=None), "null tsdf": dict(tsdf=None), "null count": dict(count=None),
                          "null aux": dict(aux=None), "min_count 0": dict(min_count=0), "aux too small": dict(bytes=dev.aux_bytes - 1), "aux misaligned": dict(aux=dev.aux.data_ptr() + 2),
                          "volume of another shape": dict(volume=volume((nx + 1, ny, nz))), "count pitch misaligned": dict(count=buffer(dev.count[1], pitch=dev.count[1].pitch + 1)),
                          "aux overlaps the tsdf volume": dict(aux=dev.tsdf[1].address, bytes=1 << 30)}.items():
        rc = prepare(**changes)
        assert rc == INVALID_ARGUMENT, (name, rc, L.bslam_last_error())
    assert prepare() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# 4. through DirectBA
# ------------------------------------------------------------------------------------------------
def test_views_through_direct_ba():
    """The three 160 x 120 keyframes of tests/scenes.py, fused at 2 cm as in tests/test_gpu_fusion.py: RenderVolume from keyframe
    0's pose equals the restatement applied to the downloaded volume, and agrees with keyframe 0's own depth image.

    Measured beforehand on the CPU with the restatements (surfels of the oracle's creation path for the box, fusion_util.fuse for
    the volume, 150 x 118 x 49 samples, depth range 0.5 - 6 m at the voxel size, 276 samples per ray): 18 989 pixels are hit,
    among them 0.9961 of the keyframe's 18 096 valid depth pixels; |ray-cast depth - keyframe depth| over the pixels that have
    both: median 2, 99th percentile 12, maximum 28 raw units (1 / 5000 m; a voxel is 100).  Asserted at 0.9 of the share and
    twice the median and the 99th percentile; the margin is for the slightly different box of the surfels this run creates."""
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
    with pytest.raises(Exception, match="no fused volume"):
        ba.RenderVolume(ba.keyframe_pose(0))
    voxel, truncation = 0.02, 0.08
    lo, hi = ba.ModelBounds()
    origin, dims = run_tum.mesh_volume(lo, hi, voxel, truncation)
    ba.FuseKeyframes(origin, voxel, dims, truncation)
    volume = ba.Volume()
    got = ba.RenderVolume(ba.keyframe_pose(0), min_depth=0.5, max_depth=6.0, views=("depth", "color", "normal"))
    camera = abi.Camera4f(*[float(v) for v in ba.intrinsics()[1]], 160, 120)
    m2d = float(F(1.0) / F(scene.raw_to_float_depth))
    want = ru.raycast(ru.Volume(volume["tsdf"], volume["count"], volume["color"], origin, voxel, 1), got["global_T_camera"], camera, 0.5, 6.0, voxel, m2d)
    assert_views_equal({k: got[k] for k in ("depth", "color", "normal")}, want)
    raw = ba.keyframe_images(0, 120, 160)[0].astype(np.int64)
    valid = (raw > 0) & (raw < fu.INVALID_DEPTH_BIT)
    both = valid & (got["depth"] > 0)
    share = both.sum() / valid.sum()
    error = np.abs(got["depth"].astype(np.int64) - raw)[both]
    print(f"{int(valid.sum())} keyframe depth pixels, share hit {share:.4f}, |difference| median {np.median(error):.1f}, p99 {np.percentile(error, 99):.1f} raw units")
    assert share >= 0.9 * MEASURED_SHARE
    assert np.median(error) <= 2 * MEASURED_MEDIAN and np.percentile(error, 99) <= 2 * MEASURED_P99
    # min_count 2 prepares again and drops what one keyframe alone saw; the default views are depth and colour; a new fusion is seen
    two = ba.RenderVolume(ba.keyframe_pose(0), min_depth=0.5, max_depth=6.0, min_count=2)
    assert set(two) == {"depth", "color", "global_T_camera"}
    want2 = ru.raycast(ru.Volume(volume["tsdf"], volume["count"], volume["color"], origin, voxel, 2), got["global_T_camera"], camera, 0.5, 6.0, voxel, m2d)
    assert_views_equal({k: two[k] for k in ("depth", "color")}, want2)
    assert (want2["depth"] != want["depth"]).any()
    ba.DeleteKeyframe(1)
    ba.FuseKeyframes(origin, voxel, dims, truncation)
    v3 = ba.Volume()
    three = ba.RenderVolume(ba.keyframe_pose(0), min_depth=0.5, max_depth=6.0, min_count=2, step=0.03, views=("depth",))
    want3 = ru.raycast(ru.Volume(v3["tsdf"], v3["count"], v3["color"], origin, voxel, 2), three["global_T_camera"], camera, 0.5, 6.0, 0.03, m2d)
    assert_views_equal({"depth": three["depth"]}, want3)
    assert (want3["depth"] != want2["depth"]).any()
    with pytest.raises(Exception, match="samples per ray"):
        ba.RenderVolume(ba.keyframe_pose(0), step=1e-5)
    ba.close()


MEASURED_SHARE, MEASURED_MEDIAN, MEASURED_P99 = 0.9961, 2.0, 12.0


@pytest.fixture(scope="module")
def fused_ba():
    """The DirectBA of test_views_through_direct_ba with its three keyframes fused once, for the tests that share it."""
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
    voxel, truncation = 0.02, 0.08
    origin, dims = run_tum.mesh_volume(*ba.ModelBounds(), voxel, truncation)
    ba.FuseKeyframes(origin, voxel, dims, truncation)
    yield ba, scene, origin, voxel
    ba.close()


def test_view_images_are_shared_across_sizes(fused_ba):
    """RenderVolume at 160 x 120 and RenderModel at 80 x 60 take turns on one object, whose device images they share and
    re-allocate for each other: each repeat equals its first call byte for byte, the small views equal render_util.render32 on the
    surfel rows and the large ones raycast_util.raycast on the downloaded volume (normals as everywhere in these files: 1e-6)."""
    from tests import render_util
    from tests.test_gpu_render import assert_equal_to_restatement
    ba, scene, origin, voxel = fused_ba
    pose = ba.keyframe_pose(0)
    fx, fy, cx, cy = [float(v) for v in ba.intrinsics()[1]]
    half = abi.Camera4f(fx / 2, fy / 2, cx / 2, cy / 2, 80, 60)
    volume_call = lambda: ba.RenderVolume(pose, min_depth=0.5, max_depth=6.0, views=("depth", "color", "normal"))
    model_call = lambda: ba.RenderModel(pose, camera=half, radius_scale=2.0, views=("depth", "index", "color", "normal"))
    volume_views, model_views, volume_again, model_again = volume_call(), model_call(), volume_call(), model_call()
    for first, again in ((volume_views, volume_again), (model_views, model_again)):
        assert set(first) == set(again)
        for name in first:
            assert first[name].shape == again[name].shape and first[name].tobytes() == again[name].tobytes(), name
    assert model_views["depth"].shape == (60, 80) and model_views["index"].shape == (60, 80) and model_views["normal"].shape == (60, 80, 3)
    assert volume_views["depth"].shape == (120, 160) and volume_views["color"].shape == (120, 160, 4)
    m2d = F(1.0) / F(scene.raw_to_float_depth)
    want_model = render_util.render32(ba.GetSurfels(8), ba.surfels_size(), model_views["camera_T_global"], half, 0.05, 50.0, 2.0, m2d)
    assert_equal_to_restatement(model_views, want_model)
    assert (model_views["depth"] != 0).mean() > 0.5
    v = ba.Volume()
    want_volume = ru.raycast(ru.Volume(v["tsdf"], v["count"], v["color"], origin, voxel, 1), volume_views["global_T_camera"], abi.Camera4f(fx, fy, cx, cy, 160, 120),
                             0.5, 6.0, voxel, float(m2d))
    assert_views_equal({k: volume_views[k] for k in ("depth", "color", "normal")}, want_volume)
    assert (volume_views["depth"] != 0).mean() > 0.5


def test_an_extraction_that_yields_nothing(fused_ba):
    """No sample is seen by four of three keyframes: ExtractMesh(min_count=4) is empty by the plain route and by the one with
    clean-up and report, SurfelMeshDistance then finds nothing near any surfel, and ExtractMesh(1) is what it was before."""
    ba = fused_ba[0]
    before = ba.ExtractMesh(1)
    assert len(before["positions"]) > 1000 and len(before["triangles"]) > 1000
    plain = ba.ExtractMesh(min_count=4)
    cleaned, report = ba.ExtractMesh(min_count=4, min_component_vertices=64, report=True)
    for mesh in (plain, cleaned):
        assert mesh["positions"].shape == (0, 3) and mesh["normals"].shape == (0, 3) and mesh["colors"].shape == (0, 4) and mesh["triangles"].shape == (0, 3)
    assert (report["components"], report["removed_vertices"], report["removed_triangles"]) == (0, 0, 0) and report["sizes_descending"].shape == (0,)
    points = ba.ExportToPointCloud()[0]
    result = ba.SurfelMeshDistance(0.1)
    assert len(points) > 4000 and result["distance"].shape == (len(points),) and result["triangle"].shape == (len(points),)
    assert np.isposinf(result["distance"]).all() and (result["triangle"] == 0xFFFFFFFF).all()
    after = ba.ExtractMesh(1)
    for name in before:
        assert before[name].dtype == after[name].dtype and np.array_equal(before[name], after[name]), name


# ------------------------------------------------------------------------------------------------
# 5. the tool
# ------------------------------------------------------------------------------------------------
def test_run_tum_renders_from_the_volume(tmp_path):
    """tools/run_tum.py --render-dir ... --render-source volume on five frames of the rendered sequence of
    tests/test_gpu_bad_slam.py: the directory loads back through read_tum_dataset and its first depth image is RenderVolume at
    keyframe 0's pose; no --mesh is given, the volume is fused all the same."""
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
    seen = {}

    def inspect(slam, result):
        seen["volume"] = slam.ba().Volume()
        seen["view"] = slam.ba().RenderVolume(slam.ba().keyframe_pose(result["rendered"][0][0]), max_depth=6.0, min_count=2)

    out = tmp_path / "views"
    r = run_tum.run(source, keyframe_interval=4, ba_iterations=2, max_depth=6.0, num_scales=4, max_surfel_count=400000, render_dir=out, render_source="volume",
                    mesh_voxel_size=0.04, mesh_min_count=2, inspect=inspect)
    assert r["keyframes"] == 2 and len(r["rendered"]) == 2 and "mesh" not in r
    assert seen["volume"]["voxel_size"] == F(0.04) and seen["volume"]["dims"] == r["volume"]["dims"]
    ds = dba.read_tum_dataset(str(out), "groundtruth.txt")
    assert len(ds["frames"]) == 2 and (ds["width"], ds["height"]) == (cam.width, cam.height)
    depth = dba.read_png(ds["frames"][0]["depth_path"])
    rgb = dba.read_png(ds["frames"][0]["rgb_path"])
    assert (seen["view"]["depth"] > 0).sum() > 1000
    assert np.array_equal(depth, seen["view"]["depth"]) and np.array_equal(rgb, seen["view"]["color"][:, :, :3])
    assert run_tum.arg_parser().parse_args(["dir"]).render_source == "surfels"
    assert run_tum.arg_parser().parse_args(["dir", "--render-source", "volume"]).render_source == "volume"
