"""-m gpu: volumetric fusion and surface nets (bslam_fuse_keyframes, bslam_extract_mesh, badslam_amd/csrc/fusion_kernels.hpp;
DirectBA.FuseKeyframes / ExtractMesh / ModelBounds / Volume; tools/run_tum.py --mesh, --point-cloud) against the NumPy float32
restatements of tests/fusion_util.py: tsdf, count, colour, vertex ids, indices, positions and vertex colours bit for bit, normals
at 1e-6.  Never against the kernels' own output, except where a test is about two calls agreeing.  No volume dimension is a
multiple of the 8 x 8 x 4 brick, no cell count a multiple of the scan tile; volumes and images are pitched wider than their content."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi
from tests import fusion_util as fu

pytestmark = pytest.mark.gpu
F = np.float32
INVALID_ARGUMENT = -1   # BSLAM_ERR_INVALID_ARGUMENT
SENTINEL = 0x5A5A5A5A   # as int32; as a float 1.5e16, as a colour alpha 0x5A: none of them a value the kernels write here

DIMS, ORIGIN, VOXEL, TRUNCATION = (37, 29, 23), (-0.37, -0.29, 1.2), 0.02, 0.08
RAW_TO_FLOAT, CELL = 1.0 / 5000.0, 4


@pytest.fixture(scope="module")
def gpu():
    import torch
    from badslam_amd import build
    build.build()
    return torch, badslam_amd.lib(), badslam_amd.Context(0)


def stream_ptr(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------
# the scene: two planes seen by six keyframes
# ------------------------------------------------------------------------------------------------
class Scene:
    """Six 80 x 60 keyframes of the two planes of fusion_util.PLANES around the volume, a colour camera of twice the size and
    slightly different intrinsics, a non-zero cfactor image at cell size 4.  Keyframes 0 - 2 look at the volume from random
    poses so close that it crosses all four image sides; 3 stands 5 m aside and sees none of it; 4 faces away (the whole
    volume is behind it); 5 holds the volume's far corner only, in the corner of its image.  A twentieth of the depth
    pixels carry the invalid bit, another twentieth are 0."""

    def __init__(self):
        rng = np.random.default_rng(17)
        self.depth_camera = abi.Camera4f(140.0, 139.0, 40.3, 29.6, 80, 60)
        self.color_camera = abi.Camera4f(281.0, 279.5, 80.9, 59.1, 160, 120)
        self.cfactor = rng.uniform(-0.02, 0.02, (15, 20)).astype(F)
        corner = np.array(ORIGIN) + np.array(DIMS) * VOXEL - 0.5 * VOXEL      # centre of the last sample
        poses = [(rng.uniform(-0.15, 0.15, 3), rng.uniform(-0.2, 0.2, 3)) for _ in range(3)]
        poses.append((np.zeros(3), np.array([5.0, 0.0, 0.0])))
        poses.append((np.array([0.0, np.pi, 0.0]), np.array([0.0, 0.0, 0.5])))
        # the corner sample at pixel (2.5, 2.5) of a camera one metre in front of it
        poses.append((np.zeros(3), corner - np.array([(2.5 - 40.3) / 140.0, (2.5 - 29.6) / 139.0, 1.0])))
        self.keyframes, self.global_R_frame = [], []
        for rotvec, translation in poses:
            T, R = fu.pose_matrices(rotvec, translation)
            depth = fu.render_planes(self.depth_camera, T, RAW_TO_FLOAT)
            holes = rng.random(depth.shape)
            depth = np.where(holes < 0.05, depth | fu.INVALID_DEPTH_BIT, np.where(holes < 0.1, 0, depth)).astype(np.uint16)
            color = rng.integers(0, 256, (120, 160, 4), dtype=np.uint8)
            self.keyframes.append(fu.Keyframe(depth, color, T))
            self.global_R_frame.append(R)

    def fuse(self, a, keyframes=None, with_color=True):
        return fu.fuse(self.keyframes if keyframes is None else keyframes, self.depth_camera, self.color_camera, self.cfactor, a, RAW_TO_FLOAT, CELL,
                       ORIGIN, VOXEL, DIMS, TRUNCATION, with_color)


@pytest.fixture(scope="module")
def scene():
    return Scene()


@pytest.fixture(scope="module")
def fused(scene):
    """The restatement's volumes of the scene for a = 0 and a != 0, computed once."""
    return {0.0: scene.fuse(0.0), 0.03: scene.fuse(0.03)}


# ------------------------------------------------------------------------------------------------
# device plumbing
# ------------------------------------------------------------------------------------------------
def pitched(torch, array, pad):
    """A 2-D array of 2- or 4-byte elements on the device in rows `pad` elements wider than the content, the padding filled
    with the sentinel: (integer tensor of the same element size, Buffer2D)."""
    itype, sentinel = {2: (np.int16, 0x5A5A), 4: (np.int32, SENTINEL)}[array.dtype.itemsize]
    host = np.full((array.shape[0], array.shape[1] + pad), sentinel, itype)
    host[:, :array.shape[1]] = np.ascontiguousarray(array).view(itype)
    t = torch.from_numpy(host).cuda()
    return t, abi.Buffer2D(t.data_ptr(), array.shape[0], array.shape[1], t.stride(0) * t.element_size())


class DeviceScene:
    def __init__(self, torch, scene, a):
        self.keep = []
        self.views = (abi.KeyframeView * len(scene.keyframes))()
        for k, kf in enumerate(scene.keyframes):
            v = self.views[k]
            for name, image, pad in (("depth", kf.depth, 3), ("normals", np.zeros_like(kf.depth), 1), ("color", kf.color.reshape(120, 160 * 4).view(np.int32), 5)):
                t, b = pitched(torch, image, pad)
                self.keep.append(t)
                setattr(v, name, b)
            v.frame_T_global = abi.Mat3x4((C.c_float * 12)(*kf.T))
            v.global_R_frame = abi.Mat3x3((C.c_float * 9)(*scene.global_R_frame[k]))
            v.activation = (abi.KF_ACTIVE, abi.KF_INACTIVE, abi.KF_COVISIBLE_ACTIVE)[k % 3]   # not looked at
            v.id = k
        t, b = pitched(torch, scene.cfactor, 2)
        self.keep.append(t)
        self.dp = abi.DepthParams(b, a, RAW_TO_FLOAT, 40.0, CELL)


def volume_struct(dims=DIMS, origin=ORIGIN, voxel=VOXEL):
    return abi.Volume((C.c_float * 3)(*origin), voxel, *dims)


def output_volumes(torch, dims=DIMS, pads=(5, 3, 7)):
    """Sentinel-filled pitched tsdf, count and colour volumes: [(tensor, Buffer2D)] * 3."""
    nx, ny, nz = dims
    return [pitched(torch, np.full((nz * ny, nx), SENTINEL, np.int32), pad) for pad in pads]


def fetch_volume(tensor, dims):
    """(content [nz, ny, nx] int32, padding) of a volume tensor."""
    nx, ny, nz = dims
    host = tensor.cpu().numpy()
    return np.ascontiguousarray(host[:, :nx]).reshape(nz, ny, nx), host[:, nx:]


def gpu_fuse(gpu, scene, dev, count=None, with_color=True, truncation=TRUNCATION):
    """bslam_fuse_keyframes into fresh sentinel-filled volumes -> (tsdf f32, count u32, colour u8 [.., 4] or the untouched tensor)."""
    torch, L, ctx = gpu
    out = output_volumes(torch)
    vol = volume_struct()
    K = len(scene.keyframes) if count is None else count
    badslam_amd.check(L.bslam_fuse_keyframes(ctx.handle, stream_ptr(torch), C.byref(scene.color_camera), C.byref(scene.depth_camera), C.byref(dev.dp), K, dev.views,
                                             C.byref(vol), truncation, C.byref(out[0][1]), C.byref(out[1][1]), C.byref(out[2][1]) if with_color else None))
    torch.cuda.synchronize()
    got = []
    for i, (t, _) in enumerate(out):
        content, padding = fetch_volume(t, DIMS)
        assert (padding == SENTINEL).all(), f"output {i}: padding written"
        got.append(content)
    if not with_color:
        assert (got[2] == SENTINEL).all(), "colour volume written although not given"
    return got[0].view(F), got[1].view(np.uint32), got[2].view(np.uint8).reshape(got[2].shape + (4,))


def assert_volumes_equal(got, want):
    for name, g, w in zip(("tsdf", "count", "colour"), got, want):
        g, w = (bits(g), bits(w)) if name == "tsdf" else (g, w)
        differ = g != w
        assert not differ.any(), f"{name}: {int(differ.sum())} values differ, first at {np.argwhere(differ)[0]}"


# ------------------------------------------------------------------------------------------------
# 1. integration
# ------------------------------------------------------------------------------------------------
def test_the_scene_has_the_cases_it_is_meant_to_have(scene, fused):
    """On the restatement alone: what each keyframe contributes, so that the comparison below covers those cases."""
    tsdf, count, color = fused[0.0]
    per_keyframe = [int(scene.fuse(0.0, [kf], with_color=False)[1].sum()) for kf in scene.keyframes]
    assert all(n > 1000 for n in per_keyframe[:3]) and per_keyframe[3] == 0 and per_keyframe[4] == 0 and 0 < per_keyframe[5] < 200
    assert count.max() >= 3 and (count == 0).any()
    assert (color[..., 3] == 255).any() and ((color[..., 3] == 0) & (count > 0)).any()       # observed, but beyond the truncation or the colour image
    assert (tsdf == F(TRUNCATION)).any() and (tsdf < 0).any()
    # samples within a pixel of each side of keyframe 0's image, and samples behind keyframe 4
    gz, gy, gx = np.meshgrid(fu.voxel_centres(ORIGIN, VOXEL, DIMS[2], 2), fu.voxel_centres(ORIGIN, VOXEL, DIMS[1], 1), fu.voxel_centres(ORIGIN, VOXEL, DIMS[0], 0),
                             indexing="ij")
    sides = {name: False for name in ("left", "right", "top", "bottom")}
    for kf in scene.keyframes[:3]:
        T = kf.T
        local = [fu.tr_row(T[4 * r], T[4 * r + 1], T[4 * r + 2], T[4 * r + 3], (gx, gy, gz)) for r in range(3)]
        px, py = fu.project(F(140.0), F(139.0), F(40.3), F(29.6), local)
        for name, inner, outer, p in (("left", 0, -1, px), ("right", 79, 80, px), ("top", 0, -1, py), ("bottom", 59, 60, py)):
            sides[name] |= bool(((p >= inner) & (p < inner + 1)).any() and ((p >= outer) & (p < outer + 1)).any())      # on both sides of the bound
    assert all(sides.values()), sides
    T = scene.keyframes[4].T
    assert (fu.tr_row(T[8], T[9], T[10], T[11], (gx, gy, gz)) < 0).all()


@pytest.mark.parametrize("a", [0.0, 0.03])
def test_fusion_equals_the_restatement(gpu, scene, fused, a):
    torch, L, ctx = gpu
    dev = DeviceScene(torch, scene, a)
    assert_volumes_equal(gpu_fuse(gpu, scene, dev), fused[a])


def test_culling_changes_no_bit_and_skips_keyframes(gpu, scene, fused):
    torch, L, ctx = gpu
    dev = DeviceScene(torch, scene, 0.0)
    stats = {}
    try:
        for on in (1, 0):
            badslam_amd.check(L.bslam_set_culling(ctx.handle, on))
            badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
            tested, culled = C.c_uint64(), C.c_uint64()
            badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))     # reset
            got = gpu_fuse(gpu, scene, dev)
            badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))
            badslam_amd.check(L.bslam_profile_enable(ctx.handle, 0))
            assert_volumes_equal(got, fused[0.0])
            stats[on] = (tested.value, culled.value)
    finally:
        L.bslam_set_culling(ctx.handle, 1)
        L.bslam_profile_enable(ctx.handle, 0)
    bricks = 5 * 4 * 6
    assert stats[0] == (bricks * 6, 0)
    assert stats[1][0] == bricks * 6 and stats[1][1] >= 2 * bricks      # at least keyframes 3 and 4, for every brick
    assert stats[1][1] < 4 * bricks                                     # keyframes 0 - 2 see most of the volume


def test_two_calls_agree_and_a_null_colour_volume_is_left_alone(gpu, scene, fused):
    torch, L, ctx = gpu
    dev = DeviceScene(torch, scene, 0.0)
    first, second = gpu_fuse(gpu, scene, dev), gpu_fuse(gpu, scene, dev)
    assert_volumes_equal(first, second)
    without = gpu_fuse(gpu, scene, dev, with_color=False)               # asserts the sentinel-filled colour volume is untouched
    assert_volumes_equal(without[:2], fused[0.0][:2])


def test_no_keyframes(gpu, scene):
    torch, L, ctx = gpu
    dev = DeviceScene(torch, scene, 0.0)
    tsdf, count, color = gpu_fuse(gpu, scene, dev, count=0)
    assert (bits(tsdf) == bits(np.array([TRUNCATION], F))[0]).all() and not count.any() and not color.any()


# ------------------------------------------------------------------------------------------------
# 2. extraction
# ------------------------------------------------------------------------------------------------
def gpu_extract(gpu, tsdf, count, color, origin, voxel, min_count, slack=3):
    """bslam_extract_mesh of host volumes [nz, ny, nx] uploaded into pitched buffers: first the counts alone, then with buffers
    `slack` elements larger than needed.  Returns (positions, normals, colours or None, triangles); asserts that the count-only
    call writes nothing and that the slack stays untouched."""
    torch, L, ctx = gpu
    nz, ny, nx = tsdf.shape
    vol = volume_struct((nx, ny, nz), origin, voxel)
    t_t, t_b = pitched(torch, np.ascontiguousarray(tsdf, F).reshape(nz * ny, nx).view(np.int32), 5)
    c_t, c_b = pitched(torch, np.ascontiguousarray(count, np.uint32).reshape(nz * ny, nx).view(np.int32), 3)
    if color is not None:
        k_t, k_b = pitched(torch, np.ascontiguousarray(color, np.uint8).reshape(nz * ny, nx * 4).view(np.int32), 7)
    V, T = C.c_uint32(77), C.c_uint32(77)
    call = lambda vcap, tcap, p, n, c, i: badslam_amd.check(L.bslam_extract_mesh(
        ctx.handle, stream_ptr(torch), C.byref(vol), C.byref(t_b), C.byref(c_b), C.byref(k_b) if color is not None else None, min_count, vcap, tcap,
        p, n, c, i, C.byref(V), C.byref(T)))
    call(0, 0, None, None, None, None)
    nv, nt = V.value, T.value
    new = lambda words: torch.full((words,), SENTINEL, dtype=torch.int32, device="cuda")
    pos, nrm, col, idx = new(3 * nv + slack), new(3 * nv + slack), new(nv + slack), new(3 * nt + slack)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    if nv:
        # a capacity one short, for vertices and for triangles, and null buffers: counts only, nothing written
        short = [(nv - 1, nt, pos, idx), (nv, nt, None, idx), (nv, nt, pos, None)] + ([(nv, nt - 1, pos, idx)] if nt else [])
        for vcap, tcap, p, i in short:
            call(vcap, tcap, ptr(p) if p is not None else None, ptr(nrm), ptr(col), ptr(i) if i is not None else None)
            assert (V.value, T.value) == (nv, nt)
        torch.cuda.synchronize()
        for t in (pos, nrm, col, idx):
            assert bool((t == SENTINEL).all()), "a count-only call wrote to a buffer"
    call(nv, nt, ptr(pos), ptr(nrm), ptr(col), ptr(idx))
    torch.cuda.synchronize()
    assert (V.value, T.value) == (nv, nt)
    pos, nrm, col, idx = [t.cpu().numpy() for t in (pos, nrm, col, idx)]
    for t, used in ((pos, 3 * nv), (nrm, 3 * nv), (idx, 3 * nt), (col, nv if color is not None else 0)):
        assert (t[used:] == SENTINEL).all(), "written beyond the counts"
    return (pos[:3 * nv].view(F).reshape(nv, 3), nrm[:3 * nv].view(F).reshape(nv, 3),
            col[:nv].view(np.uint8).reshape(nv, 4) if color is not None else None, idx[:3 * nt].view(np.uint32).reshape(nt, 3))


def assert_mesh_equal(got, want):
    (gp, gn, gc, gt), (wp, wn, wc, wt) = got, want
    assert gp.shape == wp.shape and gt.shape == wt.shape, (gp.shape, wp.shape, gt.shape, wt.shape)
    assert np.array_equal(gt, wt)
    assert np.array_equal(bits(gp), bits(wp))
    assert (gc is None) == (wc is None) and (gc is None or np.array_equal(gc, wc))
    assert len(gn) == 0 or np.abs(gn.astype(np.float64) - wn).max() <= 1e-6


def extraction_fields():
    sphere = fu.sphere_field()
    ones = np.ones(sphere.shape, np.uint32)
    zeros = sphere.copy()
    zeros[np.abs(zeros) < 0.2] = 0.0                                    # samples of exactly 0.0f next to the surface: outside
    cut = np.ascontiguousarray(sphere[:, 3:, :22])                      # the sphere runs into three faces of the grid
    return {"sphere": (sphere, ones), "holed sphere": (sphere, fu.holed_sphere_count(sphere.shape)), "exact zeros": (zeros, ones),
            "boundary": (cut, np.ones(cut.shape, np.uint32)), "no crossing": (np.full((9, 8, 7), 0.25, F), np.ones((9, 8, 7), np.uint32))}


@pytest.mark.parametrize("name", ["sphere", "holed sphere", "exact zeros", "boundary", "no crossing"])
def test_extraction_of_given_fields(gpu, name):
    field, count = extraction_fields()[name]
    assert ((field.shape[0] - 1) * (field.shape[1] - 1) * (field.shape[2] - 1)) % 1024 not in (0, 1, 1023)
    origin, voxel = (0.3, -1.7, 2.9), 0.013
    want = fu.extract_mesh(field, count, None, origin, voxel, 1)
    got = gpu_extract(gpu, field, count, None, origin, voxel, 1)
    assert_mesh_equal(got, want)
    V, T = len(want[0]), len(want[3])
    if name == "sphere":
        assert (V, T) == (1774, 3544)
    elif name == "holed sphere":
        assert (V, T) == (1702, 3364)
    elif name == "exact zeros":
        assert (field == 0).sum() > 100 and T > 0
    elif name == "boundary":
        undirected, _ = fu.edge_census(want[3])
        assert V > 0 and (undirected == 1).any()                        # vertices in the boundary cells, the surface ends there
        on_face = np.abs(want[0][:, 0] - (origin[0] + 21.0 * voxel)) < 0.5 * voxel
        assert on_face.any()
    else:
        assert (V, T) == (0, 0)


@pytest.mark.parametrize("min_count", [1, 3])
def test_extraction_of_the_fused_volume(gpu, fused, min_count):
    tsdf, count, color = fused[0.0]
    want = fu.extract_mesh(tsdf, count, color, ORIGIN, VOXEL, min_count)
    assert len(want[0]) > 100 and len(want[3]) > 100
    assert_mesh_equal(gpu_extract(gpu, tsdf, count, color, ORIGIN, VOXEL, min_count), want)
    no_colour = gpu_extract(gpu, tsdf, count, None, ORIGIN, VOXEL, min_count)     # asserts the colour buffer stays untouched
    assert_mesh_equal(no_colour, want[:2] + (None,) + want[3:])


# ------------------------------------------------------------------------------------------------
# 3. rejected arguments
# ------------------------------------------------------------------------------------------------
def test_rejected_arguments(gpu, scene):
    torch, L, ctx = gpu
    dev = DeviceScene(torch, scene, 0.0)
    out = output_volumes(torch)
    K = len(scene.keyframes)
    base = dict(ctx=ctx.handle, color_camera=C.byref(scene.color_camera), depth_camera=C.byref(scene.depth_camera), dp=C.byref(dev.dp), K=K, views=dev.views,
                volume=volume_struct(), truncation=TRUNCATION, tsdf=out[0][1], count=out[1][1], color=out[2][1])

    def fuse(**changes):
        a = dict(base, **changes)
        ref = lambda v: None if v is None else C.byref(v)
        return L.bslam_fuse_keyframes(a["ctx"], stream_ptr(torch), a["color_camera"], a["depth_camera"], a["dp"], a["K"], a["views"], ref(a["volume"]),
                                      a["truncation"], ref(a["tsdf"]), ref(a["count"]), ref(a["color"]))

    def buffer(b, **changes):
        c = abi.Buffer2D(b.address, b.height, b.width, b.pitch)
        for k, v in changes.items():
            setattr(c, k, v)
        return c

    bad_views = (abi.KeyframeView * K)(*dev.views)
    bad_views[2].depth = buffer(bad_views[2].depth, width=79)
    nx, ny, nz = DIMS
    cases = {
        "null context": dict(ctx=None), "null depth camera": dict(depth_camera=None), "null depth parameters": dict(dp=None), "null volume": dict(volume=None),
        "null tsdf": dict(tsdf=None), "null count": dict(count=None), "colour volume without colour camera": dict(color_camera=None),
        "null tsdf address": dict(tsdf=buffer(out[0][1], address=None)),
        "voxel size 0": dict(volume=volume_struct(voxel=0.0)), "voxel size < 0": dict(volume=volume_struct(voxel=-0.02)),
        "voxel size inf": dict(volume=volume_struct(voxel=float("inf"))), "voxel size nan": dict(volume=volume_struct(voxel=float("nan"))),
        "truncation 0": dict(truncation=0.0), "truncation < 0": dict(truncation=-0.08), "truncation inf": dict(truncation=float("inf")),
        "truncation nan": dict(truncation=float("nan")),
        "nx 1": dict(volume=volume_struct((1, ny, nz))), "ny 1": dict(volume=volume_struct((nx, 1, nz))), "nz 0": dict(volume=volume_struct((nx, ny, 0))),
        "more than 2^30 samples": dict(volume=volume_struct((1024, 1024, 1025))), "dimensions whose product overflows": dict(volume=volume_struct((65536, 65536, 65536))),
        "volume of another shape": dict(volume=volume_struct((nx, ny, nz + 1))),
        "pitch too small": dict(count=buffer(out[1][1], pitch=4 * nx - 4)), "pitch misaligned": dict(tsdf=buffer(out[0][1], pitch=out[0][1].pitch + 2)),
        "address misaligned": dict(color=buffer(out[2][1], address=out[2][1].address + 2)),
        "tsdf and count overlap": dict(count=out[0][1]), "colour overlaps count": dict(color=buffer(out[1][1], address=out[1][1].address + out[1][1].pitch)),
        "negative keyframe count": dict(K=-1), "null keyframe list": dict(views=None), "keyframe depth of another size": dict(views=bad_views),
    }
    for name, changes in cases.items():
        rc = fuse(**changes)
        assert rc == INVALID_ARGUMENT, (name, rc, L.bslam_last_error())
    assert fuse() == 0                                                  # the unchanged arguments are fine
    torch.cuda.synchronize()

    V, T = C.c_uint32(), C.c_uint32()

    def extract(volume=base["volume"], tsdf=out[0][1], count=out[1][1], color=out[2][1], min_count=1, v=V, t=T, ctx_=ctx.handle):
        ref = lambda x: None if x is None else C.byref(x)
        return L.bslam_extract_mesh(ctx_, stream_ptr(torch), ref(volume), ref(tsdf), ref(count), ref(color), min_count, 0, 0, None, None, None, None, ref(v), ref(t))

    for name, kwargs in {"null context": dict(ctx_=None), "null volume": dict(volume=None), "null tsdf": dict(tsdf=None), "null count": dict(count=None),
                         "null vertex count": dict(v=None), "null triangle count": dict(t=None), "min_count 0": dict(min_count=0),
                         "nz 1": dict(volume=volume_struct((nx, ny, 1))), "volume of another shape": dict(volume=volume_struct((nx + 1, ny, nz))),
                         "voxel size 0": dict(volume=volume_struct(voxel=0.0)), "pitch misaligned": dict(color=buffer(out[2][1], pitch=out[2][1].pitch + 1)),
                         "more than 2^30 samples": dict(volume=volume_struct((2048, 1024, 1024)))}.items():
        rc = extract(**kwargs)
        assert rc == INVALID_ARGUMENT, (name, rc, L.bslam_last_error())
    assert extract() == 0 and extract(color=None) == 0


# ------------------------------------------------------------------------------------------------
# 4. through DirectBA
# ------------------------------------------------------------------------------------------------
def test_fusion_through_direct_ba():
    """Three 160 x 120 keyframes of tests/scenes.py (20 random planes n . x + 2.5 = 0) at cell size 2: ModelBounds, FuseKeyframes at
    2 cm, Volume and ExtractMesh equal the restatements applied to the keyframe images, poses and calibration the object holds.

    Plane distance of the vertices, measured beforehand on the CPU with the restatement on this scene (surfels of the oracle's
    creation path, 150 x 118 x 49 samples): 24 070 vertices, median 0.74 mm, 99th percentile 4.15 mm, max 8.93 mm (at the
    creases between planes, under half a voxel).  Asserted at twice the 99th percentile and max; the margin is for the slightly
    different box of the surfels this run creates."""
    from badslam_amd.direct_ba import DirectBA
    from tests import bso, scenes
    cam = bso.make_camera(131.25, 131.25, 80.0, 60.0, 160, 120)
    scene = scenes.synthetic_scene(3, width=160, height=120, cell=2, camera=cam)
    ba = DirectBA(scene.max_surfels, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, 0.8, 1, 1, 1, scene.color_camera, scene.depth_camera, 0, True, False)
    assert ba.ModelBounds() is None
    with pytest.raises(Exception):
        ba.ExtractMesh()                                                # no volume yet
    for kf in scene.keyframes:
        ba.AddKeyframe(kf.id, max(kf.min_depth, 1e-3), max(kf.max_depth, 1e-2), kf.depth, kf.normals, kf.radius, kf.color, kf.global_T_frame)
    for kf in scene.keyframes:
        ba.CreateSurfelsForKeyframe(False, kf.id)
    rows = ba.GetSurfels(3)[:, :ba.surfels_size()]
    valid = ~np.isnan(rows[0])
    lo, hi = ba.ModelBounds()
    assert np.array_equal(lo, rows[:, valid].min(axis=1)) and np.array_equal(hi, rows[:, valid].max(axis=1))
    from tools import run_tum
    voxel, truncation = 0.02, 0.08
    origin, dims = run_tum.mesh_volume(lo, hi, voxel, truncation)
    ba.FuseKeyframes(origin, voxel, dims, truncation)
    volume = ba.Volume()
    assert volume["dims"] == dims and volume["voxel_size"] == F(voxel) and np.array_equal(volume["origin"], origin)
    keyframes = []
    for k in range(3):
        depth, _, _, color, _, _ = ba.keyframe_images(k, 120, 160)
        # frame_T_global as the library forms it from the keyframe's pose: the matrix a model view from that pose reports
        T = ba.RenderModel(ba.keyframe_pose(k), views=("depth",))["camera_T_global"]
        keyframes.append(fu.Keyframe(depth, color, T))
    _, depth4, a = ba.intrinsics()
    assert a == 0.0
    camera = abi.Camera4f(*[float(v) for v in depth4], 160, 120)
    cfactor = ba.cfactor(scene.cfactor.shape)
    want = fu.fuse(keyframes, camera, camera, cfactor, 0.0, scene.raw_to_float_depth, scene.cell, origin, voxel, dims, truncation)
    assert_volumes_equal((volume["tsdf"], volume["count"], volume["color"]), want)
    mesh = ba.ExtractMesh(1)
    want_mesh = fu.extract_mesh(*want, origin, voxel, 1)
    assert_mesh_equal((mesh["positions"], mesh["normals"], mesh["colors"], mesh["triangles"]), want_mesh)
    planes = scenes.random_planes(np.random.default_rng(0xBAD51A4), 20)
    p = mesh["positions"].astype(np.float64)
    distance = np.min([np.abs(p @ n.astype(np.float64) + 2.5) for n in planes], axis=0)
    print(f"{len(p)} vertices, {len(mesh['triangles'])} triangles: plane distance median {np.median(distance):.5f}, p99 {np.percentile(distance, 99):.5f}, max {distance.max():.5f}")
    assert len(p) > 20000
    assert np.percentile(distance, 99) < 2 * 4.15e-3 and distance.max() < 2 * 8.93e-3
    # a deleted keyframe is left out; min_count then drops what only one of the others saw
    ba.DeleteKeyframe(1)
    ba.FuseKeyframes(origin, voxel, dims, truncation)
    want2 = fu.fuse([keyframes[0], keyframes[2]], camera, camera, cfactor, 0.0, scene.raw_to_float_depth, scene.cell, origin, voxel, dims, truncation)
    v2 = ba.Volume()
    assert_volumes_equal((v2["tsdf"], v2["count"], v2["color"]), want2)
    mesh2 = ba.ExtractMesh(2)
    assert_mesh_equal((mesh2["positions"], mesh2["normals"], mesh2["colors"], mesh2["triangles"]), fu.extract_mesh(*want2, origin, voxel, 2))
    with pytest.raises(Exception, match="voxel size"):
        ba.FuseKeyframes(origin, 0.001, (2000, 2000, 2000), truncation)
    ba.close()


# ------------------------------------------------------------------------------------------------
# 5. the tool
# ------------------------------------------------------------------------------------------------
def test_run_tum_mesh_and_point_cloud(tmp_path):
    """tools/run_tum.py --mesh --point-cloud on five frames of the rendered sequence of tests/test_gpu_bad_slam.py: both files
    parse, the mesh file holds ExtractMesh of the same run and the cloud ExportToPointCloud."""
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
        seen["mesh"] = slam.ba().ExtractMesh(2)
        seen["cloud"] = slam.ba().ExportToPointCloud()
        seen["volume"] = slam.ba().Volume()

    mesh_path, cloud_path = tmp_path / "model.ply", tmp_path / "cloud.ply"
    r = run_tum.run(source, keyframe_interval=4, ba_iterations=2, max_depth=6.0, num_scales=4, max_surfel_count=400000, mesh=mesh_path, mesh_voxel_size=0.04,
                    mesh_min_count=2, point_cloud=cloud_path, inspect=inspect)
    assert r["keyframes"] == 2
    assert seen["volume"]["voxel_size"] == F(0.04) and seen["volume"]["truncation"] == F(0.16) and seen["volume"]["dims"] == r["mesh"]["dims"]
    vertices, faces, _ = fu.read_ply(mesh_path)
    mesh = seen["mesh"]
    assert len(vertices) == r["mesh"]["vertices"] == len(mesh["positions"]) > 1000 and len(faces) == r["mesh"]["triangles"] == len(mesh["triangles"]) > 1000
    assert np.array_equal(bits(np.stack([vertices["x"], vertices["y"], vertices["z"]], 1)), bits(mesh["positions"]))
    assert np.array_equal(bits(np.stack([vertices["nx"], vertices["ny"], vertices["nz"]], 1)), bits(mesh["normals"]))
    assert np.array_equal(np.stack([vertices["red"], vertices["green"], vertices["blue"]], 1), mesh["colors"][:, :3])
    assert np.array_equal(faces, mesh["triangles"].astype(np.int32))
    points, none, _ = fu.read_ply(cloud_path)
    positions, colors, normals = seen["cloud"]
    assert none is None and len(points) == r["point_cloud"][1] == len(positions) > 1000
    assert np.array_equal(bits(np.stack([points["x"], points["y"], points["z"]], 1)), bits(positions))
    assert np.array_equal(np.stack([points["red"], points["green"], points["blue"]], 1), colors)
    assert np.array_equal(bits(np.stack([points["nx"], points["ny"], points["nz"]], 1)), bits(normals))
    with pytest.raises(ValueError, match="voxel-size"):
        run_tum.mesh_volume([0, 0, 0], [10, 10, 11], 0.001, 0.004)
