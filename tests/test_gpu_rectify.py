"""-m gpu: the sensor-rectification kernels (bslam_build_undistortion_map, bslam_undistort_rgb, bslam_reproject_depth;
badslam_amd/csrc/rectify_kernels.hpp) against the NumPy restatements of tests/rectify_util.py.  Every image is tiny, of odd
size and pitched wider than its rows; the padding must come back untouched."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi
from badslam_amd import rectification as rect
from tests import rectify_util as ru

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT = -1   # BSLAM_ERR_INVALID_ARGUMENT
SCALE = 5000.0          # depth units per metre on both sides unless a test says otherwise


@pytest.fixture(scope="module")
def gpu():
    import torch
    from badslam_amd import build
    build.build()
    return torch, badslam_amd.lib(), badslam_amd.Context(0)


# ------------------------------------------------------------------------------------------------
# device calls
# ------------------------------------------------------------------------------------------------
def gpu_map(gpu, source, target):
    torch, L, ctx = gpu
    store, buf = ru.pitched(torch, np.full((target.height, 2 * target.width), -7.0, np.float32), 1, -7.0, elems_per_pixel=2)   # rows 4, not 8, byte aligned
    badslam_amd.check(L.bslam_build_undistortion_map(ctx.handle, ru.stream_ptr(torch), C.byref(source), C.byref(target), C.byref(buf)))
    torch.cuda.synchronize()
    image, padding = ru.fetch(store, 2 * target.width, np.float32)
    assert (padding == -7.0).all()
    return image.reshape(target.height, target.width, 2)


def gpu_undistort(gpu, image, mapping):
    torch, L, ctx = gpu
    h, w = image.shape[:2]
    oh, ow = mapping.shape[:2]
    in_store, in_buf = ru.pitched(torch, image.reshape(h, 3 * w), 5, 0x33, elems_per_pixel=3)
    map_store, map_buf = ru.pitched(torch, mapping.reshape(oh, 2 * ow), 3, 0.0, elems_per_pixel=2)
    out_store, out_buf = ru.pitched(torch, np.full((oh, 3 * ow), 0x5A, np.uint8), 7, 0x5A, elems_per_pixel=3)
    badslam_amd.check(L.bslam_undistort_rgb(ctx.handle, ru.stream_ptr(torch), C.byref(in_buf), C.byref(map_buf), C.byref(out_buf)))
    torch.cuda.synchronize()
    out, padding = ru.fetch(out_store, 3 * ow, np.uint8)
    assert (padding == 0x5A).all()
    return out.reshape(oh, ow, 3)


def gpu_reproject(gpu, depth, unprojection, T, target, threshold, in_scale=1.0 / SCALE, out_scale=SCALE):
    torch, L, ctx = gpu
    h, w = depth.shape
    in_store, in_buf = ru.pitched(torch, depth, 3, 0x3333)
    map_store, map_buf = ru.pitched(torch, unprojection.reshape(h, 2 * w), 1, 0.0, elems_per_pixel=2)
    out_store, out_buf = ru.pitched(torch, np.full((target.height, target.width), 0x5A5A, np.uint16), 5, 0x5A5A)
    M = None
    if T is not None:
        M = abi.Mat3x4()
        M.m[:] = [float(v) for v in np.asarray(T, np.float32).reshape(12)]
    badslam_amd.check(L.bslam_reproject_depth(ctx.handle, ru.stream_ptr(torch), C.byref(in_buf), in_scale, C.byref(map_buf),
                                              C.byref(M) if M is not None else None, C.byref(target), threshold, out_scale, C.byref(out_buf)))
    torch.cuda.synchronize()
    out, padding = ru.fetch(out_store, target.width, np.uint16)
    assert (padding.view(np.uint16) == 0x5A5A).all()
    return out


def ulp_of(value):
    return float(np.spacing(np.float32(value)))


# ------------------------------------------------------------------------------------------------
# undistortion map and colour undistortion
# ------------------------------------------------------------------------------------------------
def map_cases():
    """(source, target): 67 x 45 -> 61 x 41 is the pincushion camera with its own undistorted camera, moved by 0.8 pixels so
    that the first column looks outside the source; 33 x 31 -> 40 x 37 is a barrel camera under a target wider than its view."""
    a = rect.radtan_camera(67, 45, 60.0, 61.0, 33.2, 21.7, 0.25, -0.07, 0.0, -8e-4, 1.1e-3)
    ta = rect.decide_undistorted_camera(a, True)
    assert (ta.width, ta.height) == (61, 41)
    ta.cx += 0.8
    b = rect.radtan_camera(33, 31, 30.0, 29.0, 16.4, 14.9, -0.2, 0.05, 0.01, 2e-3, -1e-3)
    tb = abi.Camera4f(30.0, 29.0, 20.3, 18.6, 40, 37)
    return {"67x45_to_61x41": (a, ta), "33x31_to_40x37": (b, tb)}


@pytest.mark.parametrize("case", sorted(map_cases()))
def test_undistortion_map_against_float64(gpu, case):
    source, target = map_cases()[case]
    got = gpu_map(gpu, source, target)
    want, unclamped = ru.undistortion_map64(source, target)
    bound = 8 * ulp_of(max(source.width, source.height) - 1)     # 8 ulps of the largest coordinate
    err = np.abs(got.astype(np.float64) - want)
    print(f"{case}: max error {err.max():.3g} px, bound {bound:.3g} px")
    assert err.max() <= bound
    outside = (unclamped[..., 0] < 0) | (unclamped[..., 0] > source.width - 1) | (unclamped[..., 1] < 0) | (unclamped[..., 1] > source.height - 1)
    assert outside.any(), "the case must hit the clamp"
    assert got[..., 0].min() >= 0 and got[..., 0].max() <= source.width - 1 and got[..., 1].min() >= 0 and got[..., 1].max() <= source.height - 1
    # in the kernel's own expression order nothing is left to rounding
    assert np.array_equal(got, ru.undistortion_map32(source, target))


@pytest.mark.parametrize("case", sorted(map_cases()))
def test_colour_undistortion_is_byte_identical_to_the_float32_restatement(gpu, case):
    source, target = map_cases()[case]
    mapping = gpu_map(gpu, source, target)
    image = np.random.default_rng(11).integers(0, 256, (source.height, source.width, 3), dtype=np.uint8)
    got = gpu_undistort(gpu, image, mapping)
    want = ru.undistort_rgb32(image, mapping)
    assert np.array_equal(got, want), f"{(got != want).sum()} bytes differ"
    # a position on the last column / row (the clamp's upper end) takes the border texel itself
    corner = np.array([[[source.width - 1, source.height - 1], [0.0, 0.0]]], np.float32)
    assert np.array_equal(gpu_undistort(gpu, image, corner)[0], np.stack([image[-1, -1], image[0, 0]]))


# ------------------------------------------------------------------------------------------------
# depth reprojection
# ------------------------------------------------------------------------------------------------
def plain_depth_camera(width, height, f=40.0):
    return rect.radtan_camera(width, height, f, f, (width - 1) / 2.0, (height - 1) / 2.0)


def test_depth_identity(gpu):
    """Zero distortion, no transform, target = source: every vertex lands on its own pixel centre, and depths that are whole
    output units come back as they went in (scale * z sits half a unit below the rounding boundary)."""
    rng = np.random.default_rng(2)
    cam = plain_depth_camera(37, 29)
    depth = (3000 + rng.integers(-20, 21, (29, 37))).astype(np.uint16)            # 4 mm of relief, threshold 50 mm
    depth[rng.random(depth.shape) < 0.04] = 0
    depth[10:13, 20:26] = 0
    got = gpu_reproject(gpu, depth, rect.make_unprojection_map(cam), None, ru.pinhole_of(cam), 0.05)
    valid = depth != 0
    all_nine = np.zeros_like(valid)
    all_nine[1:-1, 1:-1] = np.logical_and.reduce([valid[1 + dy:28 + dy, 1 + dx:36 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    assert all_nine.sum() > 400
    assert np.array_equal(got[all_nine], depth[all_nine])
    # a pixel none of whose four blocks is complete gets nothing
    padded = np.pad(valid, 1)
    block_ok = padded[:-1, :-1] & padded[:-1, 1:] & padded[1:, :-1] & padded[1:, 1:]      # block with top-left vertex (y - 1, x - 1)
    any_block = block_ok[:-1, :-1] | block_ok[:-1, 1:] | block_ok[1:, :-1] | block_ok[1:, 1:]
    assert (~any_block).sum() > 20
    assert (got[~any_block] == 0).all()
    # the same with an explicit identity matrix
    assert np.array_equal(got, gpu_reproject(gpu, depth, rect.make_unprojection_map(cam), np.eye(4)[:3], ru.pinhole_of(cam), 0.05))


def test_depth_discontinuity(gpu):
    """A 0.4 m step: with the 0.05 m threshold the blocks across it are dropped and the target pixels strictly between the two
    surfaces stay empty; with a threshold above the step they are filled.  The target is twice as fine as the source, so two
    target columns lie strictly between the source columns 14 and 15."""
    cam = plain_depth_camera(31, 23)
    depth = np.full((23, 31), 5000, np.uint16)
    depth[:, 15:] = 7000
    target = abi.Camera4f(80.0, 80.0, 31.0, 23.0, 62, 46)
    unprojection = rect.make_unprojection_map(cam)
    cut = gpu_reproject(gpu, depth, unprojection, None, target, 0.05)
    between = slice(29, 31)       # source columns 14 and 15 land on target x = 29 and 31: the centres 29.5 and 30.5 lie between
    rows = slice(2, 44)
    assert (cut[rows, between] == 0).all()
    assert (cut[rows, 4:29] == 5000).all() and (cut[rows, 33:58] == 7000).all()
    filled = gpu_reproject(gpu, depth, unprojection, None, target, 0.5)
    assert ((filled[rows, between] > 5000) & (filled[rows, between] < 7000)).all()
    assert np.array_equal(filled[rows, 4:29], cut[rows, 4:29]) and np.array_equal(filled[rows, 33:58], cut[rows, 33:58])


def test_depth_occlusion_and_determinism(gpu):
    """A near plane (0.4 m) in front of a far one (2 m) and a 30 mm baseline: the near surface moves 6 pixels, the far one 1.2,
    so the near one covers far-surface pixels on its right side.  Those hold the near depth; two runs are bit-identical."""
    cam = plain_depth_camera(41, 27, f=80.0)
    depth = np.full((27, 41), 10000, np.uint16)
    depth[8:20, 12:24] = 2000                      # near vertices: columns 12 ... 23, rows 8 ... 19
    T = np.eye(4)[:3].copy()
    T[0, 3] = 0.03
    target = ru.pinhole_of(cam)
    unprojection = rect.make_unprojection_map(cam)
    got = gpu_reproject(gpu, depth, unprojection, T, target, 0.05)
    # near surface: pixel-corner x from 12.5 + 6 to 23.5 + 6 -> pixels 19 ... 28 strictly inside; rows 8.5 ... 19.5 -> 9 ... 18
    assert (got[9:19, 19:29] == 2000).all()
    # far surface right of the hole: blocks from column 24 on, x from 24.5 + 1.2 -> pixels 26 ... 28 are covered by both
    far_only = depth.copy()
    far_only[8:20, 12:24] = 0
    far = gpu_reproject(gpu, far_only, unprojection, T, target, 0.05)
    both = (far[9:19, 19:29] == 10000)
    assert both[:, 7:].all() and both.sum() >= 30
    assert (got == 10000).sum() > 300
    again = gpu_reproject(gpu, depth, unprojection, T, target, 0.05)
    assert np.array_equal(got, again)


def surface_scene(rng, cam, step_column):
    """Raw depth of a smooth random surface over two planes with a 0.5 m step at step_column, in units of 1 / SCALE m."""
    xs, ys = ru.pixel_grid(cam.width, cam.height)
    z = 1.2 + 0.1 * xs / cam.width + 0.04 * np.sin(0.31 * xs + rng.uniform(0, 6)) * np.cos(0.27 * ys + rng.uniform(0, 6))
    z = np.where(xs >= step_column, z + 0.5 - 0.15 * ys / cam.height, z)
    depth = (z * SCALE + 0.5).astype(np.uint16)
    depth[rng.random(depth.shape) < 0.01] = 0
    return depth


def compare_with_restatement(gpu, depth, cam, T, target, label):
    unprojection = rect.make_unprojection_map(cam)
    got = gpu_reproject(gpu, depth, unprojection, T, target, 0.05)
    want, near_edge = ru.reproject_depth64(depth, 1.0 / SCALE, unprojection, T, target, 0.05, SCALE)
    left_out = near_edge.mean()
    keep = ~near_edge
    covered = keep & (want != 0)
    assert covered.sum() > 0.3 * want.size
    equal_share = (got[covered] == want[covered]).mean()
    print(f"{label}: left out {100 * left_out:.2f} % of the pixels, covered {covered.sum()}, exactly equal {100 * equal_share:.2f} %")
    assert left_out <= 0.02
    assert np.array_equal((got != 0)[keep], (want != 0)[keep])
    assert np.abs(got[covered].astype(np.int64) - want[covered].astype(np.int64)).max() <= 1
    assert equal_share >= 0.90
    return got


def test_depth_finer_target(gpu):
    """24 x 18 into 96 x 72: a triangle's box holds dozens of pixel centres."""
    rng = np.random.default_rng(5)
    cam = rect.radtan_camera(24, 18, 22.0, 22.0, 11.3, 8.6, -0.1, 0.02, 0.0, 1e-3, -5e-4)
    depth = surface_scene(rng, cam, 13)
    target = abi.Camera4f(96.0, 96.0, 47.3, 36.4, 96, 72)
    T = np.eye(4)[:3].copy()
    T[0, 3] = 0.01
    compare_with_restatement(gpu, depth, cam, T, target, "finer target")


def test_depth_general_parity(gpu):
    """Radtan depth camera 48 x 36 into a 56 x 40 target, 25 mm beside it and turned by 1 degree."""
    from tests import scenes
    rng = np.random.default_rng(7)
    cam = rect.radtan_camera(48, 36, 42.0, 43.0, 23.4, 17.2, -0.18, 0.04, 0.0, 8e-4, -6e-4)
    depth = surface_scene(rng, cam, 27)
    target = abi.Camera4f(50.0, 50.0, 28.2, 20.1, 56, 40)
    T = np.eye(4)[:3].copy()
    T[:, :3] = scenes.rotation_from_log(np.deg2rad(1.0) * np.array([0.3, 0.9, -0.3]) / np.linalg.norm([0.3, 0.9, -0.3]))
    T[:, 3] = [0.025, 0.002, -0.001]
    compare_with_restatement(gpu, depth, cam, T, target, "general parity")


# ------------------------------------------------------------------------------------------------
# argument errors: BSLAM_ERR_INVALID_ARGUMENT, nothing launched
# ------------------------------------------------------------------------------------------------
ARGUMENT_CASES = ("null_input", "null_map", "null_output", "map_of_wrong_size", "pitch_too_small", "overlap", "threshold_zero", "threshold_negative")


@pytest.mark.parametrize("case", ARGUMENT_CASES)
def test_reproject_depth_argument_errors(gpu, case):
    torch, L, ctx = gpu
    cam = plain_depth_camera(21, 13)
    target = ru.pinhole_of(cam)
    depth = np.full((13, 21), 4000, np.uint16)
    in_store, in_buf = ru.pitched(torch, depth, 3, 0)
    map_store, map_buf = ru.pitched(torch, rect.make_unprojection_map(cam).reshape(13, 42), 2, 0.0, elems_per_pixel=2)
    out_store, out_buf = ru.pitched(torch, np.full((13, 21), 0x5A5A, np.uint16), 3, 0x5A5A)
    threshold = 0.05
    a, m, o = C.byref(in_buf), C.byref(map_buf), C.byref(out_buf)
    if case == "null_input":
        a = None
    elif case == "null_map":
        m = None
    elif case == "null_output":
        o = None
    elif case == "map_of_wrong_size":
        map_buf.width -= 1
    elif case == "pitch_too_small":
        in_buf.pitch = 2 * 21 - 2
    elif case == "overlap":
        out_buf.address = in_buf.address + in_buf.pitch * 5          # the output starts inside the input
    elif case == "threshold_zero":
        threshold = 0.0
    elif case == "threshold_negative":
        threshold = -0.05
    rc = L.bslam_reproject_depth(ctx.handle, ru.stream_ptr(torch), a, 1.0 / SCALE, m, None, C.byref(target), threshold, SCALE, o)
    torch.cuda.synchronize()
    assert rc == INVALID_ARGUMENT, (case, L.bslam_last_error())
    assert (out_store.cpu().numpy().view(np.uint16) == 0x5A5A).all()


@pytest.mark.parametrize("case", ("null_input", "null_map", "null_output", "map_of_wrong_size", "pitch_too_small", "overlap"))
def test_undistort_rgb_argument_errors(gpu, case):
    torch, L, ctx = gpu
    image = np.zeros((13, 21 * 3), np.uint8)
    in_store, in_buf = ru.pitched(torch, image, 4, 0, elems_per_pixel=3)
    map_store, map_buf = ru.pitched(torch, np.zeros((11, 19 * 2), np.float32), 2, 0.0, elems_per_pixel=2)
    out_store, out_buf = ru.pitched(torch, np.full((11, 19 * 3), 0x5A, np.uint8), 4, 0x5A, elems_per_pixel=3)
    a, m, o = C.byref(in_buf), C.byref(map_buf), C.byref(out_buf)
    if case == "null_input":
        a = None
    elif case == "null_map":
        m = None
    elif case == "null_output":
        o = None
    elif case == "map_of_wrong_size":
        map_buf.height -= 1
    elif case == "pitch_too_small":
        out_buf.pitch = 3 * 19 - 1
    elif case == "overlap":
        out_buf.address = in_buf.address + 8
    rc = L.bslam_undistort_rgb(ctx.handle, ru.stream_ptr(torch), a, m, o)
    torch.cuda.synchronize()
    assert rc == INVALID_ARGUMENT, (case, L.bslam_last_error())
    assert (out_store.cpu().numpy() == 0x5A).all()


@pytest.mark.parametrize("case", ("null_source", "null_target", "null_map", "map_of_wrong_size", "pitch_too_small"))
def test_build_undistortion_map_argument_errors(gpu, case):
    torch, L, ctx = gpu
    source, target = map_cases()["33x31_to_40x37"]
    store, buf = ru.pitched(torch, np.full((37, 80), -7.0, np.float32), 2, -7.0, elems_per_pixel=2)
    s, t, m = C.byref(source), C.byref(target), C.byref(buf)
    if case == "null_source":
        s = None
    elif case == "null_target":
        t = None
    elif case == "null_map":
        m = None
    elif case == "map_of_wrong_size":
        buf.width += 1
    elif case == "pitch_too_small":
        buf.pitch = 8 * 40 - 4
    rc = L.bslam_build_undistortion_map(ctx.handle, ru.stream_ptr(torch), s, t, m)
    torch.cuda.synchronize()
    assert rc == INVALID_ARGUMENT, (case, L.bslam_last_error())
    assert (store.cpu().numpy() == -7.0).all()
