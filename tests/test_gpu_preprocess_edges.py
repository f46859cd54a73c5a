"""-m gpu: the five preprocessing producers against the oracle, bit for bit, where the pipeline test never runs them: odd
and tiny shapes, rows that are not 4-byte aligned, a base pointer off the allocator's alignment, a pitched cfactor grid,
both signs of fy, cell sizes that do not divide the width, the other bilateral parameter sets, a radii input with a valid
border.  tests/test_preprocess_reference_cpu.py is what makes the oracle trustworthy on these inputs.

Layout of every device image: the input rows carry 3 extra elements holding 0x3333 -- a valid-looking depth below the
cut-off, so a read past the row end changes a result instead of hiding -- and every output's rows 5 extra elements
holding 0x5A5A, which must come back untouched.  `lead` additionally starts the image one element into its storage.
Every storage ends with its last row's padding, so a row and its padding lie inside the allocation."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi
from tests import preprocess_util as U
from tests.test_gpu_preprocess import stream_ptr

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT = -1                       # BSLAM_ERR_INVALID_ARGUMENT
SHAPES = [(37, 67), (5, 257), (3, 3), (1, 5)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    return torch, badslam_amd.lib(), badslam_amd.Context(0)


def gpu_bilateral(gpu, raw, params, lead=0):
    torch, L, ctx = gpu
    im = U.Images(torch, lead)
    a, b = im.input(raw), im.output(*raw.shape)
    sigma_xy, sigma_value, radius_factor, max_depth = params
    badslam_amd.check(L.bslam_bilateral_filter_and_depth_cutoff(ctx.handle, stream_ptr(torch), sigma_xy, sigma_value, radius_factor, int(max_depth),
                                                               U.RAW_TO_FLOAT, C.byref(a), C.byref(b)))
    return im.fetch()[0]


def gpu_normals(gpu, depth, camera, cfactor, cell, lead=0):
    torch, L, ctx = gpu
    im = U.Images(torch, lead)
    dp = U.depth_params(im.input(cfactor, pad=2, fill=np.float32(1e9)), cell)          # a cfactor read past its row would wreck the depth
    a, b, c = im.input(depth), im.output(*depth.shape), im.output(*depth.shape)
    badslam_amd.check(L.bslam_compute_normals(ctx.handle, stream_ptr(torch), C.byref(camera), C.byref(dp), C.byref(a), C.byref(b), C.byref(c)))
    return im.fetch()


def gpu_radii(gpu, depth, camera, lead=0):
    torch, L, ctx = gpu
    im = U.Images(torch, lead)
    a, b, c = im.input(depth), im.output(*depth.shape), im.output(*depth.shape)
    badslam_amd.check(L.bslam_compute_point_radii_and_remove_isolated_pixels(ctx.handle, stream_ptr(torch), C.byref(camera), U.RAW_TO_FLOAT,
                                                                            C.byref(a), C.byref(b), C.byref(c)))
    return im.fetch()          # radius bits, depth


def gpu_min_max(gpu, depth, lead=0, pad=U.IN_PAD):
    torch, L, ctx = gpu
    im = U.Images(torch, lead)
    a = im.input(depth, pad=pad)
    mn, mx = C.c_float(), C.c_float()
    badslam_amd.check(L.bslam_compute_min_max_depth(ctx.handle, stream_ptr(torch), C.byref(a), U.RAW_TO_FLOAT, C.byref(mn), C.byref(mx)))
    return np.float32(mn.value), np.float32(mx.value)


def gpu_brightness(gpu, rgb, lead=0):
    torch, L, ctx = gpu
    im = U.Images(torch, lead)
    a, b = im.input(rgb), im.output(rgb.shape[0], rgb.shape[1], np.uint32)
    badslam_amd.check(L.bslam_compute_brightness(ctx.handle, stream_ptr(torch), C.byref(a), C.byref(b)))
    return np.ascontiguousarray(im.fetch()[0]).view(np.uint8).reshape(rgb.shape[0], rgb.shape[1], 4)


def equal(got, want):
    return got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("fy_sign,cell", [(1, 3), (1, 4), (-1, 3), (-1, 4)])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_stage_on_pitched_odd_shapes(oracle, gpu, shape, fy_sign, cell, lead):
    """Each stage on the oracle's output of the stage before it, so a difference names its stage."""
    h, w = shape
    raw = U.shaped_raw_depth(h, w)
    camera, cfactor = U.build_camera(h, w, fy_sign), U.build_cfactor(h, w, cell)
    assert cfactor.shape == (-(-h // cell), -(-w // cell)) and (w < 4 or w % cell)
    params = U.BILATERAL_SETS["default"]
    filtered = U.oracle_bilateral(raw, *params)
    assert equal(gpu_bilateral(gpu, raw, params, lead), filtered), "bilateral"

    stage1, normals = U.oracle_normals(filtered, camera, cfactor, cell)
    got_stage1, got_normals = gpu_normals(gpu, filtered, camera, cfactor, cell, lead)
    assert equal(got_stage1, stage1) and equal(got_normals, normals), "normals"

    radius, depth = U.oracle_radii(stage1, camera)
    got_radius, got_depth = gpu_radii(gpu, stage1, camera, lead)
    assert equal(got_depth, depth) and equal(got_radius, radius), "radii"

    want = U.f32_min_max(stage1)
    assert U.oracle_min_max(stage1) == want and gpu_min_max(gpu, stage1, lead) == want, "min / max"
    assert gpu_min_max(gpu, filtered, lead) == U.f32_min_max(filtered)

    rgb = U.build_rgb(h, w)
    assert equal(gpu_brightness(gpu, rgb, lead), U.oracle_brightness(rgb)), "brightness"

    interior = (stage1 != U.UNKNOWN).sum()
    if shape == (1, 5):                                                     # no interior at all
        assert interior == 0 and (normals == 0).all() and np.isinf(want[0]) and want[1] == 0 and (radius == 0).all() and (filtered != U.UNKNOWN).all()
    elif shape == (3, 3):                                                   # a single interior pixel, kept by the normals, isolated for the radii
        assert interior == 1 and stage1[1, 1] != U.UNKNOWN and (depth == U.UNKNOWN).all() and want[0] == want[1]
    elif shape == (5, 257):                                                 # the second block's only lane holds a measurement
        assert filtered[:, 256].min() < 32768 and interior > 300 and (depth != U.UNKNOWN).sum() > 50
    else:
        assert interior > 1500 and (depth != U.UNKNOWN).sum() > 700


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("shape", [(37, 67), (5, 257)])
def test_radii_on_an_input_with_a_valid_border(oracle, gpu, shape, wide, lead):
    """The bilateral output goes straight to the radii: the kernel's own image-bounds test decides on the border, with the
    valid-looking 0x3333 padding right next to the last column."""
    h, w = shape
    filtered = U.oracle_bilateral(U.shaped_raw_depth(h, w), *U.BILATERAL_SETS["default"])
    border = np.ones(shape, bool)
    border[1:-1, 1:-1] = False
    assert ((filtered[border] & U.INVALID_BIT) == 0).sum() > 0.8 * border.sum() and (filtered[:, -1] < 32768).sum() >= 3
    camera = U.build_camera(h, w, 1, wide)
    radius, depth = U.oracle_radii(filtered, camera)
    got_radius, got_depth = gpu_radii(gpu, filtered, camera, lead)
    assert (got_depth[border] == U.UNKNOWN).all() and (got_radius[border] == 0).all()
    assert equal(got_depth, depth) and equal(got_radius, radius)
    assert (depth != U.UNKNOWN).sum() > 0.5 * (~border).sum()
    assert ((depth != U.UNKNOWN)[:, -2]).any()                              # kept pixels whose right neighbour is the last column


@pytest.mark.parametrize("shape", [(37, 67), (3, 3)])
@pytest.mark.parametrize("name", list(U.BILATERAL_SETS))
def test_bilateral_parameter_sets(oracle, gpu, name, shape):
    raw = U.shaped_raw_depth(*shape)
    want = U.oracle_bilateral(raw, *U.BILATERAL_SETS[name])
    for lead in (0, 1):
        assert equal(gpu_bilateral(gpu, raw, U.BILATERAL_SETS[name], lead), want)
    if shape == (37, 67):
        if name == "no_cutoff":
            assert ((want >= 32768) & (want < 65534)).any()
        else:
            assert (want[raw == U.MAX_DEPTH] != U.UNKNOWN).all() and (raw == U.MAX_DEPTH).any() and (want[raw > U.MAX_DEPTH] == U.UNKNOWN).all()


def test_min_max_extremes_and_reuse_of_a_context(oracle, gpu):
    h, w = 5, 257
    near, far = np.uint16(700), np.uint16(31000)

    def image(*pixels):
        depth = np.full((h, w), U.UNKNOWN, np.uint16)
        for (y, x), value in pixels:
            depth[y, x] = value
        return depth

    first, last = (0, 0), (h - 1, w - 1)
    for depth in (image((first, near), (last, far)), image((first, far), (last, near)), image(((2, 255), near), ((2, 256), far)),
                  image((last, near)), image((first, far)), image(((3, 256), np.uint16(32767)), ((1, 64), np.uint16(1)))):
        want = U.f32_min_max(depth)
        for lead in (0, 1):
            assert U.oracle_min_max(depth) == want and gpu_min_max(gpu, depth, lead) == want, (want, depth[depth != U.UNKNOWN])
        if (depth != U.UNKNOWN).sum() == 1:
            assert want[0] == want[1] > 0
    # two calls on one context, the second range strictly inside the first: a result buffer that is not re-initialised would show
    wide_range, narrow_range = image((first, near), (last, far)), image(((1, 1), np.uint16(5000)), ((3, 200), np.uint16(6000)))
    assert gpu_min_max(gpu, wide_range) == U.f32_min_max(wide_range)
    got, want = gpu_min_max(gpu, narrow_range), U.f32_min_max(narrow_range)
    assert got == want and want[0] > U.f32_min_max(wide_range)[0] and want[1] < U.f32_min_max(wide_range)[1]
    assert gpu_min_max(gpu, image()) == (np.float32(np.inf), np.float32(0))


def test_argument_checks_reject_without_launching(gpu):
    """What preprocess_abi.inc refuses: a pitch below width * element size, images of different sizes, a camera of another
    size, and for the three stages that read neighbours any image given twice."""
    torch, L, ctx = gpu
    s = stream_ptr(torch)
    h, w = 6, 10
    tensors = []

    def u16(hh=h, ww=w):
        t = torch.full((hh, ww), 0x1111, dtype=torch.int16, device="cuda")
        tensors.append(t)
        return abi.Buffer2D(t.data_ptr(), hh, ww, ww * 2)

    def bytes_image(hh, ww, per_pixel):
        t = torch.full((hh, ww * per_pixel), 0x11, dtype=torch.uint8, device="cuda")
        tensors.append(t)
        return abi.Buffer2D(t.data_ptr(), hh, ww, ww * per_pixel)

    def short_pitch(b, elem):
        return abi.Buffer2D(b.address, b.height, b.width, b.width * elem - 1)

    camera = U.build_camera(h, w)
    cf = torch.zeros((2, 3), dtype=torch.float32, device="cuda")
    dp = U.depth_params(abi.Buffer2D(cf.data_ptr(), 2, 3, 12), 4)
    mn, mx = C.c_float(7), C.c_float(7)
    ref = C.byref

    def bilateral(a, b):
        return L.bslam_bilateral_filter_and_depth_cutoff(ctx.handle, s, 3.0, 0.005, 2.0, 15000, U.RAW_TO_FLOAT, ref(a), ref(b))

    def normals(a, b, c, cam=camera):
        return L.bslam_compute_normals(ctx.handle, s, ref(cam), ref(dp), ref(a), ref(b), ref(c))

    def radii(a, b, c):
        return L.bslam_compute_point_radii_and_remove_isolated_pixels(ctx.handle, s, ref(camera), U.RAW_TO_FLOAT, ref(a), ref(b), ref(c))

    def min_max(a):
        return L.bslam_compute_min_max_depth(ctx.handle, s, ref(a), U.RAW_TO_FLOAT, ref(mn), ref(mx))

    def brightness(a, b):
        return L.bslam_compute_brightness(ctx.handle, s, ref(a), ref(b))

    a, b, c, other = u16(), u16(), u16(), u16(h, w + 1)
    rgb, color = bytes_image(h, w, 3), bytes_image(h, w, 4)
    refused = [
        bilateral(short_pitch(a, 2), b), bilateral(a, short_pitch(b, 2)), bilateral(a, other), bilateral(other, b), bilateral(a, a),
        normals(short_pitch(a, 2), b, c), normals(a, short_pitch(b, 2), c), normals(a, b, short_pitch(c, 2)), normals(a, other, c), normals(a, b, other),
        normals(a, a, c), normals(a, b, a), normals(a, b, b), normals(a, b, c, U.build_camera(h, w + 1)),
        radii(short_pitch(a, 2), b, c), radii(a, short_pitch(b, 2), c), radii(a, b, short_pitch(c, 2)), radii(a, other, c), radii(a, b, other),
        radii(a, b, a), radii(a, a, c), radii(a, b, b),
        min_max(short_pitch(a, 2)),
        brightness(short_pitch(rgb, 3), color), brightness(rgb, short_pitch(color, 4)), brightness(rgb, bytes_image(h, w + 1, 4)),
        brightness(bytes_image(h + 1, w, 3), color),
    ]
    assert all(rc == INVALID_ARGUMENT for rc in refused), refused
    assert L.bslam_last_error()
    torch.cuda.synchronize()
    assert mn.value == 7 and mx.value == 7
    for t in tensors:                                                       # nothing ran: every buffer still holds its fill
        assert bool((t == (0x11 if t.dtype == torch.uint8 else 0x1111)).all())
    assert normals(a, b, c) == 0 and radii(a, b, c) == 0                    # and the same buffers, used properly, are accepted
    torch.cuda.synchronize()
