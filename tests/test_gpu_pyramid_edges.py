"""-m gpu: the tracking-pyramid entry points, which share Img and image_grid with the preprocessing producers, against the
oracle (oracle/bso_odometry.c) bit for bit at odd shapes, on pitched rows with a base off the allocator's alignment, with
cell sizes that do not divide the width and in both texture modes; and against NumPy fp32 restatements of the three whose
arithmetic is plain unfused fp32 (tests/preprocess_util.py): the two 255 * (v / 255) truncations, the Sobel magnitude and
the 2 x 2 "closest to the block mean" selection.

255 * (v * fl(1 / 255)) truncated gives v back for every byte 0 ... 255: no value comes out as v - 1
(test_brightness_from_color_and_read_mode_normalized asserts it on all 256)."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi
from tests import bso
from tests import preprocess_util as U
from tests.test_gpu_preprocess import stream_ptr

pytestmark = pytest.mark.gpu
f32 = np.float32
SHAPES = [(37, 67), (5, 257)]
TEX_MODES = [abi.TEX_FIXED_POINT_1_8, abi.TEX_EXACT_FLOAT]
ref = C.byref


@pytest.fixture(scope="module")
def gpu():
    import torch
    return torch, badslam_amd.lib(), badslam_amd.Context(0)


def host(array):
    array = np.ascontiguousarray(array)
    return array, bso.np_buffer2d(array)


def equal(got, want):
    """same shape, same bits"""
    return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


@pytest.fixture(scope="module")
def frames(oracle):
    """Per shape: the keyframe images the oracle's producers make of the builder's input (depth, normals, colour)."""
    made = {}
    for h, w in SHAPES:
        camera = U.build_camera(h, w)
        filtered = U.oracle_bilateral(U.shaped_raw_depth(h, w), *U.BILATERAL_SETS["default"])
        stage1, normals = U.oracle_normals(filtered, camera, U.build_cfactor(h, w, 4), 4)
        _, depth = U.oracle_radii(stage1, camera)
        color = U.oracle_brightness(U.build_rgb(h, w))
        for image in (depth, normals, color):
            image.setflags(write=False)
        made[(h, w)] = (depth, normals, color)
    return made


def oracle_calibrated(depth, cell):
    h, w = depth.shape
    out, ob = host(np.zeros((h, w), f32))
    cfactor, cb = host(U.build_cfactor(h, w, cell))
    dp = U.depth_params(cb, cell)
    _, db = host(depth)
    bso.lib().bso_calibrate_depth(ref(dp), ref(db), ref(ob))
    return out


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_brightness_from_color_and_read_mode_normalized(oracle, gpu, frames, shape, lead):
    torch, L, ctx = gpu
    h, w = shape
    color = np.array(frames[shape][2])
    color[0, :, 3] = np.arange(w) % 256                                    # every byte value occurs (at 257 wide: all of them in one row)
    color[-1, :, 3] = 255 - np.arange(w) % 256
    luma = np.ascontiguousarray(color[..., 3])
    want, wb = host(np.zeros((h, w), np.uint8))
    _, cb = host(color)
    oracle.bso_brightness_from_color(ref(cb), ref(wb))
    assert equal(want, U.np_read_mode_normalized(luma)) and equal(want, luma)
    im = U.Images(torch, lead)
    a, b = im.input(color), im.output(h, w, np.uint8)
    badslam_amd.check(L.bslam_compute_brightness_from_color(ctx.handle, stream_ptr(torch), ref(a), ref(b)))
    assert equal(im.fetch()[0], want)

    want2, wb2 = host(np.zeros((h, w), np.uint8))
    _, lb = host(luma)
    oracle.bso_set_to_read_mode_normalized(ref(lb), ref(wb2))
    assert equal(want2, U.np_read_mode_normalized(luma))
    im = U.Images(torch, lead)
    a, b = im.input(luma), im.output(h, w, np.uint8)
    badslam_amd.check(L.bslam_set_to_read_mode_normalized(ctx.handle, stream_ptr(torch), ref(a), ref(b)))
    assert equal(im.fetch()[0], want2)
    every_byte = np.arange(256, dtype=np.uint8)
    assert np.array_equal(U.np_read_mode_normalized(every_byte), every_byte)     # no byte comes back as v - 1


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_sobel_gradient_magnitude(oracle, gpu, frames, shape, lead):
    torch, L, ctx = gpu
    h, w = shape
    color = np.array(frames[shape][2])
    color[h // 2:, w // 3:w // 2, 3] = 255                                  # a hard edge: magnitudes up to the top of the range
    color[h // 2:, w // 2:2 * w // 3, 3] = 0
    want, wb = host(np.zeros((h, w), np.uint8))
    _, cb = host(color)
    oracle.bso_compute_sobel_gradient_magnitude(ref(cb), ref(wb))
    assert equal(want, U.np_sobel_gradient_magnitude(np.ascontiguousarray(color[..., 3])))
    assert want.max() >= 180 and (want > 0).mean() > 0.5 and len(np.unique(want)) > 40
    im = U.Images(torch, lead)
    a, b = im.input(color), im.output(h, w, np.uint8)
    badslam_amd.check(L.bslam_compute_sobel_gradient_magnitude(ctx.handle, stream_ptr(torch), ref(a), ref(b)))
    assert equal(im.fetch()[0], want)


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("cell", [3, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_calibrate_depth(oracle, gpu, frames, shape, cell, lead):
    torch, L, ctx = gpu
    h, w = shape
    depth = frames[shape][0]
    want = oracle_calibrated(depth, cell)
    assert (want > 0).sum() > 50 and (want == 0).sum() > 50 and w % cell
    im = U.Images(torch, lead)
    dp = U.depth_params(im.input(U.build_cfactor(h, w, cell), pad=2, fill=f32(1e9)), cell)
    a, b = im.input(depth), im.output(h, w, f32)
    badslam_amd.check(L.bslam_calibrate_depth(ctx.handle, stream_ptr(torch), ref(dp), ref(a), ref(b)))
    assert equal(im.fetch()[0], want)


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("tex_mode", TEX_MODES)
@pytest.mark.parametrize("cell", [3, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_calibrate_depth_and_transform_color_to_depth(oracle, gpu, frames, shape, cell, tex_mode, lead):
    """A colour camera with a smaller image and a shifted principal point: part of the depth image projects outside the colour
    image, where the depth is forced to 0 (BS/kernel_downsample.cu:236-266)."""
    torch, L, ctx = gpu
    h, w = shape
    depth = frames[shape][0]
    depth_camera = U.build_camera(h, w)
    ch, cw = max(4, int(0.7 * h)), int(0.7 * w)
    color_camera = bso.make_camera(52.0, 50.0, 18.0, 14.5, cw, ch)
    luma = np.random.default_rng(h * w).integers(0, 256, (ch, cw), dtype=np.uint8)
    cfactor, cb = host(U.build_cfactor(h, w, cell))
    dp = U.depth_params(cb, cell)
    want_depth, wdb = host(np.zeros((h, w), f32))
    want_color, wcb = host(np.zeros((h, w), np.uint8))
    _, db = host(depth)
    _, lb = host(luma)
    oracle.bso_calibrate_depth_and_transform_color_to_depth(ref(depth_camera), ref(color_camera), ref(dp), ref(db), ref(lb), tex_mode, ref(wdb), ref(wcb))
    plain = oracle_calibrated(depth, cell)
    forced = (plain > 0) & (want_depth == 0)
    share = forced.sum() / (plain > 0).sum()
    assert 0.1 < share < 0.9, share
    assert equal(want_depth[~forced], plain[~forced])
    ctx.set_texture_mode(tex_mode)
    im = U.Images(torch, lead)
    dp_dev = U.depth_params(im.input(cfactor, pad=2, fill=f32(1e9)), cell)
    a, b, c, d = im.input(depth), im.input(luma), im.output(h, w, f32), im.output(h, w, np.uint8)
    badslam_amd.check(L.bslam_calibrate_depth_and_transform_color_to_depth(ctx.handle, stream_ptr(torch), ref(color_camera), ref(depth_camera), ref(dp_dev),
                                                                          ref(a), ref(b), ref(c), ref(d)))
    got_depth, got_color = im.fetch()
    assert equal(got_depth, want_depth) and equal(got_color, want_color)
    assert len(np.unique(want_color)) > 30


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("tex_mode", TEX_MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_downsample_images_down_the_pyramid(oracle, gpu, frames, shape, tex_mode, lead):
    """37 x 67 -> 18 x 33 -> 9 x 16 and 5 x 257 -> 2 x 128: odd sizes drop the last row and column.  Against the oracle and
    against the NumPy restatement; the normals where the level has depth, their pre-filled value where it has none."""
    torch, L, ctx = gpu
    depth16, normals, color = frames[shape]
    depth = oracle_calibrated(depth16, 4)
    luma = np.ascontiguousarray(color[..., 3])
    ctx.set_texture_mode(tex_mode)
    levels = 2 if shape == (37, 67) else 1
    for level in range(levels):
        oh, ow = depth.shape[0] // 2, depth.shape[1] // 2
        assert (oh, ow) == [(18, 33), (9, 16), (2, 128)][level if shape == (37, 67) else 2]
        prefill = np.random.default_rng(level).integers(0, 65536, (oh, ow)).astype(np.uint16)
        want_depth, wdb = host(np.zeros((oh, ow), f32))
        want_normals, wnb = host(prefill.copy())
        want_color, wcb = host(np.zeros((oh, ow), np.uint8))
        _, db = host(depth)
        _, nb = host(normals)
        _, lb = host(luma)
        oracle.bso_downsample_images(ref(db), ref(nb), ref(lb), tex_mode, ref(wdb), ref(wnb), ref(wcb))
        np_depth, np_normals, np_color = U.np_downsample(depth, normals, luma, 0)
        has_depth = want_depth > 0
        assert equal(want_depth, np_depth) and equal(want_color, np_color) and np.array_equal(want_normals[has_depth], np_normals[has_depth])
        assert np.array_equal(want_normals[~has_depth], prefill[~has_depth]) and has_depth.sum() >= 10 and (~has_depth).sum() >= 10
        im = U.Images(torch, lead)
        bufs = [im.input(depth), im.input(normals), im.input(luma), im.output(oh, ow, f32), im.output(oh, ow, np.uint16, prefill), im.output(oh, ow, np.uint8)]
        badslam_amd.check(L.bslam_downsample_images(ctx.handle, stream_ptr(torch), *[ref(b) for b in bufs]))
        got_depth, got_normals, got_color = im.fetch()
        assert equal(got_depth, want_depth) and equal(got_color, want_color)
        assert np.array_equal(got_normals[has_depth], want_normals[has_depth]) and np.array_equal(got_normals[~has_depth], prefill[~has_depth])
        depth, normals, luma = want_depth, want_normals, want_color


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("tex_mode", TEX_MODES)
@pytest.mark.parametrize("downsample_color", [1, 0])
@pytest.mark.parametrize("cell", [3, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_calibrate_and_downsample_images(oracle, gpu, frames, shape, cell, downsample_color, tex_mode, lead):
    torch, L, ctx = gpu
    h, w = shape
    depth16, normals, color = frames[shape]
    oh, ow = h // 2, w // 2
    luma = np.ascontiguousarray(color[..., 3] if downsample_color else color[:oh, :ow, 3])
    cfactor, cb = host(U.build_cfactor(h, w, cell))
    dp = U.depth_params(cb, cell)
    prefill = np.random.default_rng(cell).integers(0, 65536, (oh, ow)).astype(np.uint16)
    want_depth, wdb = host(np.zeros((oh, ow), f32))
    want_normals, wnb = host(prefill.copy())
    want_color, wcb = host(np.zeros((oh, ow), np.uint8))
    _, db = host(depth16)
    _, nb = host(normals)
    _, lb = host(luma)
    oracle.bso_calibrate_and_downsample_images(downsample_color, ref(dp), ref(db), ref(nb), ref(lb), tex_mode, ref(wdb), ref(wnb), ref(wcb))
    has_depth = want_depth > 0
    assert has_depth.sum() >= 10 and (~has_depth).sum() >= 10 and np.array_equal(want_normals[~has_depth], prefill[~has_depth])
    if downsample_color:
        assert equal(want_color, U.np_downsample(np.zeros((h, w), f32), normals, luma, 0)[2])
    else:
        assert equal(want_color, luma)
    ctx.set_texture_mode(tex_mode)
    im = U.Images(torch, lead)
    dp_dev = U.depth_params(im.input(cfactor, pad=2, fill=f32(1e9)), cell)
    bufs = [im.input(depth16), im.input(normals), im.input(luma), im.output(oh, ow, f32), im.output(oh, ow, np.uint16, prefill), im.output(oh, ow, np.uint8)]
    badslam_amd.check(L.bslam_calibrate_and_downsample_images(ctx.handle, stream_ptr(torch), downsample_color, ref(dp_dev), *[ref(b) for b in bufs]))
    got_depth, got_normals, got_color = im.fetch()
    assert equal(got_depth, want_depth) and equal(got_color, want_color)
    assert np.array_equal(got_normals[has_depth], want_normals[has_depth]) and np.array_equal(got_normals[~has_depth], prefill[~has_depth])
