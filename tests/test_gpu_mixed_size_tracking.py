"""-m gpu: colour and depth cameras of different sizes in the pairwise tracker (a colour pyramid level other than the depth
one).  bslam_downsample_images with a colour image of its own size against a NumPy restatement of the kernel's rule, and
TrackFramePairwise / TrackFramesPairwiseBatched on keyframes with a half-size colour image."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi
from badslam_amd import direct_ba as dba
from tests import bso
from tests.preprocess_util import np_downsample
from tests.test_gpu_bad_slam_input_conditioning import render_sequence
from tests.test_gpu_input_conditioning import np_downscale_rgb
from tests.test_gpu_preprocess import stream_ptr

pytestmark = pytest.mark.gpu
f32 = np.float32


def padded(torch, array, pad, fill):
    """(storage with `pad` extra columns holding `fill`, Buffer2D of the image part)."""
    t = torch.from_numpy(np.ascontiguousarray(array))
    storage = torch.empty((array.shape[0], array.shape[1] + pad), dtype=t.dtype, device="cuda")
    storage.copy_(torch.from_numpy(np.full(storage.shape, fill, array.dtype)))
    storage[:, :array.shape[1]] = t.cuda()
    return storage, abi.Buffer2D(storage.data_ptr(), array.shape[0], array.shape[1], storage.stride(0) * storage.element_size())


@pytest.mark.parametrize("color_shape", [(96, 128), (60, 84), (240, 320)])
def test_downsample_images_with_a_colour_image_of_its_own_size(color_shape):
    """Depth and normals 96 x 128 -> 48 x 64; colour of the same size, smaller and larger -> half its own size.  Every output
    bit-exact, pitched rows, output padding untouched."""
    import torch
    L = badslam_amd.lib()
    ctx = badslam_amd.Context(0)
    rng = np.random.default_rng(sum(color_shape))
    depth = rng.uniform(0.5, 3.0, (96, 128)).astype(f32)
    depth[rng.random(depth.shape) < 0.3] = 0
    depth[10:14, 20:28] = 0                                       # blocks without a valid depth
    depth[40:42, 60:62] = f32(1.25)                               # a block of equal depths: the first one wins
    normals = rng.integers(0, 65536, depth.shape).astype(np.uint16)
    color = rng.integers(0, 256, color_shape).astype(np.uint8)
    FILL_N, FILL_C = 0x5A5A, 0x5A
    want_d, want_n, want_c = np_downsample(depth, normals, color, FILL_N)
    keep = [padded(torch, depth, 3, f32(-1)), padded(torch, normals.view(np.int16), 5, np.int16(0x3333)), padded(torch, color, 7, np.uint8(0x33)),
            padded(torch, np.full((48, 64), -7, f32), 2, f32(-7)), padded(torch, np.full((48, 64), FILL_N, np.int16), 3, np.int16(FILL_N)),
            padded(torch, np.full((color_shape[0] // 2, color_shape[1] // 2), FILL_C, np.uint8), 9, np.uint8(FILL_C))]
    bufs = [C.byref(b) for _, b in keep]
    badslam_amd.check(L.bslam_downsample_images(ctx.handle, stream_ptr(torch), *bufs))
    torch.cuda.synchronize()
    got_d, got_n, got_c = (keep[i][0].cpu().numpy() for i in (3, 4, 5))
    assert np.array_equal(got_d[:, :64].view(np.uint32), want_d.view(np.uint32))
    assert np.array_equal(got_n[:, :64].view(np.uint16), want_n)
    assert np.array_equal(got_c[:, :color_shape[1] // 2], want_c), int((got_c[:, :color_shape[1] // 2] != want_c).sum())
    assert (got_d[:, 64:] == -7).all() and (got_n[:, 64:].view(np.uint16) == FILL_N).all() and (got_c[:, color_shape[1] // 2:] == FILL_C).all()


def test_downsample_images_refuses_a_colour_level_that_does_not_fit():
    import torch
    L = badslam_amd.lib()
    ctx = badslam_amd.Context(0)
    keep = [padded(torch, np.ones((96, 128), f32), 0, f32(0)), padded(torch, np.zeros((96, 128), np.int16), 0, np.int16(0)),
            padded(torch, np.zeros((60, 84), np.uint8), 0, np.uint8(0)), padded(torch, np.zeros((48, 64), f32), 0, f32(0)),
            padded(torch, np.zeros((48, 64), np.int16), 0, np.int16(0)), padded(torch, np.full((30, 43), 9, np.uint8), 0, np.uint8(9))]
    rc = L.bslam_downsample_images(ctx.handle, stream_ptr(torch), *[C.byref(b) for _, b in keep])
    torch.cuda.synchronize()
    assert rc == -1 and bool((keep[5][0] == 9).all())               # BSLAM_ERR_INVALID_ARGUMENT, nothing launched


def test_trackers_with_a_half_size_colour_camera(oracle):
    """Four rendered 640x480 frames as keyframes with a 320x240 colour image.  TrackFramesPairwiseBatched of keyframes 0 ... 2
    against keyframe 3 is bit-identical to three TrackFramePairwise calls, and each result lies nearer to the rendered
    relative pose than the initial estimate, which is that pose moved by 5 mm and 0.2 degrees."""
    full_cam, raw_to_float, frames, gt = render_sequence(4)
    half_cam = bso.make_camera(262.5, 262.5, 160.0, 120.0, 320, 240)
    ba = dba.DirectBA(400000, raw_to_float, 40.0, 4, 0.8, 1, 1, 1, half_cam, full_cam, 1, True, True)
    for k, ((depth, rgb), T) in enumerate(zip(frames, gt)):
        ba.AddKeyframeFromImages(k, depth, np_downscale_rgb(rgb, 1), T)
    offset = bso.se3_exp(np.array([0.003, -0.003, 0.0027, 0.002, -0.002, 0.002], f32))
    truth = [bso.se3_mul(bso.se3_inverse(gt[3]), gt[k]) for k in range(3)]
    inits = [bso.se3_mul(T, offset) for T in truth]
    batched, batched_its = ba.TrackKeyframesBatched(3, [0, 1, 2], inits, num_scales=4)
    for k in range(3):
        single, its = ba.TrackKeyframePair(k, 3, inits[k], num_scales=4)
        assert np.array_equal(dba.pose7(single).view(np.uint32), dba.pose7(batched[k]).view(np.uint32)) and list(its) == list(batched_its[k])
        distance = lambda T: float(np.abs(bso.se3_log(bso.se3_mul(bso.se3_inverse(T), truth[k]))).max())
        print("pair", k, "initial distance", distance(inits[k]), "tracked distance", distance(single), "iterations", its)
        assert distance(single) < 0.5 * distance(inits[k])
    ba.close()
