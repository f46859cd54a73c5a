"""-m gpu: the luma quad table as fp16 differences (C-ABI probe bslam_debug_quad_samples).

(a) The table the production kernels build -- build_quads_kernel for keyframe colour, build_quads_u8_batched_kernel
    for the odometry's u8 images (one image and several) -- equals the numpy table (tests/quad_table.py) bit for bit at every
    (i, j) in [-1, w - 1] x [-1, h - 1], clamp rows and columns included.
(b) A sample through the table (one 8-byte gather, conversions only) and a sample from four byte loads with the differences
    formed per sample in integers give the same bits in val, gx, gy, in both texture modes.  No tolerance: every operand of
    every fma is the same number on both sides.

Images of 9 x 7 and 8 x 6: odd and even width, so the 8-byte row pitch (w + 1) is and is not a multiple of 16 bytes; two images
per call, so the per-image stride of the table is in use."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from tests import quad_table as Q

pytestmark = pytest.mark.gpu
P = C.POINTER
TEX_FIXED, TEX_EXACT = 0, 1
SIZES = [(9, 7), (8, 6)]


def images(w, h, count, seed):
    """count (h, w) u8 luma images: random bytes plus a block of 0 / 255 checkerboard (differences of +-255, mixed +-510)."""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, size=(count, h, w), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    board = (255 * ((yy + xx) & 1)).astype(np.uint8)
    out[0, 1:5, 2:7] = board[1:5, 2:7]
    out[-1, :4, :4] = board[:4, :4]      # reaches the top-left clamp row and column
    out[-1, h - 3:, w - 3:] = 255 - board[h - 3:, w - 3:]
    return out


def positions(w, h, count, seed):
    """[image, x, y] in pixel-corner coordinates, about 2000: a grid whose fractions lie on and between multiples of 1 / 256, the
    half-pixel border strip on all four sides, the four corners, and positions up to one pixel outside the image."""
    rng = np.random.default_rng(seed)
    pts = []
    # grid: texel centres (x - 0.5 integral) plus k / 256 and (k + 0.5) / 256 and odd offsets in between
    fr = np.array([0.0, 1 / 256, 0.5 / 256, 37 / 256, 37.25 / 256, 128 / 256, 200.75 / 256, 255 / 256, 255.5 / 256, 1 - 2.0 ** -20])
    xs = (np.arange(0, w - 1)[:, None] + 0.5 + fr[None, :]).ravel()
    ys = (np.arange(0, h - 1)[:, None] + 0.5 + fr[None, ::3]).ravel()
    gx, gy = np.meshgrid(xs[::3], ys, indexing="ij")
    pts.append(np.stack([gx.ravel(), gy.ravel()], 1))
    # border strip and outside: x (or y) in [-1, 0.5] and [w - 0.5, w + 1], the other coordinate anywhere
    edge = np.array([-1.0, -0.5, -1 / 256, 0.0, 1 / 512, 0.25, 0.5 - 2.0 ** -20, 0.5])
    along_x = rng.uniform(-1, w + 1, 24)
    along_y = rng.uniform(-1, h + 1, 24)
    for e in edge:
        pts.append(np.stack([np.full(24, e), along_y], 1))
        pts.append(np.stack([np.full(24, w - e), along_y], 1))
        pts.append(np.stack([along_x, np.full(24, e)], 1))
        pts.append(np.stack([along_x, np.full(24, h - e)], 1))
    # the four corners: every combination of the edge offsets
    ex, ey = np.meshgrid(edge, edge, indexing="ij")
    for cx, sx in ((0.0, 1), (float(w), -1)):
        for cy, sy in ((0.0, 1), (float(h), -1)):
            pts.append(np.stack([cx + sx * ex.ravel(), cy + sy * ey.ravel()], 1))
    pts.append(np.stack([rng.uniform(-1, w + 1, 512), rng.uniform(-1, h + 1, 512)], 1))
    xy = np.concatenate(pts).astype(np.float32)
    img = (np.arange(len(xy)) % count).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([img[:, None], xy], 1))


def probe(luma, channels, pos, tex_mode):
    count, h, w = luma.shape
    if channels == 4:
        rng = np.random.default_rng(99)
        img = rng.integers(0, 256, size=(count, h, w, 4), dtype=np.uint8)   # r, g, b are noise the table must not read
        img[..., 3] = luma
    else:
        img = luma
    img = np.ascontiguousarray(img)
    out = np.full((len(pos), 6), np.nan, np.float32)
    entries = np.full((count, h + 1, w + 1, 4), 0xffff, np.uint16)
    ctx = badslam_amd.Context(0)
    badslam_amd.check(badslam_amd.lib().bslam_debug_quad_samples(
        ctx.handle, None, count, w, h, channels, img.ctypes.data_as(P(C.c_uint8)), len(pos), pos.ctypes.data_as(P(C.c_float)), tex_mode,
        out.ctypes.data_as(P(C.c_float)), entries.ctypes.data_as(P(C.c_uint16))))
    return out, entries


# (channels, images per call): keyframe colour, one u8 image (single-pair odometry), two u8 images (batched odometry)
BUILDERS = [(4, 2), (1, 1), (1, 2)]


@pytest.fixture(scope="module")
def runs():
    res = {}
    for (w, h) in SIZES:
        for channels, count in BUILDERS:
            luma = images(w, h, count, seed=100 * w + channels)
            pos = positions(w, h, count, seed=7 * w + count)
            for mode in (TEX_FIXED, TEX_EXACT):
                res[(w, h, channels, count, mode)] = (luma, pos) + probe(luma, channels, pos, mode)
    return res


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("builder", BUILDERS)
def test_entries_equal_the_numpy_table(runs, size, builder):
    for mode in (TEX_FIXED, TEX_EXACT):
        luma, _, _, entries = runs[size + builder + (mode,)]
        want = np.stack([Q.table(im) for im in luma]).view(np.uint16)
        assert entries.shape == want.shape
        assert np.array_equal(entries, want)
    assert np.abs(want.view(np.float16)[..., 3].astype(np.int32)).max() == 510   # the checkerboard's mixed difference is in the table


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("mode", [TEX_FIXED, TEX_EXACT])
def test_table_samples_equal_byte_samples_bit_for_bit(runs, size, builder, mode):
    _, pos, out, _ = runs[size + builder + (mode,)]
    assert len(pos) >= 1900
    assert np.isfinite(out).all()
    table_path, byte_path = out[:, :3].view(np.uint32), out[:, 3:].view(np.uint32)
    bad = np.nonzero((table_path != byte_path).any(axis=1))[0]
    assert bad.size == 0, (pos[bad[:5]], out[bad[:5]])
    # the samples are not trivially equal: values span the byte range and gradients both signs
    assert out[:, 0].min() < 16 and out[:, 0].max() > 240 and out[:, 1].min() < -100 and out[:, 2].max() > 100


def test_values_are_the_bilinear_interpolation_of_the_bytes(runs):
    """Anchors both paths (they share their filters): against float64 bilinear interpolation with the mode's weights."""
    for (w, h, channels, count, mode), (luma, pos, out, _) in runs.items():
        k = pos[:, 0].astype(int)
        # footprint and weights in fp32, operation by operation as tex_footprint / tex_weights form them
        xb, yb = pos[:, 1] - np.float32(0.5), pos[:, 2] - np.float32(0.5)
        fx, fy = np.floor(xb), np.floor(yb)
        a, b = xb - fx, yb - fy
        assert a.dtype == np.float32
        if mode == TEX_FIXED:
            a = np.floor(a * np.float32(256) + np.float32(0.5)) * np.float32(1 / 256)
            b = np.floor(b * np.float32(256) + np.float32(0.5)) * np.float32(1 / 256)
        a, b = a.astype(np.float64), b.astype(np.float64)
        i, j = np.clip(fx, -1, w - 1).astype(int), np.clip(fy, -1, h - 1).astype(int)
        t = lambda y, x: luma[k, np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.float64)
        top = t(j, i) + a * (t(j, i + 1) - t(j, i))
        bot = t(j + 1, i) + a * (t(j + 1, i + 1) - t(j + 1, i))
        want = top + b * (bot - top)
        # fixed point: exact (device_math.hpp: bilinear_diffs_fixed).  Exact float (bilinear_bytes): top, bot and the result round at
        # magnitude < 256 (half an ulp: 2^-17 each; top's and bot's errors enter with weights 1 - b and b), bot - top at < 512
        # (2^-16, times b <= 1): 2^-17 + 2^-16 + 2^-17 = 2^-15
        tol = 0.0 if mode == TEX_FIXED else 2.0 ** -15
        assert np.abs(out[:, 0] - want).max() <= tol, (w, h, channels, count, mode)
