"""-m gpu: the input-conditioning kernels of the raw frame (BadSlam::PreprocessFrame, BS/bad_slam.cc:645-685) -- 3x3 depth
median + densify, median downscale of the depth, half-size steps of the rgb image -- against NumPy restatements of
their rules kept in this module.  Every output is an integer image: all comparisons are bit-exact.

The rule for an even number n of collected values, in fp32 as the reference computes it: average = float(sum) / n (the
sum is below 2^24, so exact), then the lower middle value if |low - average| < |high - average|, else the upper one."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi
from tests.test_gpu_preprocess import buf, dev, raw_depth_image, stream_ptr

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT = -1   # BSLAM_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------
# NumPy restatements
# ------------------------------------------------------------------------------------------------
def np_nonzero_median(values):
    """values: (..., N) unsigned -> (median of the non-zero entries by the rule above (garbage where there are none), their count)."""
    v = values.astype(np.int64)
    n = (v != 0).sum(-1)
    ordered = np.sort(np.where(v == 0, 1 << 16, v), axis=-1)          # the non-zero values first, ascending
    low = np.take_along_axis(ordered, (np.maximum(n, 1) - 1)[..., None] // 2, -1)[..., 0]
    high = np.take_along_axis(ordered, np.minimum(n // 2, v.shape[-1] - 1)[..., None], -1)[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        average = v.sum(-1).astype(np.float32) / n.astype(np.float32)
        low_is_nearer = np.abs(low.astype(np.float32) - average) < np.abs(high.astype(np.float32) - average)
    assert average.dtype == np.float32
    return np.where((n % 2 == 1) | low_is_nearer, low, high), n


def np_median_filter_and_densify(depth, iterations=1):
    """MedianFilterAndDensifyDepthMap: windows clipped at the border = zero padding, since zeros are not collected."""
    for _ in range(iterations):
        h, w = depth.shape
        padded = np.zeros((h + 2, w + 2), depth.dtype)
        padded[1:-1, 1:-1] = depth
        windows = np.stack([padded[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], -1)
        median, n = np_nonzero_median(windows)
        depth = np.where(n >= 2, median, depth).astype(np.uint16)
    return depth


def np_window_counts(depth):
    h, w = depth.shape
    padded = np.zeros((h + 2, w + 2), np.int64)
    padded[1:-1, 1:-1] = depth != 0
    return sum(padded[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))


def np_downscale_depth_median(depth, level):
    """DownscaleUsingMedianWhileExcluding(0, ...) for an exact 2^level reduction."""
    s = 1 << level
    h, w = depth.shape[0] // s, depth.shape[1] // s
    blocks = depth.reshape(h, s, w, s).transpose(0, 2, 1, 3).reshape(h, w, s * s)
    median, n = np_nonzero_median(blocks)
    return np.where(n > 0, median, 0).astype(np.uint16)


def np_downscale_rgb(rgb, level):
    """`level` DownscaleToHalfSize steps on an (h, w, 3) u8 image: a/4 + b/4 + c/4 + d/4 with truncated quotients."""
    for _ in range(level):
        q = rgb.astype(np.uint16) // 4
        rgb = (q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2]).astype(np.uint8)
    return rgb


# ------------------------------------------------------------------------------------------------
# GPU side
# ------------------------------------------------------------------------------------------------
def pitched(torch, array, pad_elems, fill):
    """Device copy of a 2-D array in rows of width + pad_elems elements (the padding holds `fill`); returns (storage, Buffer2D)."""
    h, w = array.shape
    storage = torch.full((h, w + pad_elems), fill, dtype=torch.from_numpy(array[:1, :1].copy()).dtype, device="cuda")
    storage[:, :w] = dev(torch, array)
    return storage, abi.Buffer2D(storage.data_ptr(), h, w, storage.stride(0) * storage.element_size())


def gpu_call(fn_name, array_in, out_shape, in_pad=0, out_pad=0, rgb=False):
    """Runs one of the three entry points on a host array; returns (output image, output padding or None).  rgb: (h, w, 3) u8."""
    import torch
    L = badslam_amd.lib()
    ctx = badslam_amd.Context(0)
    flat_in = array_in.reshape(array_in.shape[0], -1) if rgb else array_in.view(np.int16)
    oh, ow = out_shape
    out_cols = ow * 3 if rgb else ow
    fill = 0x5A if rgb else 0x5A5A
    in_store, in_buf = pitched(torch, flat_in, in_pad, 0x33 if rgb else 0x3333)
    out_store, out_buf = pitched(torch, np.full((oh, out_cols), fill, flat_in.dtype), out_pad, fill)
    if rgb:
        in_buf.width, out_buf.width = array_in.shape[1], ow      # 3 bytes per pixel: width counts pixels
    badslam_amd.check(getattr(L, fn_name)(ctx.handle, stream_ptr(torch), C.byref(in_buf), C.byref(out_buf)))
    torch.cuda.synchronize()
    host = out_store.cpu().numpy()
    image = np.ascontiguousarray(host[:, :out_cols])
    padding = host[:, out_cols:] if out_pad else None
    return (image.reshape(oh, ow, 3) if rgb else image.view(np.uint16)), padding


def gpu_median(depth, iterations=1, **kw):
    for _ in range(iterations):
        depth, padding = gpu_call("bslam_median_filter_and_densify_depth", depth, depth.shape, **kw)
    return depth, padding


def gpu_downscale_depth(depth, level, **kw):
    return gpu_call("bslam_downscale_depth_median", depth, (depth.shape[0] >> level, depth.shape[1] >> level), **kw)


def gpu_downscale_rgb(rgb, level, **kw):
    return gpu_call("bslam_downscale_rgb", rgb, (rgb.shape[0] >> level, rgb.shape[1] >> level), rgb=True, **kw)


# ------------------------------------------------------------------------------------------------
# hand-made inputs
# ------------------------------------------------------------------------------------------------
def even_count_values(n, low, gap, spread, bump):
    """n (even) values whose middle pair is (low, low + gap).  bump = 0: the other values lie symmetrically around the pair,
    so the mean is exactly its midpoint (a tie: the upper value wins); bump = +1 / -1 moves one outer value by one, so the
    mean leaves the midpoint by 1 / n towards the upper / lower value (a near-tie)."""
    high = low + gap
    offsets = [1 + (spread * (i + 1)) // (n // 2) for i in range(n // 2 - 1)]
    values = [low - o for o in offsets] + [low, high] + [high + o for o in reversed(offsets)]
    if bump and n > 2:
        values[-1 if bump > 0 else 0] += bump
    assert len(values) == n and min(values) > 0 and max(values) <= 65535 and sorted(values)[n // 2 - 1:n // 2 + 1] == [low, high]
    return values


def even_count_cases(counts):
    """(values, expected result) for ties and near-ties of every count, at small values and just below 65535."""
    cases = []
    for n in counts:
        for low, gap, spread in ((1000, 6, 40), (65535 - 9 - 6, 6, 9), (40000, 1, 7), (300, 2, 200)):
            for bump in (0, 1, -1):
                if n == 2 and bump:
                    continue                    # two values are always equally far from their mean
                values = even_count_values(n, low, gap, spread, bump)
                cases.append((values, low if bump < 0 else low + gap))
    return cases


def handmade_median_image():
    """3x3 patches in a field of zeros, 5 pixels apart, so that the window of a patch centre is the patch: every count
    0 ... 9, ties and near-ties for the even counts, an isolated pixel, holes with one and with two neighbours; plus
    values on the border and in the corners.  Returns (image, [(y, x, expected value)])."""
    rng = np.random.default_rng(11)
    patches = []                                                        # (nine values row-major, expected centre or None)
    for count in range(10):                                             # counts 0 ... 9, centre present when count > 4
        cells = np.zeros(9, np.int64)
        where = rng.permutation([0, 1, 2, 3, 5, 6, 7, 8])[:count - (count > 4)]
        cells[where] = rng.integers(500, 60000, len(where))
        if count > 4:
            cells[4] = rng.integers(500, 60000)
        patches.append((cells, None))
    for values, expected in even_count_cases((2, 4, 6, 8)):
        for centre_present in (False, True):
            cells = np.zeros(9, np.int64)
            ring = list(rng.permutation([0, 1, 2, 3, 5, 6, 7, 8]))
            order = ([4] + ring) if centre_present else ring
            cells[order[:len(values)]] = rng.permutation(values)
            patches.append((cells, expected))
    patches.append((np.array([0, 0, 0, 0, 1234, 0, 0, 0, 0]), 1234))      # an isolated pixel is kept
    patches.append((np.array([0, 0, 777, 0, 0, 0, 0, 0, 0]), 0))          # a hole with one neighbour stays a hole
    patches.append((np.array([0, 0, 700, 0, 0, 0, 800, 0, 0]), 800))      # a hole with two is filled (a tie: the upper one)
    per_row = 12
    rows = (len(patches) + per_row - 1) // per_row
    image = np.zeros((5 * rows + 5, 5 * per_row + 3), np.uint16)          # 63 wide: not a multiple of 4, odd row pitch in u16
    expected = []
    for i, (cells, want) in enumerate(patches):
        y, x = 3 + 5 * (i // per_row), 3 + 5 * (i % per_row)
        image[y - 1:y + 2, x - 1:x + 2] = cells.reshape(3, 3)
        if want is not None:
            expected.append((y, x, want))
    image[0, 0], image[0, 1], image[1, 0] = 5000, 5010, 5030                                  # corners: windows of 4 pixels
    image[-1, -1], image[-2, -1] = 65535, 65533
    image[0, 30:34] = [9000, 0, 9100, 9050]                                                   # top border: windows of 6 pixels
    image[20:24, 0] = [100, 0, 65535, 7]                                                      # left border
    image[-1, 10:13] = [31000, 31001, 31003]                                                  # bottom border
    image[8:11, -1] = [2, 1, 3]                                                               # right border
    return image, expected


def handmade_downscale_image():
    """48 x 32 for level 2 (4 x 4 blocks): all-zero blocks, one-value blocks and every even count 2 ... 14 as tie and
    near-tie; the rest random with random holes.  Returns (image, [(block y, block x, expected value)])."""
    rng = np.random.default_rng(12)
    image = rng.integers(1, 65536, (32, 48)).astype(np.uint16)
    image[rng.random(image.shape) < 0.35] = 0
    blocks = [([], 0), ([4321], 4321), ([65535], 65535)] + even_count_cases((2, 4, 6, 8, 10, 12, 14))
    assert len(blocks) <= 8 * 12
    expected = []
    for i, (values, want) in enumerate(blocks):
        cells = np.zeros(16, np.int64)
        cells[rng.permutation(16)[:len(values)]] = values
        by, bx = i // 12, i % 12
        image[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = cells.reshape(4, 4)
        expected.append((by, bx, want))
    return image, expected


# ------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------
def test_the_restated_even_count_rule_on_known_answers():
    """The NumPy checker itself: ties take the upper value, near-ties the nearer one, also where sum / 6 is inexact."""
    for values, expected in even_count_cases((2, 4, 6, 8, 10, 12, 14)):
        padded = np.array([values + [0] * (16 - len(values))])
        median, n = np_nonzero_median(padded)
        assert n[0] == len(values) and median[0] == expected, (values, int(median[0]), expected)
    assert np_nonzero_median(np.array([[0, 5, 0, 9, 7]]))[0][0] == 7
    assert np_downscale_rgb(np.full((2, 2, 3), 255, np.uint8), 1)[0, 0, 0] == 252


@pytest.mark.parametrize("iterations", [1, 3])
def test_median_on_a_raw_depth_image(oracle, iterations):
    _, raw = raw_depth_image()
    want = np_median_filter_and_densify(raw, iterations)
    got, _ = gpu_median(raw, iterations)
    assert np.array_equal(got, want), int((got != want).sum())
    assert (want != raw).sum() > 0.5 * raw.size and (want == 0).sum() < (raw == 0).sum()     # it filters, and it fills holes


def test_median_on_a_handmade_image():
    image, expected = handmade_median_image()
    counts = np_window_counts(image)
    assert set(range(10)) <= set(np.unique(counts).tolist())
    want = np_median_filter_and_densify(image)
    for y, x, value in expected:
        assert want[y, x] == value, (y, x, int(want[y, x]), value)
    for n in (2, 4, 6, 8):
        assert sum(1 for y, x, _ in expected if counts[y, x] == n) >= 3
    got, _ = gpu_median(image)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]


@pytest.mark.parametrize("level", [1, 2, 3])
def test_depth_downscale_on_a_raw_depth_image(oracle, level):
    _, raw = raw_depth_image()
    want = np_downscale_depth_median(raw, level)
    got, _ = gpu_downscale_depth(raw, level)
    assert got.shape == (480 >> level, 640 >> level)
    assert np.array_equal(got, want), int((got != want).sum())
    assert (want == 0).any() and (want == 40000).any()


@pytest.mark.parametrize("level", [1, 2, 3])
def test_depth_downscale_on_a_handmade_image(level):
    image, expected = handmade_downscale_image()
    want = np_downscale_depth_median(image, level)
    if level == 2:
        for by, bx, value in expected:
            assert want[by, bx] == value, (by, bx, int(want[by, bx]), value)
        counts = (image.reshape(8, 4, 12, 4).transpose(0, 2, 1, 3).reshape(8, 12, 16) != 0).sum(-1)
        assert {0, 1, 2, 4, 6, 8, 10, 12, 14} <= set(np.unique(counts).tolist())
    got, _ = gpu_downscale_depth(image, level)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]


@pytest.mark.parametrize("level", [1, 2, 3])
def test_rgb_downscale_on_random_bytes(level):
    rgb = np.random.default_rng(20 + level).integers(0, 256, (480, 640, 3), dtype=np.uint8)
    want = np_downscale_rgb(rgb, level)
    got, _ = gpu_downscale_rgb(rgb, level)
    assert np.array_equal(got, want), int((got != want).sum())
    box = rgb.reshape(480 >> level, 1 << level, 640 >> level, 1 << level, 3).mean((1, 3))
    assert (want != np.floor(box + 0.5)).any()                              # not a rounded box mean


@pytest.mark.parametrize("level", [1, 2, 3])
def test_rgb_downscale_truncates_each_quotient(level):
    h, w = 48, 64
    checker = np.zeros((h, w, 3), np.uint8)
    checker[(np.add.outer(np.arange(h), np.arange(w)) % 2) == 0] = 255
    for image, value in ((np.full((h, w, 3), 255, np.uint8), 252), (np.full((h, w, 3), 3, np.uint8), 0), (checker, (126, 124, 124)[level - 1])):
        want = np_downscale_rgb(image, level)
        assert (want == value).all(), (int(want[0, 0, 0]), value)
        got, _ = gpu_downscale_rgb(image, level)
        assert np.array_equal(got, want)


def test_argument_checks_reject_without_launching():
    import torch
    L = badslam_amd.lib()
    ctx = badslam_amd.Context(0)
    s = stream_ptr(torch)

    def depth(h, w):
        t = torch.full((h, w), 0x1111, dtype=torch.int16, device="cuda")
        return t, buf(t)

    def rgb(h, w):
        t = torch.full((h, w * 3), 0x11, dtype=torch.uint8, device="cuda")
        return t, abi.Buffer2D(t.data_ptr(), h, w, w * 3)

    tensors = []

    def rejected(fn, a, b):
        rc = fn(ctx.handle, s, C.byref(a) if a is not None else None, C.byref(b) if b is not None else None)
        assert rc == INVALID_ARGUMENT, rc
        assert L.bslam_last_error()

    for fn, make in ((L.bslam_median_filter_and_densify_depth, depth), (L.bslam_downscale_depth_median, depth), (L.bslam_downscale_rgb, rgb)):
        downscale = fn is not L.bslam_median_filter_and_densify_depth
        t_in, b_in = make(64, 96)
        t_out, b_out = make(32, 48) if downscale else make(64, 96)
        tensors += [t_in, t_out]
        rejected(fn, b_in, b_in)                                             # the same buffer as input and output
        rejected(fn, None, b_out)                                            # null buffers
        rejected(fn, b_in, None)
        null_address = abi.Buffer2D(None, b_in.height, b_in.width, b_in.pitch)
        rejected(fn, null_address, b_out)
        rejected(fn, b_in, abi.Buffer2D(None, b_out.height, b_out.width, b_out.pitch))
        odd_shapes = [(63, 96), (64, 95)] if not downscale else [(32, 47), (31, 48), (32, 96), (64, 48), (21, 32)]
        if downscale:
            odd_shapes += [(64, 96), (4, 6)]                                 # level 0 and level 4
        for shape in odd_shapes:
            t, b = make(*shape)
            tensors.append(t)
            rejected(fn, b_in, b)
    torch.cuda.synchronize()
    for t in tensors:                                                        # nothing ran: every buffer still holds its fill
        assert bool((t == (0x11 if t.dtype == torch.uint8 else 0x1111)).all())


def test_pitched_rows_and_untouched_padding(oracle):
    """One case per kernel with a row pitch above width * element size on both sides; the output padding keeps its fill.
    A pad of 3 u16 (5 bytes) also takes the rows off the 8-byte alignment the wide loads need."""
    _, raw = raw_depth_image()
    raw = np.ascontiguousarray(raw[:96, :160])
    for pad in (4, 3):
        got, padding = gpu_median(raw, in_pad=pad, out_pad=pad + 4)
        assert np.array_equal(got, np_median_filter_and_densify(raw)) and (padding.view(np.uint16) == 0x5A5A).all()
        got, padding = gpu_downscale_depth(raw, 2, in_pad=pad, out_pad=pad)
        assert np.array_equal(got, np_downscale_depth_median(raw, 2)) and (padding.view(np.uint16) == 0x5A5A).all()
    rgb = np.random.default_rng(3).integers(0, 256, (96, 160, 3), dtype=np.uint8)
    got, padding = gpu_downscale_rgb(rgb, 2, in_pad=7, out_pad=5)
    assert np.array_equal(got, np_downscale_rgb(rgb, 2)) and (padding == 0x5A).all()
