"""Shared by the preprocessing tests: float64 NumPy restatements of the keyframe image producers, a deterministic input
builder that reaches every branch of them, oracle wrappers, and the pitched device images of the GPU tests.

The restatements are written from the reference's rules (BS/cuda_depth_processing.cu:42-357, BS/cuda_image_processing.cu:165-176,
BS/util.cuh:46-53 and 101-118, BS/surfel_projection.h:58-67), not from the kernels' instruction order: float64 throughout,
np.exp, true division, nothing fused.  Whatever is fp32 in the ABI (camera, a, cfactors, raw_to_float_depth, sigmas) and
every fp32 literal of the reference is rounded to fp32 first and then widened, so both sides start from the same numbers.
Besides its integer output each restatement returns the real value in front of the last integer conversion: a pixel on
which fp32 and float64 differ is legitimate only if that value lies at a point where the conversion changes its result."""
import ctypes as C
import math

import numpy as np

from badslam_amd import abi
from tests import bso

UNKNOWN = 65535            # BSLAM_UNKNOWN_DEPTH
INVALID_BIT = 0x8000       # BSLAM_INVALID_DEPTH_BIT
RAW_TO_FLOAT = 0.0002
MAX_DEPTH = 15000          # 3 m / RAW_TO_FLOAT, the default cut-off (BS/bad_slam.cc:694-702)
BILATERAL_SETS = {         # (sigma_xy, sigma_inv_depth, radius_factor, max_depth)
    "default": (3.0, 0.005, 2.0, MAX_DEPTH),        # radius 6
    "radius0": (0.2, 0.005, 2.0, MAX_DEPTH),        # radius 0: the pixel's own value after two reciprocals
    "no_cutoff": (3.0, 0.005, 2.0, 65535),          # raw samples >= 32768 are filtered like any other
}
A = 0.02


def w32(x):
    """An fp32 argument as float64."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------
# the input builder
# ------------------------------------------------------------------------------------------------
def build_raw_depth(h=37, w=67):
    """A small raw depth image that reaches every branch of the producers: a tent-shaped slanted surface (both signs of both
    normal components) with +-8 units of noise, a 0.35 m step down the middle and a 0.3 m step across a corner (the one-sided
    branches of both axes), 6 % holes and a rectangular hole, a block beyond the cut-off with a pixel at exactly the cut-off
    next to it, a 3 x 3 patch of raw value 2 (degenerate cross product), and raw values 1, 3 and 65535 sprinkled in."""
    rng = np.random.default_rng(20240611)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    z = 1.2 + 0.0045 * np.abs(x - 0.3 * w) + 0.006 * np.abs(y - 0.45 * h)
    z[:, w // 2:] += 0.35
    z[(2 * h) // 3:, :w // 4] += 0.3
    raw = np.rint(z / RAW_TO_FLOAT).astype(np.int64) + rng.integers(-8, 9, (h, w))
    raw[rng.random((h, w)) < 0.06] = 0
    raw[h // 2:h // 2 + 4, w // 8:w // 8 + 5] = 0
    raw[3:8, w - 16:w - 7] = 17000 + rng.integers(-8, 9, (5, 9))     # 3.4 m: beyond the cut-off
    raw[5, w - 17] = MAX_DEPTH                          # exactly the cut-off: kept
    raw[h - 9:h - 6, w - 27:w - 24] = 2
    for i, value in enumerate((1, 3, 65535, 40000, 33000)):
        raw[(5 + 7 * i) % h, (11 + 13 * i) % w] = value
    raw[0, 0], raw[h - 1, w - 1], raw[0, w - 1], raw[h - 1, 0] = 6100, 7300, 6900, 6500     # valid corners
    return raw.clip(0, 65535).astype(np.uint16)


def shaped_raw_depth(h, w):
    """The builder's image for the other shapes of the GPU tests: rows from its middle repeated sideways (5 x 257), the first
    fully measured window (3 x 3), a piece of one row (1 x 5)."""
    raw = build_raw_depth()
    if (h, w) == raw.shape:
        return raw
    if h * w <= 9:
        for y in range(raw.shape[0] - h + 1):
            for x in range(raw.shape[1] - w + 1):
                piece = raw[y:y + h, x:x + w]
                if ((piece > 0) & (piece <= MAX_DEPTH)).all():
                    return np.ascontiguousarray(piece)
    top = (raw.shape[0] - h) // 2
    return np.ascontiguousarray(np.tile(raw[top:top + h], (1, -(-w // raw.shape[1])))[:, :w])


def build_camera(h, w, fy_sign=1, wide=False):
    """fx 60 (radii above the half-precision subnormal range) or, wide, fx 500 (most radii subnormal, as at 640 x 480)."""
    if wide:
        return bso.make_camera(500.0, fy_sign * 483.0, 33.2, 18.9, w, h)
    return bso.make_camera(60.0, fy_sign * 58.0, 33.2, 18.9, w, h)


def build_cfactor(h, w, cell):
    rng = np.random.default_rng(77 + cell)
    return rng.uniform(-0.003, 0.003, (-(-h // cell), -(-w // cell))).astype(np.float32)


def depth_params(cfactor_buf, cell, a=A):
    dp = abi.DepthParams()
    dp.cfactor_buffer = cfactor_buf
    dp.a = a
    dp.raw_to_float_depth = RAW_TO_FLOAT
    dp.baseline_fx = 40.0
    dp.sparse_surfel_cell_size = cell
    return dp


def build_rgb(h, w):
    return np.random.default_rng(9).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------
# float64 restatements
# ------------------------------------------------------------------------------------------------
def f64_bilateral(raw, sigma_xy, sigma_value, radius_factor, max_depth, raw_to_float=RAW_TO_FLOAT):
    """-> (u16 output, v): v is the filtered depth in raw units in front of the truncating, saturating u16 conversion, NaN
    where the rule itself says unknown (no measurement, beyond the cut-off, no weight)."""
    h, w = raw.shape
    radius = int(np.float32(radius_factor) * np.float32(sigma_xy) + np.float32(0.5))
    denom_xy, denom_value, rtf = 2.0 * w32(sigma_xy) ** 2, 2.0 * w32(sigma_value) ** 2, w32(raw_to_float)
    d = raw.astype(np.float64)
    with np.errstate(divide="ignore"):
        inv = 1.0 / (rtf * d)
    v = np.full((h, w), np.nan)
    for y in range(h):
        y0, y1 = max(0, y - radius), min(h - 1, y + radius)
        for x in range(w):
            if raw[y, x] == 0 or raw[y, x] > max_depth:
                continue
            x0, x1 = max(0, x - radius), min(w - 1, x + radius)
            dy, dx = np.mgrid[y0 - y:y1 - y + 1, x0 - x:x1 - x + 1]
            grid = dx * dx + dy * dy
            use = (grid <= radius * radius) & (raw[y0:y1 + 1, x0:x1 + 1] != 0)
            sample = inv[y0:y1 + 1, x0:x1 + 1][use]
            weight = np.exp(-grid[use] / denom_xy - (inv[y, x] - sample) ** 2 / denom_value)
            if weight.sum() == 0:
                continue
            v[y, x] = 1.0 / (rtf * (weight * sample).sum() / weight.sum())
    out = np.where(np.isnan(v), UNKNOWN, np.minimum(np.floor(np.nan_to_num(v)), 65535)).astype(np.uint16)
    return out, v


SYMMETRIC, FIRST, SECOND = 0, 1, 2       # the three ways an axis takes its difference: right - left, centre - left, right - centre


def f64_normals(depth, camera, cfactor, cell, a=A, raw_to_float=RAW_TO_FLOAT):
    """-> dict(depth, normals (u16), nx127, ny127 (the components times 127, NaN where rejected), lr, bt (branch per axis, -1
    where rejected), degenerate)."""
    h, w = depth.shape
    fx, fy, cx, cy, rtf, a = w32(camera.fx), w32(camera.fy), w32(camera.cx), w32(camera.cy), w32(raw_to_float), w32(a)
    tiny = w32(1e-6)
    out_depth = np.full((h, w), UNKNOWN, np.uint16)
    out_normals = np.zeros((h, w), np.uint16)
    nx127, ny127 = np.full((h, w), np.nan), np.full((h, w), np.nan)
    lr, bt = np.full((h, w), -1), np.full((h, w), -1)
    degenerate = np.zeros((h, w), bool)

    def point(yy, xx):
        inv = 1.0 / (rtf * float(depth[yy, xx]))
        z = 1.0 / (inv + float(cfactor[yy // cell, xx // cell]) * np.exp(-a * inv))
        return np.array([z * (xx - (cx - 0.5)) / fx, z * (yy - (cy - 0.5)) / fy, z])

    def axis(first, centre, second):
        """first = left / bottom, second = right / top"""
        d1, d2 = ((first - centre) ** 2).sum(), ((second - centre) ** 2).sum()
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.float64(d1) / np.float64(d2)
        if 0.25 < ratio < 4.0:
            return SYMMETRIC, second - first
        if d1 < d2:
            return FIRST, centre - first
        return SECOND, second - centre

    def s8(value):
        return math.trunc(value + (0.5 if value > 0 else -0.5)) & 0xff

    for y in range(1, h - 1):
        for x in range(1, w - 1):
            five = (depth[y, x], depth[y, x + 1], depth[y, x - 1], depth[y + 1, x], depth[y - 1, x])
            if any(int(v) & INVALID_BIT for v in five):
                continue
            centre = point(y, x)
            lr[y, x], left_to_right = axis(point(y, x - 1), centre, point(y, x + 1))
            bt[y, x], bottom_to_top = axis(point(y + 1, x), centre, point(y - 1, x))
            normal = np.cross(left_to_right, bottom_to_top)
            length = math.sqrt((normal ** 2).sum())
            if not length > tiny:
                degenerate[y, x] = True
                nx, ny = 0.0, 0.0
            else:
                sign = -1.0 if fy < 0 else 1.0
                nx, ny = sign * normal[0] / length, sign * normal[1] / length
            nx127[y, x], ny127[y, x] = nx * 127, ny * 127
            out_normals[y, x] = s8(nx * 127) | (s8(ny * 127) << 8)
            out_depth[y, x] = depth[y, x]
    return dict(depth=out_depth, normals=out_normals, nx127=nx127, ny127=ny127, lr=lr, bt=bt, degenerate=degenerate)


def f64_radii(depth, camera, raw_to_float=RAW_TO_FLOAT):
    """-> (radius bits u16, output depth u16, min_sq): min_sq is the squared distance to the nearest valid 4-neighbour in front
    of the half-precision conversion, NaN where the pixel is not kept (invalid, or fewer than 4 valid neighbours)."""
    h, w = depth.shape
    fx, fy, cx, cy, rtf = w32(camera.fx), w32(camera.fy), w32(camera.cx), w32(camera.cy), w32(raw_to_float)
    valid = (depth & INVALID_BIT) == 0
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    z = rtf * depth.astype(np.float64)
    points = np.stack([z * (x - (cx - 0.5)) / fx, z * (y - (cy - 0.5)) / fy, z], -1)
    count = np.zeros((h, w), int)
    min_sq = np.full((h, w), np.inf)
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        other_valid = np.zeros((h, w), bool)
        other = np.zeros((h, w, 3))
        ys, yd = (slice(1, h), slice(0, h - 1)) if dy > 0 else (slice(0, h - 1), slice(1, h)) if dy < 0 else (slice(0, h), slice(0, h))
        xs, xd = (slice(1, w), slice(0, w - 1)) if dx > 0 else (slice(0, w - 1), slice(1, w)) if dx < 0 else (slice(0, w), slice(0, w))
        other_valid[yd, xd] = valid[ys, xs]                  # neighbours outside the image stay absent
        other[yd, xd] = points[ys, xs]
        count += other_valid
        min_sq = np.where(other_valid, np.minimum(min_sq, ((other - points) ** 2).sum(-1)), min_sq)
    kept = valid & (count >= 4)
    min_sq = np.where(kept, min_sq, np.nan)
    with np.errstate(over="ignore"):
        bits = np.where(kept, np.nan_to_num(min_sq), 0.0).astype(np.float16).view(np.uint16)      # float64 -> half, nearest even
    return bits, np.where(kept, depth, UNKNOWN).astype(np.uint16), min_sq


def f64_brightness(rgb):
    """-> ((h, w, 4) u8 r, g, b, luma; the luma + 0.5 in front of the truncation)."""
    luma = w32(0.299) * rgb[..., 0].astype(np.float64) + w32(0.587) * rgb[..., 1] + w32(0.114) * rgb[..., 2] + 0.5
    return np.concatenate([rgb, np.floor(luma).astype(np.uint8)[..., None]], -1), luma


def f32_min_max(depth, raw_to_float=RAW_TO_FLOAT):
    """One fp32 product per pixel: exact to state in NumPy, and independent of both the kernel and the oracle."""
    metres = np.float32(raw_to_float) * depth.astype(np.float32)
    valid = (depth & INVALID_BIT) == 0
    assert metres.dtype == np.float32
    return (metres[valid].min(), metres[valid].max()) if valid.any() else (np.float32(np.inf), np.float32(0))


# ------------------------------------------------------------------------------------------------
# distance of a real value to the nearest point where its integer conversion changes
# ------------------------------------------------------------------------------------------------
def distance_to_integer(v):
    """Truncating conversions (u16 depth, u8 luma) change at the integers."""
    return np.abs(v - np.rint(v))


def distance_to_s8_step(n127):
    """trunc(n * 127 +- 0.5) changes where |n * 127| + 0.5 is an integer."""
    t = np.abs(n127) + 0.5
    return np.abs(t - np.rint(t))


def distance_to_half_midpoint(x):
    """Round-to-nearest half precision changes at the midpoints of neighbouring half values; in units of the local half ulp."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        bits = x.astype(np.float16).view(np.uint16).astype(np.int64)
    here = bits.astype(np.uint16).view(np.float16).astype(np.float64)
    above = (bits + 1).astype(np.uint16).view(np.float16).astype(np.float64)
    below = np.maximum(bits - 1, 0).astype(np.uint16).view(np.float16).astype(np.float64)
    ulp = above - here
    return np.minimum(np.abs(x - (here + above) / 2), np.abs(x - (here + below) / 2)) / ulp


# ------------------------------------------------------------------------------------------------
# the oracle on host arrays
# ------------------------------------------------------------------------------------------------
def oracle_bilateral(raw, sigma_xy, sigma_value, radius_factor, max_depth, raw_to_float=RAW_TO_FLOAT, lib=None):
    out = np.zeros(raw.shape, np.uint16)
    a, b = bso.np_buffer2d(raw), bso.np_buffer2d(out)
    (lib or bso.lib()).bso_bilateral_filter_and_depth_cutoff(sigma_xy, sigma_value, radius_factor, int(max_depth), raw_to_float, C.byref(a), C.byref(b))
    return out


def oracle_normals(depth, camera, cfactor, cell, lib=None):
    out_depth, out_normals = np.zeros(depth.shape, np.uint16), np.zeros(depth.shape, np.uint16)
    dp = depth_params(bso.np_buffer2d(cfactor), cell)
    a, b, c = bso.np_buffer2d(depth), bso.np_buffer2d(out_depth), bso.np_buffer2d(out_normals)
    (lib or bso.lib()).bso_compute_normals(C.byref(camera), C.byref(dp), C.byref(a), C.byref(b), C.byref(c))
    return out_depth, out_normals


def oracle_radii(depth, camera, raw_to_float=RAW_TO_FLOAT, lib=None):
    radius, out_depth = np.zeros(depth.shape, np.uint16), np.zeros(depth.shape, np.uint16)
    a, b, c = bso.np_buffer2d(depth), bso.np_buffer2d(radius), bso.np_buffer2d(out_depth)
    (lib or bso.lib()).bso_compute_point_radii_and_remove_isolated_pixels(C.byref(camera), raw_to_float, C.byref(a), C.byref(b), C.byref(c))
    return radius, out_depth


def oracle_brightness(rgb, lib=None):
    h, w = rgb.shape[:2]
    rgb = np.ascontiguousarray(rgb)
    out = np.zeros((h, w, 4), np.uint8)
    b = bso.np_buffer2d(out)
    (lib or bso.lib()).bso_compute_brightness(w, h, rgb.ctypes.data, C.byref(b))
    return out


def oracle_min_max(depth, raw_to_float=RAW_TO_FLOAT, lib=None):
    mn, mx = C.c_float(), C.c_float()
    a = bso.np_buffer2d(depth)
    (lib or bso.lib()).bso_compute_min_max_depth(C.byref(a), raw_to_float, C.byref(mn), C.byref(mx))
    return np.float32(mn.value), np.float32(mx.value)


# ------------------------------------------------------------------------------------------------
# pitched device images
# ------------------------------------------------------------------------------------------------
# input padding holds 0x33 bytes (as u16 a valid-looking depth below the cut-off), output padding 0x5A bytes, which must survive
IN_PAD, OUT_PAD = 3, 5                         # extra elements per input / output row: u16 rows are then not 4-byte aligned


def fill_value(dtype, byte):
    """The element of `dtype` whose bytes all equal `byte` (0x33: a small positive float, 0x5A: a large one)."""
    return np.frombuffer(bytes([byte]) * np.dtype(dtype).itemsize, dtype)[0]


def storable(array):
    """torch has no unsigned 16 / 32 bit tensors everywhere: the same bits as signed."""
    return array.view({np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(array.dtype, array.dtype))


def pitched(torch, array, pad_elems, fill, lead_elems=0):
    """Device copy of a 2-D array in rows of width + pad_elems elements, the first row starting lead_elems elements into the
    storage; the padding, the lead and nothing else hold `fill`.  The storage ends with the last row's padding, so a row and
    its padding always lie inside the allocation.  Returns (storage, Buffer2D)."""
    h, w = array.shape
    dtype = torch.from_numpy(array[:1, :1].copy()).dtype
    storage = torch.full((lead_elems + h * (w + pad_elems),), fill.item() if hasattr(fill, "item") else fill, dtype=dtype, device="cuda")
    rows = storage[lead_elems:].view(h, w + pad_elems)
    rows[:, :w] = torch.from_numpy(np.array(array)).cuda()          # a copy: the source may be read-only
    item = storage.element_size()
    return storage, abi.Buffer2D(storage.data_ptr() + lead_elems * item, h, w, (w + pad_elems) * item)


def unpitch(storage, h, w, pad_elems, lead_elems=0):
    """-> (image, everything else of the storage: lead and padding, flat) as host arrays."""
    host = storage.cpu().numpy()
    rows = host[lead_elems:].reshape(h, w + pad_elems)
    return np.ascontiguousarray(rows[:, :w]), np.concatenate([host[:lead_elems], rows[:, w:].ravel()])


class Images:
    """The pitched device images of one call.  Input rows carry IN_PAD extra elements of 0x33 bytes, output rows OUT_PAD
    extra elements of 0x5A bytes; `lead` starts every image that many elements into its storage."""

    def __init__(self, torch, lead=0):
        self.torch, self.lead, self.inputs, self.outputs = torch, lead, [], []

    def input(self, array, pad=IN_PAD, fill=None):
        """array: 2-D, or (h, w, 3) u8 rgb (padded in bytes), or (h, w, 4) u8 colour (padded in pixels, rows stay 4-byte aligned)"""
        width = array.shape[1]
        if array.ndim == 3:
            array = array.reshape(array.shape[0], -1) if array.shape[2] == 3 else np.ascontiguousarray(array).view(np.uint32)[..., 0]
        array = storable(np.ascontiguousarray(array))
        storage, b = pitched(self.torch, array, pad, fill_value(array.dtype, 0x33) if fill is None else fill, self.lead)
        b.width = width
        self.inputs.append(storage)
        return b

    def output(self, h, w, dtype=np.uint16, prefill=None):
        """prefill: what the image holds before the call (default: the 0x5A fill)"""
        fill = fill_value(dtype, 0x5A)
        start = np.full((h, w), fill, dtype) if prefill is None else prefill.astype(dtype)
        storage, b = pitched(self.torch, storable(start), OUT_PAD, storable(np.array([fill]))[0], self.lead)
        self.outputs.append((storage, h, w, dtype))
        return b

    def fetch(self):
        """Every output image, after checking that nothing but the images changed."""
        self.torch.cuda.synchronize()
        images = []
        for storage, h, w, dtype in self.outputs:
            image, rest = unpitch(storage, h, w, OUT_PAD, self.lead)
            assert (rest.view(np.uint8) == 0x5A).all(), "output padding was written"
            images.append(image.view(dtype))
        return images


# ------------------------------------------------------------------------------------------------
# fp32 NumPy restatements of the pyramid kernels whose arithmetic is plain unfused fp32
# ------------------------------------------------------------------------------------------------
f32 = np.float32


def np_truncate_u8(value):
    """float -> u8 as the GPU converts: truncate, saturate."""
    return np.clip(np.trunc(value), 0, 255).astype(np.uint8)


def np_read_mode_normalized(u8):
    """255 * (v / 255) in fp32, v / 255 as v * fl(1 / 255), truncated (LV/cuda/cuda_buffer.cu:82-102, BS/cuda_image_processing.cu:196-205)."""
    value = f32(255) * (u8.astype(f32) * f32(1.0 / 255.0))
    assert value.dtype == f32
    return np_truncate_u8(value)


def np_sobel_gradient_magnitude(luma):
    """BS/cuda_image_processing.cu:104-143 on a u8 luma image: 3 x 3 Sobel with clamp addressing on 255 * (v / 255), the terms summed
    left to right, magnitude * 255.99 / (sqrt(2) * 4 * 255), truncated."""
    h, w = luma.shape
    value = f32(255) * (luma.astype(f32) * f32(1.0 / 255.0))
    padded = np.pad(value, 1, mode="edge")
    I = [[padded[dy:dy + h, dx:dx + w] for dx in range(3)] for dy in range(3)]
    one, two = f32(1), f32(2)
    gx = one * I[0][2] - one * I[0][0] + two * I[1][2] - two * I[1][0] + one * I[2][2] - one * I[2][0]
    gy = one * I[2][0] - one * I[0][0] + two * I[2][1] - two * I[0][1] + one * I[2][2] - one * I[0][2]
    normalizer = f32(255.99) / (f32(1.41421356237309504880) * f32(4) * f32(255))
    magnitude = normalizer * np.sqrt(gx * gx + gy * gy)
    assert magnitude.dtype == f32
    return np_truncate_u8(magnitude)


def np_downsample(depth, normals, color, out_normals_fill):
    """DownsampleImages (BS/kernel_downsample.cu:105-152), all in fp32.  Depth: of each 2x2 block the valid (> 0) depth nearest
    to the block's mean of valid depths (first one on a tie; 0 without a valid one), with that pixel's normal.  Colour, on its
    own grid: the bilinear sample at the block's centre, i.e. weights 1/4 on texels normalised by 1/255, then
    trunc(255 * value + 0.5).  Odd sizes drop the last row / column."""
    h, w = depth.shape[0] // 2, depth.shape[1] // 2
    d4 = np.stack([depth[i >> 1:2 * h:2, i & 1:2 * w:2] for i in range(4)], -1).astype(f32)
    n4 = np.stack([normals[i >> 1:2 * h:2, i & 1:2 * w:2] for i in range(4)], -1)
    valid = d4 > 0
    total = np.zeros((h, w), f32)
    for i in range(4):
        total = np.where(valid[..., i], total + d4[..., i], total).astype(f32)
    count = valid.sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = (total / count.astype(f32)).astype(f32)
        distance = np.abs(np.where(valid, d4, f32(np.inf)) - mean[..., None])
    pick = np.argmin(np.where(count[..., None] > 0, distance, 0), -1)[..., None]
    out_depth = np.where(count > 0, np.take_along_axis(d4, pick, -1)[..., 0], f32(0)).astype(f32)
    out_normals = np.where(count > 0, np.take_along_axis(n4, pick, -1)[..., 0], out_normals_fill).astype(np.uint16)
    ch, cw = color.shape[0] // 2, color.shape[1] // 2
    t = [color[i >> 1:2 * ch:2, i & 1:2 * cw:2].astype(f32) * f32(1.0 / 255.0) for i in range(4)]
    q = f32(0.25)
    value = ((q * t[0] + q * t[1]) + q * t[2]) + q * t[3]
    assert value.dtype == f32
    out_color = np.clip(np.trunc(f32(255) * value + f32(0.5)), 0, 255).astype(np.uint8)
    return out_depth, out_normals, out_color
