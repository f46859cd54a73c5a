"""The oracle's preprocessing producers (oracle/bso_scene.c) against float64 restatements of the reference's rules
(tests/preprocess_util.py), without a GPU.  The GPU tests compare the kernels with the oracle bit for bit; this module is
what makes the oracle trustworthy on their inputs, since kernel and oracle were written from one reading of the source.

Per producer: the validity pattern is exactly equal, and every value is equal except at a rounding boundary, where fp32
and float64 may land on either side and differ by one unit (one depth unit, one s8 step, one half-precision ulp).  A
pixel is at a rounding boundary if its float64 value in front of the integer conversion lies within DELTA of a point where
the conversion changes.  MEASURED is the largest such distance among the pixels on which the oracle and float64 do differ
on the committed inputs, DELTA four times that (the oracle's fp32 error grows with the number of terms summed; other
inputs of the same kind need headroom), in units of the output step.  At most CAP of a producer's valid pixels may differ.

One parameter set is outside the cap by construction: with a bilateral radius of 0 the filtered value is
1 / (s * (1 / (s * d))), in exact arithmetic the integer d itself, so EVERY pixel sits on a truncation boundary and d or
d - 1 comes out as the last bit falls (481 of 2260 pixels differ between fp32 and float64, at most 2e-12 from the integer).
For that set the test asserts instead that both sides give d or d - 1 everywhere, besides the boundary rule."""
import functools

import numpy as np
import pytest

from tests import preprocess_util as U

# producer: largest boundary distance measured on a differing pixel (units of the output step), rounded up
MEASURED = {"bilateral": 0.0021, "normals": 0.0003, "radii": 0.0091, "brightness": 1.2e-6}
DELTA = {name: 4 * value for name, value in MEASURED.items()}
CAP = 0.01
H, W = 37, 67
SIGNS, CELLS = (1, -1), (3, 4)


@functools.lru_cache(None)
def raw_depth():
    raw = U.build_raw_depth(H, W)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(None)
def bilateral(name):
    """(oracle output, float64 output, float64 value)"""
    got = U.oracle_bilateral(raw_depth(), *U.BILATERAL_SETS[name])
    want, v = U.f64_bilateral(raw_depth(), *U.BILATERAL_SETS[name])
    return got, want, v


@functools.lru_cache(None)
def normals(fy_sign, cell):
    """(oracle depth, oracle normals, float64 result) on the oracle's default bilateral output"""
    filtered = bilateral("default")[0]
    camera, cfactor = U.build_camera(H, W, fy_sign), U.build_cfactor(H, W, cell)
    return U.oracle_normals(filtered, camera, cfactor, cell) + (U.f64_normals(filtered, camera, cfactor, cell),)


@functools.lru_cache(None)
def radii(fy_sign, wide, valid_border=False):
    """(oracle radius bits, oracle depth, float64 radius bits, float64 depth, float64 min_sq); valid_border: on the bilateral output,
    whose border is valid, instead of the normals stage's"""
    depth = bilateral("default")[0] if valid_border else normals(fy_sign, 3)[0]
    camera = U.build_camera(H, W, fy_sign, wide)
    return U.oracle_radii(depth, camera) + U.f64_radii(depth, camera)


def s8(u16, shift):
    return ((u16.astype(np.int64) >> shift) & 0xff).astype(np.uint8).view(np.int8).astype(np.int64)


def check_values(producer, what, got, want, distance, valid, cap=True):
    """got, want: integer images; distance: per pixel, how far the float64 value is from a change of the conversion."""
    got, want = got.astype(np.int64), want.astype(np.int64)
    differ = got != want
    share = differ.sum() / max(1, valid.sum())
    worst = float(distance[differ].max()) if differ.any() else 0.0
    print(f"{producer} {what}: {differ.sum()} of {valid.sum()} valid pixels differ ({100 * share:.2f} %), largest boundary distance {worst:.3g}, "
          f"recorded {MEASURED[producer]:.3g}, delta {DELTA[producer]:.3g}")
    assert not (differ & ~valid).any(), np.argwhere(differ & ~valid)[:5]
    assert (np.abs(got - want)[differ] == 1).all(), (np.argwhere(differ)[:5], got[differ][:5], want[differ][:5])
    assert (distance[differ] <= DELTA[producer]).all(), (np.argwhere(differ)[:5], distance[differ][:5])
    if cap:
        assert share <= CAP, share
    return int(differ.sum()), worst


@pytest.mark.parametrize("name", list(U.BILATERAL_SETS))
def test_bilateral_filter_and_cutoff(oracle, name):
    got, want, v = bilateral(name)
    raw, max_depth = raw_depth(), U.BILATERAL_SETS[name][3]
    known = ~np.isnan(v)
    # which pixels are unknown: no measurement, beyond the cut-off (no weight cannot happen: the centre weighs 1)
    assert np.array_equal(known, (raw != 0) & (raw <= max_depth))
    assert (got[~known] == U.UNKNOWN).all() and (want[~known] == U.UNKNOWN).all()
    if name != "no_cutoff":
        assert np.array_equal(got == U.UNKNOWN, ~known)                     # nothing saturates: the pattern is the rule's
    check_values("bilateral", name, got, want, U.distance_to_integer(np.nan_to_num(v)), known, cap=name != "radius0")
    if name == "radius0":
        for out in (got, want):
            assert ((out[known] == raw[known]) | (out[known] == raw[known] - 1)).all()
    for out in (got, want):
        if name == "no_cutoff":
            assert (raw >= 32768).sum() >= 3 and (out[raw >= 32768] >= 32767).all() and ((out >= 32768) & (out < 65534)).any()
        else:
            assert (raw > max_depth).sum() >= 40 and (out[raw > max_depth] == U.UNKNOWN).all()          # cut by max_depth
            at_cutoff = raw == max_depth
            assert at_cutoff.sum() >= 1 and (out[at_cutoff] != U.UNKNOWN).all()                         # kept at exactly max_depth
    if name == "default":                                                    # the window is clipped at all four borders
        assert min(H, W) > 6 and all(known[edge].any() for edge in ((0, slice(None)), (H - 1, slice(None)), (slice(None), 0), (slice(None), W - 1)))


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("fy_sign", SIGNS)
def test_normals(oracle, fy_sign, cell):
    assert W % cell and U.build_cfactor(H, W, cell).shape == (-(-H // cell), -(-W // cell))
    got_depth, got_normals, ref = normals(fy_sign, cell)
    valid = ref["depth"] != U.UNKNOWN
    assert np.array_equal(got_depth, ref["depth"])                           # validity pattern, and the depth passes through
    assert (got_normals[~valid] == 0).all() and (ref["normals"][~valid] == 0).all()
    assert not valid[0].any() and not valid[-1].any() and not valid[:, 0].any() and not valid[:, -1].any()
    for component, shift in (("nx127", 0), ("ny127", 8)):
        check_values("normals", f"fy {fy_sign:+d} cell {cell} {component}", s8(got_normals, shift), s8(ref["normals"], shift),
                     U.distance_to_s8_step(np.nan_to_num(ref[component])), valid)


@pytest.mark.parametrize("valid_border", [False, True])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("fy_sign", SIGNS)
def test_radii_and_isolated_pixel_removal(oracle, fy_sign, wide, valid_border):
    got_bits, got_depth, want_bits, want_depth, min_sq = radii(fy_sign, wide, valid_border)
    kept = want_depth != U.UNKNOWN
    assert np.array_equal(got_depth, want_depth)                             # which pixels survive, with their depth
    assert (got_bits[~kept] == 0).all() and (want_bits[~kept] == 0).all()
    border = np.ones((H, W), bool)
    border[1:-1, 1:-1] = False
    assert not kept[border].any()                                            # fewer than 4 neighbours inside the image
    if valid_border:
        assert ((bilateral("default")[0] & U.INVALID_BIT) == 0)[border].sum() > H + W
    check_values("radii", f"fy {fy_sign:+d} {'fx 500' if wide else 'fx 60'} {'valid border' if valid_border else ''}", got_bits, want_bits,
                 U.distance_to_half_midpoint(np.nan_to_num(min_sq, nan=1.0)), kept)


@functools.lru_cache(None)
def brightness_image():
    r, column = np.mgrid[0:256, 0:1024]
    return np.stack([r, column % 256, np.array([0, 1, 254, 255])[column // 256]], -1).astype(np.uint8)


def test_brightness(oracle):
    rgb = brightness_image()
    got = U.oracle_brightness(rgb)
    want, luma = U.f64_brightness(rgb)
    assert np.array_equal(got[..., :3], rgb) and np.array_equal(want[..., :3], rgb)
    check_values("brightness", "all (r, g) at b in 0, 1, 254, 255", got[..., 3], want[..., 3], U.distance_to_integer(luma), np.ones(luma.shape, bool))
    grey = np.repeat(np.arange(256, dtype=np.uint8), 3).reshape(1, 256, 3)
    assert np.array_equal(U.oracle_brightness(grey)[0, :, 3], np.arange(256)) and np.array_equal(U.f64_brightness(grey)[0][0, :, 3], np.arange(256))
    assert got[..., 3].min() == 0 and got[..., 3].max() == 255


def test_min_max_is_one_fp32_product(oracle):
    for depth in (bilateral("default")[0], normals(1, 3)[0], np.full((3, 5), U.UNKNOWN, np.uint16)):
        assert U.oracle_min_max(depth) == U.f32_min_max(depth)


def test_the_inputs_reach_every_branch(oracle):
    """The counts the other tests rely on, on the float64 and on the oracle's outputs alike (the branch an axis took is only known
    on the float64 side; the oracle's normals agree with it to one step, so it took the same ones)."""
    for fy_sign in SIGNS:
        for cell in CELLS:
            got_depth, got_normals, ref = normals(fy_sign, cell)
            counts = [int((ref[axis] == branch).sum()) for axis in ("lr", "bt") for branch in (U.SYMMETRIC, U.FIRST, U.SECOND)] + [int(ref["degenerate"].sum())]
            print(f"fy {fy_sign:+d} cell {cell}: left/right symmetric, left, right = {counts[:3]}, bottom/top symmetric, bottom, top = {counts[3:6]}, "
                  f"degenerate = {counts[6]}, valid = {int((ref['depth'] != U.UNKNOWN).sum())}")
            assert min(counts) >= 3, counts
            for normal_image in (got_normals, ref["normals"]):
                for shift in (0, 8):
                    component = s8(normal_image, shift)
                    assert (component > 0).sum() >= 100 and (component < 0).sum() >= 100
            assert (got_normals[ref["degenerate"]] == 0).all()
        subnormal = normal = 0
        for wide in (False, True):
            got_bits, got_depth, want_bits, want_depth, min_sq = radii(fy_sign, wide)
            stage1_valid = normals(fy_sign, 3)[0] != U.UNKNOWN
            for depth, bits in ((got_depth, got_bits), (want_depth, want_bits)):
                kept = depth != U.UNKNOWN
                assert (stage1_valid & ~kept).sum() >= 1                      # removed as isolated
            kept = got_depth != U.UNKNOWN
            subnormal += int((got_bits[kept] < 0x0400).sum())                 # half precision: below 2^-14
            normal += int((got_bits[kept] >= 0x0400).sum())
        print(f"fy {fy_sign:+d}: kept radii over both cameras: {subnormal} subnormal, {normal} normal")
        assert 4 * subnormal >= subnormal + normal and 4 * normal >= subnormal + normal
