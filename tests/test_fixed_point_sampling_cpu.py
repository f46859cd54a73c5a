"""The fixed-point (1.8) texture mode's bilinear value, as the descriptor kernels form it from byte differences
(device_math.hpp: quad_diffs + bilinear_diffs_fixed), against the fma chain of bilinear_bytes it replaces.

With weights a = ka / 256, b = kb / 256 (ka, kb in [0, 256]) every intermediate of both chains is a multiple of 2^-16 below
2^24 in magnitude, so each fma is exact and the two chains give the same float32 -- the integer N / 2^16 with
N = (256 - kb) top' + kb bot', top' = (256 - ka) tl + ka tr, bot' = (256 - ka) bl + ka br.  An fma is emulated as a float64
product plus add rounded once to float32, which is exact at these widths."""
import numpy as np


def fma32(a, b, c):
    return (np.float64(a) * np.float64(b) + np.float64(c)).astype(np.float32)


def test_fixed_point_bilinear_from_differences_is_bit_identical():
    rng = np.random.default_rng(20261016)
    k = np.arange(257, dtype=np.int64)
    ka, kb = (x.ravel() for x in np.meshgrid(k, k, indexing="ij"))
    a = (ka.astype(np.float32) * np.float32(1.0 / 256.0)).astype(np.float32)
    b = (kb.astype(np.float32) * np.float32(1.0 / 256.0)).astype(np.float32)
    assert np.array_equal(a.astype(np.float64) * 256, ka) and np.array_equal(b.astype(np.float64) * 256, kb)
    quads = rng.integers(0, 256, size=(96, 4))
    quads[:8] = [[0, 0, 0, 0], [255, 255, 255, 255], [0, 255, 255, 0], [255, 0, 0, 255],
                 [0, 0, 255, 255], [255, 255, 0, 0], [0, 255, 0, 255], [255, 0, 255, 0]]
    for tl, tr, bl, br in quads:
        # bilinear_bytes on float texels: top = fma(a, tr - tl, tl), bot = fma(a, br - bl, bl), fma(b, bot - top, top)
        f = np.float32
        top = fma32(a, f(tr) - f(tl), f(tl))
        bot = fma32(a, f(br) - f(bl), f(bl))
        ref = fma32(b, (bot - top).astype(np.float32), top)
        # quad_diffs + bilinear_diffs_fixed: integer differences converted once
        dtop, dleft = tr - tl, bl - tl
        dmix = (br - bl) - dtop
        assert dmix == (br - tr) - (bl - tl)   # the gradient's two components share it
        got = fma32(b, fma32(a, f(dmix), f(dleft)), fma32(a, f(dtop), f(tl)))
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
        # both are N / 2^16 exactly
        n = (256 - kb) * ((256 - ka) * tl + ka * tr) + kb * ((256 - ka) * bl + ka * br)
        assert n.max() < 2 ** 24
        assert np.array_equal(ref.astype(np.float64) * 65536, n)


def test_residual_difference_of_fixed_point_values_is_exact():
    """The residual takes val1 - val0: a difference of two multiples of 2^-16 below 2^8, exact in float32."""
    rng = np.random.default_rng(7)
    n0 = rng.integers(0, 255 * 65536 + 1, size=200000)
    n1 = rng.integers(0, 255 * 65536 + 1, size=200000)
    v0 = (n0 / 65536.0).astype(np.float32)
    v1 = (n1 / 65536.0).astype(np.float32)
    assert np.array_equal(v0.astype(np.float64) * 65536, n0) and np.array_equal(v1.astype(np.float64) * 65536, n1)
    assert np.array_equal((v1 - v0).astype(np.float64) * 65536, n1 - n0)
