"""The one bilinear form of both texture modes (device_math.hpp: val = bilinear_value(b, inner, top) = fma(b, inner, top) with
top = bilinear_top = fma(a, dtop, tl) and the mode's `inner`), against the two formulas it replaces:
  fixed point  bilinear_diffs_fixed: fma(b, fma(a, dmix, dleft), fma(a, dtop, tl)), and through it the fma chain of
               bilinear_bytes on float texels (tests/test_fixed_point_sampling_cpu.py), for every weight pair of the 1/256 grid;
  exact float  bilinear_bytes_entry: top = fma(a, dtop, tl), bot = fma(a, dmix + dtop, tl + dleft), fma(b, bot - top, top), and
               bilinear_bytes on float texels (tr - tl, br - bl formed as float differences of the bytes), for random fp32 weights.
Same quads as tests/test_fixed_point_sampling_cpu.py.  An fma is emulated as a float64 product plus add rounded to float32: the
product of two float32 is exact in float64; where the float64 sum rounds, both sides of a comparison round the same operands."""
import numpy as np

from tests.test_fixed_point_sampling_cpu import fma32

f = np.float32


def quads():
    rng = np.random.default_rng(20261016)
    q = rng.integers(0, 256, size=(96, 4))
    q[:8] = [[0, 0, 0, 0], [255, 255, 255, 255], [0, 255, 255, 0], [255, 0, 0, 255],
             [0, 0, 255, 255], [255, 255, 0, 0], [0, 255, 0, 255], [255, 0, 255, 0]]
    return q


def entry(tl, tr, bl, br):
    """QuadDiffs of a quad: the integer differences of the table, converted once."""
    dtop, dleft = tr - tl, bl - tl
    return f(tl), f(dtop), f(dleft), f((br - bl) - dtop)


def one_form(a, b, t, fixed):
    tl, dtop, dleft, dmix = t
    top = fma32(a, dtop, tl)                                                        # bilinear_top
    inner = fma32(a, dmix, dleft) if fixed else (fma32(a, f(dmix + dtop), f(tl + dleft)) - top).astype(np.float32)
    return fma32(b, inner, top)                                                     # bilinear_value


def bilinear_bytes(a, b, tl, tr, bl, br):
    top = fma32(a, f(tr) - f(tl), f(tl))
    bot = fma32(a, f(br) - f(bl), f(bl))
    return fma32(b, (bot - top).astype(np.float32), top)


def test_fixed_point_inner_gives_the_old_fixed_point_value():
    k = np.arange(257, dtype=np.int64)
    ka, kb = (x.ravel() for x in np.meshgrid(k, k, indexing="ij"))
    a = (ka.astype(np.float32) * f(1.0 / 256.0)).astype(np.float32)
    b = (kb.astype(np.float32) * f(1.0 / 256.0)).astype(np.float32)
    for tl, tr, bl, br in quads():
        t = entry(tl, tr, bl, br)
        got = one_form(a, b, t, fixed=True)
        old = fma32(b, fma32(a, t[3], t[2]), fma32(a, t[1], t[0]))                  # bilinear_diffs_fixed
        assert np.array_equal(got.view(np.uint32), old.view(np.uint32))
        assert np.array_equal(got.view(np.uint32), bilinear_bytes(a, b, tl, tr, bl, br).view(np.uint32))
        # on the grid the exact-float inner is the same number too: the two arms of the mode test agree where both apply
        assert np.array_equal(got.view(np.uint32), one_form(a, b, t, fixed=False).view(np.uint32))


def test_exact_float_inner_gives_the_old_exact_float_value():
    rng = np.random.default_rng(20261020)
    a = rng.random(100000, dtype=np.float32)
    b = rng.random(100000, dtype=np.float32)
    a[:4], b[:4] = [0, 0, f(1) - f(2 ** -24), f(2 ** -30)], [0, f(1) - f(2 ** -24), 0, f(2 ** -30)]
    assert a.dtype == b.dtype == np.float32 and (a < 1).all() and (b < 1).all()
    for tl, tr, bl, br in quads():
        t = entry(tl, tr, bl, br)
        got = one_form(a, b, t, fixed=False)
        top = fma32(a, t[1], t[0])                                                  # bilinear_bytes_entry
        bot = fma32(a, f(t[3] + t[1]), f(t[0] + t[2]))
        old = fma32(b, (bot - top).astype(np.float32), top)
        assert np.array_equal(got.view(np.uint32), old.view(np.uint32))
        assert np.array_equal(got.view(np.uint32), bilinear_bytes(a, b, tl, tr, bl, br).view(np.uint32))
