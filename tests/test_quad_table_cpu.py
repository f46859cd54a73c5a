"""The luma quad table's entries in fp16 (csrc/device_math.hpp: pack_quad) lose nothing: every number an entry can hold is an
integer of magnitude <= 510, exact in a half's 11-bit significand, so the kernels' conversions return the integers that the
per-sample byte unpacking formed before.  No GPU: a numpy restatement of the packing helper (tests/quad_table.py)."""
import numpy as np

from tests import quad_table as Q


def test_every_difference_survives_float16():
    n = np.arange(-510, 511, dtype=np.int32)
    h = n.astype(np.float16)
    assert np.array_equal(h.astype(np.float32), n.astype(np.float32))
    assert np.array_equal(h.astype(np.int32), n)


def test_differences_equal_the_integer_formulas_for_all_byte_pairs():
    tl, x = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    tl, x = tl.ravel(), x.ravel()
    # each of tr, bl, br in turn takes the second byte, the others stay at tl; then the second byte in two places
    for tr, bl, br in ((x, tl, tl), (tl, x, tl), (tl, tl, x), (x, x, tl), (x, tl, x), (tl, x, x), (x, 255 - x, tl), (x, 255 - x, 255 - tl)):
        e = Q.pack_quad(tl, tr, bl, br).astype(np.float64)
        assert np.array_equal(e[:, 0], tl)
        assert np.array_equal(e[:, 1], tr - tl)
        assert np.array_equal(e[:, 2], bl - tl)
        assert np.array_equal(e[:, 3], (br - bl) - (tr - tl))


def test_extreme_quads_reach_plus_and_minus_510():
    seen = set()
    for bits in range(16):
        tl, tr, bl, br = (255 * ((bits >> s) & 1) for s in range(4))
        e = Q.pack_quad(tl, tr, bl, br).astype(np.float64)
        assert list(e) == [tl, tr - tl, bl - tl, (br - bl) - (tr - tl)]
        seen.add(int(e[3]))
    assert {-510, 510} <= seen


def test_float32_adds_return_the_bytes():
    rng = np.random.default_rng(5)
    q = rng.integers(0, 256, size=(4096, 4))
    q[:16] = [[255 * ((bits >> s) & 1) for s in range(4)] for bits in range(16)]
    tl, tr, bl, br = Q.unpack_bytes(Q.pack_quad(q[:, 0], q[:, 1], q[:, 2], q[:, 3]))
    for got, want in zip((tl, tr, bl, br), q.T):
        assert got.dtype == np.float32
        assert np.array_equal(got, want.astype(np.float32))


def test_table_holds_clamped_footprints():
    rng = np.random.default_rng(6)
    luma = rng.integers(0, 256, size=(5, 4), dtype=np.uint8)
    t = Q.table(luma)
    assert t.shape == (6, 5, 4) and t.dtype == np.float16
    for j in range(-1, 5):
        for i in range(-1, 4):
            c = lambda y, x: int(luma[min(max(y, 0), 4), min(max(x, 0), 3)])
            tl, tr, bl, br = c(j, i), c(j, i + 1), c(j + 1, i), c(j + 1, i + 1)
            assert list(t[j + 1, i + 1].astype(np.int32)) == [tl, tr - tl, bl - tl, (br - bl) - (tr - tl)]
