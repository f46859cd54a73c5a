"""Markstein's theorem for the fp32 reciprocal, stated in integers over all 2^23 significands.

rcp_rn_midrange (csrc/device_math.hpp) is a hardware seed plus Newton steps r' = fma(fma(-x, r, 1), r, r).  Scale x = X 2^-23 with
the 24-bit significand X in [2^23, 2^24); then 1 / x lies in (1/2, 1] and its floats are R 2^-24 with R in [2^23, 2^24] (X = 2^23,
x = 1, is exact and left out).  In these units
    e = fma(-x, r, 1)  =  (2^47 - X R) 2^-47      exact whenever |2^47 - X R| < 2^24,
    fma(e, r, r)       =  RN(R + E R / 2^47)      one rounding of the exact value, to the integer grid of R.
E R stays below 2^49, so everything fits int64."""
import numpy as np

X = np.arange((1 << 23) + 1, 1 << 24, dtype=np.int64)
ONE = np.int64(1) << 47
LO = ONE // X                      # lower bracketing float of 2^47 / X; never exact for X > 2^23 (X would have to be a power of two)
UP = LO + 1
ALL_ONES = (1 << 24) - 1


def rn_quotient():
    """RN(2^47 / X): the remainder decides, a tie is impossible (2 rem = X needs X even and X | 2^48)."""
    rem = ONE - LO * X
    assert (2 * rem != X).all()
    return np.where(2 * rem > X, UP, LO)


def rn_div_pow2(n, shift):
    """Round-to-nearest-even of n / 2^shift for int64 n (negative too)."""
    q = n >> shift                              # floor
    r = n - (q << shift)
    half = np.int64(1) << (shift - 1)
    up = (r > half) | ((r == half) & ((q & 1) == 1))
    return q + up.astype(np.int64)


def newton(R):
    """One step from the seed R; also whether the first fma was exact (its result fits 24 bits)."""
    E = ONE - X * R
    exact = np.abs(E) < (1 << 24)
    # where E does not fit a significand the first fma rounds; the seeds of this file's statements never get there, but the
    # 3-ulp seeds of the two-step statement do: round E to 24 significant bits as the hardware would
    mag = np.abs(E)
    extra = np.maximum(0, np.frexp(mag.astype(np.float64))[1].astype(np.int64) - 24)   # bit length - 24 (mag < 2^53: exact)
    Er = np.where(extra > 0, np.sign(E) * (rn_div_pow2(mag, np.maximum(extra, 1)) << extra), E)
    assert (np.abs(Er) * R < (np.int64(1) << 62)).all()
    # fma(e, r, r) = RN(R + Er R / 2^47), rounded to the grid of R (the result stays in the binade, or is exactly 2^24).  The sum is
    # rounded in two exact pieces: R is an integer, so the fraction and a tie are those of Er R / 2^47 alone, and a tie goes to the
    # neighbour that makes R + q even
    n = Er * R
    q = n >> 47                                              # floor
    r = n - (q << 47)
    half = np.int64(1) << 46
    up = (r > half) | ((r == half) & (((R + q) & 1) == 1))
    return R + q + up.astype(np.int64), exact


def test_first_fma_is_exact_from_a_bracketing_seed():
    for seed in (LO, UP):
        _, exact = newton(seed)
        assert exact.all()
        assert (np.abs(ONE - X * seed) < (1 << 24)).all()


def test_one_step_from_a_bracketing_seed_is_correctly_rounded():
    want = rn_quotient()
    up, _ = newton(UP)
    assert np.array_equal(up, want)                                   # upper neighbour: every significand
    lo, _ = newton(LO)
    wrong = X[lo != want]
    assert wrong.tolist() == [ALL_ONES]                               # lower neighbour: all-ones significand only


def test_one_step_from_outside_the_bracket_is_not_enough():
    want = rn_quotient()
    bad = 0
    for seed in (LO - 1, UP + 1):
        r, _ = newton(seed)
        bad += int((r != want).sum())
    assert bad > 1                                                    # so the seed's quality is a real precondition


def test_two_steps_from_any_seed_within_3_ulp_are_correctly_rounded():
    want = rn_quotient()
    for d in range(-3, 5):                                            # LO - 3 .. LO, UP .. UP + 3
        seed = LO + d
        ok = seed <= (1 << 24)                                        # above 1.0 the floats are twice as far apart: not a seed "within 3 ulp"
        r1, _ = newton(np.where(ok, seed, LO))
        r2, _ = newton(r1)
        wrong = X[ok & (r2 != want)]
        assert set(wrong.tolist()) <= {ALL_ONES}, (d, wrong[:8])
