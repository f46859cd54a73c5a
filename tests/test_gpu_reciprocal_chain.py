"""-m gpu: rcp_rn_midrange (csrc/device_math.hpp) equals the IEEE quotient 1.0f / x for EVERY float a surfel depth can be in a
bundle-adjustment kernel: all 2^23 significands at each biased exponent 117 .. 134 (2^-10 .. 2^7 m), and one exponent of negative
values, through probe kind 7 of bslam_debug_jacobians, one exponent (about 100 MB) per call.

Only the equality with the quotient is asserted.  Why it holds is Markstein's theorem (tests/test_reciprocal_chain_cpu.py): it
needs the hardware seed v_rcp_f32 to be one of the two floats that bracket 1 / x.  Probe kind 8 returns the raw seed and one and
two Newton steps from it; test_seed_census prints what the seed is on this device.

Measured on MI355X (gfx950), the 2^23 - 1 significands other than 1.0 at biased exponent 127 (profiles/r09a_rcp_seed.txt):
the seed is ALWAYS a bracketing float -- the lower neighbour of 1 / x for 4 820 636 significands, the upper for 3 567 971, and the
upper one for the all-ones significand 0xffffff; one Newton step is wrong for 0 significands, two steps for 0.
"""
import ctypes as C

import numpy as np
import pytest

import badslam_amd

pytestmark = pytest.mark.gpu

MANT = np.arange(1 << 23, dtype=np.uint32)


@pytest.fixture(scope="module")
def probe():
    ctx = badslam_amd.Context(0)
    L = badslam_amd.lib()

    def run(kind, x, width):
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros((x.size, width), np.float32)
        badslam_amd.check(L.bslam_debug_jacobians(ctx.handle, None, kind, x.size, x.ctypes.data_as(C.POINTER(C.c_float)),
                                                  out.ctypes.data_as(C.POINTER(C.c_float))))
        return out
    run.ctx = ctx
    return run


def floats(exp, sign=0):
    return (MANT | np.uint32(exp << 23) | np.uint32(sign << 31)).view(np.float32)


@pytest.mark.parametrize("exp,sign", [(e, 0) for e in range(117, 135)] + [(127, 1)])
def test_reciprocal_equals_the_quotient(probe, exp, sign):
    x = floats(exp, sign)
    out = probe(7, x, 2)
    want = (np.float32(1) / x).astype(np.float32)
    bad = np.flatnonzero(out[:, 0].view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (exp, sign, bad.size, [hex(int(m)) for m in MANT[bad[:8]]])
    assert np.array_equal(out[:, 1].view(np.uint32), want.view(np.uint32))     # the compiler's own division agrees with numpy's


def seed_census(probe, exp=127):
    """Where the raw seed lies relative to the two floats bracketing 1 / x, and how one and two Newton steps from it do."""
    x = floats(exp)[1:]                                    # x = 2^k is exact: no bracket
    out = probe(8, x, 3)
    want = (np.float32(1) / x).astype(np.float32)
    x64, r64 = x.astype(np.float64), out[:, 0].astype(np.float64)
    lo = np.where(want.astype(np.float64) * x64 <= 1.0, want, np.nextafter(want, np.float32(0)))   # largest float <= 1 / x (product exact in fp64)
    pos = (out[:, 0].view(np.int32).astype(np.int64) - lo.view(np.int32).astype(np.int64))          # 0: lower neighbour, 1: upper
    assert (np.abs(r64 * x64 - 1.0) < 2.0 ** -20).all()
    ones = x.view(np.uint32) & 0x7fffff == 0x7fffff
    return {
        "seed_minus_lower_neighbour_in_ulp": {int(k): int(v) for k, v in zip(*np.unique(pos, return_counts=True))},
        "all_ones_significand_seed": int(pos[ones][0]),
        "one_step_wrong": int((out[:, 1].view(np.uint32) != want.view(np.uint32)).sum()),
        "one_step_wrong_significands": [hex(int(m) | 0x800000) for m in (x.view(np.uint32) & 0x7fffff)[out[:, 1].view(np.uint32) != want.view(np.uint32)][:16]],
        "two_steps_wrong": int((out[:, 2].view(np.uint32) != want.view(np.uint32)).sum()),
        "two_steps_wrong_significands": [hex(int(m) | 0x800000) for m in (x.view(np.uint32) & 0x7fffff)[out[:, 2].view(np.uint32) != want.view(np.uint32)][:16]],
    }


def test_seed_census(probe):
    """The explanation, not the contract: printed (pytest -s); asserted is only that the probe's own Newton steps are the ones the
    formula gives from the seed it returns, so that the printed figures describe the chain the kernels run."""
    census = seed_census(probe)
    print("rcp seed census:", census)
    x = floats(127)[1:]
    steps = probe(8, x, 3).astype(np.float64)
    x64 = x.astype(np.float64)
    e0 = (1.0 - x64 * steps[:, 0]).astype(np.float32).astype(np.float64)          # x r0 is exact in fp64, and so is 1 - it
    assert np.abs(steps[:, 1] - (steps[:, 0] + e0 * steps[:, 0])).max() <= 2.0 ** -24
