"""-m gpu: the photometric pose and geometry kernels in both texture modes.  The mode is a property of the context
(bslam_set_texture_mode) that every launch reads afresh -- today as a wave-uniform branch inside the kernels; a per-mode
instantiation chosen at launch (tried and measured slower) has to pass the same checks.

On the smallest stack that uses the per-surfel work order (K = 8 dense: one chunk, two keyframes per wave), for both modes:
  (i)   H / b of bslam_accumulate_pose_coeffs_batched against the oracle's coefficients in the same mode (1e-4 of the largest
        entry, the bound of tests/test_gpu_large_configs.py), residual counts equal;
  (ii)  a context that ran mode A, then B, then A returns the first result's bits: the dispatch follows bslam_set_texture_mode;
  (iii) the two modes differ somewhere: two kernels did run;
  (iv)  one photometric geometry iteration in each mode leaves the surfel rows of a context that never saw the other mode."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi, synthetic
from tests.test_gpu_pose_rows import Runner, bits

pytestmark = pytest.mark.gpu
P = C.POINTER
MODES = (abi.TEX_FIXED_POINT_1_8, abi.TEX_EXACT_FLOAT)
K = 8


@pytest.fixture(scope="module")
def dev():
    d = synthetic.TorchStack(K, "cuda:0", kind="dense", border_valid=True)
    assert d.surfels_size >= 64 * 256                      # the per-surfel work order is in use
    rng = np.random.default_rng(11)
    pix = 1.0 / 525.0
    d.xis = [np.concatenate([rng.uniform(-1, 1, 3) * 0.002, rng.uniform(-1, 1, 3) * pix]) for _ in range(K)]
    return d


def fresh_runner(dev, mode=None):
    run = Runner(dev)
    if mode is not None:
        run.ctx.set_texture_mode(mode)
    return run


@pytest.fixture(scope="module")
def per_mode(dev):
    """H / b and counts of each mode, each from a context of its own that never saw the other mode."""
    out = {}
    for mode in MODES:
        run = fresh_runner(dev, mode)
        out[mode] = run.coeffs(run.views(dev.xis))
    return out


def oracle_coefficients(dev, k, surf, tex_mode):
    from tests import bso
    L = bso.lib()
    cf = bso.np_buffer2d(dev.stack.cfactor)
    dp = abi.DepthParams(cf, 0.0, float(dev.stack.raw_to_float_depth), dev.stack.baseline_fx, dev.stack.cell)
    depth, normals, radius, color = dev.host_keyframe(k)
    _, M, _ = dev.stack.pose(k, dev.xis[k])
    H, b = np.zeros(21, np.float32), np.zeros(6, np.float32)
    H64, b64 = np.zeros(21, np.float64), np.zeros(6, np.float64)
    count, cost = C.c_uint32(), C.c_float()
    L.bso_accumulate_pose_estimation_coeffs(1, 1, C.byref(dev.stack.camera), C.byref(dev.stack.camera), C.byref(dp), C.byref(bso.np_buffer2d(depth)),
                                            C.byref(bso.np_buffer2d(normals)), C.byref(bso.np_buffer2d(color)), C.byref(M), dev.surfels_size,
                                            C.byref(bso.np_buffer2d(surf)), tex_mode, C.byref(count), C.byref(cost), bso.fptr(H), bso.fptr(b),
                                            H64.ctypes.data_as(P(C.c_double)), b64.ctypes.data_as(P(C.c_double)), None)
    return H64, b64, count.value


@pytest.mark.parametrize("mode", MODES)
def test_pose_coefficients_match_the_oracle_in_the_same_mode(oracle, dev, per_mode, mode):
    Hb, counts = per_mode[mode]
    surf = np.ascontiguousarray(dev.surfels.cpu().numpy())
    for k in range(K):
        H64, b64, count = oracle_coefficients(dev, k, surf, mode)
        assert count == counts[k] and count > 1000, (k, count, counts[k])
        assert np.abs(Hb[k, :21] - H64).max() <= 1e-4 * np.abs(H64).max(), k
        assert np.abs(Hb[k, 21:27] - b64).max() <= 1e-4 * max(np.abs(b64).max(), 1e-3 * np.abs(H64).max()), k


def test_dispatch_follows_the_context_mode(dev, per_mode):
    a, b = MODES
    run = fresh_runner(dev)                                   # the default mode is the fixed-point one
    kfs = run.views(dev.xis)
    first = run.coeffs(kfs)
    assert np.array_equal(bits(first[0]), bits(per_mode[a][0])) and np.array_equal(first[1], per_mode[a][1])
    run.ctx.set_texture_mode(b)
    second = run.coeffs(kfs)
    assert np.array_equal(bits(second[0]), bits(per_mode[b][0])) and np.array_equal(second[1], per_mode[b][1])
    run.ctx.set_texture_mode(a)
    third = run.coeffs(kfs)
    assert np.array_equal(bits(third[0]), bits(first[0])) and np.array_equal(third[1], first[1])


def test_the_two_modes_differ(per_mode):
    a, b = MODES
    assert not np.array_equal(bits(per_mode[a][0]), bits(per_mode[b][0]))     # both filters ran


def geometry_rows(dev, run, kfs):
    """The surfel rows after one photometric geometry iteration on a copy of the stack's surfels."""
    import torch
    surfels = dev.surfels.clone()
    dp, sb, ab = dev.depth_params(), dev.buf(surfels), dev.buf(dev.active)
    badslam_amd.check(run.L.bslam_optimize_geometry_iteration(run.ctx.handle, run.stream, 1, 1, C.byref(run.cam), C.byref(run.cam), C.byref(dp), K, kfs,
                                                              dev.surfels_size, C.byref(sb), C.byref(ab)))
    torch.cuda.synchronize()
    return surfels.cpu().numpy()


def test_geometry_iteration_per_mode(dev):
    a, b = MODES
    alone = {}
    for mode in MODES:
        run = fresh_runner(dev, mode)
        alone[mode] = geometry_rows(dev, run, run.views(dev.xis))
    assert not np.array_equal(bits(alone[a]), bits(alone[b]))             # the descriptor rows depend on the filter
    assert not np.array_equal(bits(alone[a]), bits(dev.surfels.cpu().numpy()))   # and the iteration did move the surfels
    run = fresh_runner(dev)
    kfs = run.views(dev.xis)
    for mode in (a, b, a):
        run.ctx.set_texture_mode(mode)
        assert np.array_equal(bits(geometry_rows(dev, run, kfs)), bits(alone[mode])), mode
