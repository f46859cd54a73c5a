"""-m gpu: the photometric pose kernel's descriptor normal equations on the device arithmetic (C-ABI probe bslam_debug_desc_pair).

accumulate_h_b_desc_pair forms the two descriptor rows of a pair as ONE rank-two update A^T G A, A^T h
(tests/test_desc_pair_normal_equations_cpu.py holds the identity in float64).  Here both device forms -- the rank-two one and the
two descriptor_pose_jacobian + accumulate_h_b rows it replaces in the pose kernel -- are evaluated in fp32 on the same points and
compared with the float64 value of the two-row formulas.

Bar: the rank-two form's worst error (per point, relative to the point's largest H resp. b entry) may be at most 2 x the
two-row form's worst error on the same inputs.  The two-row form is the arithmetic the kernel used before and is not the code
under test; the margin of 2 is there because the two forms round different intermediate products (the rank-two form has one more
level of products: G, then G A, then A^T (G A)).  Measured on an MI355X on these inputs (4096 points, seed 21):
two-row form 5.576e-07 (H) / 2.168e-06 (b), rank-two form 3.506e-07 (H) / 1.710e-06 (b) -- ratios 0.63 and 0.79 (b is the
larger figure in both forms because the two residuals' terms of a b entry may cancel).

The wave-uniform Huber path (desc_weights_pair) must return desc_weight's bits: kDescWeight where a whole wave's residuals lie
below kDescHuber (the branch not taken), and the per-lane weights where some do not."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from tests import desc_pair_fixtures as F

pytestmark = pytest.mark.gpu
P = C.POINTER


def probe(points):
    x = np.ascontiguousarray(points, np.float32)
    assert x.ndim == 2 and x.shape[1] == 9
    out = np.zeros((x.shape[0], 58), np.float32)
    ctx = badslam_amd.Context(0)
    badslam_amd.check(badslam_amd.lib().bslam_debug_desc_pair(ctx.handle, None, x.shape[0], x.ctypes.data_as(P(C.c_float)), out.ctypes.data_as(P(C.c_float))))
    return x, out


def worst_errors(got, want):
    """(H, b): largest error over the points, each point relative to its largest H resp. b entry."""
    res = []
    for cols in (slice(0, 21), slice(21, 27)):
        scale = np.abs(want[:, cols]).max(axis=1, keepdims=True)
        res.append(float((np.abs(got[:, cols].astype(np.float64) - want[:, cols]) / scale).max()))
    return res


def test_rank_two_form_is_as_accurate_as_the_two_rows():
    x, out = probe(F.random_points(4096, seed=21))
    want = F.two_row_form(x.astype(np.float64))
    assert np.isfinite(out).all()
    pair, rows = worst_errors(out[:, :27], want), worst_errors(out[:, 27:54], want)
    print("worst relative error (H, b): two-row form %.3e %.3e, rank-two form %.3e %.3e" % (rows[0], rows[1], pair[0], pair[1]))
    assert pair[0] <= 2.0 * rows[0], (pair, rows)
    assert pair[1] <= 2.0 * rows[1], (pair, rows)


def test_uniform_huber_path_below_the_threshold_returns_the_constant():
    p = F.random_points(1024, seed=22, huber_fraction=0.0)
    assert (np.abs(p[:, [5, 8]]) < F.K_DESC_HUBER).all()
    _, out = probe(p)
    const = np.float32(1.0) * np.float32(F.K_DESC_WEIGHT)
    assert np.all(out[:, 54:56].view(np.uint32) == const.view(np.uint32))
    assert np.array_equal(out[:, 54:56].view(np.uint32), out[:, 56:58].view(np.uint32))


def test_uniform_huber_path_with_mixed_lanes_equals_the_per_lane_weights():
    p = F.random_points(4096, seed=23, huber_fraction=0.25)
    # one wave (64 consecutive points) with a single lane above the threshold, one with every lane above it
    p[1024:1088, 5] = 0.5
    p[1024:1088, 8] = -0.25
    p[1024 + 17, 8] = -37.0
    p[2048:2112, 5] = 25.0
    x, out = probe(p)
    assert np.array_equal(out[:, 54:56].view(np.uint32), out[:, 56:58].view(np.uint32))
    want = F.desc_weight(x[:, [5, 8]].astype(np.float64))
    assert (np.abs(out[:, 54:56] - want) / want).max() < 1e-6      # the 1-ulp reciprocal and two roundings
    big = np.abs(x[:, [5, 8]]) >= F.K_DESC_HUBER
    assert big.any() and (~big).any()
    assert np.all(out[:, 54:56][~big].view(np.uint32) == (np.float32(1.0) * np.float32(F.K_DESC_WEIGHT)).view(np.uint32))
