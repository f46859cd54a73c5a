"""The identity behind accumulate_h_b_desc_pair (csrc/device_math.hpp), in float64: both descriptor rows of a pair are built from
the same point, J_r = gx_r a0 + gy_r a1, so the pair's normal equations are A^T G A and A^T h with one 2 x 6 factor A.  Checked
against the sum of the two rank-one rows built from the formulas of descriptor_pose_jacobian as written.  An algebraic identity:
the bar is float64 rounding."""
import numpy as np

from tests import desc_pair_fixtures as F


def test_pair_form_equals_the_two_rank_one_rows():
    p = F.random_points(1000, seed=11)
    assert (np.abs(p[:, [5, 8]]) >= F.K_DESC_HUBER).any() and (np.abs(p[:, [5, 8]]) < F.K_DESC_HUBER).any()
    assert p[:, 2].min() >= F.Z_RANGE[0] and p[:, 2].max() <= F.Z_RANGE[1]
    want, got = F.two_row_form(p), F.pair_form(p)
    # per point, relative to the largest entry of H and of b (single entries cancel: u v gx + (1 + v^2) gy may be near zero)
    for cols in (slice(0, 21), slice(21, 27)):
        scale = np.abs(want[:, cols]).max(axis=1, keepdims=True)
        assert (np.abs(got[:, cols] - want[:, cols]) / scale).max() < 1e-12


def test_the_factor_reproduces_each_jacobian_row():
    """J = gx a0 + gy a1 entry by entry (only the three translation columns carry 1 / z)."""
    p = F.random_points(1000, seed=12)
    iz = 1.0 / p[:, 2]
    u, v = p[:, 0] * iz, p[:, 1] * iz
    a0 = np.stack([-iz, 0 * iz, u * iz, u * v, -(1 + u * u), v], axis=1)
    a1 = np.stack([0 * iz, -iz, v * iz, 1 + v * v, -u * v, -u], axis=1)
    J = F.jacobian_rows(p[:, 3], p[:, 4], p[:, :3])
    got = p[:, 3:4] * a0 + p[:, 4:5] * a1
    assert (np.abs(got - J) / np.abs(J).max(axis=1, keepdims=True)).max() < 1e-12
