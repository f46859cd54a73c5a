"""Inputs and float64 forms of the descriptor normal equations of one (surfel, keyframe) pair, shared by
tests/test_desc_pair_normal_equations_cpu.py and tests/test_gpu_desc_pair_probe.py.

A point is [ls(3), gx1, gy1, r1, gx2, gy2, r2]: the surfel position in the frame and the two descriptor residuals with their
image gradients times the colour camera's fx, fy -- the layout of the C-ABI probe bslam_debug_desc_pair."""
import numpy as np

K_DESC_WEIGHT = 1e-2
K_DESC_HUBER = 10.0
Z_RANGE = (0.3, 6.0)   # the depth range of the stacks (the AddKeyframe limits bench.py uses)


def random_points(n, seed, huber_fraction=0.25):
    """ls inside a 90-degree frustum at z in Z_RANGE; gradients of a few hundred (texel differences in [-1, 1] times a focal
    length of some hundred pixels); residuals in [-1, 1] of the descriptor range 180, a fraction beyond +-kDescHuber."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(*Z_RANGE, n)
    p = np.empty((n, 9))
    p[:, 0] = rng.uniform(-1, 1, n) * z
    p[:, 1] = rng.uniform(-1, 1, n) * z
    p[:, 2] = z
    for c in (3, 4, 6, 7):
        p[:, c] = rng.uniform(-1, 1, n) * 525.0
    for c in (5, 8):
        r = rng.uniform(-K_DESC_HUBER, K_DESC_HUBER, n) * 0.999
        big = rng.random(n) < huber_fraction
        r[big] = rng.choice([-1.0, 1.0], big.sum()) * rng.uniform(K_DESC_HUBER, 180.0, big.sum())
        p[:, c] = r
    return p


def desc_weight(r):
    a = np.abs(r)
    return K_DESC_WEIGHT * np.where(a < K_DESC_HUBER, 1.0, K_DESC_HUBER / np.maximum(a, 1e-300))


def jacobian_rows(gx, gy, ls):
    """The six formulas of descriptor_pose_jacobian (csrc/device_math.hpp) as written, float64; [n, 6]."""
    x, y, z = ls[:, 0], ls[:, 1], ls[:, 2]
    iz = 1.0 / z
    z2 = z * z
    iz2 = iz * iz
    xy = x * y
    return np.stack([-gx * iz, -gy * iz, (x * gx + y * gy) * iz2, ((y * y + z2) * gy + xy * gx) * iz2,
                     -((x * x + z2) * gx + xy * gy) * iz2, -(x * gy - y * gx) * iz], axis=1)


TRIU = np.triu_indices(6)   # row-major upper triangle: the order of the 21 H columns


def two_row_form(p):
    """sum over the two residuals of w J^T J (upper triangle, 21) and w r J (6): [n, 27], float64."""
    out = np.zeros((p.shape[0], 27))
    for gx, gy, r in ((3, 4, 5), (6, 7, 8)):
        J = jacobian_rows(p[:, gx], p[:, gy], p[:, :3])
        w = desc_weight(p[:, r])
        H = w[:, None, None] * J[:, :, None] * J[:, None, :]
        out[:, :21] += H[:, TRIU[0], TRIU[1]]
        out[:, 21:] += (w * p[:, r])[:, None] * J
    return out


def pair_form(p):
    """A^T G A (upper triangle, 21) and A^T h (6) with the 2 x 6 factor A of the pair: [n, 27], float64."""
    n = p.shape[0]
    iz = 1.0 / p[:, 2]
    u, v = p[:, 0] * iz, p[:, 1] * iz
    zero = np.zeros(n)
    A = np.stack([np.stack([-iz, zero, u * iz, u * v, -(1 + u * u), v], axis=1),
                  np.stack([zero, -iz, v * iz, 1 + v * v, -u * v, -u], axis=1)], axis=1)          # [n, 2, 6]
    G = np.zeros((n, 2, 2))
    h = np.zeros((n, 2))
    for gx, gy, r in ((3, 4, 5), (6, 7, 8)):
        g = p[:, [gx, gy]]
        w = desc_weight(p[:, r])
        G += w[:, None, None] * g[:, :, None] * g[:, None, :]
        h += (w * p[:, r])[:, None] * g
    H = np.einsum("nki,nkl,nlj->nij", A, G, A)
    b = np.einsum("nki,nk->ni", A, h)
    return np.concatenate([H[:, TRIU[0], TRIU[1]], b], axis=1)
