"""NumPy restatement of the surface sampling rule (include/badslam_hip.h "Surface sampling", csrc/sampling_kernels.hpp), brute
force: uint32 hashing and float32 arithmetic per triangle and per sample, no scan and no search.  The GPU tests compare the kernels
with this, bit for bit.  Also: the float64 areas, the count bound, and the wall and the strip both test files use."""
import numpy as np

from tests import point_mesh_util as pm
from tests.fusion_util import fma32

F = np.float32
U = np.uint32
ONE = 1 << 24
MAX_SAMPLES = (1 << 32) - 256


def mix(x):
    x = np.asarray(x, U).copy()
    x ^= x >> U(16)
    x *= U(0x7feb352d)
    x ^= x >> U(15)
    x *= U(0x846ca68b)
    x ^= x >> U(16)
    return x


def h(seed, s, t, j):
    """h(s, t, j) of the rule for arrays t, j; uint32 with wrap-around."""
    with np.errstate(over="ignore"):
        base = U((int(seed) + int(s) * 0x9e3779b9) & 0xFFFFFFFF)
        return mix(mix(base ^ mix(t)) + np.asarray(j, U))


def u24(x):
    return x >> U(8)


def triangle_frames(positions, triangles):
    """(a, u, v, n, nn, valid) in float32 for every triangle; valid: nine finite coordinates and nn > 0."""
    positions = np.asarray(positions, F).reshape(-1, 3)
    tri = positions[np.asarray(triangles, np.int64).reshape(-1, 3)]
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    with np.errstate(all="ignore"):
        u, v = b - a, c - a
        n = pm.cross(u, v)
        nn = pm.dot(n, n)
        valid = np.isfinite(tri).all(axis=(1, 2)) & (nn > 0)
    return a, u, v, n, nn, valid


def expected_counts(positions, triangles, density):
    """x = area * density in float32 per triangle (0 where the triangle yields nothing)."""
    _, _, _, _, nn, valid = triangle_frames(positions, triangles)
    with np.errstate(all="ignore"):
        x = (F(0.5) * np.sqrt(nn)) * F(density)
    return np.where(valid, x, F(0)).astype(F)


def counts(positions, triangles, density, seed):
    """The number of samples per triangle, as Python-sized integers (int64; 2^32 where x is not below it)."""
    triangles = np.asarray(triangles, np.int64).reshape(-1, 3)
    T = len(triangles)
    if T == 0:
        return np.zeros(0, np.int64)
    _, _, _, _, nn, valid = triangle_frames(positions, triangles)
    with np.errstate(all="ignore"):
        x = (F(0.5) * np.sqrt(nn)) * F(density)
        huge = ~(x < F(4294967296.0))
        k = np.floor(np.where(huge, F(0), x)).astype(F)
        r = u24(h(seed, 0, np.arange(T, dtype=U), np.zeros(T, U))).astype(F) * F(2.0 ** -24)
        n = k.astype(np.int64) + (r < x - k)
    return np.where(valid, np.where(huge, np.int64(1) << 32, n), 0).astype(np.int64)


def sample_mesh(positions, triangles, density, seed):
    """-> (points f32 [N, 3], normals f32 [N, 3], triangle u32 [N]) ordered by (triangle, j)."""
    triangles = np.asarray(triangles, np.int64).reshape(-1, 3)
    count = counts(positions, triangles, density, seed)
    N = int(count.sum())
    assert N <= MAX_SAMPLES, "the call refuses this total"
    t = np.repeat(np.arange(len(triangles), dtype=np.int64), count)
    j = np.arange(N, dtype=np.int64) - np.repeat(np.cumsum(count) - count, count)
    if N == 0:
        return np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros(0, U)
    a, u, v, n, nn, _ = triangle_frames(positions, triangles)
    i1, i2 = u24(h(seed, 1, t.astype(U), j.astype(U))).astype(np.int64), u24(h(seed, 2, t.astype(U), j.astype(U))).astype(np.int64)
    return place(a[t], u[t], v[t], i1, i2), (n[t] / np.sqrt(nn[t])[:, None]).astype(F), t.astype(U)


def place(a, u, v, i1, i2):
    """The point of the fixed-point coordinates (i1, i2) in [0, 2^24) each: the reflection, then two fused multiply-adds per axis."""
    i1, i2 = np.asarray(i1, np.int64), np.asarray(i2, np.int64)
    over = i1 + i2 > ONE
    i1, i2 = np.where(over, ONE - i1, i1), np.where(over, ONE - i2, i2)
    w1, w2 = (i1.astype(F) * F(2.0 ** -24))[:, None], (i2.astype(F) * F(2.0 ** -24))[:, None]
    return fma32(w2, v, fma32(w1, u, a))


# ----------------------------------------------------------------------------- float64 measures

def areas64(positions, triangles):
    tri = np.asarray(positions, np.float64).reshape(-1, 3)[np.asarray(triangles, np.int64).reshape(-1, 3)]
    return 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)


def count_bound(x):
    """4 standard deviations of the sum of the rounding draws: one Bernoulli(f) per triangle, f the fractional part of x."""
    f = np.asarray(x, np.float64) - np.floor(np.asarray(x, np.float64))
    return 4.0 * np.sqrt((f * (1.0 - f)).sum())


# ----------------------------------------------------------------------------- the wall and the strip

def wall(size=1.0):
    """A square of two triangles in the plane z = 0."""
    s = F(size)
    return np.array([[0, 0, 0], [s, 0, 0], [s, s, 0], [0, s, 0]], F), np.array([[0, 1, 2], [0, 2, 3]], U)


STRIP_WIDTH, STRIP_HEIGHT = 0.6, 0.003


def strip():
    """A grid mesh over x in [0, 0.6], y in [0, 1] at 2 cm, lying at z = 3 mm: 31 x 51 vertices, 3 000 triangles."""
    nx, ny = 31, 51
    x, y = np.meshgrid(np.arange(nx) * 0.02, np.arange(ny) * 0.02, indexing="xy")
    positions = np.stack([x, y, np.full_like(x, STRIP_HEIGHT)], -1).reshape(-1, 3).astype(F)
    i = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)[None, :]).reshape(-1)
    triangles = np.concatenate([np.stack([i, i + 1, i + nx + 1], -1), np.stack([i, i + nx + 1, i + nx], -1)]).astype(U)
    return positions, triangles


def wall_to_strip_distance(points):
    """Closed form, float64: the distance of points of the wall (z = 0, inside [0, 1]^2) to the strip."""
    x = np.asarray(points, np.float64)[:, 0]
    z0 = float(F(STRIP_HEIGHT))
    edge = float(F(30 * 0.02))
    return np.where(x <= edge, z0, np.sqrt((x - edge) ** 2 + z0 ** 2))


RECALL_THRESHOLD = 0.01
ANALYTIC_RECALL = STRIP_WIDTH + np.sqrt(RECALL_THRESHOLD ** 2 - STRIP_HEIGHT ** 2)   # 0.60954: the share of the wall within 1 cm of the strip
EVAL_DENSITY, EVAL_SEED = 1e4, 1                                                    # test_sample_mesh_cpu.py asserts that no sample lies on a threshold
EVAL_THRESHOLDS = (0.01, 0.02, 0.05)
