"""NumPy float32 restatement of the point-to-mesh distance rule (include/badslam_hip.h "Surface evaluation",
csrc/distance_kernels.hpp), brute force: the box predicate of every point against every triangle, no grid, no sorting.  The GPU
tests compare the kernels with this, bit for bit.  Also: the grid's own binning (for the entry count), an independent float64
closest-point-on-triangle, and the sphere and points both test files use."""
import numpy as np

from tests import fusion_util as fu
from tests.fusion_util import fma32

F = np.float32
NO_TRIANGLE = 0xFFFFFFFF


def dot(a, b):
    return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def cross(a, b):
    """csrc/device_math.hpp: unfused components, in the order written there."""
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], b[..., 0] * a[..., 2] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], -1)


def seg(p, a, b):
    e, w = b - a, p - a
    ee, we = dot(e, e), dot(w, e)
    t = np.where(ee > 0, we / ee, F(0))
    t = np.where(t < 0, F(0), np.where(t > 1, F(1), t)).astype(F)
    q = fma32(-t[..., None], e, w)
    return dot(q, q)


def face(p, a, b, c):
    """(value, there is a face term)."""
    u, v, w = b - a, c - a, p - a
    n = cross(u, v)
    nn = dot(n, n)
    has = (nn > 0) & (dot(cross(u, w), n) >= 0) & (dot(cross(c - b, p - b), n) >= 0) & (dot(cross(a - c, p - c), n) >= 0)
    d = dot(w, n) / np.sqrt(nn)
    return d * d, has


def pair_d2(p, a, b, c):
    """d2 of the rule for arrays of pairs [..., 3]: the minimum of the three segments and the face term; a NaN is no value."""
    with np.errstate(all="ignore"):
        m = np.full(p.shape[:-1], np.inf, F)
        for s in (seg(p, a, b), seg(p, b, c), seg(p, c, a)):
            m = np.where(s < m, s, m)
        f, has = face(p, a, b, c)
        return np.where(has & (f < m), f, m).astype(F)


def dilated_boxes(positions, triangles, R):
    """(valid [T], lo - R [T, 3], hi + R [T, 3]) in float32."""
    tri = np.asarray(positions, F).reshape(-1, 3)[np.asarray(triangles, np.int64).reshape(-1, 3)]            # [T, 3 vertices, 3]
    valid = np.isfinite(tri).all(axis=(1, 2))
    with np.errstate(all="ignore"):
        return valid, (tri.min(axis=1) - F(R)).astype(F), (tri.max(axis=1) + F(R)).astype(F)


def point_mesh_distance(points, positions, triangles, R):
    """-> (distance f32 [N], triangle u32 [N]): the rule, over all N x T pairs."""
    points = np.asarray(points, F).reshape(-1, 3)
    positions = np.asarray(positions, F).reshape(-1, 3)
    triangles = np.asarray(triangles, np.int64).reshape(-1, 3)
    N = len(points)
    best = np.full(N, np.inf, F)
    which = np.full(N, NO_TRIANGLE, np.int64)
    if len(triangles) and N:
        valid, lo, hi = dilated_boxes(positions, triangles, R)
        with np.errstate(all="ignore"):
            candidate = valid[None, :] & ((points[:, None, :] >= lo[None]) & (points[:, None, :] <= hi[None])).all(-1)
        pi, ti = np.nonzero(candidate)                                                                         # ti ascends within a point
        tri = positions[triangles[ti]]
        d2 = pair_d2(points[pi], tri[:, 0], tri[:, 1], tri[:, 2])
        np.minimum.at(best, pi, d2)
        attains = d2 == best[pi]
        np.minimum.at(which, pi[attains], ti[attains])                                                        # the lowest index
    hit = best <= F(R) * F(R)
    with np.errstate(all="ignore"):
        return np.where(hit, np.sqrt(best), F(np.inf)).astype(F), np.where(hit, which, NO_TRIANGLE).astype(np.uint32)


def grid_census(positions, triangles, R, cell_size):
    """(cells, (triangle, cell) entries) of the uniform grid as the header defines it."""
    valid, lo, hi = dilated_boxes(positions, triangles, R)
    if not valid.any():
        return 0, 0
    lo, hi = lo[valid], hi[valid]
    origin = lo.min(axis=0)
    inv = F(1) / F(cell_size)
    first, last = np.floor((lo - origin) * inv).astype(np.int64), np.floor((hi - origin) * inv).astype(np.int64)
    return int(np.prod(last.max(axis=0) + 1)), int(np.prod(last - first + 1, axis=1).sum())


# ----------------------------------------------------------------------------- an independent float64 reference

def distances64(points, positions, triangles):
    """[N, T] float64 distances of every point to every triangle (fp32 inputs taken as they are): the closest point by the region
    form of Ericson, Real-Time Collision Detection 5.1.5 -- vertex regions, edge regions, face -- one row of points at a time."""
    points, positions = np.asarray(points, np.float64), np.asarray(positions, np.float64)
    tri = positions[np.asarray(triangles, np.int64).reshape(-1, 3)]
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    ab, ac = b - a, c - a
    rows = lambda u, v: np.einsum("ij,ij->i", u, v)
    out = np.empty((len(points), len(tri)))
    with np.errstate(all="ignore"):
        for i, p in enumerate(points):
            ap, bp, cp = p - a, p - b, p - c
            d1, d2, d3, d4, d5, d6 = rows(ab, ap), rows(ac, ap), rows(ab, bp), rows(ac, bp), rows(ab, cp), rows(ac, cp)
            vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
            denom = 1.0 / (va + vb + vc)
            conditions = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                          (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
            closest = [a, b, a + (d1 / (d1 - d3))[:, None] * ab, c, a + (d2 / (d2 - d6))[:, None] * ac,
                       b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None] * (c - b)]
            q = a + ab * (vb * denom)[:, None] + ac * (vc * denom)[:, None]
            for cond, point in reversed(list(zip(conditions, closest))):
                q = np.where(cond[:, None], point, q)
            out[i] = np.linalg.norm(p - q, axis=1)
    return out


# ----------------------------------------------------------------------------- the sphere and its points

SPHERE_CENTRE, SPHERE_RADIUS = (16.3, 15.1, 14.2), 9.7


def sphere_mesh():
    """The sphere of fusion_util.sphere_field() through the surface-nets restatement: 1 774 vertices, 3 544 triangles, voxel units."""
    field = fu.sphere_field()
    positions, _, _, triangles = fu.extract_mesh(field, np.ones(field.shape, np.uint32), None, np.zeros(3, F), 1.0, 1)
    return np.ascontiguousarray(positions, F), np.ascontiguousarray(triangles, np.uint32)


def sphere_points(positions, triangles, seed=7):
    """680 points: 600 on random rays from the centre at radius 9.7 +- 3, the first 40 vertices, and the midpoints of 40 triangles'
    first edges (every 88th triangle)."""
    rng = np.random.default_rng(seed)
    rays = rng.standard_normal((600, 3))
    rays /= np.linalg.norm(rays, axis=1, keepdims=True)
    radius = SPHERE_RADIUS + rng.uniform(-3.0, 3.0, 600)
    random = (np.array(SPHERE_CENTRE) + rays * radius[:, None]).astype(F)
    chosen = triangles[::88][:40].astype(np.int64)
    mid = (F(0.5) * (positions[chosen[:, 0]] + positions[chosen[:, 1]])).astype(F)
    return np.ascontiguousarray(np.concatenate([random, positions[:40], mid]), F)
