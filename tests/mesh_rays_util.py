"""NumPy float32 restatement of the mesh-ray rule (include/badslam_hip.h "Mesh rays", csrc/ray_kernels.hpp), brute force over all
N x T pairs: no tree, no sorting, no pruning.  The GPU tests compare the kernels with this, bit for bit.  Also: the float64
Moeller-Trumbore the CPU test measures the rule against, the fixtures both GPU test files use, and a stand-in for DirectBA."""
import numpy as np

from tests import point_mesh_util as pm
from tests.fusion_util import fma32
from tests.nearest_triangle_util import RestatementBA as NearestRestatementBA
from tests.nearest_triangle_util import check_tree, order_key, plane_mesh, triangle_boxes  # noqa: F401  (re-exported for the tests)

F = np.float32
NO_TRIANGLE = 0xFFFFFFFF
NO_VIEW = 0xFFFFFFFF
PAD_ULPS = 4                        # BSLAM_RAY_PAD_ULPS: DESIGN.md 8 "Mesh rays" derives it
INF = F(np.inf)
CHUNK = 64                          # rays per block of the brute force


def pad(x, k):
    """x moved k representable floats up (k > 0) or down (k < 0), never beyond an infinity; -0 counts as +0."""
    with np.errstate(all="ignore"):
        x = (np.asarray(x, F) + F(0)).astype(F)
    key = np.clip(order_key(x).astype(np.int64) + k, 0x007FFFFF, 0xFF800000).astype(np.uint32)
    return np.where(key & 0x80000000, key & 0x7FFFFFFF, ~key).astype(np.uint32).view(F)


def ray_valid(o, d, t_min, t_max):
    """[N] bool: six finite components, a direction that is not zero, bounds that are no NaN and t_min <= t_max."""
    with np.errstate(all="ignore"):
        return np.isfinite(o).all(axis=-1) & np.isfinite(d).all(axis=-1) & (d != 0).any(axis=-1) & (t_min <= t_max)


def ray_axes(d):
    """-> (kx, ky, kz) int arrays [N]: kz the axis of the largest |d| (the first of equals), kx, ky the two behind it in cyclic
    order, swapped where d[kz] < 0."""
    m = np.abs(d)
    kz = np.where((m[:, 0] >= m[:, 1]) & (m[:, 0] >= m[:, 2]), 0, np.where(m[:, 1] >= m[:, 2], 1, 2))
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    negative = np.take_along_axis(d, kz[:, None], 1)[:, 0] < 0
    return np.where(negative, ky, kx), np.where(negative, kx, ky), kz


def _pick(v, k):
    """Component k[n] of v[n, T, 3] -> [n, T]."""
    return np.take_along_axis(v, np.broadcast_to(k[:, None, None], v.shape[:2] + (1,)), 2)[..., 0]


def ray_triangle(o, d, a, b, c):
    """The triangle test for rays o, d [n, 3] against triangles a, b, c [T, 3] (all finite, d != 0):
    -> (accepted [n, T] bool, t, u, v [n, T] f32, front [n, T] bool).  t may be a NaN or infinite where accepted."""
    o, d = np.asarray(o, F), np.asarray(d, F)
    kx, ky, kz = ray_axes(d)
    with np.errstate(all="ignore"):
        dz = np.take_along_axis(d, kz[:, None], 1)[:, 0]
        Sx = (np.take_along_axis(d, kx[:, None], 1)[:, 0] / dz).astype(F)[:, None]
        Sy = (np.take_along_axis(d, ky[:, None], 1)[:, 0] / dz).astype(F)[:, None]
        Sz = (F(1) / dz).astype(F)[:, None]
        sheared = []
        for vertex in (a, b, c):
            rel = (np.asarray(vertex, F)[None, :, :] - o[:, None, :]).astype(F)
            z = _pick(rel, kz)
            sheared.append(((_pick(rel, kx) - (Sx * z).astype(F)).astype(F), (_pick(rel, ky) - (Sy * z).astype(F)).astype(F), (Sz * z).astype(F)))
        (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = sheared
        U = ((Cx * By).astype(F) - (Cy * Bx).astype(F)).astype(F)
        V = ((Ax * Cy).astype(F) - (Ay * Cx).astype(F)).astype(F)
        W = ((Bx * Ay).astype(F) - (By * Ax).astype(F)).astype(F)
        # where an edge function is exactly 0 all three are formed in float64: the difference of two exact products has the exact sign
        D = np.float64
        again = (U == 0) | (V == 0) | (W == 0)
        U64 = np.where(again, Cx.astype(D) * By.astype(D) - Cy.astype(D) * Bx.astype(D), U.astype(D))
        V64 = np.where(again, Ax.astype(D) * Cy.astype(D) - Ay.astype(D) * Cx.astype(D), V.astype(D))
        W64 = np.where(again, Bx.astype(D) * Ay.astype(D) - By.astype(D) * Ax.astype(D), W.astype(D))
        one_sign = ~(((U64 < 0) | (V64 < 0) | (W64 < 0)) & ((U64 > 0) | (V64 > 0) | (W64 > 0)))
        U, V, W = U64.astype(F), V64.astype(F), W64.astype(F)
        det = ((U + V).astype(F) + W).astype(F)
        T = (((U * Az).astype(F) + (V * Bz).astype(F)).astype(F) + (W * Cz).astype(F)).astype(F)
        t = (T / det).astype(F)
        u = (V / det).astype(F)
        v = (W / det).astype(F)
    return one_sign & (det != 0), t, u, v, det > 0


def slab(o, d, lo, hi):
    """(enter, exit) of rays o, d [n, 3] against boxes lo, hi [..., 3] (broadcast against [n, 1, 3]), padded.  Empty iff enter > exit."""
    o, d = np.asarray(o, F)[:, None, :], np.asarray(d, F)[:, None, :]
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    with np.errstate(all="ignore"):
        inv = (F(1) / d).astype(F)
        t0 = ((lo - o).astype(F) * inv).astype(F)
        t1 = ((hi - o).astype(F) * inv).astype(F)
        free = np.isnan(t0) | np.isnan(t1)                                     # 0 x inf: the axis does not constrain
        near = np.where(free, -INF, np.minimum(t0, t1))
        far = np.where(free, INF, np.maximum(t0, t1))
        parallel = np.broadcast_to(d == 0, near.shape)
        inside = (lo <= o) & (o <= hi)
        near = np.where(parallel, np.where(inside, -INF, INF), near).astype(F)
        far = np.where(parallel, np.where(inside, INF, -INF), far).astype(F)
    return pad(near.max(axis=-1), -PAD_ULPS), pad(far.min(axis=-1), PAD_ULPS)


def _t_range(t_range, N):
    if t_range is None:
        return np.zeros(N, F), np.full(N, np.inf, F)
    t_range = np.asarray(t_range, F).reshape(-1, 2)
    return t_range[:, 0].copy(), t_range[:, 1].copy()


def pair_hits(origins, directions, t_range, positions, triangles):
    """-> dict of [N, T] arrays: t (t_hit of the rule, +inf where the pair does not hit), u, v, front."""
    o = np.asarray(origins, F).reshape(-1, 3)
    d = np.asarray(directions, F).reshape(-1, 3)
    N = len(o)
    t_min, t_max = _t_range(t_range, N)
    positions = np.asarray(positions, F).reshape(-1, 3)
    tri = positions[np.asarray(triangles, np.int64).reshape(-1, 3)]
    valid_t, lo, hi = triangle_boxes(positions, triangles)
    T = len(tri)
    out = dict(t=np.full((N, T), np.inf, F), u=np.zeros((N, T), F), v=np.zeros((N, T), F), front=np.zeros((N, T), bool))
    rays = np.flatnonzero(ray_valid(o, d, t_min, t_max))
    tri, lo, hi = tri[valid_t], lo[valid_t], hi[valid_t]
    columns = np.flatnonzero(valid_t)
    if len(columns) == 0:
        return out
    for start in range(0, len(rays), CHUNK):
        r = rays[start:start + CHUNK]
        accepted, t, u, v, front = ray_triangle(o[r], d[r], tri[:, 0], tri[:, 1], tri[:, 2])
        enter, leave = slab(o[r], d[r], lo[None], hi[None])
        with np.errstate(all="ignore"):
            accepted &= ~np.isnan(t) & ~(enter > leave)
            t_hit = np.minimum(np.maximum(np.where(accepted, t, F(0)), enter), leave).astype(F)
            accepted &= (t_hit >= t_min[r, None]) & (t_hit <= t_max[r, None]) & np.isfinite(t_hit)
        block = np.ix_(r, columns)
        out["t"][block] = np.where(accepted, t_hit, INF)
        out["u"][block] = np.where(accepted, u, F(0))
        out["v"][block] = np.where(accepted, v, F(0))
        out["front"][block] = accepted & front
    return out


def closest_hit(origins, directions, t_range, positions, triangles):
    """-> dict of t f32 [N] (+inf: a miss), triangle u32 [N] (0xFFFFFFFF), uv f32 [N, 2], front u8 [N]."""
    N = len(np.asarray(origins).reshape(-1, 3))
    if len(np.asarray(triangles).reshape(-1, 3)) == 0 or N == 0:
        return dict(t=np.full(N, np.inf, F), triangle=np.full(N, NO_TRIANGLE, np.uint32), uv=np.zeros((N, 2), F), front=np.zeros(N, np.uint8))
    pairs = pair_hits(origins, directions, t_range, positions, triangles)
    which = pairs["t"].argmin(axis=1)                                          # the first, that is the lowest, index of the minimum
    rows = np.arange(N)
    t = pairs["t"][rows, which]
    hit = np.isfinite(t)
    return dict(t=t, triangle=np.where(hit, which, NO_TRIANGLE).astype(np.uint32),
                uv=np.stack([pairs["u"][rows, which], pairs["v"][rows, which]], -1).astype(F), front=(pairs["front"][rows, which] & hit).astype(np.uint8))


def any_hit(origins, directions, t_range, positions, triangles):
    """-> u8 [N]: whether some valid triangle hits."""
    N = len(np.asarray(origins).reshape(-1, 3))
    if len(np.asarray(triangles).reshape(-1, 3)) == 0 or N == 0:
        return np.zeros(N, np.uint8)
    return np.isfinite(pair_hits(origins, directions, t_range, positions, triangles)["t"]).any(axis=1).astype(np.uint8)


def transform_rows(camera_T_global, p):
    """L = camera_T_global . p in the row expression of bslam_render_mesh: ((m0 x + m1 y) + m2 z) + m3, nothing fused.  p [N, 3] -> [N, 3]."""
    m = np.asarray(camera_T_global, F).reshape(3, 4)
    p = np.asarray(p, F)
    with np.errstate(all="ignore"):
        return np.stack([((((m[r, 0] * p[:, 0]).astype(F) + (m[r, 1] * p[:, 1]).astype(F)).astype(F) + (m[r, 2] * p[:, 2]).astype(F)).astype(F) + m[r, 3]).astype(F)
                         for r in range(3)], -1)


def visible_pairs(points, normals, positions, triangles, camera_T_global, centres, camera, min_depth, max_depth, margin):
    """[N, K] bool: point n is seen from view k.  camera = (fx, fy, cx, cy, width, height)."""
    p = np.asarray(points, F).reshape(-1, 3)
    views = np.asarray(camera_T_global, F).reshape(-1, 3, 4)
    centres = np.asarray(centres, F).reshape(-1, 3)
    fx, fy, cx, cy = (F(x) for x in camera[:4])
    width, height = F(camera[4]), F(camera[5])
    seen = np.zeros((len(p), len(views)), bool)
    for k in range(len(views)):
        with np.errstate(all="ignore"):
            L = transform_rows(views[k], p)
            px = ((fx * (L[:, 0] / L[:, 2]).astype(F)).astype(F) + cx).astype(F)
            py = ((fy * (L[:, 1] / L[:, 2]).astype(F)).astype(F) + cy).astype(F)
            ok = (L[:, 2] >= F(min_depth)) & (L[:, 2] <= F(max_depth)) & (px >= 0) & (px < width) & (py >= 0) & (py < height)
            d = (p - centres[k][None]).astype(F)
            if normals is not None:
                n = np.asarray(normals, F).reshape(-1, 3)
                ok &= fma32(n[:, 2], d[:, 2], fma32(n[:, 1], d[:, 1], n[:, 0] * d[:, 0])) < 0
            dd = fma32(d[:, 2], d[:, 2], fma32(d[:, 1], d[:, 1], d[:, 0] * d[:, 0]))
            t_max = (F(1) - (F(margin) / np.sqrt(dd).astype(F)).astype(F)).astype(F)
        rows = np.flatnonzero(ok)
        if len(rows):
            t_range = np.stack([np.zeros(len(rows), F), t_max[rows]], -1)
            blocked = any_hit(np.broadcast_to(centres[k], (len(rows), 3)), d[rows], t_range, positions, triangles)
            seen[rows, k] = blocked == 0
    return seen


def visibility(points, normals, positions, triangles, camera_T_global, centres, camera, min_depth, max_depth, margin):
    """-> (count u32 [N], first u32 [N]): the views that see each point and the lowest of them (0xFFFFFFFF: none)."""
    seen = visible_pairs(points, normals, positions, triangles, camera_T_global, centres, camera, min_depth, max_depth, margin)
    count = seen.sum(axis=1).astype(np.uint32)
    first = np.where(count > 0, seen.argmax(axis=1) if seen.shape[1] else 0, NO_VIEW).astype(np.uint32)
    return count, first


def moller_trumbore(o, d, a, b, c):
    """float64: rays [n, 3] against triangles [T, 3] -> (hit [n, T] for t of any sign, t, u, v, front, edge): edge = the smallest of
    u, v, 1 - u - v in magnitude, the distance from an edge in barycentric units."""
    D = np.float64
    o, d = np.asarray(o, D)[:, None, :], np.asarray(d, D)[:, None, :]
    a, b, c = (np.asarray(x, D)[None] for x in (a, b, c))
    e1, e2 = b - a, c - a
    with np.errstate(all="ignore"):
        h = np.cross(d, e2)
        det = (e1 * h).sum(-1)
        s = o - a
        u = (s * h).sum(-1) / det
        q = np.cross(s, e1)
        v = (d * q).sum(-1) / det
        t = (e2 * q).sum(-1) / det
        w = 1 - u - v
        hit = (det != 0) & (u >= 0) & (v >= 0) & (w >= 0)
        edge = np.minimum(np.minimum(np.abs(u), np.abs(v)), np.abs(w))
        front = (np.cross(e1, e2) * d).sum(-1) < 0
    return hit, t, u, v, front, edge


# ----------------------------------------------------------------------------- fixtures

def icosphere(subdivisions=3, centre=(0.4, -0.3, 2.0), radius=1.5):
    """An icosphere: 20 * 4^subdivisions triangles (1 280 at 3), counter-clockwise seen from outside, vertices in float32."""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6),
             (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        middle, new = {}, []

        def mid(i, j):
            key = (min(i, j), max(i, j))
            if key not in middle:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                middle[key] = len(v) - 1
            return middle[key]
        for i, j, k in faces:
            ij, jk, ki = mid(i, j), mid(j, k), mid(k, i)
            new += [(i, ij, ki), (j, jk, ij), (k, ki, jk), (ij, jk, ki)]
        faces = new
    positions = np.ascontiguousarray(np.array(v) * radius + np.array(centre, np.float64), F)
    return positions, np.ascontiguousarray(np.array(faces, np.uint32))


def edge_points(positions, triangles):
    """Every vertex, and on every edge its midpoint and the points at 1/3 and 2/3, formed in float32."""
    tri = np.asarray(triangles, np.int64)
    edges = np.unique(np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), axis=1), axis=0)
    a, b = positions[edges[:, 0]], positions[edges[:, 1]]
    on_edge = [(a + (b - a).astype(F) * F(s)).astype(F) for s in (0.5, 1.0 / 3.0, 2.0 / 3.0)]
    return np.ascontiguousarray(np.concatenate([positions] + on_edge), F)


def room():
    """Two parallel walls, z = 0 (near, with the cameras in front of it at z > 0) ... in detail: the far wall at z = 4 spanning
    [-3, 3] x [-2, 2], a near wall at z = -1 of the same size behind the cameras, and between them an occluding panel at z = 2
    spanning [-0.5, 0.5] x [-0.5, 0.5].  Every rectangle is a grid of quads split in two; normals face the cameras' side (z = 0).
    -> (positions, triangles, dict of the rectangles)."""
    def rectangle(x0, x1, y0, y1, z, nx, ny, towards_minus_z):
        xs, ys = np.linspace(x0, x1, nx + 1), np.linspace(y0, y1, ny + 1)
        gx, gy = np.meshgrid(xs, ys, indexing="ij")
        pos = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, z)], -1)
        idx = lambda i, j: i * (ny + 1) + j
        tri = []
        for i in range(nx):
            for j in range(ny):
                quad = [idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)]
                if towards_minus_z:
                    quad = quad[::-1]
                tri += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
        return pos, np.array(tri, np.int64)
    spec = dict(far=(-3.0, 3.0, -2.0, 2.0, 4.0, 12, 8, True), near=(-3.0, 3.0, -2.0, 2.0, -1.0, 6, 4, False), panel=(-0.5, 0.5, -0.5, 0.5, 2.0, 4, 4, True))
    positions, triangles, parts, base_v, base_t = [], [], {}, 0, 0
    for name, args in spec.items():
        pos, tri = rectangle(*args)
        positions.append(pos)
        triangles.append(tri + base_v)
        parts[name] = dict(vertices=(base_v, base_v + len(pos)), triangles=(base_t, base_t + len(tri)), z=args[4], rect=args[:4])
        base_v += len(pos)
        base_t += len(tri)
    return np.ascontiguousarray(np.concatenate(positions), F), np.ascontiguousarray(np.concatenate(triangles), np.uint32), parts


def look(centre, towards_plus_z=True):
    """global_T_camera (4 x 4, float64) of a camera at `centre` whose axes are the world's (z forward), or turned by pi about y."""
    pose = np.eye(4)
    if not towards_plus_z:
        pose[0, 0] = pose[2, 2] = -1.0
    pose[:3, 3] = centre
    return pose


def room_views():
    """Four global_T_camera: two look through to the far wall beside the panel, one is behind the panel's centre, one faces away."""
    return [look((-1.5, 0.3, 0.0)), look((1.5, -0.2, 0.0)), look((0.0, 0.0, 0.0)), look((0.2, 0.1, 0.0), towards_plus_z=False)]


ROOM_CAMERA = (60.0, 60.0, 64.0, 48.0, 128, 96)      # fx, fy, cx, cy, width, height: half angles of 46.8 and 38.7 degrees


def view_arrays(poses):
    """(camera_T_global f32 [K, 3, 4], centres f32 [K, 3]) of global_T_camera poses, as DirectBA.MeshVisibility forms them."""
    from badslam_amd.direct_ba import view_rows
    return view_rows(list(poses))


class RestatementBA(NearestRestatementBA):
    """Stands in for a DirectBA where only NearestTriangle and MeshVisibility are called: the restatements on the CPU."""

    def __init__(self, camera=ROOM_CAMERA):
        self.camera = camera

    def MeshVisibility(self, points, mesh, poses, camera=None, min_depth=0.05, max_depth=50.0, margin=0.02, normals=None):
        cam = self.camera if camera is None else camera
        if not isinstance(cam, tuple):
            cam = (cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height)
        positions = np.asarray(mesh["positions"], F).reshape(-1, 3)
        triangles = np.asarray(mesh["triangles"], np.uint32).reshape(-1, 3)
        views, centres = view_arrays(poses)
        count, first = visibility(points, normals, positions, triangles, views, centres, cam, min_depth, max_depth, margin)
        return dict(count=count, first=first, leaves=int(triangle_boxes(positions, triangles)[0].sum()), height=0)
