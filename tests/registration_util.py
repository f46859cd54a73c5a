"""NumPy restatement of surface registration (include/badslam_hip.h "Surface registration", csrc/registration_kernels.hpp):
the step in float32, brute force over all point x triangle pairs on top of tests/point_mesh_util.py, and the host loop of
DirectBA::RegisterPoints in float64.  The GPU tests compare per-point outputs with `step` bit for bit and the sums with the float64
sums of its float32 terms.  Also: the corner surface both test files register against, and its source points."""
import numpy as np

from tests import point_mesh_util as pm
from tests.fusion_util import fma32

F = np.float32
PLANE, POINT = 0, 1
INF = F(np.inf)
TERMS = 29                       # 21 H, 6 b, cost, r * r
UPPER = [(i, j) for i in range(6) for j in range(i, 6)]

# the loop's constants (DirectBA::RegisterPoints)
STEP_TRANSLATION, STEP_ROTATION = 1e-5, 1e-6   # metres, radians: the step below which a stage has converged
SINGULAR_PIVOT = 1e-5                          # a pivot below this share of its variable's diagonal: the system is singular


# ----------------------------------------------------------------------------- the step, float32

def transform32(M, points):
    """p'.a = fmaf(M[a][2], p.z, fmaf(M[a][1], p.y, fmaf(M[a][0], p.x, M[a][3])))."""
    M = np.asarray(M, F).reshape(3, 4)
    p = np.asarray(points, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([fma32(M[a, 2], p[:, 2], fma32(M[a, 1], p[:, 1], fma32(M[a, 0], p[:, 0], M[a, 3]))) for a in range(3)], -1).astype(F)


def correspondences(moved, positions, triangles, R0, R):
    """point_mesh_util.point_mesh_distance with the boxes dilated by R0 and the hit test at R <= R0."""
    positions = np.asarray(positions, F).reshape(-1, 3)
    triangles = np.asarray(triangles, np.int64).reshape(-1, 3)
    N = len(moved)
    best = np.full(N, np.inf, F)
    which = np.full(N, pm.NO_TRIANGLE, np.int64)
    if len(triangles) and N:
        valid, lo, hi = pm.dilated_boxes(positions, triangles, R0)
        with np.errstate(all="ignore"):
            candidate = valid[None, :] & ((moved[:, None, :] >= lo[None]) & (moved[:, None, :] <= hi[None])).all(-1)
        pi, ti = np.nonzero(candidate)
        tri = positions[triangles[ti]]
        d2 = pm.pair_d2(moved[pi], tri[:, 0], tri[:, 1], tri[:, 2])
        np.minimum.at(best, pi, d2)
        attains = d2 == best[pi]
        np.minimum.at(which, pi[attains], ti[attains])
    hit = best <= F(R) * F(R)
    with np.errstate(all="ignore"):
        return np.where(hit, np.sqrt(best), INF).astype(F), np.where(hit, which, pm.NO_TRIANGLE).astype(np.uint32)


def seg_offset(p, a, b):
    """The q of seg(p, a, b)."""
    e, w = b - a, p - a
    ee, we = pm.dot(e, e), pm.dot(w, e)
    with np.errstate(all="ignore"):
        t = np.where(ee > 0, we / ee, F(0))
    t = np.where(t < 0, F(0), np.where(t > 1, F(1), t)).astype(F)
    return fma32(-t[..., None], e, w).astype(F)


def offset_vector(p, a, b, c):
    """v of the winner: the terms in the order seg ab, seg bc, seg ca, face; a later one replaces an earlier one only when it is
    strictly smaller."""
    with np.errstate(all="ignore"):
        m = np.full(len(p), np.inf, F)
        v = np.zeros((len(p), 3), F)
        for q in (seg_offset(p, a, b), seg_offset(p, b, c), seg_offset(p, c, a)):
            s = pm.dot(q, q)
            take = s < m
            m, v = np.where(take, s, m), np.where(take[:, None], q, v)
        u, w = b - a, p - a
        n = pm.cross(u, c - a)
        nn = pm.dot(n, n)
        has = (nn > 0) & (pm.dot(pm.cross(u, w), n) >= 0) & (pm.dot(pm.cross(c - b, p - b), n) >= 0) & (pm.dot(pm.cross(a - c, p - c), n) >= 0)
        root = np.sqrt(nn)
        d = pm.dot(w, n) / root
        take = has & (d * d < m)
        s = d / root
        return np.where(take[:, None], s[:, None] * n, v).astype(F)


def huber(a, k):
    """(w, rho) of the magnitude a."""
    k = F(k)
    with np.errstate(all="ignore"):
        inside = a <= k
        return np.where(inside, F(1), k / a).astype(F), np.where(inside, (F(0.5) * a) * a, k * (a - F(0.5) * k)).astype(F)


def jacobian(p, m):
    """J = (m, cross(p', m)): the derivative of m . (Exp(delta) p') by delta = (translation, rotation) at 0."""
    return np.concatenate([m, pm.cross(p, m)], -1).astype(F)


def row_terms(p, m, r, w):
    """[n, TERMS] float32 terms of row(m, r, w), the cost left at zero."""
    J = jacobian(p, m)
    out = np.zeros((len(p), TERMS), F)
    for k, (i, j) in enumerate(UPPER):
        out[:, k] = (w * J[:, i]) * J[:, j]
    for i in range(6):
        out[:, 21 + i] = (w * J[:, i]) * r
    out[:, 28] = r * r
    return out


def step(points, M, positions, triangles, R0, R, mode, huber_k, found=None):
    """found: (distance, triangle) of the moved points from another search that follows the rule (a pruned one, for a large mesh).
    -> dict: moved [N, 3] (p'), distance [N], triangle [N], v [N, 3] (zero for a miss), residual magnitude a [N], used and
    degenerate [N] bool, terms [rows, TERMS] float32 (the rows of every used pair, in point order; the cost in the pair's first
    row), owner [rows] (the point of a row), counts (points, hits, used, degenerate)."""
    positions = np.asarray(positions, F).reshape(-1, 3)
    triangles = np.asarray(triangles, np.int64).reshape(-1, 3)
    moved = transform32(M, points)
    distance, triangle = correspondences(moved, positions, triangles, R0, R) if found is None else found(moved)
    N = len(moved)
    hit = triangle != pm.NO_TRIANGLE
    idx = np.flatnonzero(hit)
    p = moved[idx]
    tri = positions[triangles[triangle[idx].astype(np.int64)]] if len(idx) else np.zeros((0, 3, 3), F)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    v = np.zeros((N, 3), F)
    mag = np.zeros(N, F)
    used = np.zeros(N, bool)
    with np.errstate(all="ignore"):
        if mode == PLANE:
            n = pm.cross(b - a, c - a)
            nn = pm.dot(n, n)
            ok = nn > 0
            root = np.sqrt(nn)
            d = (pm.dot(p - a, n) / root).astype(F)
            nh = (n / root[:, None]).astype(F)
            w, rho = huber(np.abs(d), huber_k)
            terms = row_terms(p[ok], nh[ok], d[ok], w[ok])
            terms[:, 27] = rho[ok]
            owner = idx[ok]
            used[idx[ok]] = True
            mag[idx] = np.abs(d)
        else:
            vv = offset_vector(p, a, b, c)
            v[idx] = vv
            mag_hit = np.sqrt(pm.dot(vv, vv)).astype(F)
            w, rho = huber(mag_hit, huber_k)
            rows = []
            for axis in range(3):
                m = np.zeros((len(p), 3), F)
                m[:, axis] = 1
                rows.append(row_terms(p, m, vv[:, axis], w))
            rows[0][:, 27] = rho
            terms = np.stack(rows, 1).reshape(-1, TERMS)
            owner = np.repeat(idx, 3)
            used[idx] = True
            mag[idx] = mag_hit
    degenerate = hit & ~used
    return dict(moved=moved, distance=distance, triangle=triangle, v=v, a=mag, used=used, degenerate=degenerate, terms=terms, owner=owner,
                counts=(N, int(hit.sum()), int(used.sum()), int(degenerate.sum())))


def sums64(terms):
    """(float64 sums [TERMS], sums of magnitudes [TERMS]) of float32 terms."""
    t = np.asarray(terms, np.float64)
    return t.sum(axis=0), np.abs(t).sum(axis=0)


def additions(N, mode):
    """D: the number of additions a term passes through in the kernels' order -- in the thread (one per row of the pair), the
    six levels of the wave's shuffle tree, then over the rows of the 4 * ceil(N / 256) waves: a thread of one of the 8 parts adds
    every 8th row of its contiguous share, 8 such sums make the part, and the 8 parts make the total."""
    waves = 4 * ((N + 255) // 256)
    per_part = (waves + 7) // 8
    return (3 if mode == POINT else 1) + 6 + (per_part + 7) // 8 + 8 + 8


# ----------------------------------------------------------------------------- the loop, float64

def hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def se3_exp(delta):
    """4 x 4 matrix of delta = (translation, rotation)."""
    delta = np.asarray(delta, np.float64)
    u, w = delta[:3], delta[3:]
    theta = np.linalg.norm(w)
    W = hat(w)
    if theta < 1e-8:
        A, B, Cc = 1.0 - theta * theta / 6, 0.5 - theta * theta / 24, 1.0 / 6 - theta * theta / 120
    else:
        A, B, Cc = np.sin(theta) / theta, (1 - np.cos(theta)) / theta ** 2, (theta - np.sin(theta)) / theta ** 3
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * W + B * W @ W
    T[:3, 3] = (np.eye(3) + B * W + Cc * W @ W) @ u
    return T


def se3_log(T):
    """(translation part, rotation part) of log(T)."""
    R, t = T[:3, :3], T[:3, 3]
    theta = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
    if theta > 1e-8:
        w = w * theta / np.sin(theta)
    W = hat(w)
    if theta < 1e-8:
        Vinv = np.eye(3) - 0.5 * W + W @ W / 12
    else:
        Vinv = np.eye(3) - 0.5 * W + (1 - theta * np.cos(theta / 2) / (2 * np.sin(theta / 2))) / theta ** 2 * W @ W
    return Vinv @ t, w


def unpack(sums):
    H = np.zeros((6, 6))
    for k, (i, j) in enumerate(UPPER):
        H[i, j] = H[j, i] = sums[k]
    return H, np.asarray(sums[21:27], np.float64)


def solve_ldlt(H, b):
    """x = H^-1 b by LDL^T with diagonal pivoting (host/se3.hpp SolveLDLTUpper) and the smallest share a pivot keeps of its
    variable's diagonal."""
    n = len(b)
    A = np.array(H, np.float64)
    diag = np.diag(A).copy()
    perm = list(range(n))
    share = np.inf
    for k in range(n):
        p = k + int(np.argmax(np.abs(np.diag(A)[k:])))
        if p != k:
            A[[k, p], :] = A[[p, k], :]
            A[:, [k, p]] = A[:, [p, k]]
            perm[k], perm[p] = perm[p], perm[k]
        temp = np.array([A[j, j] * A[k, j] for j in range(k)])
        dk = A[k, k] - sum(A[k, j] * temp[j] for j in range(k))
        A[k, k] = dk
        d0 = diag[perm[k]]
        share = min(share, dk / d0 if d0 > 0 else 0.0)
        for i in range(k + 1, n):
            val = A[i, k] - sum(A[i, j] * temp[j] for j in range(k))
            A[i, k] = val / dk if abs(dk) > 0 else 0.0
    y = np.array(b, np.float64)[perm]
    for i in range(n):
        for j in range(i):
            y[i] -= A[i, j] * y[j]
    y = np.array([y[i] / A[i, i] if abs(A[i, i]) > 2.2250738585072014e-308 else 0.0 for i in range(n)])
    for i in range(n - 1, -1, -1):
        for j in range(i + 1, n):
            y[i] -= A[j, i] * y[j]
    x = np.zeros(n)
    x[perm] = y
    return x, share


def register(points, positions, triangles, max_distance, min_distance=None, initial=None, mode=PLANE, huber_k=None, shrink=0.5, iterations_per_stage=20,
             sums_of=None):
    """The loop of DirectBA::RegisterPoints in float64 over `step` (sums_of: another source of (sums[29], counts) per step, for
    the same loop over another step).  -> dict of target_T_source 4 x 4, iterations, converged, reason, history."""
    T = np.eye(4) if initial is None else np.array(initial, np.float64).reshape(4, 4)
    min_distance = max_distance / 8 if min_distance is None else min_distance
    history, reason, converged = [], "iterations exhausted", False
    R = float(max_distance)
    stop = False
    while not stop and R >= min_distance:
        k = R / 2 if huber_k is None else huber_k
        converged, reason = False, "iterations exhausted"
        for _ in range(iterations_per_stage):
            if sums_of is None:
                s = step(points, T[:3].astype(F), positions, triangles, max_distance, R, mode, k)
                sums, counts = sums64(s["terms"])[0], s["counts"]
            else:
                sums, counts = sums_of(T[:3].astype(F), R, k)
            entry = dict(radius=R, hits=counts[1], used=counts[2], cost=float(sums[27]), rmse=float(np.sqrt(sums[28] / counts[2])) if counts[2] else float("nan"),
                         step_translation=float("nan"), step_rotation=float("nan"))
            history.append(entry)
            if counts[2] < 6:
                reason, stop = "fewer than 6 pairs", True
                break
            H, b = unpack(sums)
            x, share = solve_ldlt(H, -b)
            if not share > SINGULAR_PIVOT or not np.isfinite(x).all():
                reason, stop = "singular system", True
                break
            T = se3_exp(x) @ T
            entry["step_translation"], entry["step_rotation"] = float(np.linalg.norm(x[:3])), float(np.linalg.norm(x[3:]))
            if entry["step_translation"] ** 2 + (entry["step_rotation"] * (STEP_TRANSLATION / STEP_ROTATION)) ** 2 < STEP_TRANSLATION ** 2:
                converged, reason = True, "converged"
                break
        R *= shrink
    return dict(target_T_source=T, iterations=len(history), converged=converged, reason=reason, history=history)


def pose_error(result, truth):
    """(metres, radians): the norms of the translation and rotation parts of log(result * truth^-1)."""
    t, w = se3_log(np.asarray(result, np.float64) @ np.linalg.inv(truth))
    return float(np.linalg.norm(t)), float(np.linalg.norm(w))


# ----------------------------------------------------------------------------- the corner surface

CORNER = np.array([0.3, -0.2, 1.5])
EDGES = np.array([[1.0, 0.35, 0.2], [-0.1, 1.0, 0.5], [0.4, -0.15, 1.0]])      # mutually oblique, and so are the patches' normals
SIDE, CELLS = 0.8, 8
RIDGE_HEIGHT = 0.05
CORNER_R0 = 0.08
DISPLACEMENT = (0.02, np.deg2rad(1.0))                                         # 2 cm, 1 degree


def _patch_vertices(e1, e2, cells, ridge):
    e1, e2 = e1 / np.linalg.norm(e1), e2 / np.linalg.norm(e2)
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n)
    i, j = np.meshgrid(np.arange(cells + 1), np.arange(cells + 1), indexing="ij")
    h = SIDE / cells
    P = CORNER + (i * h)[..., None] * e1 + (j * h)[..., None] * e2
    if ridge:                                                                   # a ridge along e2 at u = 3 / 8 of the side, v from 1 / 8 to 4 / 8
        lift = np.zeros(i.shape)
        lift[(i * 8 == 3 * cells) & (j * 8 >= cells) & (j * 8 <= 4 * cells)] = RIDGE_HEIGHT
        P = P + lift[..., None] * n
    return P


def _patch(e1, e2, cells, ridge):
    """vertices [(cells + 1)^2, 3] float64, triangles, and per triangle whether it lies in the inner 5 / 8 of both sides."""
    P = _patch_vertices(e1, e2, cells, ridge)
    ids = np.arange((cells + 1) ** 2).reshape(cells + 1, cells + 1)
    a, b, c, d = ids[:-1, :-1], ids[1:, :-1], ids[1:, 1:], ids[:-1, 1:]
    tri = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    i = np.arange(cells)
    inner = ((i[:, None] + 1) * 8 <= 5 * cells) & ((i[None, :] + 1) * 8 <= 5 * cells)
    return P.reshape(-1, 3), tri, np.concatenate([inner.reshape(-1), inner.reshape(-1)])


def corner_surface(cells=CELLS):
    """Three plane patches of 0.8 m that meet in a corner, spanned by pairs of three mutually oblique directions, with a ridge of
    5 cm on the first: 3 * 2 * cells^2 triangles (384), no rigid motion maps it onto itself.  The patches' outer sides are open.
    -> (positions f32, triangles u32, inner [T] bool: the triangles at least 0.3 m from every open side)."""
    positions, triangles, inner, base = [], [], [], 0
    for k, (x, y) in enumerate(((0, 1), (1, 2), (2, 0))):
        P, tri, inn = _patch(EDGES[x], EDGES[y], cells, ridge=(k == 0))
        positions.append(P); triangles.append(tri + base); inner.append(inn)
        base += len(P)
    return np.concatenate(positions).astype(F), np.concatenate(triangles).astype(np.uint32), np.concatenate(inner)


def corner_cloud(spacing_cells=64):
    """The same surface as a dense cloud: the vertices of its tessellation at 1.25 cm (the ridge's creases lie on grid lines of
    the coarse mesh, which the fine grid contains, and are sampled exactly by interpolating the coarse mesh)."""
    positions, triangles, _ = corner_surface()
    out = []
    f = spacing_cells // CELLS
    s = np.arange(f + 1) / f
    for t in triangles.astype(np.int64):
        a, b, c = positions[t].astype(np.float64)
        u, v = np.meshgrid(s, s, indexing="ij")
        keep = u + v <= 1 + 1e-12
        out.append(a + u[keep][:, None] * (b - a) + v[keep][:, None] * (c - a))
    cloud = np.unique(np.round(np.concatenate(out), 9), axis=0)
    return np.ascontiguousarray(cloud, F)


def corner_points(count=600, seed=11):
    """Source points on the surface, sampled in float64 on the inner triangles (further than R0 and the displacement from every open
    side) and rounded to float32."""
    positions, triangles, inner = corner_surface()
    rng = np.random.default_rng(seed)
    chosen = triangles[inner][rng.integers(0, int(inner.sum()), count)].astype(np.int64)
    u, v = rng.uniform(size=count), rng.uniform(size=count)
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    P = positions.astype(np.float64)
    a, b, c = P[chosen[:, 0]], P[chosen[:, 1]], P[chosen[:, 2]]
    return np.ascontiguousarray(a + u[:, None] * (b - a) + v[:, None] * (c - a), F)


def known_displacement(seed=5):
    """A 4 x 4 motion of 2 cm and 1 degree about the surface's corner, in random directions."""
    rng = np.random.default_rng(seed)
    t, w = rng.standard_normal(3), rng.standard_normal(3)
    t, w = DISPLACEMENT[0] * t / np.linalg.norm(t), DISPLACEMENT[1] * w / np.linalg.norm(w)
    T = np.eye(4)
    T[:3, :3] = se3_exp(np.concatenate([np.zeros(3), w]))[:3, :3]
    T[:3, 3] = CORNER - T[:3, :3] @ CORNER + t
    return T


def displaced(points, truth):
    """Source points such that `truth` (target_T_source) maps them onto `points`: truth^-1 applied in float64, rounded to float32."""
    inv = np.linalg.inv(truth)
    return np.ascontiguousarray(np.asarray(points, np.float64) @ inv[:3, :3].T + inv[:3, 3], F)


def flat_plane(cells=6):
    """One oblique flat patch: three directions of motion leave it in itself, the system of a registration against it is singular."""
    P, tri, inner = _patch(EDGES[0], EDGES[1], cells, ridge=False)
    return P.astype(F), tri.astype(np.uint32), inner
