"""NumPy restatement of place recognition (badslam_amd/csrc/place_kernels.hpp, badslam_amd/host/place_recognition.cpp):
the point-pair table, corner score, cell selection and descriptor; matching with the ratio test; the 3D-3D RANSAC with the
same generator.  Everything up to the matches is integer arithmetic and must agree with the kernels bit for bit; the
RANSAC is double precision with the same expression order where a comparison depends on it.  Also the scene the tests
share: the random planes of tests/scenes.py with a blocky world-space texture (the smooth texture_at has no corners)."""
import numpy as np

from tests import bso, scenes

CELL = 16
EMPTY = 0xFFFFFFFF
NO_SECOND = 257
W, H = 320, 240
RAW_TO_FLOAT = float(np.float32(1.0 / 5000))
DEFAULTS = dict(min_keyframe_gap=10, score_threshold=10 ** 11, max_distance=64, min_matches=25, ransac_iterations=500, ransac_min_inliers=10,
                ransac_inlier_threshold=0.06)


# ---- generator and point pairs ----------------------------------------------------------------------------------
class Lcg:
    def __init__(self, seed):
        self.s = seed & 0xFFFFFFFF

    def draw(self):
        self.s = (self.s * 1664525 + 1013904223) & 0xFFFFFFFF
        return self.s >> 16


def pattern():
    """(256, 4) int: ax, ay, bx, by of every pair, each in -13 ... 13."""
    g = Lcg(0x0BAD51A4)
    pairs = []
    while len(pairs) < 256:
        v = [g.draw() % 27 - 13 for _ in range(4)]
        if v[0] == v[2] and v[1] == v[3]:
            continue
        pairs.append(v)
    return np.array(pairs, np.int64)


# ---- extraction ---------------------------------------------------------------------------------------------------
def box5(a):
    p = np.pad(a, 2)
    h, w = a.shape
    return sum(p[dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5))


def corner_score(L):
    """int64 score of every pixel; the kernel's clamped addressing and this zero padding differ only within 3 pixels of
    the border, where no pixel is eligible."""
    Lp = np.pad(L.astype(np.int64), 1, mode="edge")
    gx = (Lp[:-2, 2:] + 2 * Lp[1:-1, 2:] + Lp[2:, 2:]) - (Lp[:-2, :-2] + 2 * Lp[1:-1, :-2] + Lp[2:, :-2])
    gy = (Lp[2:, :-2] + 2 * Lp[2:, 1:-1] + Lp[2:, 2:]) - (Lp[:-2, :-2] + 2 * Lp[:-2, 1:-1] + Lp[:-2, 2:])
    A, B, Cs = box5(gx * gx), box5(gy * gy), box5(gx * gy)
    return 16 * (A * B - Cs * Cs) - (A + B) ** 2


def extract(L, depth, score_threshold=DEFAULTS["score_threshold"]):
    """L (h, w) uint8 intensity, depth (h, w) uint16 -> xy (cells,) uint32, desc (cells, 8) uint32."""
    h, w = L.shape
    cy, cx = h // CELL, w // CELL
    score = corner_score(L)
    ys, xs = np.mgrid[0:h, 0:w]
    d = depth.astype(np.int64)
    eligible = (xs >= CELL) & (xs < w - CELL) & (ys >= CELL) & (ys < h - CELL) & (d != 0) & ((d & 0x8000) == 0) & (score > score_threshold)
    S = box5(L.astype(np.int64))
    pairs = pattern()
    xy = np.full(cy * cx, EMPTY, np.uint32)
    desc = np.zeros((cy * cx, 8), np.uint32)
    for c in range(cy * cx):
        y0, x0 = (c // cx) * CELL, (c % cx) * CELL
        e = eligible[y0:y0 + CELL, x0:x0 + CELL].reshape(-1)
        if not e.any():
            continue
        s = score[y0:y0 + CELL, x0:x0 + CELL].reshape(-1)
        best = s[e].max()
        i = int(np.flatnonzero(e & (s == best))[0])          # the lowest y, then the lowest x
        y, x = y0 + i // CELL, x0 + i % CELL
        bits = S[y + pairs[:, 1], x + pairs[:, 0]] < S[y + pairs[:, 3], x + pairs[:, 2]]
        xy[c] = x | (y << 16)
        desc[c] = (bits.reshape(8, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    return xy, desc


# ---- matching -----------------------------------------------------------------------------------------------------
def _bits(desc):
    return np.unpackbits(np.ascontiguousarray(desc, np.uint32).view(np.uint8), axis=-1).astype(np.float32)


def match(query_xy, query_desc, db_xy, db_desc, max_distance=DEFAULTS["max_distance"]):
    """query_xy (cells,), query_desc (cells, 8); db_xy (n, cells), db_desc (n, cells, 8) -> match (n, cells) int32, count (n,) uint32."""
    n, cells = db_xy.shape[0], len(query_xy)
    out, count = np.full((n, cells), -1, np.int32), np.zeros(n, np.uint32)
    q = _bits(query_desc)
    q_live = query_xy != EMPTY
    q_ones = q.sum(axis=1)
    for k in range(n):
        live = db_xy[k] != EMPTY
        if not live.any():
            continue
        b = _bits(db_desc[k])
        dist = np.rint(q_ones[:, None] + b.sum(axis=1)[None, :] - 2 * (q @ b.T)).astype(np.int64)   # |q| + |b| - 2 q.b; exact in float32
        dist[:, ~live] = 1000
        best_slot = dist.argmin(axis=1)                                   # the lowest slot among equals
        best = dist[np.arange(cells), best_slot]
        rest = dist.copy()
        rest[np.arange(cells), best_slot] = 1000
        second = rest.min(axis=1)
        second = np.where(second >= 1000, NO_SECOND, second)
        accepted = q_live & (best <= max_distance) & (4 * best < 3 * second)
        out[k] = np.where(accepted, best_slot, -1)
        count[k] = accepted.sum()
    return out, count


def query(counts, exists, min_matches=DEFAULTS["min_matches"]):
    """The candidate among the database keyframes: the highest count >= min_matches, the lower id among equals; -1 if none."""
    best = -1
    for k, c in enumerate(counts):
        if exists[k] and c >= min_matches and (best < 0 or c > counts[best]):
            best = k
    return best


# ---- RANSAC -------------------------------------------------------------------------------------------------------
def ransac_seed(current_id, matched_id):
    return (0x0BAD51A4 ^ ((current_id * 0x9E3779B1) & 0xFFFFFFFF) ^ ((matched_id * 0x85EBCA6B) & 0xFFFFFFFF)) & 0xFFFFFFFF


def absolute_orientation(pc, po):
    """Horn's closed form: R, t, q (x, y, z, w) with po ~ R pc + t."""
    cc, co = pc.sum(axis=0) / len(pc), po.sum(axis=0) / len(po)
    S = (pc - cc).T @ (po - co)
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    N = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                  [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                  [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    _, vecs = np.linalg.eigh(N)
    e = vecs[:, -1]
    e = e / np.linalg.norm(e)
    if e[0] < 0:
        e = -e
    w, x, y, z = e
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    t = co - ((R[:, 0] * cc[0] + R[:, 1] * cc[1]) + R[:, 2] * cc[2])
    return R, t, np.array([x, y, z, w])


def inlier_mask(R, t, pc, po, threshold):
    d = (((R[:, 0][None, :] * pc[:, 0:1] + R[:, 1][None, :] * pc[:, 1:2]) + R[:, 2][None, :] * pc[:, 2:3]) + t[None, :]) - po
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= threshold


def collinear(p, i0, i1, i2):
    a, b = p[i1] - p[i0], p[i2] - p[i0]
    c = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
    cross2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
    scale = ((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]) * ((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])
    return not (cross2 > 1e-6 * scale)


def ransac(current_id, matched_id, p_cur, p_old, iterations=500, threshold=0.06, min_inliers=10):
    """dict(found, old_T_cur (7,) [qx qy qz qw tx ty tz], inlier_count, inliers (n,) bool)."""
    pc, po = np.asarray(p_cur, np.float64).reshape(-1, 3), np.asarray(p_old, np.float64).reshape(-1, 3)
    n = len(pc)
    out = dict(found=False, old_T_cur=np.array([0, 0, 0, 1, 0, 0, 0], np.float64), inlier_count=0, inliers=np.zeros(n, bool))
    if n < 3:
        return out
    g = Lcg(ransac_seed(current_id, matched_id))
    best, best_count = None, -1
    for _ in range(iterations):
        idx = [g.draw() % n for _ in range(3)]
        if len(set(idx)) < 3 or collinear(pc, *idx) or collinear(po, *idx):
            continue
        R, t, _q = absolute_orientation(pc[idx], po[idx])
        count = int(inlier_mask(R, t, pc, po, threshold).sum())
        if count > best_count:
            best, best_count = (R, t), count
    if best_count < 3:
        return out
    mask = inlier_mask(best[0], best[1], pc, po, threshold)
    R, t, q = absolute_orientation(pc[mask], po[mask])
    mask = inlier_mask(R, t, pc, po, threshold)
    out.update(found=bool(mask.sum() >= min_inliers), old_T_cur=np.concatenate([q, t]), inlier_count=int(mask.sum()), inliers=mask)
    return out


def unproject(xy, depth, cam, raw_to_float_depth=RAW_TO_FLOAT):
    """Points of feature slots xy (uint32 x | y << 16) in the camera frame, double: pixel centre in the pixel-corner convention."""
    x, y = (xy & 0xFFFF).astype(np.int64), (xy >> 16).astype(np.int64)
    z = depth[y, x].astype(np.float64) * np.float64(np.float32(raw_to_float_depth))
    fx, fy, cx, cy = (np.float64(np.float32(v)) for v in (cam.fx, cam.fy, cam.cx, cam.cy))
    return np.stack([((x + 0.5) - cx) / fx * z, ((y + 0.5) - cy) / fy * z, z], axis=1)


def matched_points(xy_cur, depth_cur, xy_old, depth_old, match_row, cam):
    q = np.flatnonzero(match_row >= 0)
    return unproject(xy_cur[q], depth_cur, cam), unproject(xy_old[match_row[q]], depth_old, cam)


def pose_difference(a7, b7):
    """(translation distance in metres, rotation angle in degrees) between two [qx qy qz qw tx ty tz] poses."""
    a7, b7 = np.asarray(a7, np.float64), np.asarray(b7, np.float64)
    dot = min(1.0, abs(float(a7[:4] @ b7[:4]) / (np.linalg.norm(a7[:4]) * np.linalg.norm(b7[:4]))))
    return float(np.linalg.norm(a7[4:] - b7[4:])), float(np.degrees(2 * np.arccos(dot)))


# ---- the scene ----------------------------------------------------------------------------------------------------
def blocky_texture(points, plane_index):
    """World-space texture with corners: a hash of floor(point / 0.12 m) and the plane index, 0 ... 255."""
    c = np.floor(points / 0.12).astype(np.int64)
    h = (c[..., 0] * 73856093) ^ (c[..., 1] * 19349663) ^ (c[..., 2] * 83492791) ^ (plane_index.astype(np.int64) * 2654435761)
    h = (h ^ (h >> 13)) * 1274126177
    return ((h >> 7) & 0xFF).astype(np.uint8)


def path_poses():
    """Leave and return, 10 keyframes: 0-2 at home, 3-6 turned away (no view in common with home), 7-9 back near home."""
    xi = [(0.00, 0.00, 0.00, 0.00, 0.00, 0.00), (0.04, 0.01, 0.00, 0.00, 0.01, 0.00), (0.08, 0.02, 0.01, 0.005, 0.02, 0.00),
          (0.15, 0.02, 0.02, 0.00, 0.45, 0.00), (0.25, 0.00, 0.05, 0.02, 0.95, 0.00), (0.30, -0.03, 0.05, 0.03, 1.25, 0.02),
          (0.22, -0.02, 0.03, 0.02, 0.90, 0.01), (0.09, 0.00, 0.02, 0.01, 0.03, -0.01), (0.05, -0.01, 0.015, -0.005, 0.015, 0.01),
          (0.015, -0.015, 0.01, 0.01, -0.01, 0.005)]
    return [bso.se3_exp(np.array(v, np.float32)) for v in xi]


HOME, AWAY, BACK = (0, 1, 2), (4, 5, 6), (7, 8, 9)


def drifted_poses(poses, end=(0.16, -0.09, 0.08, 0.08, -0.09, 0.06), first=3):
    """Drift that starts after the home keyframes and grows to `end` (about 20 cm and 8 degrees) at the last keyframe."""
    n = len(poses)
    out = []
    for k, T in enumerate(poses):
        f = max(0, k - first + 1) / (n - first)
        out.append(bso.se3_copy(T) if f == 0 else bso.se3_mul(T, bso.se3_exp((np.array(end, np.float32) * np.float32(f)).astype(np.float32))))
    return out


def camera(width=W, height=H):
    return bso.make_camera(262.5 * width / W, 262.5 * width / W, width / 2.0, height / 2.0, width, height)


def render(poses, seed=5, width=W, height=H):
    """(camera, [(depth uint16, rgb uint8 (h, w, 3))]) of the 20 random planes seen from `poses`."""
    rng = np.random.default_rng(seed)
    cam = camera(width, height)
    planes = scenes.random_planes(rng, 20)
    frames = []
    for T in poses:
        M = np.array(list(bso.se3_matrix3x4(T).m), np.float64).reshape(3, 4)
        tt, pidx, dg, o = scenes.render_planes(cam, width, height, M[:, :3], M[:, 3], planes)
        valid = np.isfinite(tt) & (tt < 6.0)
        depth = np.where(valid, tt / RAW_TO_FLOAT + 0.5, 0).astype(np.uint32)
        depth = np.where(depth >= 32768, 0, depth).astype(np.uint16)
        pts = o[None, None, :] + dg * np.where(valid, tt, 0.0)[..., None]
        lum = np.where(valid, blocky_texture(pts, pidx), 0).astype(np.uint8)
        frames.append((depth, np.ascontiguousarray(np.repeat(lum[:, :, None], 3, axis=2))))
    return cam, frames


def intensity_of_gray(rgb):
    """What bslam_compute_brightness writes into byte 3 for a grey pixel (r = g = b = v): v itself (0.299 + 0.587 + 0.114 = 1 up
    to float rounding, and + 0.5 truncates back to v)."""
    return np.ascontiguousarray(rgb[:, :, 0])


_cache = {}


def path_scene():
    """(ground-truth poses, camera, frames) of the leave-and-return path, rendered once per process."""
    if "scene" not in _cache:
        gt = path_poses()
        cam, frames = render(gt)
        _cache["scene"] = (gt, cam, frames)
    return _cache["scene"]


def path_features():
    """[(xy, desc)] of the path's frames by the restatement, on the rendered (unfiltered) depth; once per process."""
    if "features" not in _cache:
        _, _, frames = path_scene()
        _cache["features"] = [extract(intensity_of_gray(rgb), depth) for depth, rgb in frames]
    return _cache["features"]
