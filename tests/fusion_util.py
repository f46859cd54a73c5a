"""NumPy float32 restatements of the volumetric fusion and surface-nets rules (csrc/fusion_kernels.hpp), brute force: every
voxel against every keyframe, no bricks, no culling, no scans.  The GPU tests compare the kernels with these, bit for bit."""
import ctypes as C

import numpy as np

from badslam_amd import abi

F = np.float32
INVALID_DEPTH_BIT = 1 << 15


# ----------------------------------------------------------------------------- exact float32 fma

def fma32(a, b, c):
    """fl32(a * b + c) with one rounding.  The float64 product of two float32 is exact (48 <= 53 bits); TwoSum gives the error
    of adding c to it; where the float64 sum is inexact it is rounded to odd, after which narrowing to float32 (53 >= 2 * 24 + 2)
    rounds like the exact sum."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        odd = (s.view(np.int64) & 1) == 1
        fix = (err != 0) & ~odd & np.isfinite(s)
        other = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        return np.where(fix, other, s).astype(F)


def f2i(v):
    """float -> int32, truncating and saturating; NaN -> 0 (v_cvt_i32_f32)."""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        t = np.trunc(np.nan_to_num(v.astype(np.float64), nan=0.0, posinf=2.0 ** 31, neginf=-2.0 ** 31))
    return np.clip(t, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def tr_row(a, b, c, d, p):
    return fma32(c, p[2], fma32(b, p[1], fma32(a, p[0], d)))


def project(fx, fy, cx, cy, local):
    with np.errstate(all="ignore"):
        inv_z = F(1.0) / local[2]
        return fma32(fx, local[0] * inv_z, cx), fma32(fy, local[1] * inv_z, cy)


# ----------------------------------------------------------------------------- keyframes

class Keyframe:
    """What fusion reads of a keyframe: raw u16 depth, uchar4 colour [h, w, 4] and frame_T_global as 12 float32."""

    def __init__(self, depth_u16, color_u8, frame_T_global):
        self.depth = np.ascontiguousarray(depth_u16, np.uint16)
        self.color = np.ascontiguousarray(color_u8, np.uint8)
        self.T = np.asarray(frame_T_global, F).reshape(12)


def calibrated_depth(depth_u16, cfactor, a, raw_to_float_depth, cell):
    """The derived records' depth: 0 for pixels with the invalid bit, else RawToCalibratedDepth.  a == 0 in float32 here
    (exp(0) = 1 exactly); a != 0 from the oracle's bso_calibrate_depth."""
    h, w = depth_u16.shape
    if a == 0.0:
        cf = np.asarray(cfactor, F)[np.arange(h)[:, None] // cell, np.arange(w)[None, :] // cell]
        with np.errstate(all="ignore"):
            inv = F(1.0) / (F(raw_to_float_depth) * depth_u16.astype(F))
            d = F(1.0) / (inv + cf)
        return np.where(depth_u16 & INVALID_DEPTH_BIT, F(0), d).astype(F)
    from tests import bso
    L = bso.lib()
    L.bso_calibrate_depth.restype = None
    L.bso_calibrate_depth.argtypes = [C.POINTER(abi.DepthParams), C.POINTER(abi.Buffer2D), C.POINTER(abi.Buffer2D)]
    cfa = np.ascontiguousarray(cfactor, F)
    dp = abi.DepthParams(bso.np_buffer2d(cfa), a, raw_to_float_depth, 1.0, cell)
    raw = np.ascontiguousarray(depth_u16, np.uint16)
    out = np.zeros((h, w), F)
    rb, ob = bso.np_buffer2d(raw), bso.np_buffer2d(out)
    L.bso_calibrate_depth(C.byref(dp), C.byref(rb), C.byref(ob))
    return out


def voxel_centres(origin, voxel, n, axis):
    return (F(origin[axis]) + (np.arange(n).astype(F) + F(0.5)) * F(voxel)).astype(F)


def fuse(keyframes, depth_camera, color_camera, cfactor, a, raw_to_float_depth, cell, origin, voxel, dims, truncation, with_color=True):
    """-> tsdf f32, count u32, colour u8 [.., 4] (or None), each [nz, ny, nx].  Cameras are abi.Camera4f."""
    nx, ny, nz = dims
    trunc = F(truncation)
    gz, gy, gx = np.meshgrid(voxel_centres(origin, voxel, nz, 2), voxel_centres(origin, voxel, ny, 1), voxel_centres(origin, voxel, nx, 0), indexing="ij")
    gp = (gx, gy, gz)
    S = np.zeros((nz, ny, nx), F)
    n = np.zeros((nz, ny, nx), np.uint32)
    nc = np.zeros((nz, ny, nx), np.uint32)
    rgb = np.zeros((nz, ny, nx, 3), np.uint32)
    dc = depth_camera
    for kf in keyframes:
        T = kf.T
        lz = tr_row(T[8], T[9], T[10], T[11], gp)
        lx = tr_row(T[0], T[1], T[2], T[3], gp)
        ly = tr_row(T[4], T[5], T[6], T[7], gp)
        px, py = project(F(dc.fx), F(dc.fy), F(dc.cx), F(dc.cy), (lx, ly, lz))
        ix, iy = f2i(px), f2i(py)
        with np.errstate(all="ignore"):
            ok = (lz > 0) & ~((px < 0) | (py < 0) | (ix >= dc.width) | (iy >= dc.height))
        d = calibrated_depth(kf.depth, cfactor, a, raw_to_float_depth, cell)[np.where(ok, iy, 0), np.where(ok, ix, 0)]
        with np.errstate(all="ignore"):
            ok &= d != 0
            sdf = (d - lz).astype(F)
            ok &= ~(sdf < -trunc)
            S = np.where(ok, S + np.fmin(sdf, trunc), S).astype(F)
        n += ok
        if with_color:
            cc = color_camera
            cx_, cy_ = project(F(cc.fx), F(cc.fy), F(cc.cx), F(cc.cy), (lx, ly, lz))
            jx, jy = f2i(cx_), f2i(cy_)
            with np.errstate(all="ignore"):
                okc = ok & (sdf <= trunc) & ~((cx_ < 0) | (cy_ < 0) | (jx >= cc.width) | (jy >= cc.height))
            texel = kf.color[np.where(okc, jy, 0), np.where(okc, jx, 0)]
            rgb += np.where(okc[..., None], texel[..., :3].astype(np.uint32), 0).astype(np.uint32)
            nc += okc
    with np.errstate(all="ignore"):
        tsdf = np.where(n > 0, S / np.maximum(n, 1).astype(F), trunc).astype(F)
    color = None
    if with_color:
        color = np.zeros((nz, ny, nx, 4), np.uint8)
        k = np.maximum(nc, 1)[..., None]
        color[..., :3] = np.where(nc[..., None] > 0, (rgb + k // 2) // k, 0)
        color[..., 3] = np.where(nc > 0, 255, 0)
    return tsdf, n, color


# ----------------------------------------------------------------------------- surface nets

def extract_mesh(tsdf, count, color, origin, voxel, min_count):
    """Volumes [nz, ny, nx] (colour [.., 4] u8 or None) -> positions f32 [V, 3], normals f32 [V, 3], colours u8 [V, 4] or None,
    triangles u32 [T, 3]."""
    tsdf = np.asarray(tsdf, F)
    nz, ny, nx = tsdf.shape
    observed = np.asarray(count) >= min_count
    inside = tsdf < 0

    def corner(arr, dx, dy, dz):
        return arr[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]

    all_observed = np.ones((nz - 1, ny - 1, nx - 1), bool)
    n_inside = np.zeros((nz - 1, ny - 1, nx - 1), np.int32)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                all_observed &= corner(observed, dx, dy, dz)
                n_inside += corner(inside, dx, dy, dz)
    active = all_observed & (n_inside != 0) & (n_inside != 8)
    zs, ys, xs = np.nonzero(active)          # C order: ascending linear cell index
    V = len(zs)
    vid = np.full(active.shape, -1, np.int64)
    vid[zs, ys, xs] = np.arange(V)

    D = {(dx, dy, dz): corner(tsdf, dx, dy, dz)[zs, ys, xs] for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)}
    s = [np.zeros(V, F), np.zeros(V, F), np.zeros(V, F)]
    g = [np.zeros(V, F), np.zeros(V, F), np.zeros(V, F)]
    edges = np.zeros(V, np.int32)
    for axis in range(3):
        for u, v in ((0, 0), (1, 0), (0, 1), (1, 1)):
            a = {0: (0, u, v), 1: (u, 0, v), 2: (u, v, 0)}[axis]
            b = tuple(a[i] + (1 if i == axis else 0) for i in range(3))
            Da, Db = D[a], D[b]
            cross = (Da < 0) != (Db < 0)
            with np.errstate(all="ignore"):
                t = (Da / (Da - Db)).astype(F)
            for comp in range(3):
                add = t if comp == axis else np.full(V, a[comp], F)
                s[comp] = np.where(cross, s[comp] + add, s[comp]).astype(F)
            edges += cross
            g[axis] = (g[axis] + (Db - Da)).astype(F)
    m = np.maximum(edges, 1).astype(F)
    cell = (xs, ys, zs)
    positions = np.stack([F(origin[i]) + ((cell[i].astype(F) + F(0.5)) + s[i] / m) * F(voxel) for i in range(3)], axis=1).astype(F)
    length = np.sqrt(((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]).astype(F)).astype(F)
    with np.errstate(all="ignore"):
        normals = np.stack([np.where(length == 0, F(0), gi / length) for gi in g], axis=1).astype(F)

    colors = None
    if color is not None:
        k = np.zeros(V, np.uint32)
        rgb = np.zeros((V, 3), np.uint32)
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    c = color[zs + dz, ys + dy, xs + dx]
                    has = c[:, 3] == 255
                    rgb += np.where(has[:, None], c[:, :3].astype(np.uint32), 0).astype(np.uint32)
                    k += has
        colors = np.zeros((V, 4), np.uint8)
        kk = np.maximum(k, 1)[:, None]
        colors[:, :3] = np.where(k[:, None] > 0, (rgb + kk // 2) // kk, 0)
        colors[:, 3] = np.where(k > 0, 255, 0)

    # faces: per active cell, the edges from its minimum corner along x, y, z; (u, v) = the two other axes in cyclic order
    unit = np.eye(3, dtype=np.int64)
    xyz = np.stack([xs, ys, zs], axis=1).astype(np.int64)

    def is_active(p):
        ok = np.all(p >= 0, axis=1)
        q = np.where(ok[:, None], p, 0)
        return ok & active[q[:, 2], q[:, 1], q[:, 0]]

    def vertex_of(p):
        return vid[p[:, 2], p[:, 1], p[:, 0]]

    a_inside = inside[zs, ys, xs]
    ok = np.zeros((V, 3), bool)
    quads = np.zeros((V, 3, 4), np.int64)
    for axis in range(3):
        u, v = unit[(axis + 1) % 3], unit[(axis + 2) % 3]
        b = xyz + unit[axis]
        differ = a_inside != inside[b[:, 2], b[:, 1], b[:, 0]]
        ok[:, axis] = differ & is_active(xyz - u - v) & is_active(xyz - v) & is_active(xyz - u)
        sel = ok[:, axis]
        q = np.zeros((V, 4), np.int64)
        for j, p in enumerate((xyz - u - v, xyz - v, xyz, xyz - u)):
            q[sel, j] = vertex_of(p[sel])
        q[~a_inside] = q[~a_inside][:, ::-1]
        quads[:, axis] = q
    q = quads[ok]                             # boolean mask over (cell, axis) in C order: ordered by (cell, axis)
    triangles = np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1).reshape(-1, 3).astype(np.uint32)
    return positions, normals, colors, triangles


# ----------------------------------------------------------------------------- mesh properties

def edge_census(triangles):
    """-> (counts of every undirected edge, counts of every directed edge)."""
    t = np.asarray(triangles, np.int64)
    directed = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    n = int(t.max()) + 1 if len(t) else 1
    _, dcount = np.unique(directed[:, 0] * n + directed[:, 1], return_counts=True)
    und = np.sort(directed, axis=1)
    _, ucount = np.unique(und[:, 0] * n + und[:, 1], return_counts=True)
    return ucount, dcount


def signed_volume(positions, triangles):
    p = np.asarray(positions, np.float64)[np.asarray(triangles, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def face_normals(positions, triangles):
    p = np.asarray(positions, np.float64)[np.asarray(triangles, np.int64)]
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])


# ----------------------------------------------------------------------------- synthetic inputs

def sphere_field(dims=(33, 31, 29), centre=(16.3, 15.1, 14.2), radius=9.7, clamp=3.0):
    """Clamped distance to a sphere in voxel units (origin 0, voxel size 1: sample i lies at i + 0.5): [nz, ny, nx] f32,
    negative inside."""
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz) + 0.5, np.arange(ny) + 0.5, np.arange(nx) + 0.5, indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius
    return np.clip(d, -clamp, clamp).astype(F)


def holed_sphere_count(shape):
    """Observation counts for sphere_field with a block of samples unobserved: the surface opens there."""
    count = np.ones(shape, np.uint32)
    count[10:16, 12:18, 20:] = 0
    return count


def pose_matrices(rotvec, translation):
    """global_T_frame = (R(rotvec), translation) in float64 -> (frame_T_global 12 f32, global_R_frame 9 f32)."""
    w = np.asarray(rotvec, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
    t = np.asarray(translation, np.float64)
    M = np.concatenate([R.T, (-R.T @ t)[:, None]], axis=1)
    return M.astype(F).reshape(12), R.astype(F).reshape(9)


# the two planes of the plane scene: a . X = b; the surface is the first one a camera ray from z ~ 0 meets
PLANES = ((np.array([0.3, 0.1, -1.0]), -1.6), (np.array([-0.8, 0.0, -1.0]), -1.9))


def render_planes(camera, frame_T_global, raw_to_float_depth, planes=PLANES):
    """Raw u16 depth of the planes seen from a pose, through the centres of the pixels of a pixel-corner camera; 0 where
    nothing is hit or the value does not fit 15 bits."""
    M = np.asarray(frame_T_global, np.float64).reshape(3, 4)
    R, t = M[:, :3].T, -M[:, :3].T @ M[:, 3]            # global_T_frame
    j, i = np.meshgrid(np.arange(camera.height), np.arange(camera.width), indexing="ij")
    rays = np.stack([(i + 0.5 - camera.cx) / camera.fx, (j + 0.5 - camera.cy) / camera.fy, np.ones(i.shape)], axis=-1) @ R.T
    best = np.full(i.shape, np.inf)
    for a, b in planes:
        with np.errstate(all="ignore"):
            s = (b - a @ t) / (rays @ a)
        best = np.where((s > 0) & (s < best), s, best)
    raw = np.rint(np.where(np.isfinite(best), best, 0.0) / raw_to_float_depth)
    return np.where(raw < INVALID_DEPTH_BIT, raw, 0).astype(np.uint16)


def plane_distance(positions, planes=PLANES):
    """Distance of every point to the nearest of the planes."""
    p = np.asarray(positions, np.float64)
    return np.min([np.abs(p @ a - b) / np.linalg.norm(a) for a, b in planes], axis=0)


def plane_scene(seed=5, count=5, width=80, height=60, focal=70.0, raw_to_float_depth=1.0 / 5000.0):
    """Keyframes of the two planes from random poses within +-0.15 rad / +-0.2 m -> (camera, [Keyframe])."""
    rng = np.random.default_rng(seed)
    camera = abi.Camera4f(focal, focal, width / 2.0, height / 2.0, width, height)
    kfs = []
    for _ in range(count):
        T, _ = pose_matrices(rng.uniform(-0.15, 0.15, 3), rng.uniform(-0.2, 0.2, 3))
        depth = render_planes(camera, T, raw_to_float_depth)
        color = rng.integers(0, 256, (height, width, 4), dtype=np.uint8)
        kfs.append(Keyframe(depth, color, T))
    return camera, kfs


# ----------------------------------------------------------------------------- PLY reader

PLY_TYPES = {"float": "<f4", "uchar": "u1", "int": "<i4", "uint": "<u4"}


def read_ply(path):
    """Binary little-endian PLY with a vertex element of scalar properties and, optionally, a face element with one list
    property of three indices per face -> (vertex structured array, faces (T, 3) or None, header lines)."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")[:-1]
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elements = []
    for line in lines[2:-1]:
        words = line.split()
        if words[0] == "element":
            elements.append((words[1], int(words[2]), []))
        elif words[0] == "property":
            elements[-1][2].append(words[1:])
    body, vertices, faces = data[end:], None, None
    for name, count, props in elements:
        if name == "vertex":
            dtype = np.dtype([(p[1], PLY_TYPES[p[0]]) for p in props])
            vertices = np.frombuffer(body, dtype, count)
            body = body[count * dtype.itemsize:]
        else:
            assert name == "face" and len(props) == 1 and props[0][0] == "list" and props[0][3] == "vertex_indices"
            dtype = np.dtype([("n", PLY_TYPES[props[0][1]]), ("v", PLY_TYPES[props[0][2]], 3)])
            rec = np.frombuffer(body, dtype, count)
            assert np.all(rec["n"] == 3)
            faces = rec["v"].copy()
            body = body[count * dtype.itemsize:]
    assert len(body) == 0
    return vertices, faces, lines
