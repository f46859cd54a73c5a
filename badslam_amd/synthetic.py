"""Synthetic 640x480 keyframe stacks for bench.py: random planes, a
photo-consistent texture, keyframe poses T0 * exp(xi), cell-4 surfel creation from every
keyframe without merging (19 200 surfels per keyframe).

Pure numpy input synthesis in the formats the hot path reads (BS/kernels.cuh:38-93,
BS/util.cuh:105-130); it does not go through the reference's
preprocessing kernels and it uses nothing but numpy.
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import abi


def so3_exp(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def se3_exp(x):
    """Returns (R, t) of exp(x), x = [translation(3), rotation(3)] (Sophus tangent order)."""
    x = np.asarray(x, np.float64)
    w = x[3:]
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    R = so3_exp(w)
    if th < 1e-12:
        V = np.eye(3) + 0.5 * K
    else:
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * (K @ K)
    return R, V @ x[:3]


def rot_to_quat(R):
    """Unit quaternion (x, y, z, w) of a rotation matrix."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = np.zeros(4)
        q[i] = 0.25 * s
        q[j] = (R[j, i] + R[i, j]) / s
        q[k] = (R[k, i] + R[i, k]) / s
        q[3] = (R[k, j] - R[j, k]) / s
    return q / np.linalg.norm(q)


def make_se3f(R, t):
    T = abi.SE3f()
    q = rot_to_quat(R)
    for i in range(4):
        T.q[i] = float(q[i])
    for i in range(3):
        T.t[i] = float(t[i])
    return T


def mat3x4(R, t):
    M = abi.Mat3x4()
    A = np.concatenate([R, t.reshape(3, 1)], axis=1).astype(np.float32)
    for i in range(12):
        M.m[i] = float(A.flat[i])
    return M


def mat3x3(R):
    M = abi.Mat3x3()
    A = R.astype(np.float32)
    for i in range(9):
        M.m[i] = float(A.flat[i])
    return M


def s8_pack(nx, ny):
    """ImageSpaceNormalToU16 (BS/util.cuh:102-117)."""
    def s8(v):
        return (v * np.float32(127) + np.where(v > 0, np.float32(0.5), np.float32(-0.5))).astype(np.int8)
    return s8(nx).view(np.uint8).astype(np.uint16) | (s8(ny).view(np.uint8).astype(np.uint16) << 8)


def s10_pack(n):
    """SurfelSetNormal (BS/util_nvcc_only.cuh:67-84): three signed 10-bit fields."""
    def s10(v):
        return (v * np.float32(511) + np.where(v > 0, np.float32(0.5), np.float32(-0.5))).astype(np.int16).astype(np.uint16).astype(np.uint32) & 0x3FF
    return s10(n[..., 0]) | (s10(n[..., 1]) << 10) | (s10(n[..., 2]) << 20)


# Scene kinds.  Every kind is a convex arrangement of planes n.p + d = 0 seen from inside (n.p + d > 0), so the
# surface a pixel sees is the nearest front-facing plane along its ray.
#   "dense"      20 random planes n = (u1, u2, -1)/|.| at offset 2.5 m, keyframe poses exp(xi) with xi_t ~ U(-0.25, 0.25) m,
#                xi_r ~ U(-0.12, 0.12) rad: every keyframe stares at the same planes (the bench headline since round 1).
#   "survey"     the same planes with the pose ranges of the reference's test scene, xi_t ~ U(-1.5, 1.5) m, xi_r ~ U(-0.7, 0.7) rad
#                (BS/test/test_intrinsics_optimization_geometric_residual.cc:286-296).
#   "trajectory" a room (16 jittered walls around a 5 m apothem, floor, ceiling) and a camera that walks one smooth lap at
#                2.2 m from the centre looking outward, K poses along the lap: a keyframe sees a bounded part of the scene
#                (about a tenth of the wall ring), as on a real sequence.
SCENE_KINDS = ("dense", "survey", "trajectory")
POSE_RANGES = {"dense": (0.25, 0.12), "survey": (1.5, 0.7)}


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


def scene_planes(kind, rng, plane_count=20):
    """(normals [P, 3], offsets [P]) of the scene's planes n.p + d = 0; the free space is n.p + d > 0 for every plane."""
    if kind in ("dense", "survey"):
        planes = []
        for _ in range(plane_count):
            n = rng.uniform(-1, 1, 3)
            n[2] = -1.0
            planes.append(n / np.linalg.norm(n))
        return np.stack(planes, axis=0), np.full(plane_count, 2.5)
    if kind != "trajectory":
        raise ValueError(f"unknown scene kind {kind!r}")
    normals, offsets = [], []
    walls = 16
    for i in range(walls):
        th = 2 * np.pi * i / walls
        n = -np.array([np.cos(th), 0.0, np.sin(th)]) + rng.uniform(-0.08, 0.08, 3)   # inward, slightly tilted
        normals.append(n / np.linalg.norm(n))
        offsets.append(5.0 + rng.uniform(-0.4, 0.4))
    for sign in (+1.0, -1.0):   # floor (y = +1.4: y points down in the camera convention) and ceiling
        n = np.array([0.0, -sign, 0.0]) + rng.uniform(-0.03, 0.03, 3)
        normals.append(n / np.linalg.norm(n))
        offsets.append(1.4 + rng.uniform(-0.05, 0.05))
    return np.stack(normals, axis=0), np.array(offsets)


def trajectory_pose(k, K):
    """(R, t) = global_T_frame of pose k of K along one smooth lap through the room of scene_planes("trajectory"): the camera
    (z forward, x right, y down) stands about 2.2 m from the room's axis and looks outward, with slow changes of radius,
    height, heading, pitch and roll."""
    phi = 2 * np.pi * k / K
    radius = 2.2 + 0.3 * np.sin(2 * phi + 1.0)
    t = np.array([radius * np.cos(phi), 0.25 * np.sin(3 * phi), radius * np.sin(phi)])
    heading = phi + 0.25 * np.sin(5 * phi)
    R = rot_y(np.pi / 2 - heading) @ rot_x(0.15 * np.sin(4 * phi + 0.5)) @ rot_z(0.05 * np.sin(7 * phi))
    return R, t


class SyntheticStack:
    """Host arrays of a synthetic keyframe stack + surfel SoA."""

    def __init__(self, num_keyframes, width=640, height=480, cell=4, seed=0xBAD51A4,
                 fx=525.0, fy=525.0, cx=320.0, cy=240.0, raw_to_float_depth=1.0 / 5000, baseline_fx=40.0,
                 translation_range=None, rotation_range=None, plane_count=20, surfel_noise=0.002, kind="dense", threads=1):
        """threads > 1: each keyframe's image is rendered in that many bands of rows at once; the stack is the same."""
        rng = np.random.default_rng(seed)
        self.kind = kind
        if kind in POSE_RANGES:
            translation_range = POSE_RANGES[kind][0] if translation_range is None else translation_range
            rotation_range = POSE_RANGES[kind][1] if rotation_range is None else rotation_range
        self.width, self.height, self.cell = width, height, cell
        self.camera = abi.Camera4f(fx, fy, cx, cy, width, height)   # pixel-corner convention
        self.raw_to_float_depth = np.float32(raw_to_float_depth)
        self.baseline_fx = float(baseline_fx)
        self.K = num_keyframes
        plane_matrix, plane_d = scene_planes(kind, rng, plane_count)
        xs = (np.arange(width) - (cx - 0.5)) / fx
        ys = (np.arange(height) - (cy - 0.5)) / fy
        dxg, dyg = np.meshgrid(xs, ys)
        dirs = np.stack([dxg, dyg, np.ones_like(dxg)], axis=-1)
        self.depth = np.zeros((num_keyframes, height, width), np.uint16)
        self.normals = np.zeros((num_keyframes, height, width), np.uint16)
        self.radius = np.zeros((num_keyframes, height, width), np.uint16)
        self.color = np.zeros((num_keyframes, height, width, 4), np.uint8)
        self.R = []
        self.t = []
        surf = []
        cw, ch = (width - 1) // cell + 1, (height - 1) // cell + 1
        # per-pixel products of the keyframe being rendered, filled band by band (rows [lo, hi)); the surfel noise below draws
        # from rng in keyframe order on the calling thread, so the stack does not depend on `threads`
        valid = np.zeros((height, width), bool)
        z = np.zeros((height, width), np.float32)
        bestn = np.zeros((height, width, 3), np.float64)
        r2 = np.zeros((height, width), np.float16)
        rows = -(-height // max(1, threads))
        bands = [(lo, min(height, lo + rows)) for lo in range(0, height, rows)]
        pool = ThreadPoolExecutor(len(bands)) if len(bands) > 1 else None
        for k in range(num_keyframes):
            if kind == "trajectory":
                R, t = trajectory_pose(k, num_keyframes)
            else:
                xi = np.concatenate([rng.uniform(-translation_range, translation_range, 3), rng.uniform(-rotation_range, rotation_range, 3)])
                R, t = se3_exp(xi)
            self.R.append(R)
            self.t.append(t)
            num = -(plane_d + plane_matrix @ t)
            args = (k, R, t, num, dirs, plane_matrix, raw_to_float_depth, fx, valid, z, bestn, r2)
            if pool is None:
                self._render_rows(*args, 0, height)
            else:
                list(pool.map(lambda band: self._render_rows(*args, *band), bands))
            # cell-4 surfel creation without merge: first pixel of each cell, if valid
            yy, xx = np.meshgrid(np.arange(ch) * cell + 1, np.arange(cw) * cell + 1, indexing="ij")
            yy = np.minimum(yy, height - 2)
            xx = np.minimum(xx, width - 2)
            v = valid[yy, xx]
            zc = z[yy, xx][v].astype(np.float32)
            pcam = np.stack([zc * dxg[yy, xx][v].astype(np.float32), zc * dyg[yy, xx][v].astype(np.float32), zc], axis=-1)
            pg = (pcam.astype(np.float64) @ R.T + t[None, :])
            pg += bestn[yy, xx][v] * rng.uniform(-surfel_noise, surfel_noise, (pg.shape[0], 1))   # off-surface noise along the normal
            s = np.zeros((abi.SURFEL_ATTRIBUTE_COUNT, pg.shape[0]), np.float32)
            s[0:3] = pg.T.astype(np.float32)
            s[3] = s10_pack(bestn[yy, xx][v].astype(np.float32)).view(np.float32)
            s[4] = r2[yy, xx][v].astype(np.float32)
            surf.append(s)
        if pool is not None:
            pool.shutdown()
        self.surfels = np.ascontiguousarray(np.concatenate(surf, axis=1))
        self.surfels_size = self.surfels.shape[1]
        self.cfactor = np.zeros(((height - 1) // cell + 1, (width - 1) // cell + 1), np.float32)

    def _render_rows(self, k, R, t, num, dirs, plane_matrix, raw_to_float_depth, fx, valid, z, bestn, r2, lo, hi):
        """Image rows [lo, hi) of keyframe k: depth, normals, radius and colour into the stack, and the per-pixel valid / z / bestn /
        r2 the surfel creation reads.  Every operation is per pixel or per image row, so a band gives the same bits as the whole
        image (numpy's matmul of [rows, w, 3] stacks is one BLAS call per row)."""
        dg = dirs[lo:hi] @ R.T
        # nearest front-facing plane per pixel, all planes at once (first plane wins ties, as a plane-by-plane sweep would)
        denom = dg @ plane_matrix.T                                  # [rows, w, planes]
        with np.errstate(divide="ignore", invalid="ignore"):
            tt = num[None, None, :] / denom
        tt = np.where((denom < 0) & (tt > 0.3), tt, np.inf)
        which = np.argmin(tt, axis=2)
        best = np.take_along_axis(tt, which[..., None], axis=2)[..., 0]
        bn = np.where(np.isfinite(best)[..., None], plane_matrix[which], 0.0)
        v = np.isfinite(best) & (best < 6.0)
        if lo == 0:
            v[0, :] = False
        if hi == self.height:
            v[-1, :] = False
        v[:, 0] = v[:, -1] = False
        d16 = np.where(v, best / float(raw_to_float_depth) + 0.5, 65535).astype(np.uint32)
        v &= d16 < 32768
        d16 = np.where(v, d16, 65535).astype(np.uint16)
        self.depth[k, lo:hi] = d16
        n_cam = (bn @ R).astype(np.float32)          # R^T n, rows
        self.normals[k, lo:hi] = np.where(v, s8_pack(n_cam[..., 0], n_cam[..., 1]), 0).astype(np.uint16)
        zb = (d16.astype(np.float32) * self.raw_to_float_depth)
        r2b = np.where(v, (zb / np.float32(fx)) ** 2, 0).astype(np.float16)
        self.radius[k, lo:hi] = r2b.view(np.uint16)
        pts = t[None, None, :] + dg * np.where(v, best, 0.0)[..., None]
        lum = (np.sin(7.0 * pts[..., 0] + 0.37) + np.sin(9.0 * pts[..., 1] + 0.5) + np.sin(11.0 * pts[..., 2] + 0.7)
               + 0.5 * np.sin(23.0 * (pts[..., 0] + pts[..., 1])) + 0.5 * np.cos(17.0 * (pts[..., 1] - pts[..., 2])))
        lum = np.clip((lum + 4.0) / 8.0 * 255.0, 0, 255).astype(np.uint8)
        self.color[k, lo:hi] = np.repeat(lum[:, :, None], 4, axis=2)
        valid[lo:hi], z[lo:hi], bestn[lo:hi], r2[lo:hi] = v, zb, bn, r2b

    def pose(self, k, xi=None):
        """(global_T_frame as SE3f, frame_T_global 3x4, global_R_frame) of keyframe k, optionally * exp(xi)."""
        R, t = self.R[k], self.t[k]
        if xi is not None:
            dR, dt = se3_exp(xi)
            t = t + R @ dt
            R = R @ dR
        Ri = R.T
        ti = -R.T @ t
        return make_se3f(R, t), mat3x4(Ri, ti), mat3x3(R)


class DeviceStack:
    """The stack in HBM (torch tensors) with POD views for the C ABI."""

    def __init__(self, stack, device, surfel_range=None):
        import torch
        self.torch = torch
        self.stack = stack
        self.device = device
        lo, hi = surfel_range if surfel_range is not None else (0, stack.surfels_size)
        self.surfels = torch.from_numpy(np.ascontiguousarray(stack.surfels[:, lo:hi])).to(device)
        self.surfels_size = hi - lo
        self.active = torch.ones((1, max(1, self.surfels_size)), dtype=torch.uint8, device=device)
        self.cfactor = torch.from_numpy(stack.cfactor).to(device)
        self.depth = torch.from_numpy(stack.depth.view(np.int16)).to(device)
        self.normals = torch.from_numpy(stack.normals.view(np.int16)).to(device)
        self.radius = torch.from_numpy(stack.radius.view(np.int16)).to(device)
        self.color = torch.from_numpy(stack.color).to(device)

    @staticmethod
    def buf(tensor):
        return abi.Buffer2D(tensor.data_ptr(), tensor.shape[0], tensor.shape[1], tensor.stride(0) * tensor.element_size())

    def depth_params(self):
        dp = abi.DepthParams()
        dp.cfactor_buffer = self.buf(self.cfactor)
        dp.a = 0.0
        dp.raw_to_float_depth = float(self.stack.raw_to_float_depth)
        dp.baseline_fx = self.stack.baseline_fx
        dp.sparse_surfel_cell_size = self.stack.cell
        return dp

    def keyframe_views(self, activation=abi.KF_ACTIVE):
        K = self.stack.K
        arr = (abi.KeyframeView * K)()
        for k in range(K):
            v = arr[k]
            v.depth, v.normals = self.buf(self.depth[k]), self.buf(self.normals[k])
            v.radius, v.color = self.buf(self.radius[k]), self.buf(self.color[k])
            _, M, Rg = self.stack.pose(k)
            v.frame_T_global, v.global_R_frame = M, Rg
            v.activation = activation
            v.id = k
        return arr


class GeneratedStackMeta:
    """Host-side description of a stack whose images live only in HBM (TorchStack): cameras, scalars and poses."""

    def __init__(self, K, width, height, cell, camera, raw_to_float_depth, baseline_fx, R, t):
        self.K, self.width, self.height, self.cell = K, width, height, cell
        self.camera, self.raw_to_float_depth, self.baseline_fx = camera, np.float32(raw_to_float_depth), float(baseline_fx)
        self.R, self.t = R, t
        self.surfels_size = 0
        self.cfactor = np.zeros(((height - 1) // cell + 1, (width - 1) // cell + 1), np.float32)

    pose = SyntheticStack.pose


class TorchStack(DeviceStack):
    """The same synthetic scene family as SyntheticStack (random planes, photo-consistent texture, poses T0 * exp(xi), cell-4
    surfels without merging), rendered directly in HBM with torch ops: the 300- and 1000-keyframe stacks of BASELINE.json
    configs[2] / configs[4] take seconds instead of minutes.  Not bit-identical to SyntheticStack (different random streams for
    the surfel noise, float64 on the device); the -m gpu tests that use it are property tests and oracle comparisons on data
    copied back from the device."""

    def __init__(self, num_keyframes, device, width=640, height=480, cell=4, seed=0xBAD51A4, fx=525.0, fy=525.0, cx=320.0, cy=240.0,
                 raw_to_float_depth=1.0 / 5000, baseline_fx=40.0, translation_range=None, rotation_range=None, plane_count=20,
                 surfel_noise=0.002, kind="dense", border_valid=False):
        """border_valid: the outermost pixel rows / columns carry measurements too (the default leaves them empty, as the
        reference's preprocessing does for normals); tests of the image-bound handling use it."""
        import torch
        self.torch = torch
        self.device = device
        self.kind = kind
        if kind in POSE_RANGES:
            translation_range = POSE_RANGES[kind][0] if translation_range is None else translation_range
            rotation_range = POSE_RANGES[kind][1] if rotation_range is None else rotation_range
        rng = np.random.default_rng(seed)
        planes, plane_d = scene_planes(kind, rng, plane_count)
        Rs, ts = [], []
        for k in range(num_keyframes):
            if kind == "trajectory":
                R, t = trajectory_pose(k, num_keyframes)
            else:
                xi = np.concatenate([rng.uniform(-translation_range, translation_range, 3), rng.uniform(-rotation_range, rotation_range, 3)])
                R, t = se3_exp(xi)
            Rs.append(R)
            ts.append(t)
        cam = abi.Camera4f(fx, fy, cx, cy, width, height)
        self.stack = GeneratedStackMeta(num_keyframes, width, height, cell, cam, raw_to_float_depth, baseline_fx, Rs, ts)
        f64 = dict(dtype=torch.float64, device=device)
        P = torch.tensor(np.asarray(planes), **f64)                                 # [planes, 3]
        Pd = torch.tensor(np.asarray(plane_d), **f64)                               # [planes]
        xs = (torch.arange(width, **f64) - (cx - 0.5)) / fx
        ys = (torch.arange(height, **f64) - (cy - 0.5)) / fy
        dyg, dxg = torch.meshgrid(ys, xs, indexing="ij")
        dirs = torch.stack([dxg, dyg, torch.ones_like(dxg)], dim=-1)                # [h, w, 3]
        K = num_keyframes
        self.depth = torch.empty((K, height, width), dtype=torch.int16, device=device)
        self.normals = torch.empty((K, height, width), dtype=torch.int16, device=device)
        self.radius = torch.empty((K, height, width), dtype=torch.int16, device=device)
        self.color = torch.empty((K, height, width, 4), dtype=torch.uint8, device=device)
        cw, ch = (width - 1) // cell + 1, (height - 1) // cell + 1
        yy = torch.clamp(torch.arange(ch, device=device) * cell + 1, max=height - 2)
        xx = torch.clamp(torch.arange(cw, device=device) * cell + 1, max=width - 2)
        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed) & 0x7FFFFFFF)
        surf = []

        def s8(v):
            return (v * 127.0 + torch.where(v > 0, 0.5, -0.5)).to(torch.float32).to(torch.int32).to(torch.int8)

        def s10(v):
            return (v * 511.0 + torch.where(v > 0, 0.5, -0.5)).to(torch.float32).to(torch.int32) & 0x3FF

        for k in range(K):
            R = torch.tensor(Rs[k], **f64)
            t = torch.tensor(ts[k], **f64)
            dg = dirs @ R.T
            denom = dg @ P.T
            num = -(Pd + P @ t)
            tt = num[None, None, :] / denom
            tt = torch.where((denom < 0) & (tt > 0.3), tt, torch.full_like(tt, float("inf")))
            best, which = tt.min(dim=2)
            bestn = P[which]
            valid = torch.isfinite(best) & (best < 6.0)
            if not border_valid:
                valid[0, :] = False; valid[-1, :] = False; valid[:, 0] = False; valid[:, -1] = False
            d = torch.where(valid, best / float(raw_to_float_depth) + 0.5, torch.full_like(best, 65535.0)).to(torch.int64)
            valid &= d < 32768
            d = torch.where(valid, d, torch.full_like(d, 65535))
            self.depth[k] = d.to(torch.int32).to(torch.int16)               # two's complement bit pattern of the u16 value
            n_cam = (bestn @ R).to(torch.float32)
            packed = (s8(n_cam[..., 0]).to(torch.int32) & 0xFF) | ((s8(n_cam[..., 1]).to(torch.int32) & 0xFF) << 8)
            self.normals[k] = torch.where(valid, packed, torch.zeros_like(packed)).to(torch.int16)
            z = d.to(torch.float32) * float(np.float32(raw_to_float_depth))
            r2 = torch.where(valid, (z / float(fx)) ** 2, torch.zeros_like(z)).to(torch.float16)
            self.radius[k] = r2.view(torch.int16)
            pts = t[None, None, :] + dg * torch.where(valid, best, torch.zeros_like(best))[..., None]
            lum = (torch.sin(7.0 * pts[..., 0] + 0.37) + torch.sin(9.0 * pts[..., 1] + 0.5) + torch.sin(11.0 * pts[..., 2] + 0.7)
                   + 0.5 * torch.sin(23.0 * (pts[..., 0] + pts[..., 1])) + 0.5 * torch.cos(17.0 * (pts[..., 1] - pts[..., 2])))
            lum = torch.clamp((lum + 4.0) / 8.0 * 255.0, 0, 255).to(torch.uint8)
            self.color[k] = lum[..., None].expand(-1, -1, 4)
            v = valid[yy][:, xx]
            zc = z[yy][:, xx][v]
            pcam = torch.stack([zc * dxg[yy][:, xx][v].to(torch.float32), zc * dyg[yy][:, xx][v].to(torch.float32), zc], dim=-1).to(torch.float64)
            bn = bestn[yy][:, xx][v]
            pg = pcam @ R.T + t[None, :]
            pg = pg + bn * ((torch.rand((pg.shape[0], 1), generator=gen, **f64) * 2 - 1) * surfel_noise)
            s = torch.zeros((abi.SURFEL_ATTRIBUTE_COUNT, pg.shape[0]), dtype=torch.float32, device=device)
            s[0:3] = pg.T.to(torch.float32)
            bnf = bn.to(torch.float32)
            s[3] = (s10(bnf[:, 0]) | (s10(bnf[:, 1]) << 10) | (s10(bnf[:, 2]) << 20)).view(torch.float32)
            s[4] = r2[yy][:, xx][v].to(torch.float32)
            surf.append(s)
        self.surfels = torch.cat(surf, dim=1).contiguous()
        self.surfels_size = self.surfels.shape[1]
        self.stack.surfels_size = self.surfels_size
        self.active = torch.ones((1, max(1, self.surfels_size)), dtype=torch.uint8, device=device)
        self.cfactor = torch.zeros(self.stack.cfactor.shape, dtype=torch.float32, device=device)

    def host_keyframe(self, k):
        """(depth u16, normals u16, radius u16, color uchar4) of keyframe k copied back to host arrays (oracle comparisons)."""
        g = lambda t: np.ascontiguousarray(t[k].cpu().numpy())
        return g(self.depth).view(np.uint16), g(self.normals).view(np.uint16), g(self.radius).view(np.uint16), g(self.color)
