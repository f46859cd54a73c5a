"""Helpers of the sensor-rectification tests: the radtan camera model in NumPy float64 with its Gauss-Newton inverse, NumPy
float32 restatements of the undistortion-map and bilinear kernels in the kernels' expression order
(badslam_amd/csrc/rectify_kernels.hpp), a float64 restatement of the depth rasteriser from its rules (include/badslam_hip.h,
bslam_reproject_depth), a ray-caster for the plane scenes that takes per-pixel rays and a pose, and the device plumbing.

Conventions: a radtan camera (abi.RadtanCamera) is pixel-CENTRE, the centre of pixel (x, y) at (x, y); abi.Camera4f is
pixel-CORNER, the centre at (x + 0.5, y + 0.5)."""
import ctypes as C

import numpy as np

from badslam_amd import abi

f32 = np.float32
FLT_EPSILON = f32(1.1920929e-07)


# ------------------------------------------------------------------------------------------------
# radtan model, float64
# ------------------------------------------------------------------------------------------------
def distort64(cam, x, y):
    """RadtanDistortion5::Project on normalised points."""
    k1, k2, k3, p1, p2 = (float(v) for v in (cam.k1, cam.k2, cam.k3, cam.p1, cam.p2))
    x2, y2, xy = x * x, y * y, x * y
    r2 = x2 + y2
    radial = k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    return x + x * radial + 2 * p1 * xy + p2 * (r2 + 2 * x2), y + y * radial + 2 * p2 * xy + p1 * (r2 + 2 * y2)


def undistort64(cam, dx, dy, iterations=100):
    """The inverse by Gauss-Newton with a numerical-free Jacobian; runs all points for the full number of useful iterations."""
    k1, k2, k3, p1, p2 = (float(v) for v in (cam.k1, cam.k2, cam.k3, cam.p1, cam.p2))
    x, y = np.array(dx, np.float64), np.array(dy, np.float64)
    for _ in range(iterations):
        fx_, fy_ = distort64(cam, x, y)
        rx, ry = fx_ - dx, fy_ - dy
        if max(np.abs(rx).max(), np.abs(ry).max()) < 1e-15:
            break
        x2, y2, xy = x * x, y * y, x * y
        r2 = x2 + y2
        radial = k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
        dradial = k1 + 2 * k2 * r2 + 3 * k3 * r2 * r2
        j00 = 1 + radial + 2 * x2 * dradial + 2 * p1 * y + 6 * p2 * x
        j01 = 2 * xy * dradial + 2 * p1 * x + 2 * p2 * y
        j11 = 1 + radial + 2 * y2 * dradial + 6 * p1 * y + 2 * p2 * x
        det = j00 * j11 - j01 * j01
        x = x - (j11 * rx - j01 * ry) / det
        y = y - (j00 * ry - j01 * rx) / det
    return x, y


def pixel_grid(width, height):
    xs, ys = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    return xs, ys


def unprojection_map64(cam):
    """(h, w, 2) float64: normalised undistorted (x, y) of every raw pixel centre."""
    xs, ys = pixel_grid(cam.width, cam.height)
    x, y = undistort64(cam, (xs - float(cam.cx)) / float(cam.fx), (ys - float(cam.cy)) / float(cam.fy))
    return np.stack([x, y], -1)


def source_position64(source, target, xs, ys):
    """Where the rays through the centres of the target pixels (xs, ys) land in the source image (pixel-centre), unclamped."""
    nx, ny = (xs + 0.5 - float(target.cx)) / float(target.fx), (ys + 0.5 - float(target.cy)) / float(target.fy)
    dx, dy = distort64(source, nx, ny)
    return float(source.fx) * dx + float(source.cx), float(source.fy) * dy + float(source.cy)


def undistortion_map64(source, target):
    xs, ys = pixel_grid(target.width, target.height)
    px, py = source_position64(source, target, xs, ys)
    # the clamp's upper end is the fp32 value float(w - 1) - FLT_EPSILON, which is w - 1
    hi_x, hi_y = float(f32(source.width - 1) - FLT_EPSILON), float(f32(source.height - 1) - FLT_EPSILON)
    return np.stack([np.clip(px, 0.0, hi_x), np.clip(py, 0.0, hi_y)], -1), np.stack([px, py], -1)


# ------------------------------------------------------------------------------------------------
# float32 restatements in the kernels' expression order
# ------------------------------------------------------------------------------------------------
def undistortion_map32(source, target):
    xs, ys = pixel_grid(target.width, target.height)
    xs, ys = xs.astype(f32), ys.astype(f32)
    s = {n: f32(getattr(source, n)) for n in ("fx", "fy", "cx", "cy", "k1", "k2", "k3", "p1", "p2")}
    nx = ((xs + f32(0.5)) - f32(target.cx)) / f32(target.fx)
    ny = ((ys + f32(0.5)) - f32(target.cy)) / f32(target.fy)
    mx2, my2, mxy = nx * nx, ny * ny, nx * ny
    rho2 = mx2 + my2
    rad = (s["k1"] * rho2 + (s["k2"] * rho2) * rho2) + ((s["k3"] * rho2) * rho2) * rho2
    dx = ((nx + nx * rad) + (f32(2) * s["p1"]) * mxy) + s["p2"] * (rho2 + f32(2) * mx2)
    dy = ((ny + ny * rad) + (f32(2) * s["p2"]) * mxy) + s["p1"] * (rho2 + f32(2) * my2)
    px = np.minimum(np.maximum(s["fx"] * dx + s["cx"], f32(0)), f32(source.width - 1) - FLT_EPSILON)
    py = np.minimum(np.maximum(s["fy"] * dy + s["cy"], f32(0)), f32(source.height - 1) - FLT_EPSILON)
    out = np.stack([px, py], -1)
    assert out.dtype == f32
    return out


def undistort_rgb32(image, mapping):
    """image (h, w, 3) u8, mapping (oh, ow, 2) float32 -> (oh, ow, 3) u8."""
    h, w = image.shape[:2]
    mx = np.minimum(np.maximum(mapping[..., 0], f32(0)), f32(w - 1))
    my = np.minimum(np.maximum(mapping[..., 1], f32(0)), f32(h - 1))
    ix, iy = np.minimum(mx.astype(np.int32), w - 2), np.minimum(my.astype(np.int32), h - 2)
    fx, fy = mx - ix.astype(f32), my - iy.astype(f32)
    one = f32(1)
    w00, w10, w01, w11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
    img = image.astype(f32)
    a, b, c, d = img[iy, ix], img[iy, ix + 1], img[iy + 1, ix], img[iy + 1, ix + 1]
    v = ((w00[..., None] * a + w10[..., None] * b) + w01[..., None] * c) + w11[..., None] * d
    assert v.dtype == f32
    return (v + f32(0.5)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------
# the depth rasteriser, float64, from rules 1-6 of its description
# ------------------------------------------------------------------------------------------------
def reproject_depth64(depth, input_depth_to_metres, unprojection, T, target, threshold, output_metres_to_depth, edge_band=1e-3):
    """depth (h, w) u16, unprojection (h, w, 2) float32 (as uploaded), T 3x4 or None.  Returns (u16 image of the target's size,
    bool image: the pixel centre lies within edge_band pixels of an edge line of a triangle whose box contains it)."""
    h, w = depth.shape
    tw, th = target.width, target.height
    M = np.eye(4)[:3] if T is None else np.asarray(T, np.float64).reshape(3, 4)
    d = depth.astype(np.float64) * float(f32(input_depth_to_metres))
    pts = np.stack([d * unprojection[..., 0].astype(np.float64), d * unprojection[..., 1].astype(np.float64), d], -1)
    pts = pts @ M[:, :3].T + M[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        px = float(target.fx) * (pts[..., 0] / pts[..., 2]) + float(target.cx)
        py = float(target.fy) * (pts[..., 1] / pts[..., 2]) + float(target.cy)
    z = pts[..., 2]
    zbuf = np.full((th, tw), np.inf)
    near_edge = np.zeros((th, tw), bool)
    for y in range(h - 1):
        for x in range(w - 1):
            quad = [(y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1)]
            dd = [d[q] for q in quad]
            if min(dd) <= 0:
                continue
            if not max(abs(dd[a] - dd[b]) for a in range(4) for b in range(a + 1, 4)) < float(f32(threshold)):
                continue
            if any(z[q] < 0.05 or z[q] > 50 for q in quad):
                continue
            for tri in ((quad[0], quad[1], quad[2]), (quad[1], quad[3], quad[2])):
                vx, vy, vz = [px[q] for q in tri], [py[q] for q in tri], [z[q] for q in tri]
                area = (vx[1] - vx[0]) * (vy[2] - vy[0]) - (vy[1] - vy[0]) * (vx[2] - vx[0])
                if area == 0:
                    continue
                i0, i1 = max(int(np.ceil(min(vx) - 0.5)), 0), min(int(np.floor(max(vx) - 0.5)), tw - 1)
                j0, j1 = max(int(np.ceil(min(vy) - 0.5)), 0), min(int(np.floor(max(vy) - 0.5)), th - 1)
                if i0 > i1 or j0 > j1:
                    continue
                cx, cy = np.meshgrid(np.arange(i0, i1 + 1) + 0.5, np.arange(j0, j1 + 1) + 0.5)
                e = []
                for a, b in ((1, 2), (2, 0), (0, 1)):
                    value = (vx[b] - vx[a]) * (cy - vy[a]) - (vy[b] - vy[a]) * (cx - vx[a])
                    e.append(value)
                    length = np.hypot(vx[b] - vx[a], vy[b] - vy[a])
                    near_edge[j0:j1 + 1, i0:i1 + 1] |= np.abs(value) < edge_band * length
                inside = ((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0))
                s = e[0] + e[1] + e[2]
                with np.errstate(divide="ignore", invalid="ignore"):
                    zz = 1.0 / (e[0] / s / vz[0] + e[1] / s / vz[1] + e[2] / s / vz[2])
                zz = np.where(inside & (s != 0), zz, np.inf)
                view = zbuf[j0:j1 + 1, i0:i1 + 1]
                np.minimum(view, zz, out=view)
    r = float(f32(output_metres_to_depth)) * np.where(np.isfinite(zbuf), zbuf, 0.0) + 0.5
    out = np.where(np.isfinite(zbuf) & (r < 65536), r, 0).astype(np.uint16)
    return out, near_edge


# ------------------------------------------------------------------------------------------------
# plane scenes seen by an arbitrary camera
# ------------------------------------------------------------------------------------------------
def cast_planes(rays_xy, R, t, planes, offset=2.5):
    """The geometry of scenes.render_planes for per-pixel unit-z rays (h, w, 2) of a camera at global_T_camera = (R, t): nearest
    front-facing intersection with the planes {n.x + offset = 0}.  Returns (z-depth in the camera frame, inf = none; plane index;
    global ray directions; camera centre)."""
    rays = np.concatenate([rays_xy.astype(np.float64), np.ones(rays_xy.shape[:2] + (1,))], -1)
    dg = rays @ np.asarray(R, np.float64).T
    o = np.asarray(t, np.float64)
    best = np.full(rays.shape[:2], np.inf)
    best_plane = np.zeros(rays.shape[:2], np.int32)
    for pi, n in enumerate(planes):
        n64 = n.astype(np.float64)
        denom = dg @ n64
        num = -(offset + o @ n64)
        with np.errstate(divide="ignore", invalid="ignore"):
            tt = num / denom
        tt = np.where((denom < 0) & (tt > 0.3), tt, np.inf)
        upd = tt < best
        best = np.where(upd, tt, best)
        best_plane = np.where(upd, pi, best_plane)
    return best, best_plane, dg, o


def pinhole_rays(cam):
    """(h, w, 2) unit-z rays through the pixel centres of a pixel-corner abi.Camera4f."""
    xs, ys = pixel_grid(cam.width, cam.height)
    return np.stack([(xs + 0.5 - float(cam.cx)) / float(cam.fx), (ys + 0.5 - float(cam.cy)) / float(cam.fy)], -1)


def pinhole_of(radtan):
    """The pixel-corner pinhole camera with a radtan camera's fx, fy, cx, cy and size (its undistorted twin when k = p = 0)."""
    return abi.Camera4f(radtan.fx, radtan.fy, radtan.cx + 0.5, radtan.cy + 0.5, radtan.width, radtan.height)


# ------------------------------------------------------------------------------------------------
# device plumbing
# ------------------------------------------------------------------------------------------------
def stream_ptr(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def pitched(torch, array, pad_elems, fill, elems_per_pixel=1):
    """Device copy of a 2-D host array in rows of (columns + pad_elems) elements, the padding holding `fill`.
    Returns (storage tensor, abi.Buffer2D whose width counts pixels of elems_per_pixel elements)."""
    array = np.ascontiguousarray(array)
    h, cols = array.shape
    signed = {np.dtype(np.uint16): np.int16}.get(array.dtype)
    host = array.view(signed) if signed else array
    storage = torch.full((h, cols + pad_elems), fill, dtype=torch.from_numpy(host[:1, :1].copy()).dtype, device="cuda")
    storage[:, :cols] = torch.from_numpy(host).cuda()
    return storage, abi.Buffer2D(storage.data_ptr(), h, cols // elems_per_pixel, storage.stride(0) * storage.element_size())


def fetch(storage, cols, dtype):
    """(image part, padding part) of a pitched storage tensor as host arrays of `dtype`."""
    host = storage.cpu().numpy()
    return np.ascontiguousarray(host[:, :cols]).view(dtype), host[:, cols:]
