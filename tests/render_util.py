"""NumPy float32 restatement of the model-view rule (bslam_render_surfels, badslam_amd/csrc/render_kernels.hpp, DESIGN.md 8
"Model views"), operation by operation in the kernel's expression order, so that the depth, index and colour views can be
compared bit for bit.  It tests every pixel centre against every surfel: there is no box logic here, a wrong box in the
kernel shows as a missing pixel.  Also the plane scene of the CPU test and small helpers for the GPU tests."""
import numpy as np

from badslam_amd import abi

f32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_INDEX = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------
# packed normals (BS/util_nvcc_only.cuh:67-95)
# ------------------------------------------------------------------------------------------------
def pack_normals(n):
    """(count, 3) normals with components in [-1, 1] -> uint32: three signed 10-bit fields, value * 511 rounded half away from zero."""
    n = np.asarray(n, np.float32)
    q = (n * f32(511) + np.where(n > 0, f32(0.5), f32(-0.5))).astype(np.int16).astype(np.int32) & 0x3ff
    return (q[:, 0] | (q[:, 1] << 10) | (q[:, 2] << 20)).astype(np.uint32)


def packed_fields(packed):
    """The three sign-extended 10-bit integers of packed normals as float32 arrays."""
    p = np.asarray(packed, np.uint32)
    return [((p << np.uint32(shift)).view(np.int32) >> 22).astype(np.float32) for shift in (22, 12, 2)]


def unit_normals(packed):
    """unpack_normal in float64: (count, 3)."""
    n = np.stack([v.astype(np.float64) / 511.0 for v in packed_fields(packed)], -1)
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def surfel_rows(positions, packed_normals, radius_squared, colors=None, columns=None):
    """(8, columns) float32 surfel rows from (count, 3) positions, uint32 packed normals, radius^2 and uint32 colours."""
    count = len(positions)
    rows = np.zeros((abi.SURFEL_DATA_ATTRIBUTE_COUNT, columns or count), np.float32)
    rows[abi.SURFEL_X:abi.SURFEL_Z + 1, :count] = np.asarray(positions, np.float32).T
    rows[abi.SURFEL_NORMAL, :count] = np.asarray(packed_normals, np.uint32).view(np.float32)
    rows[abi.SURFEL_RADIUS_SQUARED, :count] = np.asarray(radius_squared, np.float32)
    if colors is not None:
        rows[abi.SURFEL_COLOR, :count] = np.asarray(colors, np.uint32).view(np.float32)
    return rows


# ------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------
def splat_keys32(rows, surfels_size, camera_T_global, cam, min_depth, max_depth, radius_scale, chunk=128):
    """The two smallest keys per pixel, (best, second) as (h, w) uint64 arrays; key = (float bits of t << 32) | surfel index,
    EMPTY where fewer surfels cover the pixel.  rows: (>= 6, n) float32 surfel rows (bits), camera_T_global: 12 values."""
    rows = np.ascontiguousarray(rows, np.float32)
    m = np.asarray(camera_T_global, np.float32).reshape(12)
    w, h = int(cam.width), int(cam.height)
    fx, fy, cx, cy = f32(cam.fx), f32(cam.fy), f32(cam.cx), f32(cam.cy)
    n = int(surfels_size)
    best = np.full((h, w), EMPTY, np.uint64)
    second = best.copy()
    if n == 0:
        return best, second
    with np.errstate(all="ignore"):
        x, y, z = rows[abi.SURFEL_X, :n], rows[abi.SURFEL_Y, :n], rows[abi.SURFEL_Z, :n]
        live = ~(x != x)
        Lx = ((m[0] * x + m[1] * y) + m[2] * z) + m[3]
        Ly = ((m[4] * x + m[5] * y) + m[6] * z) + m[7]
        Lz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11]
        sx, sy, sz = packed_fields(rows[abi.SURFEL_NORMAL, :n].view(np.uint32))
        nx = (m[0] * sx + m[1] * sy) + m[2] * sz
        ny = (m[4] * sx + m[5] * sy) + m[6] * sz
        nz = (m[8] * sx + m[9] * sy) + m[10] * sz
        r2 = rows[abi.SURFEL_RADIUS_SQUARED, :n] * (f32(radius_scale) * f32(radius_scale))
        live &= r2 > 0
        r = np.sqrt(np.where(r2 > 0, r2, f32(0)))
        live &= (Lz - r >= f32(min_depth)) & (Lz <= f32(max_depth))
        k = (nx * Lx + ny * Ly) + nz * Lz
        live &= k < 0
        dx = ((np.arange(w).astype(np.float32) + f32(0.5)) - cx) / fx
        dy = ((np.arange(h).astype(np.float32) + f32(0.5)) - cy) / fy
        dx, dy = dx[None, None, :], dy[None, :, None]
        index = np.nonzero(live)[0]
        for start in range(0, len(index), chunk):
            s = index[start:start + chunk]
            c = lambda a: a[s][:, None, None]
            den = (c(nx) * dx + c(ny) * dy) + c(nz)
            t = c(k) / den
            hx, hy, hz = t * dx - c(Lx), t * dy - c(Ly), t - c(Lz)
            covered = (den < 0) & ((hx * hx + hy * hy) + hz * hz <= c(r2))
            assert t.dtype == np.float32
            keys = (t.view(np.uint32).astype(np.uint64) << np.uint64(32)) | s.astype(np.uint64)[:, None, None]
            keys[~covered] = EMPTY
            first = keys.min(0)
            np.put_along_axis(keys, keys.argmin(0)[None], EMPTY, 0)
            runner_up = keys.min(0)
            second = np.minimum(np.maximum(best, first), np.minimum(second, runner_up))
            best = np.minimum(best, first)
    return best, second


def depth_bits(keys):
    return (keys >> np.uint64(32)).astype(np.uint32)


def views32(keys, rows, camera_T_global, metres_to_depth):
    """The four views of a key image: depth u16, index u32, colour (h, w, 4) u8 (bits of the colour row), normal (h, w, 3) float64."""
    rows = np.ascontiguousarray(rows, np.float32)
    empty = keys == EMPTY
    index = np.where(empty, NO_INDEX, keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    safe = np.where(empty, 0, index).astype(np.int64)
    with np.errstate(all="ignore"):
        v = f32(metres_to_depth) * depth_bits(keys).view(np.float32) + f32(0.5)
    depth = np.where(~empty & (v < 65536), v, 0).astype(np.uint16)
    color = np.where(empty, np.uint32(0), rows[abi.SURFEL_COLOR].view(np.uint32)[safe]).astype(np.uint32)
    color = np.ascontiguousarray(color).view(np.uint8).reshape(keys.shape + (4,))
    R = np.asarray(camera_T_global, np.float64).reshape(3, 4)[:, :3]
    normal = unit_normals(rows[abi.SURFEL_NORMAL].view(np.uint32)[safe]) @ R.T
    normal[empty] = 0
    return dict(depth=depth, index=index, color=color, normal=normal)


def render32(rows, surfels_size, camera_T_global, cam, min_depth, max_depth, radius_scale, metres_to_depth):
    best, second = splat_keys32(rows, surfels_size, camera_T_global, cam, min_depth, max_depth, radius_scale)
    out = views32(best, rows, camera_T_global, metres_to_depth)
    out["keys"], out["second"] = best, second
    return out


# ------------------------------------------------------------------------------------------------
# poses
# ------------------------------------------------------------------------------------------------
def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def invert(T):
    """(3, 4) rigid transform -> its inverse (3, 4), float64."""
    T = np.asarray(T, np.float64).reshape(3, 4)
    return np.hstack([T[:, :3].T, -T[:, :3].T @ T[:, 3:]])


def mat3x4(T):
    M = abi.Mat3x4()
    M.m[:] = [float(v) for v in np.asarray(T, np.float32).reshape(12)]
    return M


# ------------------------------------------------------------------------------------------------
# the plane scene: a tilted plane seen by a 64 x 48 camera of focal length 60
# ------------------------------------------------------------------------------------------------
PLANE_CAMERA = (60.0, 60.0, 32.0, 24.0, 64, 48)
PLANE_NORMAL = np.array([0.31, -0.22, -0.925])          # in the generating camera's frame, towards the camera
PLANE_POINT = np.array([0.0, 0.0, 1.5])


def plane_camera():
    return abi.Camera4f(*PLANE_CAMERA)


def plane_global_T_camera():
    """The generating pose, (3, 4) float64."""
    return np.hstack([rotation([0.2, 1.0, -0.1], 0.4), np.array([[0.3], [-0.1], [0.2]])])


def plane_depth_at_centres(global_T_view):
    """Exact depth (float64, (h, w)) of the plane along the rays through the pixel centres of a camera at global_T_view."""
    cam = plane_camera()
    G = plane_global_T_camera()
    n = G[:, :3] @ (PLANE_NORMAL / np.linalg.norm(PLANE_NORMAL))
    p = G[:, :3] @ PLANE_POINT + G[:, 3]
    V = np.asarray(global_T_view, np.float64).reshape(3, 4)
    xs, ys = np.meshgrid(np.arange(cam.width), np.arange(cam.height))
    rays = np.stack([(xs + 0.5 - cam.cx) / cam.fx, (ys + 0.5 - cam.cy) / cam.fy, np.ones(xs.shape)], -1) @ V[:, :3].T
    return ((p - V[:, 3]) @ n) / (rays @ n)


def plane_scene(step):
    """Surfels at every step-th pixel centre of the generating view: positions on the plane, the plane's normal packed into
    10 bits per component, radius = distance to the diagonal neighbour (the next one, or the previous one on the last row /
    column).  Returns ((8, n) rows, largest radius)."""
    cam = plane_camera()
    G = plane_global_T_camera()
    depth = plane_depth_at_centres(G)
    xs, ys = np.meshgrid(np.arange(0, cam.width, step), np.arange(0, cam.height, step))
    point = lambda px, py: np.stack([(px + 0.5 - cam.cx) / cam.fx, (py + 0.5 - cam.cy) / cam.fy, np.ones(px.shape)], -1) * depth[py, px][..., None]
    here = point(xs, ys)
    sign_x = np.where(xs + step < cam.width, 1, -1)
    sign_y = np.where(ys + step < cam.height, 1, -1)
    radius = np.linalg.norm(point(xs + sign_x * step, ys + sign_y * step) - here, axis=-1)
    positions = here.reshape(-1, 3) @ G[:, :3].T + G[:, 3]
    normal = G[:, :3] @ (PLANE_NORMAL / np.linalg.norm(PLANE_NORMAL))
    count = len(positions)
    colors = (np.arange(count, dtype=np.uint32) * np.uint32(2654435761)) & np.uint32(0x00FFFFFF)
    rows = surfel_rows(positions, pack_normals(np.tile(normal, (count, 1))), (radius.reshape(-1) ** 2), colors)
    return rows, float(radius.max())

