"""NumPy float32 restatement of the surface view rule (csrc/raycast_kernels.hpp), brute force: every ray visits every sample k
until it ends; no blocks, no flags, no validity bits, no clip of the walked range.  The GPU tests compare the kernels with it:
depth and colour bit for bit, normals at 1e-6."""
import numpy as np

from tests.fusion_util import fma32

F = np.float32
MAX_SAMPLES = 65536


def sample_count(min_depth, max_depth, step):
    """N: the number of k >= 0 with fmaf(float(k), step, min_depth) <= max_depth (t is monotone in k)."""
    t = fma32(np.arange(MAX_SAMPLES + 2).astype(F), F(step), F(min_depth))
    n = int((t <= F(max_depth)).sum())
    if n > MAX_SAMPLES:
        raise ValueError("more than 65536 samples per ray")
    return n


def lerp(a, b, w):
    with np.errstate(all="ignore"):
        return fma32(w, (np.asarray(b, F) - np.asarray(a, F)).astype(F), a)


class Volume:
    """tsdf f32, count u32 [nz, ny, nx], colour u8 [nz, ny, nx, 4] or None; sample i lies at origin + (i + 0.5) * voxel."""

    def __init__(self, tsdf, count, color, origin, voxel, min_count=1):
        self.tsdf = np.ascontiguousarray(tsdf, F)
        self.color = None if color is None else np.ascontiguousarray(color, np.uint8)
        self.origin = np.asarray(origin, F)
        self.voxel = F(voxel)
        self.inv_voxel = F(1.0) / F(voxel)
        nz, ny, nx = self.tsdf.shape
        self.dims = (nx, ny, nz)
        observed = np.asarray(count) >= min_count
        valid = np.ones((nz - 1, ny - 1, nx - 1), bool)
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    valid &= observed[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
        self.cell_valid = valid

    def corners(self, cx, cy, cz, of=None):
        """D[corner] with corner = dz * 4 + dy * 2 + dx, of the tsdf (or of another sample array)."""
        a = self.tsdf if of is None else of
        return [a[cz + (c >> 2), cy + ((c >> 1) & 1), cx + (c & 1)] for c in range(8)]


def sample(vol, G, dx, dy, t):
    """-> (in_range, (cx, cy, cz) int with 0 where out of range, (fx, fy, fz) f32) of the point at depth t of the rays (dx, dy)."""
    with np.errstate(all="ignore"):
        t = np.broadcast_to(np.asarray(t, F), dx.shape)
        a, b = (dx * t).astype(F), (dy * t).astype(F)
        in_range = np.ones(dx.shape, bool)
        cells, fracs = [], []
        for r in range(3):
            P = fma32(G[r, 2], t, fma32(G[r, 1], b, fma32(G[r, 0], a, G[r, 3])))
            g = (((P - vol.origin[r]).astype(F) * vol.inv_voxel).astype(F) - F(0.5)).astype(F)
            c = np.floor(g).astype(F)
            in_range &= (g >= 0) & (c <= F(vol.dims[r] - 2))
            cells.append(c)
            fracs.append((g - c).astype(F))
        cells = [np.where(in_range, c, 0).astype(np.int64) for c in cells]
    return in_range, cells, fracs


def value(D, f):
    e00, e10, e01, e11 = lerp(D[0], D[1], f[0]), lerp(D[2], D[3], f[0]), lerp(D[4], D[5], f[0]), lerp(D[6], D[7], f[0])
    return lerp(lerp(e00, e10, f[1]), lerp(e01, e11, f[1]), f[2])


def gradient(D, f):
    e00, e10, e01, e11 = lerp(D[0], D[1], f[0]), lerp(D[2], D[3], f[0]), lerp(D[4], D[5], f[0]), lerp(D[6], D[7], f[0])
    gx = (lerp(lerp(D[1], D[3], f[1]), lerp(D[5], D[7], f[1]), f[2]) - lerp(lerp(D[0], D[2], f[1]), lerp(D[4], D[6], f[1]), f[2])).astype(F)
    gy = (lerp(e10, e11, f[2]) - lerp(e00, e01, f[2])).astype(F)
    gz = (lerp(e01, e11, f[1]) - lerp(e00, e10, f[1])).astype(F)
    return gx, gy, gz


def raycast(vol, global_T_camera, camera, min_depth, max_depth, step, metres_to_depth):
    """camera: anything with fx, fy, cx, cy (pixel-corner), width, height.  -> dict of depth u16 (h, w), color u8 (h, w, 4),
    normal f32 (h, w, 3), hit bool (h, w), t f32 (h, w) (t* at the hits) and samples = N."""
    G = np.asarray(global_T_camera, F).reshape(3, 4)
    w, h = int(camera.width), int(camera.height)
    step, min_depth = F(step), F(min_depth)
    N = sample_count(min_depth, max_depth, step)
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    dx = (((ii.ravel().astype(F) + F(0.5)) - F(camera.cx)) / F(camera.fx)).astype(F)
    dy = (((jj.ravel().astype(F) + F(0.5)) - F(camera.cy)) / F(camera.fy)).astype(F)
    pixels = w * h
    end_k = np.full(pixels, -1, np.int64)
    end_F = np.zeros(pixels, F)
    active = np.arange(pixels)
    for k in range(N):
        if len(active) == 0:
            break
        t = fma32(F(k), step, min_depth)
        in_range, c, f = sample(vol, G, dx[active], dy[active], t)
        valid = in_range & vol.cell_valid[c[2], c[1], c[0]]
        Fk = value(vol.corners(*c), f)
        with np.errstate(all="ignore"):
            end = valid & (Fk < 0)
        end_k[active[end]] = k
        end_F[active[end]] = Fk[end]
        active = active[~end]

    hit = np.zeros(pixels, bool)
    t_hit = np.zeros(pixels, F)
    normal = np.zeros((pixels, 3), F)
    color = np.zeros((pixels, 4), np.uint8)
    cand = np.nonzero(end_k >= 1)[0]
    if len(cand):
        tb = fma32((end_k[cand] - 1).astype(F), step, min_depth)
        in_range, c, f = sample(vol, G, dx[cand], dy[cand], tb)
        valid = in_range & vol.cell_valid[c[2], c[1], c[0]]
        Fb = value(vol.corners(*c), f)
        with np.errstate(all="ignore"):
            ok = valid & (Fb >= 0)
            ts = (tb + (step * (Fb / (Fb - end_F[cand])).astype(F)).astype(F)).astype(F)
        hit[cand[ok]] = True
        t_hit[cand[ok]] = ts[ok]
    rays = np.nonzero(hit)[0]
    if len(rays):
        in_a, ca, fa = sample(vol, G, dx[rays], dy[rays], t_hit[rays])
        use_a = in_a & vol.cell_valid[ca[2], ca[1], ca[0]]
        _, ck, fk = sample(vol, G, dx[rays], dy[rays], fma32(end_k[rays].astype(F), step, min_depth))
        c = [np.where(use_a, a, b) for a, b in zip(ca, ck)]
        f = [np.where(use_a, a, b).astype(F) for a, b in zip(fa, fk)]
        g = gradient(vol.corners(*c), f)
        with np.errstate(all="ignore"):
            r = [((G[0, a] * g[0] + G[1, a] * g[1]).astype(F) + G[2, a] * g[2]).astype(F) for a in range(3)]
            length = np.sqrt(((r[0] * r[0] + r[1] * r[1]).astype(F) + r[2] * r[2]).astype(F)).astype(F)
            normal[rays] = np.stack([np.where(length == 0, F(0), ri / length) for ri in r], axis=1).astype(F)
        if vol.color is not None:
            W = np.zeros(len(rays), F)
            S = [np.zeros(len(rays), F) for _ in range(3)]
            for corner in range(8):
                texel = vol.color[c[2] + (corner >> 2), c[1] + ((corner >> 1) & 1), c[0] + (corner & 1)]
                wx = f[0] if corner & 1 else (F(1) - f[0]).astype(F)
                wy = f[1] if corner & 2 else (F(1) - f[1]).astype(F)
                wz = f[2] if corner & 4 else (F(1) - f[2]).astype(F)
                wgt = ((wx * wy).astype(F) * wz).astype(F)
                has = texel[:, 3] == 255
                W = np.where(has, W + wgt, W).astype(F)
                for ch in range(3):
                    S[ch] = np.where(has, S[ch] + (wgt * texel[:, ch].astype(F)).astype(F), S[ch]).astype(F)
            with np.errstate(all="ignore"):
                some = W > 0
                for ch in range(3):
                    color[rays, ch] = np.where(some, np.trunc(np.where(some, S[ch] / W, 0).astype(F) + F(0.5)), 0).astype(np.uint8)
                color[rays, 3] = np.where(some, 255, 0)
    with np.errstate(all="ignore"):
        v = (F(metres_to_depth) * t_hit + F(0.5)).astype(F)
        depth = np.where(hit & (v < 65536), np.trunc(v), 0).astype(np.uint16)
    return dict(depth=depth.reshape(h, w), color=color.reshape(h, w, 4), normal=normal.reshape(h, w, 3), hit=hit.reshape(h, w), t=t_hit.reshape(h, w), samples=N)
