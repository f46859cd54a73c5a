"""NumPy float32 restatement of the mesh-view rule (bslam_render_mesh, include/badslam_hip.h, DESIGN.md 8 "Mesh views"), written
from the rule, operation by operation in its expression order, so that the depth, index and colour views can be compared bit for
bit and the normal view at 1e-6.  A loop over the triangles with the box of each vectorised.  Also the scenes of
tests/test_render_mesh_cpu.py and tests/test_gpu_render_mesh.py."""
import numpy as np

from badslam_amd import abi
from tests import render_util as ru

f32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_INDEX = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------
def camera_points32(positions, camera_T_global):
    """L = ((m0 x + m1 y) + m2 z) + m3 per row: (V, 3) float32."""
    m = np.asarray(camera_T_global, np.float32).reshape(12)
    p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3] for r in range(3)], -1)


def project32(L, cam):
    """(px, py, vz) of camera-frame points: vz is L.z, NaN where a coordinate is not finite."""
    with np.errstate(all="ignore"):
        px = f32(cam.fx) * (L[:, 0] / L[:, 2]) + f32(cam.cx)
        py = f32(cam.fy) * (L[:, 1] / L[:, 2]) + f32(cam.cy)
    vz = np.where(np.isfinite(L).all(-1), L[:, 2], f32(np.nan)).astype(np.float32)
    return px, py, vz


def edge32(apx, apy, bpx, bpy, px, py):
    """Edge function of (px, py) against the line a -> b."""
    return (bpx - apx) * (py - apy) - (bpy - apy) * (px - apx)


def pixel32(v0, v1, v2, cx, cy):
    """The pixel rule at centres (cx, cy) for vertices v_k = (px, py, z) in ascending vertex id; everything broadcasts.
    Returns (drawn, b0, b1, b2, z), float32."""
    with np.errstate(all="ignore"):
        w0 = edge32(v1[0], v1[1], v2[0], v2[1], cx, cy)
        w1 = -edge32(v0[0], v0[1], v2[0], v2[1], cx, cy)
        w2 = edge32(v0[0], v0[1], v1[0], v1[1], cx, cy)
        covered = ((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0))
        s = (w0 + w1) + w2
        covered &= s != 0
        b0, b1, b2 = (w0 / s) / v0[2], (w1 / s) / v1[2], (w2 / s) / v2[2]
        z = f32(1) / ((b0 + b1) + b2)
        assert z.dtype == np.float32
        return covered & (z > 0), b0, b1, b2, z


def draw_keys32(positions, triangles, camera_T_global, cam, min_depth, max_depth, cull_backfaces):
    """(keys (h, w) uint64, drawn_triangles bool (T,), bad_index): key = (float bits of z << 32) | triangle id, EMPTY where nothing
    is drawn; drawn_triangles marks the triangles that passed the per-triangle tests; bad_index: some index is >= V."""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    L = camera_points32(positions, camera_T_global)
    V = len(L)
    px, py, vz = project32(L, cam)
    w, h = int(cam.width), int(cam.height)
    keys = np.full((h, w), EMPTY, np.uint64)
    passed = np.zeros(len(tri), bool)
    bad_index = False
    lo, hi = f32(min_depth), f32(max_depth)
    half = f32(0.5)
    for t, (a, b, c) in enumerate(tri):
        if a >= V or b >= V or c >= V:
            bad_index = True
            continue
        if a == b or a == c or b == c:
            continue
        if not all(vz[k] >= lo and vz[k] <= hi for k in (a, b, c)):
            continue
        with np.errstate(all="ignore"):
            area = (px[b] - px[a]) * (py[c] - py[a]) - (py[b] - py[a]) * (px[c] - px[a])
        if area == 0 or (cull_backfaces and not area < 0):
            continue
        passed[t] = True
        i0, i1, i2 = sorted((int(a), int(b), int(c)))
        with np.errstate(all="ignore"):
            min_x, max_x = np.fmin(np.fmin(px[i0], px[i1]), px[i2]), np.fmax(np.fmax(px[i0], px[i1]), px[i2])
            min_y, max_y = np.fmin(np.fmin(py[i0], py[i1]), py[i2]), np.fmax(np.fmax(py[i0], py[i1]), py[i2])
            x0 = int(np.fmin(np.fmax(np.ceil(min_x - half), f32(0)), f32(w)))
            x1 = min(int(np.fmax(np.fmin(np.floor(max_x - half), f32(w) - f32(1)), f32(-1))), w - 1)
            y0 = int(np.fmin(np.fmax(np.ceil(min_y - half), f32(0)), f32(h)))
            y1 = min(int(np.fmax(np.fmin(np.floor(max_y - half), f32(h) - f32(1)), f32(-1))), h - 1)
        if x1 < x0 or y1 < y0:
            continue
        cx = (np.arange(x0, x1 + 1).astype(np.float32) + half)[None, :]
        cy = (np.arange(y0, y1 + 1).astype(np.float32) + half)[:, None]
        drawn, _, _, _, z = pixel32(*[(px[k], py[k], vz[k]) for k in (i0, i1, i2)], cx, cy)
        key = (np.ascontiguousarray(z).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
        box = keys[y0:y1 + 1, x0:x1 + 1]
        box[...] = np.where(drawn, np.minimum(box, key), box)
    return keys, passed, bad_index


def resolve32(keys, positions, normals, colors, triangles, camera_T_global, cam, metres_to_depth):
    """The four views of a key image: depth u16, index u32, colour (h, w, 4) u8 (None without colours), normal (h, w, 3) f32."""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    m = np.asarray(camera_T_global, np.float32).reshape(12)
    h, w = keys.shape
    empty = keys == EMPTY
    index = np.where(empty, NO_INDEX, keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    zkey = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        v = f32(metres_to_depth) * zkey + f32(0.5)
    depth = np.where(~empty & (v < 65536), v, 0).astype(np.uint16)
    color = None if colors is None else np.zeros((h, w, 4), np.uint8)
    normal = np.zeros((h, w, 3), np.float32)
    ys, xs = np.nonzero(~empty)
    if len(ys) == 0:
        return dict(depth=depth, index=index, color=color, normal=normal)
    own = tri[index[ys, xs]]                      # (n, 3) in the triangle's own winding
    ids = np.sort(own, axis=1)                    # ascending vertex id
    L = camera_points32(positions, camera_T_global)
    px, py, vz = project32(L, cam)
    cx, cy = xs.astype(np.float32) + f32(0.5), ys.astype(np.float32) + f32(0.5)
    drawn, b0, b1, b2, z = pixel32(*[(px[ids[:, k]], py[ids[:, k]], vz[ids[:, k]]) for k in range(3)], cx, cy)
    assert drawn.all() and np.array_equal(z.view(np.uint32), zkey[ys, xs].view(np.uint32)), "the resolve pass recomputes the key's depth"
    with np.errstate(all="ignore"):
        if colors is not None:
            col = np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
            for ch in range(3):
                c0, c1, c2 = [col[ids[:, k], ch].astype(np.float32) for k in range(3)]
                value = np.fmin(z * ((b0 * c0 + b1 * c1) + b2 * c2) + f32(0.5), f32(255))
                color[ys, xs, ch] = value.astype(np.uint8)
            color[ys, xs, 3] = 255
        if normals is not None:
            nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
            n = [z * ((b0 * nrm[ids[:, 0], k] + b1 * nrm[ids[:, 1], k]) + b2 * nrm[ids[:, 2], k]) for k in range(3)]
            r = [(m[4 * k] * n[0] + m[4 * k + 1] * n[1]) + m[4 * k + 2] * n[2] for k in range(3)]
        else:
            La, Lb, Lc = L[own[:, 0]], L[own[:, 1]], L[own[:, 2]]
            e, f = Lb - La, Lc - La
            r = [e[:, 1] * f[:, 2] - e[:, 2] * f[:, 1], e[:, 2] * f[:, 0] - e[:, 0] * f[:, 2], e[:, 0] * f[:, 1] - e[:, 1] * f[:, 0]]
            away = (r[0] * La[:, 0] + r[1] * La[:, 1]) + r[2] * La[:, 2] > 0
            r = [np.where(away, -v, v) for v in r]
        length = np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
        for k in range(3):
            normal[ys, xs, k] = np.where(length > 0, r[k] / length, f32(0))
    assert normal.dtype == np.float32
    return dict(depth=depth, index=index, color=color, normal=normal)


def render32(mesh, camera_T_global, cam, min_depth, max_depth, cull_backfaces, metres_to_depth):
    """The views of a mesh dict (positions, triangles, optionally normals and colors (V, 4)), plus keys, the triangles that passed
    the per-triangle tests, and bad_index."""
    keys, passed, bad_index = draw_keys32(mesh["positions"], mesh["triangles"], camera_T_global, cam, min_depth, max_depth, cull_backfaces)
    out = resolve32(keys, mesh["positions"], mesh.get("normals"), mesh.get("colors"), mesh["triangles"], camera_T_global, cam, metres_to_depth)
    out.update(keys=keys, passed=passed, bad_index=bad_index)
    return out


# ------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------
IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)


def mesh_dict(positions, triangles, normals=None, colors=None):
    out = dict(positions=np.ascontiguousarray(positions, np.float32).reshape(-1, 3), triangles=np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3))
    if normals is not None:
        out["normals"] = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if colors is not None:
        out["colors"] = np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
    return out


def random_colors(rng, count):
    c = rng.integers(0, 256, (count, 4), dtype=np.uint8)
    c[:, 3] = 255
    return c


def at_pixel(cam, px, py, depth):
    """The camera-frame point that projects to the pixel-corner position (px, py) at `depth`."""
    return np.array([(px - cam.cx) / cam.fx * depth, (py - cam.cy) / cam.fy * depth, depth], np.float64)


def front_facing(cam, corners):
    """Three (px, py, depth) corners -> (3, 3) camera-frame points, ordered so that the triangle is front-facing (A < 0)."""
    (ax, ay, _), (bx, by, _), (cx, cy, _) = corners
    area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    order = (0, 1, 2) if area < 0 else (0, 2, 1)
    return np.stack([at_pixel(cam, *corners[k]) for k in order])


def plane_mesh(n):
    """The plane of tests/render_util.py over the whole generating view, as an n x n grid of quads, two triangles each, front-facing
    for that view: vertices on the plane along the rays through a regular lattice over the image outline (pushed out by a pixel).
    Returns the mesh dict in the global frame."""
    cam = ru.plane_camera()
    G = ru.plane_global_T_camera()
    nrm = ru.PLANE_NORMAL / np.linalg.norm(ru.PLANE_NORMAL)
    us, vs = np.meshgrid(np.linspace(-1.0, cam.width + 1.0, n + 1), np.linspace(-1.0, cam.height + 1.0, n + 1))
    rays = np.stack([(us - cam.cx) / cam.fx, (vs - cam.cy) / cam.fy, np.ones(us.shape)], -1).reshape(-1, 3)
    points = rays * ((ru.PLANE_POINT @ nrm) / (rays @ nrm))[:, None]
    tris = []
    for j in range(n):
        for i in range(n):
            v00, v10, v01, v11 = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i, (j + 1) * (n + 1) + i + 1
            tris += [(v00, v01, v10), (v10, v01, v11)]     # pixel-space area < 0: y runs down
    positions = points @ G[:, :3].T + G[:, 3]
    normals = np.tile(G[:, :3] @ nrm, (len(positions), 1))
    return mesh_dict(positions, tris, normals)


def exact_centre_mesh():
    """A camera with fx = fy = 8 and a fan of four front-facing triangles at z = 1 around vertex 4, whose five vertices project
    exactly onto pixel centres: x = (k + 0.5 - cx) / fx is exact in fp32, and so is fx * (x / 1) + cx.  The four shared edges are
    diagonals through pixel centres.  Every edge value is a small dyadic number and s is +-72 in all four triangles, so the two
    triangles at a shared pixel compute the same quotients and bit-equal depths: the lower id has to win.  Returns (mesh, camera)."""
    cam = abi.Camera4f(8.0, 8.0, 10.0, 8.0, 21, 17)
    centres = [(2, 2), (14, 2), (2, 14), (14, 14), (8, 8)]      # pixel indices (i, j)
    positions = [((i + 0.5 - cam.cx) / cam.fx, (j + 0.5 - cam.cy) / cam.fy, 1.0) for i, j in centres]
    tris = [(4, 1, 0), (4, 3, 1), (4, 2, 3), (4, 0, 2)]        # top, right, bottom, left
    colors = np.array([[250, 10, 10, 255], [10, 250, 10, 255], [10, 10, 250, 255], [200, 200, 10, 255], [128, 128, 128, 255]], np.uint8)
    return mesh_dict(positions, tris, None, colors), cam


def coincident_pair(reverse_second=False):
    """Two triangles over the same three vertices under ids 0 and 1, in a 40 x 30 camera; with reverse_second the second one is
    wound the other way (back-facing).  Returns (mesh, camera)."""
    cam = abi.Camera4f(30.0, 31.0, 19.7, 15.2, 40, 30)
    p = front_facing(cam, [(3.3, 4.1, 1.0), (36.2, 9.7, 1.4), (12.9, 27.6, 1.9)])
    tris = [(0, 1, 2), (0, 2, 1) if reverse_second else (1, 2, 0)]
    colors = np.array([[255, 0, 0, 255], [0, 255, 0, 255], [0, 0, 255, 255]], np.uint8)
    return mesh_dict(p, tris, None, colors), cam


def cooperative_scene(seed=5):
    """One triangle that covers most of a 96 x 64 image, under id 37, among 130 small ones in front of and behind it: ids 0 .. 36
    and 38 .. 63 share its wave, 64 .. 130 lie in the second wave.  Each triangle has vertices of its own.  Returns (mesh, camera)."""
    rng = np.random.default_rng(seed)
    cam = abi.Camera4f(80.0, 78.0, 47.6, 32.3, 96, 64)
    tris = []
    for t in range(131):
        if t == 37:
            tris.append(front_facing(cam, [(-3.0, -2.0, 1.6), (101.0, 5.0, 2.4), (20.0, 75.0, 2.0)]))
            continue
        x, y = rng.uniform(4, 92), rng.uniform(4, 60)
        depth = rng.choice([rng.uniform(0.9, 1.4), rng.uniform(2.6, 3.2)])
        corners = [(x + rng.uniform(-4, 4), y + rng.uniform(-4, 4), depth + rng.uniform(-0.05, 0.05)) for _ in range(3)]
        tris.append(front_facing(cam, corners))
    positions = np.concatenate(tris)
    triangles = np.arange(3 * 131).reshape(131, 3)
    normals = rng.normal(size=(len(positions), 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    return mesh_dict(positions, triangles, normals, random_colors(rng, len(positions))), cam


EDGE_CASES = ("repeated index", "zero-area sliver", "NaN vertex", "nearer than min_depth", "beyond max_depth", "left of the image", "cut by the border",
              "behind the camera")


def edge_case_scene(min_depth, max_depth, seed=9):
    """A 70 x 50 view of a front-facing backdrop of two triangles (ids 0, 1) and, in front of it, one triangle per entry of
    EDGE_CASES (ids 2 ..) followed by an ordinary one.  Returns (mesh, camera, {case: triangle id})."""
    rng = np.random.default_rng(seed)
    cam = abi.Camera4f(55.0, 54.0, 35.4, 24.8, 70, 50)
    mid = 0.5 * (min_depth + max_depth)
    P, T = [], []

    def add(points):
        P.extend(points)
        T.append((len(P) - 3, len(P) - 2, len(P) - 1))

    quad = [at_pixel(cam, x, y, 0.8 * max_depth) for x, y in ((2.0, 3.0), (66.0, 2.0), (3.0, 47.0), (67.0, 46.0))]
    P.extend(quad)
    T += [(0, 2, 1), (1, 2, 3)]
    add(front_facing(cam, [(10.0, 10.0, mid), (20.0, 10.0, mid), (15.0, 20.0, mid)]))
    T[-1] = (T[-1][0], T[-1][0], T[-1][2])                                              # repeated index
    add([at_pixel(cam, x, 30.0, mid) for x in (10.0, 10.0, 30.0)])                     # two vertices at one position: a sliver of area exactly 0
    add(front_facing(cam, [(30.0, 8.0, mid), (42.0, 9.0, mid), (35.0, 19.0, mid)]))
    P[-2] = np.array([np.nan, P[-2][1], P[-2][2]])                                     # NaN vertex
    add(front_facing(cam, [(44.0, 20.0, mid), (58.0, 22.0, 0.5 * min_depth), (50.0, 33.0, mid)]))      # one vertex nearer than min_depth
    add(front_facing(cam, [(5.0, 35.0, 1.2 * max_depth), (18.0, 36.0, 1.3 * max_depth), (9.0, 46.0, 1.2 * max_depth)]))   # beyond max_depth
    add(front_facing(cam, [(-30.0, 10.0, mid), (-12.0, 12.0, mid), (-20.0, 30.0, mid)]))              # wholly left of the image
    add(front_facing(cam, [(60.0, 30.0, mid), (82.0, 34.0, mid), (64.0, 58.0, mid)]))                 # cut by the right and bottom border
    add(front_facing(cam, [(25.0, 34.0, mid), (37.0, 35.0, mid), (30.0, 45.0, mid)]))
    P[-1] = at_pixel(cam, 30.0, 45.0, -mid)                                            # a vertex behind the camera
    add(front_facing(cam, [(46.0, 4.0, mid), (60.0, 6.0, 1.1 * mid), (52.0, 16.0, 0.9 * mid)]))        # an ordinary triangle
    positions = np.array(P)
    normals = rng.normal(size=(len(positions), 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    return mesh_dict(positions, T, normals, random_colors(rng, len(positions))), cam, {name: 2 + k for k, name in enumerate(EDGE_CASES)}
