"""A NumPy restatement of the vertex clustering rule of include/badslam_hip.h "Mesh simplification" (bslam_simplify_mesh,
badslam_amd/csrc/simplify_kernels.hpp), brute force: float32 cell arithmetic in separate operations, np.unique over the cell
triples for the cluster numbering, np.add.at -- unbuffered, so in ascending vertex id -- for the ordered double and integer sums.
No sort of (key, id) pairs, no head flags, no scans.  Also the small meshes the tests share."""
import numpy as np

F = np.float32
CELLS = 1 << 21   # per axis


class Refused(ValueError):
    """What the library answers with BSLAM_ERR_INVALID_ARGUMENT behind its launches."""


def cells(positions, origin, cell_size):
    """(c [V, 3] float32, valid [V]) of the rule: c = floorf((x - origin) * inv) with inv = 1.0f / cell_size."""
    positions = np.ascontiguousarray(positions, F).reshape(-1, 3)
    origin = np.ascontiguousarray(origin, F).reshape(3)
    inv = F(1.0) / F(cell_size)
    with np.errstate(invalid="ignore", over="ignore"):
        d = positions - origin[None, :]          # one fp32 operation
        c = np.floor(d * inv)                    # ... and another
        assert d.dtype == F and c.dtype == F
        valid = np.isfinite(positions).all(axis=1) & (c >= 0).all(axis=1) & (c < CELLS).all(axis=1)
    return c, valid


def simplify(positions, normals, colors, triangles, origin, cell_size):
    """-> dict of positions (C, 3) f32, normals (C, 3) f32 or None, colors (C, 4) u8 or None, triangles (T', 3) u32, vertex_cluster (V,)
    u32.  normals, colors (V, 4) and triangles may be None.  Raises Refused for an invalid vertex or an index >= V."""
    positions = np.ascontiguousarray(positions, F).reshape(-1, 3)
    V = len(positions)
    triangles = np.zeros((0, 3), np.uint32) if triangles is None else np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    if (triangles >= V).any():
        raise Refused("a triangle names a vertex beyond vertex_count")
    c, valid = cells(positions, origin, cell_size)
    if not valid.all():
        raise Refused("a vertex is not finite or lies outside the grid")
    c = c.astype(np.int64)
    # clusters in ascending (c_z, c_y, c_x): np.unique sorts the rows lexicographically, so the columns go (z, y, x)
    _, cluster = np.unique(c[:, ::-1], axis=0, return_inverse=True)
    cluster = cluster.reshape(-1).astype(np.int64)
    C = int(cluster.max()) + 1 if V else 0
    n = np.bincount(cluster, minlength=C).astype(np.int64)
    # the sums start from -0.0, which any first member replaces with its own bits: "a cluster of one keeps its bits"
    sums = np.full((C, 3), -0.0, np.float64)
    np.add.at(sums, cluster, positions.astype(np.float64))
    out = dict(positions=(sums / n[:, None].astype(np.float64)).astype(F), normals=None, colors=None, vertex_cluster=cluster.astype(np.uint32))
    if normals is not None:
        normals = np.ascontiguousarray(normals, F).reshape(-1, 3)
        s = np.full((C, 3), -0.0, np.float64)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            np.add.at(s, cluster, normals.astype(np.float64))
            bad = np.zeros(C, bool)
            np.logical_or.at(bad, cluster, ~np.isfinite(normals).all(axis=1))
            ss = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
            ok = ~bad & (ss > 0)
            unit = (s / np.sqrt(ss)[:, None]).astype(F)
        out["normals"] = np.where(ok[:, None], unit, F(0)).astype(F)
    if colors is not None:
        colors = np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
        total = np.zeros((C, 4), np.uint64)
        np.add.at(total, cluster, colors.astype(np.uint64))
        nn = n[:, None].astype(np.uint64)
        out["colors"] = ((total + nn // np.uint64(2)) // nn).astype(np.uint8)
    mapped = cluster[triangles.astype(np.int64)].reshape(-1, 3)
    keep = (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 0] != mapped[:, 2]) & (mapped[:, 1] != mapped[:, 2])
    out["triangles"] = np.ascontiguousarray(mapped[keep], np.uint32)
    return out


# ------------------------------------------------------------------------------------------------
# meshes
# ------------------------------------------------------------------------------------------------
def plane(n=17):
    """n x n vertices at (i + 0.25, j + 0.25, 0.5), vertex j * n + i, two counter-clockwise (seen from +z) triangles per quad."""
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    positions = np.stack([i + 0.25, j + 0.25, np.full(i.shape, 0.5)], axis=-1).reshape(-1, 3).astype(F)
    v = (j * n + i)[:-1, :-1].reshape(-1)
    triangles = np.concatenate([np.stack([v, v + 1, v + n + 1], axis=1), np.stack([v, v + n + 1, v + n], axis=1)]).astype(np.uint32)
    return positions, triangles


def uv_sphere(segments=96, rings=48, radius=1.0, centre=(1.3, 1.1, 1.2)):
    """A UV sphere: the south pole, rings - 1 rings of `segments` vertices from south to north, the north pole; outward faces.
    96 x 48: 4 514 vertices, 9 024 triangles.  -> (positions f32, outward unit normals f32, triangles u32)."""
    theta = np.pi * np.arange(1, rings) / rings            # from the south pole
    phi = 2.0 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.outer(np.sin(theta), np.cos(phi)), np.outer(np.sin(theta), np.sin(phi)), np.outer(-np.cos(theta), np.ones(segments))], axis=-1)
    unit = np.concatenate([[[0.0, 0.0, -1.0]], ring.reshape(-1, 3), [[0.0, 0.0, 1.0]]])
    positions = (np.asarray(centre) + radius * unit).astype(F)
    at = lambda r, s: 1 + r * segments + (s % segments)
    last = 1 + (rings - 1) * segments
    tri = []
    for s in range(segments):
        tri.append((0, at(0, s + 1), at(0, s)))
        tri.append((last, at(rings - 2, s), at(rings - 2, s + 1)))
    for r in range(rings - 2):
        for s in range(segments):
            a, b, c, d = at(r, s), at(r, s + 1), at(r + 1, s + 1), at(r + 1, s)
            tri.append((a, b, c))
            tri.append((a, c, d))
    return positions, unit.astype(F), np.array(tri, np.uint32)


def face_normals(positions, triangles):
    p = positions.astype(np.float64)
    t = triangles.astype(np.int64)
    return np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])


def edge_counts(triangles):
    """(uses of every undirected edge, uses of every directed edge) as arrays of counts."""
    t = triangles.astype(np.int64)
    directed = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    _, d = np.unique(directed, axis=0, return_counts=True)
    _, u = np.unique(np.sort(directed, axis=1), axis=0, return_counts=True)
    return u, d
