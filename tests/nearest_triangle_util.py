"""NumPy float32 restatement of the nearest-triangle rule (include/badslam_hip.h "Nearest triangle", csrc/bvh_kernels.hpp), brute
force over all N x T pairs: no tree, no sorting, no pruning.  The GPU tests compare the kernels with this, bit for bit.  Also: the
checker of the tree bslam_debug_nearest_triangle_tree returns, and the fixtures both test files use."""
import numpy as np

from tests import point_mesh_util as pm
from tests.fusion_util import fma32

F = np.float32
NO_TRIANGLE = pm.NO_TRIANGLE
NO_NODE = 0xFFFFFFFF
KEY_BITS = 30
HEIGHT_BOUND = KEY_BITS + 32          # delta grows strictly on the way down: 30 key bits, then 32 index bits


def box_d2(p, lo, hi):
    """b2 of the rule for arrays [..., 3]: per axis max(lo - p, p - hi, 0), squared and summed in the nesting of dot."""
    with np.errstate(all="ignore"):
        e = np.maximum(np.maximum(lo - p, p - hi), F(0)).astype(F)
        return fma32(e[..., 2], e[..., 2], fma32(e[..., 1], e[..., 1], e[..., 0] * e[..., 0]))


def triangle_boxes(positions, triangles):
    """(valid [T], lo [T, 3], hi [T, 3]): nine finite coordinates, the component-wise float32 minimum and maximum."""
    tri = np.asarray(positions, F).reshape(-1, 3)[np.asarray(triangles, np.int64).reshape(-1, 3)]
    valid = np.isfinite(tri).all(axis=(1, 2))
    with np.errstate(all="ignore"):
        return valid, tri.min(axis=1), tri.max(axis=1)


def pair_values(points, positions, triangles):
    """[N, T] float32: d2 of the rule for every pair, +inf for an invalid triangle.  Points have to be finite."""
    points = np.asarray(points, F).reshape(-1, 3)
    positions = np.asarray(positions, F).reshape(-1, 3)
    tri = positions[np.asarray(triangles, np.int64).reshape(-1, 3)]
    valid, lo, hi = triangle_boxes(positions, triangles)
    out = np.empty((len(points), len(tri)), F)
    for start in range(0, len(points), 64):
        p = np.broadcast_to(points[start:start + 64, None, :], (len(points[start:start + 64]), len(tri), 3))
        with np.errstate(all="ignore"):
            d = np.maximum(pm.pair_d2(p, tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]), box_d2(p, lo[None], hi[None]))
        out[start:start + 64] = np.where(valid[None, :], d, F(np.inf))
    return out


def nearest_triangle(points, positions, triangles, R=np.inf):
    """-> (distance f32 [N], triangle u32 [N]): the rule over all N x T pairs; R = inf: no radius."""
    points = np.asarray(points, F).reshape(-1, 3)
    triangles = np.asarray(triangles, np.int64).reshape(-1, 3)
    N = len(points)
    best = np.full(N, np.inf, F)
    which = np.full(N, NO_TRIANGLE, np.int64)
    finite = np.isfinite(points).all(axis=1)
    if len(triangles) and finite.any():
        d = pair_values(points[finite], positions, triangles)
        best[finite] = d.min(axis=1)
        which[finite] = d.argmin(axis=1)                                       # the first, that is the lowest, index of the minimum
    with np.errstate(all="ignore"):
        hit = np.isfinite(best) & (best <= F(R) * F(R))
        return np.where(hit, np.sqrt(best), F(np.inf)).astype(F), np.where(hit, which, NO_TRIANGLE).astype(np.uint32)


# ----------------------------------------------------------------------------- the tree

def order_key(x):
    """uint32 keys whose unsigned order is the float order (and -0 < +0): minima and maxima of boxes are taken on these."""
    u = np.ascontiguousarray(x, F).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def check_tree(tree, positions, triangles):
    """tree: dict of leaves, parent [2 L - 1], children [2 (L - 1)], boxes [2 L - 1, 6], leaf_triangle [L] in the form of
    bslam_debug_nearest_triangle_tree.  Asserts what the query relies on; -> the height (edges to the deepest leaf)."""
    valid, lo, hi = triangle_boxes(positions, triangles)
    L = int(tree["leaves"])
    assert L == int(valid.sum()), f"{L} leaves for {int(valid.sum())} valid triangles"
    if L == 0:
        return 0
    I = L - 1
    parent = np.asarray(tree["parent"], np.int64)
    children = np.asarray(tree["children"], np.int64).reshape(I, 2)
    boxes = np.asarray(tree["boxes"], F).reshape(2 * L - 1, 6)
    leaf_triangle = np.asarray(tree["leaf_triangle"], np.int64)
    # every valid triangle in exactly one leaf, no invalid one in any
    assert np.array_equal(np.sort(leaf_triangle), np.flatnonzero(valid)), "the leaves are not the valid triangles, each once"
    # one root; every internal node has two children whose parent it is; every other node is somebody's child exactly once
    assert parent[0] == NO_NODE and np.count_nonzero(parent == NO_NODE) == 1, "not exactly one root, node 0"
    assert ((children >= 1) & (children < 2 * L - 1)).all() if I else True, "a child reference leaves the tree"
    if I:
        assert np.array_equal(np.sort(children.reshape(-1)), np.arange(1, 2 * L - 1)), "a node is the child of none or of several"
        assert np.array_equal(parent[children[:, 0]], np.arange(I)) and np.array_equal(parent[children[:, 1]], np.arange(I)), "a child's parent is another node"
    # the leaves' boxes are their triangles', bit for bit in value (the sign of a zero is the minimum's business)
    assert np.array_equal(boxes[I:, :3], lo[leaf_triangle]) and np.array_equal(boxes[I:, 3:], hi[leaf_triangle]), "a leaf's box is not its triangle's"
    # depth of every node from the root; the parents form a tree, so this ends
    depth = np.full(2 * L - 1, -1, np.int64)
    depth[0] = 0
    frontier = np.array([0], np.int64)
    while len(frontier):
        inner = frontier[frontier < I]
        kids = children[inner].reshape(-1)
        assert (depth[kids] == -1).all(), "a cycle"
        depth[kids] = np.repeat(depth[inner] + 1, 2)
        frontier = kids
    assert (depth >= 0).all(), "a node is not below the root"
    height = int(depth[I:].max())
    assert height <= HEIGHT_BOUND, f"height {height} beyond the bound {HEIGHT_BOUND}"
    # every node's box = the min and max of the leaves' boxes below it: fold the leaves up, deepest level first
    lo_key = np.full((2 * L - 1, 3), 0xFFFFFFFF, np.uint32)
    hi_key = np.zeros((2 * L - 1, 3), np.uint32)
    lo_key[I:], hi_key[I:] = order_key(boxes[I:, :3]), order_key(boxes[I:, 3:])
    for level in range(int(depth.max()), 0, -1):
        nodes = np.flatnonzero(depth == level)
        np.minimum.at(lo_key, parent[nodes], lo_key[nodes])
        np.maximum.at(hi_key, parent[nodes], hi_key[nodes])
    got_lo, got_hi = order_key(boxes[:, :3]), order_key(boxes[:, 3:])
    bad = (got_lo != lo_key).any(axis=1) | (got_hi != hi_key).any(axis=1)
    assert not bad.any(), f"{int(bad.sum())} boxes are not the bounds of their leaves, first node {np.flatnonzero(bad)[0]} at depth {depth[np.flatnonzero(bad)[0]]}"
    return height


# ----------------------------------------------------------------------------- fixtures

def plane_mesh(n=9, step=0.37, z=1.3):
    """An axis-aligned n x n vertex plane at height z: every box has zero thickness and every z key is equal."""
    xs = np.arange(n, dtype=F) * F(step)
    gx, gy = np.meshgrid(xs, xs, indexing="ij")
    positions = np.stack([gx.ravel(), gy.ravel(), np.full(n * n, F(z))], -1).astype(F)
    idx = lambda i, j: i * n + j
    triangles = np.array([[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)] for i in range(n - 1) for j in range(n - 1)] +
                         [[idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)] for i in range(n - 1) for j in range(n - 1)], np.uint32)
    return np.ascontiguousarray(positions, F), np.ascontiguousarray(triangles, np.uint32)


def plane_points(count=300, seed=3):
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(-1, 4, (count, 3)), F)


def scaled_about(positions, centre, factor):
    """positions scaled by `factor` about `centre`, in float64, rounded to float32."""
    c = np.asarray(centre, np.float64)
    return np.ascontiguousarray((np.asarray(positions, np.float64) - c) * factor + c, F)


class RestatementBA:
    """Stands in for a DirectBA where only NearestTriangle is called: the restatement on the CPU."""

    def NearestTriangle(self, points, mesh, max_distance=None):
        positions = np.asarray(mesh["positions"], F).reshape(-1, 3)
        triangles = mesh.get("triangles")
        if triangles is None or len(triangles) == 0:
            triangles = np.repeat(np.arange(len(positions), dtype=np.uint32)[:, None], 3, axis=1)
        d, t = nearest_triangle(points, positions, triangles, np.inf if max_distance is None else max_distance)
        return dict(distance=d, triangle=t, leaves=int(triangle_boxes(positions, triangles)[0].sum()), height=0)
