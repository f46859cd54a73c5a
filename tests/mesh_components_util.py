"""Brute-force restatement of the mesh component rule (include/badslam_hip.h, DESIGN.md 8 "Mesh components"): a sequential
union-find in plain Python and the filter as index arithmetic.  No atomics, no path tricks shared with the kernels of
csrc/mesh_kernels.hpp: the GPU tests compare those with this, bit for bit."""
import numpy as np

from tests import fusion_util as fu


def components(vertex_count, triangles):
    """-> (labels u32 [V], sizes u32 [V], component count).  label[v]: the smallest id of v's component; size[v]: its vertex count."""
    V = int(vertex_count)
    parent = list(range(V))

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v

    for a, b, c in np.asarray(triangles, np.int64).reshape(-1, 3).tolist():
        for u, w in ((a, b), (a, c)):
            ru, rw = find(u), find(w)
            if ru != rw:
                parent[max(ru, rw)] = min(ru, rw)           # the smaller id stays the root: the root is the minimum
    labels = np.array([find(v) for v in range(V)], np.uint32).reshape(V)
    per_label = np.bincount(labels, minlength=V) if V else np.zeros(0, np.int64)
    sizes = per_label[labels].astype(np.uint32)
    return labels, sizes, int((labels == np.arange(V)).sum())


def filter_mesh(sizes, min_vertices, triangles, *attributes):
    """Keeps the vertices with size >= min_vertices and the triangles whose first vertex is kept, in order, indices remapped to the
    rank among the kept vertices -> (triangles' u32 [T', 3], [attribute[kept] or None for each attribute])."""
    sizes = np.asarray(sizes)
    triangles = np.asarray(triangles, np.uint32).reshape(-1, 3)
    keep = sizes >= min_vertices
    rank = np.cumsum(keep) - keep                           # exclusive
    keep_t = keep[triangles[:, 0]] if len(triangles) else np.zeros(0, bool)
    return rank[triangles[keep_t]].astype(np.uint32).reshape(-1, 3), [None if a is None else np.asarray(a)[keep] for a in attributes]


# ----------------------------------------------------------------------------- inputs

SPECK_BALLS = (((14.3, 15.1, 14.2), 8.2), ((28.6, 4.4, 4.3), 2.1), ((28.2, 26.3, 24.1), 1.6), ((3.4, 27.2, 3.3), 1.2), ((3.5, 3.5, 25.5), 0.8))


def specks_field(dims=(33, 31, 29), balls=SPECK_BALLS, clamp=3.0):
    """fusion_util.sphere_field's grid with the distance to the nearest of five balls: one surface and four specks."""
    d = np.min([fu.sphere_field(dims, centre, radius, np.inf) for centre, radius in balls], axis=0)
    return np.clip(d, -clamp, clamp).astype(np.float32)


def specks_mesh():
    """-> (positions, normals, None, triangles) of fusion_util.extract_mesh on the specks field, all counts 1."""
    field = specks_field()
    return fu.extract_mesh(field, np.ones(field.shape, np.uint32), None, (0.0, 0.0, 0.0), 1.0, 1)


def strip(rungs):
    """A ladder of `rungs` rungs: 2 n vertices, 2 (n - 1) triangles (2a, 2a+1, 2a+2), (2a+1, 2a+3, 2a+2)."""
    a = np.arange(rungs - 1, dtype=np.int64)
    return np.stack([np.stack([2 * a, 2 * a + 1, 2 * a + 2], 1), np.stack([2 * a + 1, 2 * a + 3, 2 * a + 2], 1)], 1).reshape(-1, 3).astype(np.uint32)


STRIP_RUNGS = 4001


def permuted_strip(rungs=STRIP_RUNGS, seed=3):
    return np.random.default_rng(seed).permutation(2 * rungs).astype(np.uint32)[strip(rungs)]


def interleaved_strips(rungs=STRIP_RUNGS):
    """Two strips on the even and on the odd ids of one range of 4 n vertices."""
    s = strip(rungs)
    return np.concatenate([2 * s, 2 * s + 1]).astype(np.uint32)


def star(spokes=4096):
    """Hub V - 1 with triangles (hub, 2 i, 2 i + 1): V = 2 * spokes + 1."""
    i = np.arange(spokes, dtype=np.int64)
    hub = 2 * spokes
    return hub + 1, np.stack([np.full(spokes, hub), 2 * i, 2 * i + 1], 1).astype(np.uint32)


def random_sparse(vertex_count=5003, triangles=1500, seed=11):
    """Random index triples: many singletons and small pieces, with some duplicated and some degenerate triangles."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, vertex_count, (triangles, 3))
    t[::50, 1] = t[::50, 0]                                  # (a, a, b)
    t[7::100] = t[7::100, :1]                                # (a, a, a)
    t[3::60] = t[2::60][:len(t[3::60])]                      # duplicates
    return vertex_count, t.astype(np.uint32)
