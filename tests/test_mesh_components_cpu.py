"""The restatement of the mesh component rule (tests/mesh_components_util.py) on inputs whose answers were worked out beforehand:
the specks field's mesh (one surface, four detached specks) and ladders whose ids are in order, permuted and interleaved.  No GPU."""
import numpy as np
import pytest

from tests import fusion_util as fu
from tests import mesh_components_util as mu


@pytest.fixture(scope="module")
def specks():
    positions, normals, _, triangles = mu.specks_mesh()
    labels, sizes, count = mu.components(len(positions), triangles)
    return positions, normals, triangles, labels, sizes, count


def test_specks_components(specks):
    positions, normals, triangles, labels, sizes, count = specks
    assert (len(positions), len(triangles)) == (1420, 2820)
    assert count == 5
    per_triangle = labels[triangles]
    assert (per_triangle[:, 0] == per_triangle[:, 1]).all() and (per_triangle[:, 0] == per_triangle[:, 2]).all()
    table = {int(l): (int((labels == l).sum()), int((per_triangle[:, 0] == l).sum())) for l in np.unique(labels)}
    assert table == {0: (76, 148), 8: (28, 52), 104: (1260, 2516), 1364: (48, 92), 1391: (8, 12)}
    for l, (vertices, _) in table.items():
        assert (sizes[labels == l] == vertices).all()
        assert labels[l] == l and (np.nonzero(labels == l)[0] >= l).all()          # the label is the component's smallest id


BANDS = [(1, 8, 1420, 2820), (9, 28, 1412, 2808), (29, 48, 1384, 2756), (49, 76, 1336, 2664), (77, 1260, 1260, 2516), (1261, 1261, 0, 0)]


@pytest.mark.parametrize("low, high, vertices, triangles", BANDS)
def test_specks_filter_bands(specks, low, high, vertices, triangles):
    positions, normals, tri, labels, sizes, count = specks
    for min_vertices in (low, high):
        kept, (p, n) = mu.filter_mesh(sizes, min_vertices, tri, positions, normals)
        assert (len(p), len(kept)) == (vertices, triangles) and len(n) == vertices
        assert len(kept) == 0 or int(kept.max()) < vertices
        # kept vertices keep their order and their bits; kept triangles name the same positions as before
        keep = sizes >= min_vertices
        assert np.array_equal(p.view(np.uint32), positions[keep].view(np.uint32))
        assert np.array_equal(p[kept].view(np.uint32), positions[tri[keep[tri[:, 0]]]].view(np.uint32))


def test_specks_filtered_surface_is_closed(specks):
    positions, normals, tri, labels, sizes, count = specks
    kept, _ = mu.filter_mesh(sizes, 77, tri)
    undirected, directed = fu.edge_census(kept)
    assert (undirected == 2).all() and (directed == 1).all()
    assert mu.components(1260, kept)[2] == 1


def test_strips():
    n = mu.STRIP_RUNGS
    assert len(mu.strip(n)) == 2 * (n - 1)
    for triangles in (mu.permuted_strip(), mu.strip(n)):
        labels, sizes, count = mu.components(2 * n, triangles)
        assert count == 1 and not labels.any() and (sizes == 8002).all()
    assert not np.array_equal(mu.permuted_strip(), mu.strip(n))
    labels, sizes, count = mu.components(4 * n, mu.interleaved_strips())
    assert count == 2 and np.array_equal(labels, np.arange(4 * n) % 2) and (sizes == 8002).all()


def test_degenerate_duplicated_and_unused():
    V, triangles = mu.random_sparse()
    t = triangles.astype(np.int64)
    assert (t[:, 0] == t[:, 1]).sum() >= 30 and ((t[:, 0] == t[:, 1]) & (t[:, 0] == t[:, 2])).sum() >= 10
    assert len(np.unique(t, axis=0)) < len(t)
    labels, sizes, count = mu.components(V, triangles)
    unused = np.setdiff1d(np.arange(V), t)
    assert len(unused) > 1000 and np.array_equal(labels[unused], unused) and (sizes[unused] == 1).all()
    assert count == len(np.unique(labels)) and sizes.max() > 3
    # against an independent closure: labels by repeated minimum over triangles until nothing changes
    want = np.arange(V)
    while True:
        m = want[t].min(axis=1)
        new = want.copy()
        for k in range(3):
            np.minimum.at(new, t[:, k], m)
        new = new[new]
        if np.array_equal(new, want):
            break
        want = new
    assert np.array_equal(labels, want)
    labels0, sizes0, count0 = mu.components(5, np.zeros((0, 3), np.uint32))
    assert np.array_equal(labels0, np.arange(5)) and (sizes0 == 1).all() and count0 == 5
    assert mu.components(0, np.zeros((0, 3), np.uint32))[2] == 0
