"""CPU: known answers of the vertex clustering restatement (tests/simplify_mesh_util.py), the checker of bslam_simplify_mesh in
tests/test_gpu_simplify_mesh.py, and the --mesh-simplify-cell plumbing of tools/run_tum.py with DirectBA.SimplifyMesh stubbed.

The plane's figures are integers of the rule.  The sphere's inputs go through sin and cos, so its figures -- 1 409 vertices and
2 814 triangles at cell 0.1 from origin 0, no input vertex farther than 0.85 cells from its representative -- are what this
restatement gives and are asserted as such; what has to hold whatever the rounding (a closed, consistently oriented, outward-facing
surface of genus 0, the sqrt(3) cell bound) is asserted beside them."""
import inspect
import json

import numpy as np
import pytest

from tests import simplify_mesh_util as su

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def sphere():
    return su.uv_sphere()


# ------------------------------------------------------------------------------------------------
# 1. known answers
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell, vertices, triangles, largest", [(2.0, 81, 128, 4), (4.0, 25, 32, 16)])
def test_plane(cell, vertices, triangles, largest):
    positions, tri = su.plane()
    assert positions.shape == (289, 3) and tri.shape == (512, 3)
    normals = np.tile(np.array([0, 0, 1], F), (289, 1))
    colors = np.tile(np.array([10, 20, 30, 255], np.uint8), (289, 1))
    r = su.simplify(positions, normals, colors, tri, np.zeros(3, F), cell)
    assert r["positions"].shape == (vertices, 3) and r["triangles"].shape == (triangles, 3)
    sizes = np.bincount(r["vertex_cluster"])
    assert sizes.min() == 1 and sizes.max() == largest and sizes.sum() == 289
    if cell == 2.0:
        assert sorted(set(sizes.tolist())) == [1, 2, 4]
    assert (su.face_normals(r["positions"], r["triangles"])[:, 2] > 0).all(), "a face was turned over"
    assert np.array_equal(r["normals"], np.tile(np.array([0, 0, 1], F), (vertices, 1))) and (r["colors"] == colors[0]).all()
    assert (r["positions"][:, 2] == F(0.5)).all()
    # clusters are numbered in ascending (z, y, x): on the plane row by row
    side = int(round(np.sqrt(vertices)))
    cx, cy = np.floor(r["positions"][:, 0] / cell), np.floor(r["positions"][:, 1] / cell)
    assert np.array_equal(cy * side + cx, np.arange(vertices))
    # the first cluster at cell 2: the vertices (0.25, 0.25), (1.25, 0.25), (0.25, 1.25), (1.25, 1.25)
    if cell == 2.0:
        assert np.array_equal(r["positions"][0], np.array([0.75, 0.75, 0.5], F))


def test_sphere(sphere):
    positions, normals, tri = sphere
    assert positions.shape == (4514, 3) and tri.shape == (9024, 3)
    centre, cell = np.array([1.3, 1.1, 1.2]), 0.1
    r = su.simplify(positions, normals, None, tri, np.zeros(3, F), cell)
    print(f"sphere at cell {cell}: {len(r['positions'])} vertices, {len(r['triangles'])} triangles")
    assert (len(r["positions"]), len(r["triangles"])) == (1409, 2814)
    undirected, directed = su.edge_counts(r["triangles"])
    assert (undirected == 2).all(), "an edge is not shared by exactly two triangles"
    assert (directed == 1).all(), "two triangles run along an edge in the same direction"
    assert len(r["positions"]) - len(undirected) + len(r["triangles"]) == 2
    face = su.face_normals(r["positions"], r["triangles"])
    centroid = r["positions"][r["triangles"].astype(np.int64)].astype(np.float64).mean(axis=1)
    assert (np.einsum("ij,ij->i", face, centroid - centre) > 0).all(), "a face looks inwards"
    moved = np.linalg.norm(positions.astype(np.float64) - r["positions"][r["vertex_cluster"]].astype(np.float64), axis=1).max() / cell
    print(f"largest distance of a vertex to its representative: {moved:.4f} cells")
    assert moved <= np.sqrt(3.0)
    assert abs(moved - 0.8467) < 1e-3
    # representatives' normals: unit length, outwards
    length = np.linalg.norm(r["normals"].astype(np.float64), axis=1)
    assert np.abs(length - 1).max() < 1e-6 and (np.einsum("ij,ij->i", r["normals"], r["positions"] - centre) > 0).all()


def test_single_member_clusters_keep_their_bits():
    rng = np.random.default_rng(3)
    positions = (rng.uniform(0, 1, (200, 3)) + np.arange(200)[:, None] * 2).astype(F)   # one vertex per cell of size 1
    positions[5, 1] = F(-0.0) + F(10.0)
    positions[0] = [-0.0, 0.0, -0.0]
    normals = rng.standard_normal((200, 3)).astype(F)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    colors = rng.integers(0, 256, (200, 4), dtype=np.uint8)
    r = su.simplify(positions, normals, colors, None, np.zeros(3, F), 1.0)
    assert len(r["positions"]) == 200 and len(r["triangles"]) == 0
    assert np.array_equal(bits(r["positions"][r["vertex_cluster"]]), bits(positions)), "a cluster of one changed its position bits (-0.0 included)"
    assert np.array_equal(r["colors"][r["vertex_cluster"]], colors)
    assert np.abs(r["normals"][r["vertex_cluster"]] - normals).max() <= 1e-6


def test_sums_rounding_and_degenerate_normals():
    positions = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.3, 0.3, 0.3], [1.5, 0.5, 0.5], [1.6, 0.5, 0.5]], F)
    normals = np.array([[0, 0, 1], [0, 1, 0], [0, 0, 1], [1, 0, 0], [-1, 0, 0]], F)
    colors = np.array([[0, 1, 255, 255], [1, 1, 255, 0], [1, 2, 255, 0], [255, 0, 0, 7], [254, 1, 0, 8]], np.uint8)
    r = su.simplify(positions, normals, colors, None, np.zeros(3, F), 1.0)
    assert np.array_equal(r["vertex_cluster"], [0, 0, 0, 1, 1])
    mean = ((np.float64(F(0.1)) + np.float64(F(0.2))) + np.float64(F(0.3))) / 3.0
    assert r["positions"][0, 0] == F(mean)
    assert np.allclose(r["normals"][0], np.array([0, 1, 2]) / np.sqrt(5.0), atol=1e-7)
    assert np.array_equal(r["normals"][1], np.zeros(3, F)), "a zero normal sum has to give (0, 0, 0)"
    # (S + n / 2) / n in integers: (2 + 1) / 3, (4 + 1) / 3, 255, (255 + 1) / 3; (509 + 1) / 2, (1 + 1) / 2, 0, (15 + 1) / 2
    assert np.array_equal(r["colors"], [[1, 1, 255, 85], [255, 1, 0, 8]])
    normals[1, 0] = np.inf
    r = su.simplify(positions, normals, None, None, np.zeros(3, F), 1.0)
    assert np.array_equal(r["normals"], np.zeros((2, 3), F)), "a non-finite member normal has to give (0, 0, 0)"


def test_a_cell_far_larger_than_the_mesh(sphere):
    positions, normals, tri = sphere
    r = su.simplify(positions, normals, None, tri, np.zeros(3, F), 100.0)
    assert r["positions"].shape == (1, 3) and r["triangles"].shape == (0, 3) and (r["vertex_cluster"] == 0).all()
    assert np.abs(r["positions"][0] - np.array([1.3, 1.1, 1.2])).max() < 1e-6


def test_a_point_cloud(sphere):
    positions, normals, tri = sphere
    cloud = su.simplify(positions, normals, None, None, np.zeros(3, F), 0.1)
    mesh = su.simplify(positions, normals, None, tri, np.zeros(3, F), 0.1)
    assert cloud["triangles"].shape == (0, 3)
    for k in ("positions", "normals", "vertex_cluster"):
        assert np.array_equal(cloud[k], mesh[k])


def test_cell_faces_and_negative_zero():
    """Values exactly on a face belong to the upper cell, and -0.0 - 0.0 = -0.0 has the cell floorf(-0.0 * inv) = -0.0, which is cell 0."""
    positions = np.array([[-0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.24999999, 0.0, 0.0], [0.5, 0.0, 0.0]], F)
    c, valid = su.cells(positions, np.zeros(3, F), 0.25)
    assert valid.all() and np.array_equal(c[:, 0], [0, 1, 0, 2])
    # a reciprocal that is not representable: the cell is that of the rounded product, here one above the real quotient's
    inv = F(1.0) / F(0.03)
    x = F(0.03) * F(7)
    c, _ = su.cells(np.array([[x, 0, 0]], F), np.zeros(3, F), 0.03)
    assert c[0, 0] == np.floor(x * inv)


@pytest.mark.parametrize("position, origin, cell", [((np.nan, 0.5, 0.5), 0.0, 1.0), ((0.5, np.inf, 0.5), 0.0, 1.0), ((0.5, 0.5, 0.25), 0.5, 1.0),
                                                     ((2097152.5, 0.5, 0.5), 0.0, 1.0), ((0.5, 0.5, 2097152.0), 0.0, 1.0)])
def test_refusals(position, origin, cell):
    positions = np.array([[0.5, 0.5, 0.5], position, [1.5, 0.5, 0.5]], F)
    with pytest.raises(su.Refused, match="not finite or lies outside the grid"):
        su.simplify(positions, None, None, None, np.full(3, origin, F), cell)


def test_the_last_cell_is_accepted_and_a_bad_index_is_not():
    positions = np.array([[0.5, 0.5, 0.5], [2097151.5, 2097151.5, 2097151.5]], F)
    r = su.simplify(positions, None, None, [[0, 1, 1]], np.zeros(3, F), 1.0)
    assert len(r["positions"]) == 2 and len(r["triangles"]) == 0
    with pytest.raises(su.Refused, match="beyond vertex_count"):
        su.simplify(positions, None, None, [[0, 1, 2]], np.zeros(3, F), 1.0)


# ------------------------------------------------------------------------------------------------
# 2. tools/run_tum.py --mesh-simplify-cell, with everything that needs a GPU stubbed
# ------------------------------------------------------------------------------------------------
def test_run_tum_plumbing(monkeypatch, tmp_path):
    from tools import run_tum
    assert "mesh_simplify_cell" in inspect.signature(run_tum.run).parameters
    assert run_tum.arg_parser().parse_args(["somewhere"]).mesh_simplify_cell is None
    assert run_tum.arg_parser().parse_args(["somewhere", "--mesh-simplify-cell", "0.04"]).mesh_simplify_cell == 0.04

    positions, normals, tri = su.uv_sphere(12, 6)
    extracted = dict(positions=positions, normals=normals, colors=np.zeros((len(positions), 4), np.uint8), triangles=tri)
    calls = []

    class StubBA:
        def keyframe_count(self):
            return 0

        def surfels_size(self):
            return 0

        def SimplifyMesh(self, mesh, cell_size, origin=None):
            calls.append(("simplify", mesh, cell_size, origin))
            r = su.simplify(mesh["positions"], mesh["normals"], mesh["colors"], mesh["triangles"], mesh["positions"].min(axis=0), cell_size)
            return r

    class StubSlam:
        def __init__(self, *args, **kwargs):
            self._ba = StubBA()

        def ba(self):
            return self._ba

        def frame_poses(self):
            return []

    def fuse_and_mesh(ba, path, *args):
        calls.append(("extract", path))
        return extracted, (0.0, 0.0, 0.0), (1, 1, 1), None

    def evaluate(ba, mesh, truth, *args, **kwargs):
        calls.append(("evaluate", mesh))
        return {"accuracy": {"count": len(mesh["positions"])}}

    monkeypatch.setattr(run_tum.dba, "read_tum_dataset", lambda d, t: dict(frames=[], width=64, height=48, camera=(50.0, 50.0, 32.0, 24.0)))
    monkeypatch.setattr(run_tum.dba, "save_poses", lambda *a: None)
    monkeypatch.setattr(run_tum.dba, "SaveMeshAsPLY", lambda path, mesh: calls.append(("save", path, mesh)))
    monkeypatch.setattr(run_tum.dba, "LoadPLY", lambda path: {"positions": positions})
    monkeypatch.setattr(run_tum.bad_slam, "BadSlam", StubSlam)
    monkeypatch.setattr(run_tum, "fuse_and_mesh", fuse_and_mesh)
    monkeypatch.setattr(run_tum.surface_eval, "evaluate", evaluate)

    # off by default: the extraction writes the file itself and nothing is simplified
    r = run_tum.run(tmp_path, out=str(tmp_path / "poses.txt"), mesh="m.ply")
    assert calls == [("extract", "m.ply")] and "simplification" not in r["mesh"] and r["mesh"]["vertices"] == len(positions)

    del calls[:]
    report = tmp_path / "surface.json"
    r = run_tum.run(tmp_path, out=str(tmp_path / "poses.txt"), mesh="m.ply", mesh_simplify_cell=0.5, ground_truth_surface="truth.ply", surface_report=str(report))
    assert [c[0] for c in calls] == ["extract", "simplify", "save", "evaluate"]
    assert calls[0][1] is None, "the unsimplified mesh must not be written"
    assert calls[1][1] is extracted and calls[1][2] == 0.5 and calls[1][3] is None
    simplified = calls[2][2]
    assert calls[2][1] == "m.ply" and calls[3][1] is simplified, "the simplified mesh is what is written and what is scored"
    assert 1 < len(simplified["positions"]) < len(positions)
    want = {"cell": 0.5, "vertices_before": len(positions), "triangles_before": len(tri), "vertices": len(simplified["positions"]),
            "triangles": len(simplified["triangles"])}
    assert r["mesh"]["simplification"] == want and r["mesh"]["vertices"] == want["vertices"] and r["mesh"]["triangles"] == want["triangles"]
    assert r["surface"]["mesh_simplification"] == want and json.loads(report.read_text())["mesh_simplification"] == want
