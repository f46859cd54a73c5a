"""The restatement of the edge-collapse rule (tests/decimate_mesh_util.py) on meshes whose answer is known by their shape -- a closed
sphere stays a closed 2-manifold, a flat plane keeps its area and its box, a roof keeps its crease, a bump keeps its vertices -- and
the plumbing of tools/run_tum.py --mesh-decimate-ratio / --mesh-decimate-vertices with everything that needs a GPU stubbed.
Properties, not recorded bits; the GPU tests compare bslam_decimate_mesh with the restatement bit for bit."""
import inspect

import numpy as np
import pytest

from tests import decimate_mesh_util as du
from tests import point_mesh_util as pm
from tests import simplify_mesh_util as su

F = np.float32


def box(positions):
    return positions.min(axis=0).tolist(), positions.max(axis=0).tolist()


# ------------------------------------------------------------------------------------------------
# 1. the rule
# ------------------------------------------------------------------------------------------------
def test_the_sphere_stays_a_closed_manifold():
    positions, normals, triangles = du.uv_sphere(48, 24)
    assert len(positions) == 1106
    trace = []
    r = du.decimate(positions, normals, None, triangles, 300, trace=trace)
    assert len(r["positions"]) == 300 and len(r["triangles"]) == 596
    uses, directed = du.edge_counts(r["triangles"])
    assert (uses == 2).all() and (directed == 1).all()
    assert 300 - len(uses) + 596 == 2, "V - E + F"
    centre = np.array([1.3, 1.1, 1.2])
    p = r["positions"].astype(np.float64)
    t = r["triangles"].astype(np.int64)
    outward = np.einsum("ij,ij->i", du.face_normals(r["positions"], r["triangles"]), p[t].mean(axis=1) - centre)
    assert (outward > 0).all(), "a face was turned inward"
    radii = np.linalg.norm(p - centre, axis=1)
    print(f"radii {radii.min():.4f} .. {radii.max():.4f}, {r['rounds']} rounds, collapses per round {trace}")
    assert 0.99 < radii.min() and radii.max() < 1.0 + 1e-6
    assert sum(trace) == 1106 - 300 and r["rounds"] == len(trace)
    # vertex_map: onto the survivors, the identity on them in their order
    assert set(r["vertex_map"].tolist()) == set(range(300))
    assert np.abs(np.linalg.norm(r["normals"].astype(np.float64), axis=1) - 1).max() < 1e-6


def test_the_flat_plane_keeps_its_area_and_its_box():
    positions, triangles = du.plane(17)
    r = du.decimate(positions, None, None, triangles, 40)
    assert len(r["positions"]) == 40
    assert du.mesh_area(r["positions"], r["triangles"]) == 256.0 and box(r["positions"]) == box(positions)
    assert (r["positions"][:, 2] == F(0.5)).all()
    assert (du.face_normals(r["positions"], r["triangles"])[:, 2] > 0).all()


def test_boundary_weight():
    """Without the boundary quadrics nothing holds the rim of a flat plane: every collapse costs 0."""
    positions, triangles = du.plane(17)
    free = du.decimate(positions, None, None, triangles, 40, boundary_weight=0.0)
    held = du.decimate(positions, None, None, triangles, 40, boundary_weight=1.0)
    assert len(free["positions"]) == 40 and du.mesh_area(free["positions"], free["triangles"]) < 256.0
    assert box(held["positions"]) == box(positions)


def test_the_roof_keeps_its_crease():
    positions, triangles = du.roof()
    assert len(positions) == 441
    r = du.decimate(positions, None, None, triangles, 60)
    assert len(r["positions"]) == 60
    off = np.abs(r["positions"][:, 2].astype(np.float64) - du.roof_height(r["positions"][:, 0]))
    assert off.max() <= 1e-6
    assert (r["positions"][:, 0] == F(10.25)).any() and box(r["positions"]) == box(positions)
    clustered = su.simplify(positions, None, None, triangles, positions.min(axis=0), 3.0)
    worst = np.abs(clustered["positions"][:, 2].astype(np.float64) - du.roof_height(clustered["positions"][:, 0])).max()
    print(f"clustering to {len(clustered['positions'])} vertices: worst vertex {worst:.4f} from the roof; decimation to 60: {off.max():.1e}")
    assert len(clustered["positions"]) == 49 and worst > 0.3


def test_max_cost_zero_on_the_roof():
    """Only the collapses inside the two flat halves and along the crease and the rim cost nothing; they suffice for 60 vertices but
    not for 4."""
    positions, triangles = du.roof()
    r = du.decimate(positions, None, None, triangles, 60, max_cost=0.0)
    assert len(r["positions"]) == 60 and np.abs(r["positions"][:, 2].astype(np.float64) - du.roof_height(r["positions"][:, 0])).max() == 0.0
    r = du.decimate(positions, None, None, triangles, 4, max_cost=0.0)
    assert len(r["positions"]) >= 6, "the four corners and the two ends of the crease cannot go at cost 0"
    assert np.abs(r["positions"][:, 2].astype(np.float64) - du.roof_height(r["positions"][:, 0])).max() == 0.0 and box(r["positions"]) == box(positions)


def test_the_bump_keeps_its_vertices():
    """Twice the figures of the float64 prototype of the rule (mean 0.0037, max 0.050 in units of the mesh) bound the distance from the
    input vertices to the decimated surface; clustering at a like vertex count is an order of magnitude farther."""
    positions, triangles = du.bumpy_plane()
    assert len(positions) == 625
    r = du.decimate(positions, None, None, triangles, 80)
    assert len(r["positions"]) == 80
    d = pm.distances64(positions, r["positions"], r["triangles"]).min(axis=1)
    clustered = su.simplify(positions, None, None, triangles, positions.min(axis=0), 3.0)
    dc = pm.distances64(positions, clustered["positions"], clustered["triangles"]).min(axis=1)
    near = int((np.hypot(r["positions"][:, 0] - 12.25, r["positions"][:, 1] - 12.25) < 6).sum())
    print(f"decimation to 80: mean {d.mean():.4f}, max {d.max():.4f}, {near} vertices within r < 6; clustering to {len(clustered['positions'])}: "
          f"mean {dc.mean():.4f}, max {dc.max():.4f}")
    assert d.mean() <= 2 * 0.0037 and d.max() <= 2 * 0.050
    assert 75 <= len(clustered["positions"]) <= 90 and d.mean() < dc.mean() and d.max() < dc.max()
    assert near > 40, "the vertices went to the flat part"


def test_a_tetrahedron_never_collapses():
    positions, triangles = du.tetrahedron()
    r = du.decimate(positions, None, None, triangles, 0)
    assert len(r["positions"]) == 4 and np.array_equal(r["triangles"], triangles) and r["rounds"] == 1
    assert np.array_equal(r["vertex_map"], np.arange(4))


def test_an_edge_with_three_triangles_is_not_collapsed_and_isolated_vertices_stay():
    positions, triangles = du.three_wings()
    normals, colors = du.attributes(len(positions))
    trace = []
    r = du.decimate(positions, normals, colors, triangles, 0, max_rounds=1, trace=trace)
    assert trace[0] >= 1 and r["vertex_map"][0] != r["vertex_map"][1]
    r = du.decimate(positions, normals, colors, triangles, 0)
    for v in (8, 9):
        k = r["vertex_map"][v]
        assert np.array_equal(r["positions"][k], positions[v]) and np.array_equal(r["colors"][k], colors[v]) and np.array_equal(r["normals"][k], normals[v])
    assert r["vertex_map"][8] != r["vertex_map"][9]


def test_max_rounds_and_the_identity():
    positions, triangles = du.noisy_plane(9, seed=1)
    normals, colors = du.attributes(81, 1)
    trace = []
    one = du.decimate(positions, normals, colors, triangles, 10, max_rounds=1, trace=trace)
    assert one["rounds"] == 1 and len(trace) == 1 and len(one["positions"]) == 81 - trace[0] and 0 < trace[0] < 71
    for target in (81, 82, 1 << 31):
        same = du.decimate(positions, normals, colors, triangles, target)
        assert same["rounds"] == 0 and np.array_equal(same["vertex_map"], np.arange(81)) and np.array_equal(same["triangles"], triangles)
        assert np.array_equal(same["positions"].view(np.uint32), positions.view(np.uint32)) and np.array_equal(same["colors"], colors)
        assert np.array_equal(same["normals"].view(np.uint32), normals.view(np.uint32))
    # ... less the triangles that repeat an index
    with_degenerate = np.concatenate([triangles, [[3, 3, 4], [5, 6, 5]]]).astype(np.uint32)
    assert np.array_equal(du.decimate(positions, None, None, with_degenerate, 81)["triangles"], triangles)


def test_the_target_is_met_exactly():
    positions, triangles = du.noisy_plane(9, seed=2)
    for target in (80, 64, 41, 17):
        r = du.decimate(positions, None, None, triangles, target)
        assert len(r["positions"]) == target and r["triangles"].max() < target


def test_refusals():
    positions, triangles = du.plane(3)
    with pytest.raises(du.Refused, match="beyond vertex_count"):
        du.decimate(positions, None, None, [[0, 1, 9]], 4)
    bad = positions.copy()
    bad[4, 1] = np.nan
    with pytest.raises(du.Refused, match="not finite"):
        du.decimate(bad, None, None, triangles, 4)


def test_the_abi_declares_the_call():
    from badslam_amd import abi
    assert len(abi.SIGNATURES["bslam_decimate_mesh"][1]) == 20


# ------------------------------------------------------------------------------------------------
# 2. tools/run_tum.py --mesh-decimate-ratio / --mesh-decimate-vertices, with everything that needs a GPU stubbed
# ------------------------------------------------------------------------------------------------
def test_run_tum_plumbing(monkeypatch, tmp_path):
    from tools import run_tum
    parameters = inspect.signature(run_tum.run).parameters
    assert parameters["mesh_decimate_ratio"].default is None and parameters["mesh_decimate_vertices"].default is None
    a = run_tum.arg_parser().parse_args(["somewhere"])
    assert a.mesh_decimate_ratio is None and a.mesh_decimate_vertices is None
    a = run_tum.arg_parser().parse_args(["somewhere", "--mesh-decimate-ratio", "0.25", "--mesh-decimate-vertices", "500"])
    assert a.mesh_decimate_ratio == 0.25 and a.mesh_decimate_vertices == 500

    positions, normals, tri = du.uv_sphere(12, 6)
    extracted = dict(positions=positions, normals=normals, colors=np.zeros((len(positions), 4), np.uint8), triangles=tri)
    calls = []

    class StubBA:
        def keyframe_count(self):
            return 0

        def surfels_size(self):
            return 0

        def SimplifyMesh(self, mesh, cell_size, origin=None):
            calls.append(("simplify", mesh, cell_size))
            return su.simplify(mesh["positions"], mesh["normals"], mesh["colors"], mesh["triangles"], mesh["positions"].min(axis=0), cell_size)

        def DecimateMesh(self, mesh, target_vertices=None, ratio=None, boundary_weight=1.0, max_cost=None, max_rounds=0):
            calls.append(("decimate", mesh, target_vertices, ratio))
            target = target_vertices if ratio is None else int(np.ceil(ratio * len(mesh["positions"])))
            return du.decimate(mesh["positions"], mesh["normals"], mesh["colors"], mesh["triangles"], target)

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

    # off by default: the extraction writes the file itself and nothing is decimated
    r = run_tum.run(tmp_path, out=str(tmp_path / "poses.txt"), mesh="m.ply")
    assert calls == [("extract", "m.ply")] and "decimation" not in r["mesh"] and r["mesh"]["vertices"] == len(positions)

    del calls[:]
    report = tmp_path / "surface.json"
    r = run_tum.run(tmp_path, out=str(tmp_path / "poses.txt"), mesh="m.ply", mesh_decimate_vertices=30, ground_truth_surface="truth.ply", surface_report=str(report))
    assert [c[0] for c in calls] == ["extract", "decimate", "save", "evaluate"]
    assert calls[0][1] is None, "the undecimated mesh must not be written"
    assert calls[1][1] is extracted and calls[1][2] == 30 and calls[1][3] is None
    decimated = calls[2][2]
    assert calls[2][1] == "m.ply" and calls[3][1] is decimated, "the decimated mesh is what is written and what is scored"
    want = {"target_vertices": 30, "ratio": None, "vertices_before": len(positions), "triangles_before": len(tri), "vertices": 30,
            "triangles": len(decimated["triangles"]), "rounds": decimated["rounds"]}
    assert r["mesh"]["decimation"] == want and r["mesh"]["vertices"] == 30 and r["mesh"]["triangles"] == want["triangles"]
    import json
    assert json.loads(report.read_text())["mesh_decimation"] == want

    # after the clustering, by ratio, with no file
    del calls[:]
    r = run_tum.run(tmp_path, out=str(tmp_path / "poses.txt"), mesh_simplify_cell=0.5, mesh_decimate_ratio=0.5, ground_truth_surface="truth.ply")
    assert [c[0] for c in calls] == ["extract", "simplify", "decimate", "evaluate"]
    simplified_vertices = r["surface"]["mesh_simplification"]["vertices"]
    assert calls[2][1]["positions"].shape[0] == simplified_vertices and calls[2][2] is None and calls[2][3] == 0.5
    assert r["surface"]["mesh_decimation"]["vertices_before"] == simplified_vertices and "mesh" not in r
    assert r["surface"]["mesh_decimation"]["vertices"] <= int(np.ceil(0.5 * simplified_vertices)) < simplified_vertices
    assert calls[3][1]["positions"].shape[0] == r["surface"]["mesh_decimation"]["vertices"]

    with pytest.raises(ValueError, match="at most one"):
        run_tum.run(tmp_path, mesh="m.ply", mesh_decimate_ratio=0.5, mesh_decimate_vertices=30)
