"""The brute-force restatement of the mesh repair rules (tests/mesh_repair_util.py) on its own: the numbers below were measured with
a prototype of the rule of include/badslam_hip.h "Mesh repair" and pin the restatement that tests/test_gpu_mesh_repair.py holds the
device against.

  cube as a soup                  36 vertices, 12 triangles: 36 boundary edges, 12 loops of 3; cleaned: 8 / 12, 18 edges, closed, volume 1
  sphere_field(), all observed    1774 / 3544, 5316 edges, no boundary slot
  ... holed_sphere_count          1702 / 3364, 5065 edges, one loop of 38
  ... and count[16, 15, 5:8] = 0  1698 / 3346, 5044 edges, 50 boundary slots, loops of 12 and 38, no blocked vertex, euler 0
  FillHoles(16) of the last       1 filled, 1699 / 3358, 38 boundary slots left, euler 1
  FillHoles(64)                   2 filled, 1700 / 3396, 5094 edges, closed, euler 2, volume 3741.36 (the unholed sphere: 3776.69)
  FillHoles(8)                    nothing filled, the input comes back"""
import numpy as np
import pytest

from tests import fusion_util as fu
from tests import mesh_repair_util as ru

F = np.float32


def report(vertex_count, triangles):
    return ru.topology(vertex_count, triangles)


def same_mesh(a, b):
    for k in ("positions", "normals", "colors", "triangles"):
        if (a[k] is None) != (b[k] is None):
            return False
        if a[k] is not None and not (a[k].shape == b[k].shape and np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes()):
            return False
    return True


@pytest.fixture(scope="module")
def spheres():
    return [ru.sphere(holes) for holes in (0, 1, 2)]


def test_cube_as_a_soup():
    positions, triangles = ru.cube()
    assert fu.signed_volume(positions, triangles) == 1.0
    sp, _, _, st = ru.soup(positions, None, None, triangles)
    assert (len(sp), len(st)) == (36, 12)
    before = report(36, st)
    assert before["boundary_edges"] == 36 and before["loops"] == 12 and before["longest_loop"] == 3 and before["loop_edges"] == 36
    assert before["blocked_vertices"] == 0 and before["open_boundary_slots"] == 0
    cleaned = ru.clean(sp, None, None, st)
    assert (len(cleaned["positions"]), len(cleaned["triangles"])) == (8, 12)
    assert cleaned["report"] == dict(welded_vertices=28, unreferenced_vertices=0, degenerate_triangles=0, duplicate_triangles=0)
    after = report(8, cleaned["triangles"])
    assert after["unique_edges"] == 18 and after["boundary_edges"] == 0 and after["nonmanifold_edges"] == 0 and after["euler"] == 2
    assert fu.signed_volume(cleaned["positions"], cleaned["triangles"]) == 1.0
    # the representative is the first corner that names the place: the soup's order decides the vertex order
    assert np.array_equal(cleaned["vertex_map"][:3], [0, 1, 2]) and np.array_equal(cleaned["triangle_map"], np.arange(12))


def test_spheres(spheres):
    want = [((1774, 3544), 5316, 0, []), ((1702, 3364), 5065, 38, [38]), ((1698, 3346), 5044, 50, [38, 12])]
    for (positions, _, triangles), (counts, edges, boundary, loops) in zip(spheres, want):
        r = report(len(positions), triangles)
        assert (len(positions), len(triangles)) == counts and r["unique_edges"] == edges and r["boundary_edges"] == boundary
        assert [len(walk) for walk in r["loop_slots"]] == loops and r["loop_edges"] == boundary
        assert r["blocked_vertices"] == 0 and r["open_boundary_slots"] == 0 and r["nonmanifold_edges"] == 0 and r["inconsistent_edges"] == 0
        assert r["euler"] == 2 - len(loops)
        assert ((r["loop_of_slot"] != ru.NONE) == (r["edge_uses"] == 1)).all()


def test_fill_holes(spheres):
    closed_volume = fu.signed_volume(spheres[0][0], spheres[0][2])
    positions, normals, triangles = spheres[2]
    small = ru.fill_holes(positions, normals, None, triangles, 16)
    r = report(len(small["positions"]), small["triangles"])
    assert (small["filled_holes"], len(small["positions"]), len(small["triangles"])) == (1, 1699, 3358)
    assert r["boundary_edges"] == 38 and r["euler"] == 1 and r["loops"] == 1
    both = ru.fill_holes(positions, normals, None, triangles, 64)
    r = report(len(both["positions"]), both["triangles"])
    assert (both["filled_holes"], len(both["positions"]), len(both["triangles"])) == (2, 1700, 3396)
    assert r["unique_edges"] == 5094 and r["boundary_edges"] == 0 and r["nonmanifold_edges"] == 0 and r["euler"] == 2 and r["inconsistent_edges"] == 0
    undirected, directed = fu.edge_census(both["triangles"])
    assert (undirected == 2).all() and (directed == 1).all()
    volume = fu.signed_volume(both["positions"], both["triangles"])
    assert abs(volume - 3741.36) < 0.01 and abs(closed_volume - 3776.69) < 0.01
    assert 0.98 * closed_volume < volume < closed_volume
    assert np.array_equal(both["hole_of_triangle"], [0] * 38 + [1] * 12)                   # the loop of 38 has the smaller slot
    assert np.array_equal(both["positions"][:1698].view(np.uint32), positions.view(np.uint32)) and np.array_equal(both["triangles"][:3346], triangles)
    unit = np.linalg.norm(both["normals"][1698:].astype(np.float64), axis=1)
    assert np.abs(unit - 1.0).max() < 1e-6
    none = ru.fill_holes(positions, normals, None, triangles, 8)
    assert none["filled_holes"] == 0 and same_mesh(none, dict(positions=positions, normals=normals, colors=None, triangles=triangles))


def test_constructed_topology():
    cases = ru.constructed_cases()
    bow = report(5, cases["bow-tie"][3])
    assert bow["blocked_vertices"] == 1 and bow["loops"] == 0 and bow["open_boundary_slots"] == 6 and (bow["loop_of_slot"] == ru.NONE).all()
    flipped = report(4, cases["flipped neighbour"][3])
    assert flipped["inconsistent_edges"] == 1 and flipped["interior_edges"] == 1
    fan = report(5, cases["three on an edge"][3])
    assert fan["nonmanifold_edges"] == 1 and fan["interior_edges"] == 0 and sorted(fan["edge_uses"].reshape(-1))[-3:] == [3, 3, 3]
    with pytest.raises(ValueError, match="repeats an index"):
        ru.topology(5, cases["named by a dropped triangle only"][3])


def test_constructed_cleaning():
    cases = ru.constructed_cases()
    p, n, c, t = cases["rotated and flipped duplicates"]
    r = ru.clean(p, n, c, t)
    assert r["report"]["duplicate_triangles"] == 2 and np.array_equal(r["triangle_map"], [0, ru.NONE, ru.NONE, 1]) and np.array_equal(r["triangles"][0], t[0])
    assert len(ru.clean(p, n, c, t, remove_duplicates=False)["triangles"]) == 4
    p, n, c, t = cases["degenerate after welding"]
    r = ru.clean(p, n, c, t)
    assert r["report"] == dict(welded_vertices=1, unreferenced_vertices=0, degenerate_triangles=1, duplicate_triangles=0)
    assert np.array_equal(r["vertex_map"], [0, 1, 2, 1, 3]) and np.array_equal(r["triangles"], [[0, 1, 2], [1, 3, 2]])
    assert np.array_equal(r["normals"], n[[0, 1, 2, 4]]) and np.array_equal(r["colors"], c[[0, 1, 2, 4]])       # the representative's, nothing averaged
    assert ru.clean(p, n, c, t, weld=False)["report"]["degenerate_triangles"] == 0
    p, n, c, t = cases["one coordinate apart"]
    r = ru.clean(p, n, c, t)
    assert np.array_equal(r["vertex_map"], [0, 1, 2, 3, 0, 4, 4, 5, 5]) and r["report"]["welded_vertices"] == 3 and r["report"]["degenerate_triangles"] == 2
    assert np.array_equal(r["positions"][4:].view(np.uint32), p[[5, 7]].view(np.uint32))                           # the bits of the representative, not canonical ones
    p, n, c, t = cases["named by a dropped triangle only"]
    r = ru.clean(p, n, c, t)
    assert np.array_equal(r["vertex_map"], [0, 1, 2, ru.NONE, ru.NONE]) and r["report"]["unreferenced_vertices"] == 2
    assert len(ru.clean(p, n, c, t, remove_unreferenced=False)["positions"]) == 5
    p, n, c, t = cases["point cloud with duplicates"]
    r = ru.clean(p, n, c, t)
    assert np.array_equal(r["vertex_map"], [0, 1, 0, 2, 1, 0]) and len(r["triangles"]) == 0 and r["report"]["unreferenced_vertices"] == 0
    with pytest.raises(ValueError, match="not finite"):
        ru.clean(np.array([[0, 0, np.nan]], F), None, None, None)
    with pytest.raises(ValueError, match="beyond vertex_count"):
        ru.clean(np.zeros((3, 3), F), None, None, [[0, 1, 3]])


def test_all_flags_off_drops_degenerate_triangles_alone():
    p, n, c, t = ru.constructed_cases()["named by a dropped triangle only"]
    r = ru.clean(p, n, c, t, weld=False, remove_duplicates=False, remove_unreferenced=False)
    assert np.array_equal(r["triangles"], [[0, 1, 2], [0, 1, 2]]) and same_mesh(dict(r, triangles=t), dict(positions=p, normals=n, colors=c, triangles=t))


def test_idempotence(spheres):
    for name, (p, n, c, t) in ru.constructed_cases().items():
        once = ru.clean(p, n, c, t)
        twice = ru.clean(once["positions"], once["normals"], once["colors"], once["triangles"])
        assert same_mesh(once, twice) and not any(twice["report"].values()), name
        assert np.array_equal(twice["vertex_map"], np.arange(len(once["positions"]))) and np.array_equal(twice["triangle_map"], np.arange(len(once["triangles"])))
    positions, normals, triangles = spheres[0]
    assert same_mesh(ru.clean(positions, normals, None, triangles), dict(positions=positions, normals=normals, colors=None, triangles=triangles))


def test_sheet_with_a_hole_is_filled_after_cleaning():
    p, n, c, t = ru.constructed_cases()["sheet with a hole"]
    cleaned = ru.clean(p, n, c, t)
    assert cleaned["report"] == dict(welded_vertices=0, unreferenced_vertices=1, degenerate_triangles=0, duplicate_triangles=1)
    r = report(25, cleaned["triangles"])
    assert sorted(len(walk) for walk in r["loop_slots"]) == [4, 16]
    filled = ru.fill_holes(cleaned["positions"], cleaned["normals"], cleaned["colors"], cleaned["triangles"], 4)
    assert filled["filled_holes"] == 1 and np.array_equal(filled["positions"][25], [2.5, 2.5, F(0.25 * (4 + 6 + 9 + 6) / 4)])
    members = sorted(set(int(v) for v in filled["triangles"][30:, :2].reshape(-1)))
    assert members == [12, 13, 17, 18]
    want = (c[members].astype(np.int64).sum(axis=0) + 2) // 4
    assert np.array_equal(filled["colors"][25], want)
    after = report(26, filled["triangles"])
    assert after["loops"] == 1 and after["longest_loop"] == 16 and after["inconsistent_edges"] == 0


# ------------------------------------------------------------------------------------------------
# tools/run_tum.py --mesh-fill-holes / --mesh-clean, with everything that needs a GPU stubbed by the restatement
# ------------------------------------------------------------------------------------------------
def test_run_tum_plumbing(monkeypatch, tmp_path, spheres):
    import inspect
    import json

    from tests import simplify_mesh_util as su
    from tools import run_tum
    assert {"mesh_fill_holes", "mesh_clean"} <= set(inspect.signature(run_tum.run).parameters)
    off = run_tum.arg_parser().parse_args(["somewhere"])
    assert off.mesh_fill_holes is None and off.mesh_clean is False
    on = run_tum.arg_parser().parse_args(["somewhere", "--mesh-fill-holes", "32", "--mesh-clean"])
    assert on.mesh_fill_holes == 32 and on.mesh_clean is True

    positions, normals, triangles = spheres[2]
    extracted = dict(positions=positions, normals=normals, colors=np.zeros((len(positions), 4), np.uint8), triangles=triangles)
    calls = []
    four = lambda m: (m["positions"], m["normals"], m["colors"], m["triangles"])

    class StubBA:
        def keyframe_count(self):
            return 0

        def surfels_size(self):
            return 0

        def FillHoles(self, mesh, max_hole_edges):
            calls.append(("fill", mesh, max_hole_edges))
            return ru.fill_holes(*four(mesh), max_hole_edges)

        def SmoothMesh(self, mesh, **kwargs):
            calls.append(("smooth", mesh))
            return dict(mesh)

        def SimplifyMesh(self, mesh, cell_size, origin=None):
            calls.append(("simplify", mesh))
            return su.simplify(*four(mesh), mesh["positions"].min(axis=0), cell_size)

        def DecimateMesh(self, mesh, target_vertices=None, ratio=None):
            calls.append(("decimate", mesh))
            return dict(mesh, rounds=0)

        def CleanMesh(self, mesh):
            calls.append(("clean", mesh))
            return ru.clean(*four(mesh))

        def MeshTopology(self, mesh):
            calls.append(("topology", mesh))
            r = ru.topology(len(mesh["positions"]), mesh["triangles"])
            return {k: r[k] for k in ru.REPORT_FIELDS}

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

    monkeypatch.setattr(run_tum.dba, "read_tum_dataset", lambda d, t: dict(frames=[], width=64, height=48, camera=(50.0, 50.0, 32.0, 24.0)))
    monkeypatch.setattr(run_tum.dba, "save_poses", lambda *a: None)
    monkeypatch.setattr(run_tum.dba, "SaveMeshAsPLY", lambda path, mesh: calls.append(("save", mesh, path)))
    monkeypatch.setattr(run_tum.bad_slam, "BadSlam", StubSlam)
    monkeypatch.setattr(run_tum, "fuse_and_mesh", fuse_and_mesh)

    # off by default: the extraction writes the file itself; nothing is repaired, inspected or reported
    report = tmp_path / "surface.json"
    r = run_tum.run(tmp_path, out=str(tmp_path / "poses.txt"), mesh="m.ply", surface_report=str(report))
    assert calls == [("extract", "m.ply")] and set(r["mesh"]) == {"path", "vertices", "triangles", "origin", "dims"} and "surface" not in r and not report.exists()

    del calls[:]
    r = run_tum.run(tmp_path, out=str(tmp_path / "poses.txt"), mesh="m.ply", mesh_fill_holes=16, mesh_clean=True, mesh_smooth_iterations=2, mesh_simplify_cell=2.0,
                    mesh_decimate_ratio=0.5, surface_report=str(report))
    assert [c[0] for c in calls] == ["extract", "fill", "smooth", "simplify", "clean", "decimate", "clean", "save", "topology"]
    assert calls[0][1] is None and calls[1][1] is extracted and calls[1][2] == 16
    for before, after in zip(calls[1:-1], calls[2:]):
        assert after[0] == "topology" or len(after[1]["positions"]) <= len(before[1]["positions"]) + 1, "every stage takes the result of the one before"
    assert calls[-1][1] is calls[-2][1], "the census is that of the mesh as written"
    surface = json.loads(report.read_text())
    assert surface["mesh_hole_filling"] == dict(max_hole_edges=16, filled_holes=1, vertices_before=1698, triangles_before=3346, vertices=1699, triangles=3358)
    assert [c["after"] for c in surface["mesh_cleaning"]] == ["simplification", "decimation"] and surface["mesh_cleaning"][0]["duplicate_triangles"] > 0
    assert surface["mesh_cleaning"][1]["duplicate_triangles"] == 0 and surface["mesh_topology"]["euler"] == r["surface"]["mesh_topology"]["euler"]
    assert r["mesh"]["hole_filling"] == surface["mesh_hole_filling"] and r["mesh"]["cleaning"] == surface["mesh_cleaning"]
    assert r["mesh"]["vertices"] == surface["mesh_cleaning"][1]["vertices"]

    # --mesh-clean alone has nothing to clean behind: the mesh is written as extracted, with its census
    del calls[:]
    r = run_tum.run(tmp_path, out=str(tmp_path / "poses.txt"), mesh="m.ply", mesh_clean=True)
    assert [c[0] for c in calls] == ["extract", "save", "topology"] and calls[1][1] is extracted and "cleaning" not in r["mesh"]
