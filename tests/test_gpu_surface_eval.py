"""-m gpu: surface evaluation through DirectBA (PointMeshDistance, SurfelMeshDistance, badslam_amd/surface_eval.py) and
tools/run_tum.py --ground-truth-surface, on the three 160 x 120 keyframes of tests/scenes.py fused at 2 cm into the fixed volume
of tests/test_gpu_mesh_components.py.  Distances and triangles are compared bit for bit with the restatement of
tests/point_mesh_util.py on the arrays the object returned.

Measured beforehand on the CPU with the restatements alone (fusion_util.fuse and extract_mesh on the scene's images with the
oracle's pose matrices, point_mesh_util.point_mesh_distance against the tessellated planes of plane_ground_truth -- 57 557
vertices, 108 560 triangles -- search radius 0.1 m): accuracy median 0.763 mm over 24 070 vertices (mean 1.1 mm, 99th percentile
5.4 mm, all within 1 cm but three); completeness median 0.645 mm (96.4 % within 1 cm, 99.9 % within 5 cm: the keyframes see more
of the planes than the volume's box holds).  F-score 0.981 / 0.986 / 0.999 at 1 / 2 / 5 cm."""
import json

import numpy as np
import pytest

from tests import point_mesh_util as pm
from tests.test_gpu_fusion import bits
from tests.test_gpu_mesh_components import VOLUME_DIMS, VOLUME_ORIGIN

pytestmark = pytest.mark.gpu
F = np.float32
CPU_ACCURACY_MEDIAN = 7.63e-4        # metres; from the CPU run of the docstring
CPU_COMPLETENESS_MEDIAN = 6.45e-4


def make_scene():
    from tests import bso, scenes
    cam = bso.make_camera(131.25, 131.25, 80.0, 60.0, 160, 120)
    return cam, scenes.synthetic_scene(3, width=160, height=120, cell=2, camera=cam)


def plane_ground_truth(cam, scene):
    """The scene's analytic surface, tessellated at 2 cm: for every keyframe the exact intersections of its pixel rays with the 20
    planes (a pixel is 1.9 cm wide at the planes' 2.5 m), two triangles per pixel square whose four corners are valid and lie on
    one plane -- so every triangle lies in its plane, and the creases between planes stay open by at most a pixel.
    -> mesh dict of positions f32 and triangles u32."""
    from tests import bso, scenes
    planes = scenes.random_planes(np.random.default_rng(0xBAD51A4), 20)
    positions, triangles, base = [], [], 0
    for kf in scene.keyframes:
        M = np.array(list(bso.se3_matrix3x4(kf.global_T_frame).m), np.float64).reshape(3, 4)
        t, plane, dg, o = scenes.render_planes(cam, 160, 120, M[:, :3], M[:, 3], planes)
        valid = np.isfinite(t) & (t < 6.0)
        points = o[None, None, :] + dg * np.where(valid, t, 0.0)[..., None]
        ids = np.arange(160 * 120).reshape(120, 160) + base
        a, b, c, d = ids[:-1, :-1], ids[:-1, 1:], ids[1:, 1:], ids[1:, :-1]
        same = (valid[:-1, :-1] & valid[:-1, 1:] & valid[1:, 1:] & valid[1:, :-1] & (plane[:-1, :-1] == plane[:-1, 1:]) & (plane[:-1, :-1] == plane[1:, 1:]) &
                (plane[:-1, :-1] == plane[1:, :-1]))
        triangles += [np.stack([a[same], b[same], c[same]], 1), np.stack([a[same], c[same], d[same]], 1)]
        positions.append(points.reshape(-1, 3))
        base += 160 * 120
    positions, triangles = np.concatenate(positions).astype(F), np.concatenate(triangles)
    used = np.zeros(len(positions), bool)
    used[triangles.reshape(-1)] = True                                   # completeness is sampled at the vertices: only those of the surface
    rank = np.cumsum(used) - 1
    return dict(positions=np.ascontiguousarray(positions[used]), triangles=np.ascontiguousarray(rank[triangles].astype(np.uint32)))


@pytest.fixture(scope="module")
def fused():
    """(ba, mesh, scene, camera): the keyframes added, surfels created, the volume fused and the mesh extracted once."""
    from badslam_amd.direct_ba import DirectBA
    cam, scene = make_scene()
    ba = DirectBA(scene.max_surfels, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, 0.8, 1, 1, 1, scene.color_camera, scene.depth_camera, 0, True, False)
    for kf in scene.keyframes:
        ba.AddKeyframe(kf.id, max(kf.min_depth, 1e-3), max(kf.max_depth, 1e-2), kf.depth, kf.normals, kf.radius, kf.color, kf.global_T_frame)
    for kf in scene.keyframes:
        ba.CreateSurfelsForKeyframe(False, kf.id)
    with pytest.raises(Exception, match="ExtractMesh"):
        ba.SurfelMeshDistance(0.1)                                       # nothing extracted yet
    ba.FuseKeyframes(np.array(VOLUME_ORIGIN, F), 0.02, VOLUME_DIMS, 0.08)
    mesh = ba.ExtractMesh(1)
    yield ba, mesh, scene, cam
    ba.close()


def assert_result_equals(result, want):
    assert np.array_equal(bits(result["distance"]), bits(want[0])) and np.array_equal(result["triangle"], want[1])


def test_surfel_centres_against_the_mesh_equal_the_restatement(fused):
    ba, mesh, _, _ = fused
    positions, _, _ = ba.ExportToPointCloud()
    assert len(mesh["positions"]) > 20000 and len(positions) > 5000
    chosen = positions[np.random.default_rng(17).choice(len(positions), 500, replace=False)]
    for R, cell in ((0.05, None), (0.05, 0.02), (0.01, None)):
        got = ba.PointMeshDistance(chosen, mesh, R, cell)
        want = pm.point_mesh_distance(chosen, mesh["positions"], mesh["triangles"], R)
        assert 50 < np.isfinite(want[0]).sum()
        assert_result_equals(got, want)
        assert got["cell_size"] == F(R if cell is None else cell)
        assert (got["grid_cells"], got["grid_entries"]) == pm.grid_census(mesh["positions"], mesh["triangles"], R, got["cell_size"])


def test_the_cell_doubles_while_the_grid_is_over_budget(fused):
    ba, mesh, _, _ = fused
    points = mesh["positions"][::50]
    entries = {c: pm.grid_census(mesh["positions"], mesh["triangles"], 0.01, c)[1] for c in (F(0.01), F(0.02), F(0.04))}
    assert entries[F(0.01)] > entries[F(0.02)] > entries[F(0.04)]
    got = ba.PointMeshDistance(points, mesh, 0.01, None, max_grid_entries=entries[F(0.02)] - 1)
    assert got["cell_size"] == F(0.04) and got["grid_entries"] == entries[F(0.04)]
    assert_result_equals(got, pm.point_mesh_distance(points, mesh["positions"], mesh["triangles"], 0.01))
    with pytest.raises(Exception, match="max_grid_entries"):               # a cell that was asked for is not changed
        ba.PointMeshDistance(points, mesh, 0.01, 0.01, max_grid_entries=entries[F(0.02)] - 1)


def test_the_point_cloud_form(fused):
    ba, mesh, _, _ = fused
    cloud = mesh["positions"][::7]
    points = mesh["positions"][3::41]
    want = pm.point_mesh_distance(points, cloud, np.repeat(np.arange(len(cloud), dtype=np.uint32)[:, None], 3, axis=1), 0.05)
    assert_result_equals(ba.PointMeshDistance(points, {"positions": cloud}, 0.05), want)
    assert_result_equals(ba.PointMeshDistance(points, {"positions": cloud, "triangles": np.zeros((0, 3), np.uint32)}, 0.05), want)


def test_surfel_mesh_distance_is_point_mesh_distance_of_the_exported_cloud(fused):
    ba, mesh, _, _ = fused
    positions, _, _ = ba.ExportToPointCloud()
    a = ba.SurfelMeshDistance(0.05)
    b = ba.PointMeshDistance(positions, mesh, 0.05)
    assert len(a["distance"]) == len(positions)
    assert_result_equals(a, (b["distance"], b["triangle"]))
    assert (a["cell_size"], a["grid_cells"], a["grid_entries"]) == (b["cell_size"], b["grid_cells"], b["grid_entries"])
    hits = np.isfinite(a["distance"])
    print(f"{int(hits.sum())} of {len(hits)} surfel centres within 0.05 m of the mesh, median {np.median(a['distance'][hits]):.5f}")
    assert hits.mean() > 0.95 and np.median(a["distance"][hits]) < 0.01      # half a voxel
    # the mesh of the last extraction is the one measured: a filtered one drops what hung on the removed pieces
    filtered = ba.ExtractMesh(1, min_component_vertices=len(mesh["positions"]) // 2)
    c = ba.SurfelMeshDistance(0.05)
    d = ba.PointMeshDistance(positions, filtered, 0.05)
    assert_result_equals(c, (d["distance"], d["triangle"]))
    ba.ExtractMesh(1)


def test_a_mesh_against_itself(fused):
    from badslam_amd import surface_eval
    ba, _, _, _ = fused
    mesh = ba.ExtractMesh(1, min_component_vertices=3)                   # without the vertices in no triangle, which are near nothing of their own
    in_a_triangle = np.zeros(len(mesh["positions"]), bool)
    in_a_triangle[mesh["triangles"].reshape(-1)] = True
    assert in_a_triangle.all() and len(mesh["positions"]) > 20000
    r = surface_eval.evaluate(ba, mesh, mesh, 0.05, (0.01, 0.02))
    for side in ("accuracy", "completeness"):
        s = r[side]
        assert s["hits"] == s["count"] == len(mesh["positions"]) and s["mean"] == 0.0 and s["median"] == 0.0 and s["p99"] == 0.0 and s["rmse"] == 0.0
        assert s["within"] == [1.0, 1.0] and s["beyond"] == 0.0
    assert [row["f_score"] for row in r["f_scores"]] == [1.0, 1.0]
    ba.ExtractMesh(1)


def test_against_the_analytic_planes(fused):
    from badslam_amd import surface_eval
    ba, mesh, scene, cam = fused
    truth = plane_ground_truth(cam, scene)
    r = surface_eval.evaluate(ba, mesh, truth, 0.1, (0.01, 0.02, 0.05))
    print(surface_eval.format_summary("accuracy", r["accuracy"]))
    print(surface_eval.format_summary("completeness", r["completeness"]))
    print(r["f_scores"])
    assert r["accuracy"]["count"] == len(mesh["positions"]) and r["completeness"]["count"] == len(truth["positions"])
    assert r["accuracy"]["median"] <= 2 * CPU_ACCURACY_MEDIAN
    assert r["completeness"]["median"] <= 2 * CPU_COMPLETENESS_MEDIAN
    assert r["f_scores"][2]["precision"] > 0.9 and r["f_scores"][2]["recall"] > 0.9


def test_run_tum_ground_truth_surface(tmp_path):
    """tools/run_tum.py on five frames of the rendered sequence of tests/test_gpu_bad_slam.py, with --mesh and that
    file as --ground-truth-surface: the report parses and holds what evaluate gives for the run's mesh against the file, a mesh
    against itself."""
    from badslam_amd import direct_ba as dba
    from badslam_amd import png, surface_eval
    from tests.test_gpu_bad_slam import render_sequence
    from tools import run_tum
    cam, raw_to_float, frames, gt = render_sequence(5, seed=5)
    source = tmp_path / "source"
    (source / "rgb").mkdir(parents=True)
    (source / "depth").mkdir()
    assoc = []
    for k, (depth, rgb) in enumerate(frames):
        ts = f"{200.0 + 0.1 * k:.6f}"
        png.write_png(source / "rgb" / f"{ts}.png", rgb)
        png.write_png(source / "depth" / f"{ts}.png", depth)
        assoc.append(f"{ts} rgb/{ts}.png {ts} depth/{ts}.png")
    (source / "associated.txt").write_text("\n".join(assoc) + "\n")
    (source / "calibration.txt").write_text(f"{cam.fx} {cam.fy} {cam.cx - 0.5} {cam.cy - 0.5}\n")
    truth_path, report_path = tmp_path / "truth.ply", tmp_path / "surface.json"
    seen = {}

    def inspect(slam, result):
        truth = dba.LoadPLY(truth_path)
        mesh = slam.ba().ExtractMesh(2, min_component_vertices=50)
        seen["evaluate"] = surface_eval.evaluate(slam.ba(), mesh, truth, 0.1, (0.01, 0.02, 0.05))
        seen["surfels"] = surface_eval.distance_summary(slam.ba().SurfelMeshDistance(0.1)["distance"], (0.01, 0.02, 0.05))

    # --mesh writes the file before the evaluation reads it
    r = run_tum.run(source, keyframe_interval=4, ba_iterations=2, max_depth=6.0, num_scales=4, max_surfel_count=400000, mesh=truth_path, mesh_voxel_size=0.04,
                    mesh_min_count=2, mesh_min_component=50, ground_truth_surface=truth_path, surfel_mesh_distance=True, surface_report=report_path, inspect=inspect)
    assert r["mesh"]["vertices"] > 1000
    report = json.loads(report_path.read_text())
    assert report == json.loads(json.dumps(r["surface"]))
    for key in ("accuracy", "completeness", "f_scores", "max_distance"):
        assert report[key] == json.loads(json.dumps(seen["evaluate"][key])), key
    assert report["surfel_mesh_distance"] == json.loads(json.dumps(seen["surfels"]))
    assert report["accuracy"]["count"] == r["mesh"]["vertices"] and report["accuracy"]["median"] == 0.0 and report["f_scores"][0]["f_score"] == 1.0
    assert report["surfel_mesh_distance"]["hits"] > 1000
    a = run_tum.arg_parser().parse_args(["x"])
    assert (a.ground_truth_surface, a.surface_max_distance, a.surface_thresholds, a.surfel_mesh_distance, a.surface_report) == (None, 0.1, (0.01, 0.02, 0.05), False, None)
    assert run_tum.arg_parser().parse_args(["x", "--surface-thresholds", "0.005,0.03"]).surface_thresholds == (0.005, 0.03)
