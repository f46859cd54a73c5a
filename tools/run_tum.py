#!/usr/bin/env python3
"""Runs the sequential BadSlam front end over a TUM RGB-D directory (associated.txt + calibration.txt, as the reference's
dataset reader expects, LV/rgbd_video_io_tum_dataset.h:128-240), writes the trajectory in TUM format and, if the directory
has a ground truth, prints the ATE RMSE.

    python tools/run_tum.py <dataset_dir> [--trajectory groundtruth.txt] [--out poses.txt] [--keyframe-interval 10]
                            [--ba-iterations 10] [--max-depth 3.0] [--end-frame N] [--ba-cost]
                            [--pyramid-level-for-depth L] [--pyramid-level-for-color L]
                            [--median-filter-and-densify-iterations N] [--render-dir DIR] [--render-every N] [--render-radius-scale S]
                            [--render-source {surfels,volume,mesh}]
                            [--place-recognition] [--place-min-gap N]
                            [--mesh PATH] [--mesh-voxel-size M] [--mesh-truncation M] [--mesh-min-count N] [--mesh-min-component N]
                            [--mesh-smooth-iterations N] [--mesh-smooth-lambda L] [--mesh-smooth-mu M] [--mesh-smooth-boundary fixed|rim|free]
                            [--mesh-simplify-cell M] [--mesh-decimate-ratio R | --mesh-decimate-vertices N]
                            [--mesh-fill-holes N] [--mesh-clean]
                            [--point-cloud PATH]
                            [--ground-truth-surface FILE.ply] [--surface-max-distance M] [--surface-thresholds M,M,...]
                            [--surfel-mesh-distance] [--surface-report FILE.json] [--register-surface] [--surface-sample-spacing M]
                            [--surface-visible-only] [--surface-visibility-margin M]
                            [--mesh-deviation]

--pyramid-level-for-depth / --pyramid-level-for-color (0 ... 3): the stream is halved L times on the GPU before anything else
sees it and its camera is scaled to match (level 1 runs a 640x480 dataset at 320x240).  --median-filter-and-densify-iterations:
3x3 depth median that also fills holes, for noisy sensors; not together with a depth level.

--ba-cost: after the last frame, one more BA over the whole window (poses + geometry), with the BA objective printed before and
after it (DirectBA.ComputeCost: Tukey depth terms + weighted Huber descriptor terms over all surfel / keyframe pairs).

--place-recognition: every new keyframe is matched against the keyframes at least --place-min-gap (default 10) ids older
(BadSlam.set_place_recognition: one Harris / BRIEF feature per 16 x 16 cell, brute-force matching, 3D-3D RANSAC start pose,
CloseLoop); the recognised places and what became of them are printed after the run.  Both streams must use the same level.

--render-dir DIR: after the run, the reconstructed surfel model is rendered from the pose of every keyframe (--render-every N:
of every N-th) with the depth camera as the run left it (DirectBA.RenderModel) and written to DIR as a TUM-style directory that
the dataset reader loads back: depth/<timestamp>.png (16-bit, the units of the input depth), rgb/<timestamp>.png, associated.txt,
calibration.txt and groundtruth.txt (the keyframe poses the views were rendered from).  --render-radius-scale S: the discs are
drawn with S times the surfels' radii; the default is the sparse surfel cell size of the run (4), because a surfel stands for a
cell of that many pixels a side while its radius is that of one pixel, so that scale closes the gaps between neighbours.
--render-source volume: the views are ray-cast from the fused surface instead of drawn from the discs (DirectBA.RenderVolume):
the keyframes are fused once with the --mesh-* options, whether or not --mesh is given, and every view is sampled at the voxel
size up to --max-depth.  The directory has the same layout.
--render-source mesh: the views are drawn from the triangle mesh that --mesh writes (DirectBA.RenderMesh), i.e. after
--mesh-min-component, the smoothing, --mesh-simplify-cell and the decimation, back faces culled, up to --max-depth; it needs --mesh.

--mesh PATH: after the last BA, all keyframes are fused into a truncated signed distance volume at their optimised poses
(DirectBA.FuseKeyframes) over the box of the surfel model (DirectBA.ModelBounds) padded by the truncation, and its surface
(DirectBA.ExtractMesh, surface nets) is written as a binary PLY with normals and colours.  --mesh-voxel-size M: metres, default
0.01; --mesh-truncation M: metres, default 4 voxels; --mesh-min-count N: a sample takes part when N keyframes saw it, default 1.
--mesh-min-component N: connected pieces of the surface with fewer than N vertices (flying pixels at occlusion edges, single noisy
blobs) are removed on the GPU before the file is written (DirectBA.ExtractMesh(min_component_vertices=N)); default 0, off.  The
summary line then names the pieces found and the vertices and triangles removed.
--mesh-smooth-iterations N: the mesh (after --mesh-min-component, before --mesh-simplify-cell and the decimation) is smoothed by N
iterations of the Taubin lambda|mu filter (DirectBA.SmoothMesh: a one-ring step with --mesh-smooth-lambda, default 0.5, then one with
--mesh-smooth-mu, default -0.53; 0 makes it plain Laplacian smoothing) and gets the normals of the smoothed geometry; default 0, off.
--mesh-smooth-boundary: open boundaries are held (fixed, the default), smoothed along themselves (rim) or like the rest (free).  The
defaults are provisional: they have been tried on synthetic meshes only.  The smoothed mesh is what is written, simplified, decimated
and scored; the parameters are printed and reported.
--mesh-simplify-cell M: the mesh (after --mesh-min-component and the smoothing) is simplified by vertex clustering on a grid of M metres
(DirectBA.SimplifyMesh: all vertices of a cell become their mean, collapsed triangles are dropped) without coarsening the volume
itself; default off.  The simplified mesh is what is written and what --ground-truth-surface scores (--surfel-mesh-distance keeps
measuring against the extracted one); the counts before and after are printed and reported.
--mesh-decimate-ratio R / --mesh-decimate-vertices N: the mesh (after --mesh-min-component and --mesh-simplify-cell) is decimated by
quadric-error edge collapse (DirectBA.DecimateMesh) to R times its vertices, or to N vertices; default off, and at most one of the
two.  Unlike clustering it spends the vertices where the surface bends and keeps creases and open boundaries.  The decimated mesh is
what is written and scored; the counts before and after and the number of rounds are printed and reported.
--mesh-fill-holes N: every hole of the mesh whose boundary has at most N (3 .. 4096) edges is closed by a vertex at the centroid of
its boundary and a fan of triangles (DirectBA.FillHoles), after --mesh-min-component and before the smoothing; larger boundaries, such
as the outer rim of an open scan, stay.  --mesh-clean: duplicate and degenerate triangles and the vertices only they name are removed
(DirectBA.CleanMesh) after --mesh-simplify-cell, so that the decimation sees no doubled face, and after the decimation.  Both are
off by default.  With either, the census of the mesh as written (DirectBA.MeshTopology: boundary, non-manifold and inconsistently
oriented edges, boundary loops, Euler characteristic, components) is printed and reported as mesh_topology, with the counts before and
after under mesh_hole_filling and mesh_cleaning.
--mesh-orient {majority,normals,volume}: the mesh gets one winding per connected patch (DirectBA.OrientMesh) right behind the extraction
and before --mesh-fill-holes, whose walk along a boundary a flipped triangle would stop: majority keeps the side most triangles of a
patch face, normals the side the vertex normals vote for, volume the side that encloses a positive volume (closed patches; others fall
back to majority); the normals are recomputed from the oriented triangles.  Off by default.  The counts (patches, those that cannot be
oriented, seams that disagreed before and after, flipped triangles, inverted and fallback patches) are printed and reported as
mesh_orientation, and mesh_topology is reported as with the other two.
A volume of more than 2^30 samples is refused: choose a larger voxel size.  --point-cloud PATH: the surfel cloud
(DirectBA.ExportToPointCloud) as a binary PLY with colours and normals.

--ground-truth-surface FILE.ply: the fused mesh (after --mesh-min-component) is evaluated against a ground-truth mesh or point
cloud given in the frame of the run (badslam_amd/surface_eval.py: accuracy from the mesh's vertices to the ground truth,
completeness from the ground truth's vertices to the mesh, precision / recall / F-score per threshold; for a coarse ground truth
see --surface-sample-spacing).  --surface-max-distance M: the search radius, default 0.1; a point with nothing within it fails
every threshold.  --surface-thresholds: default 0.01,0.02,0.05.  --surfel-mesh-distance: the summary of the distances from the
surfels' centres to the fused mesh (DirectBA.SurfelMeshDistance), a consistency figure that needs no ground truth.
--register-surface: the ground truth is in a frame of its own; the mesh's vertices are registered to it first (DirectBA.RegisterPoints
from the rigid alignment of the trajectories when --trajectory is given, else from the identity, within --surface-max-distance), and
the transform and the figures before it are printed and reported with the rest.
--surface-sample-spacing S: both figures are measured at points drawn uniformly by area, one per S x S metres on average, from each
side that has triangles (DirectBA.SampleMesh; surface_eval.evaluate(sample_density=1 / S^2)) instead of at the vertices, so that they
no longer depend on how either mesh is tessellated; the numbers of samples are printed and reported.
--surface-max-distance inf: no search radius.  Both directions then run through a bounding-volume hierarchy (DirectBA.NearestTriangle;
surface_eval.evaluate(max_distance=None)), every point hits and nothing is `beyond`; --register-surface needs a finite radius.
--surface-visible-only: completeness and recall are taken over the part of the ground truth the run could have observed -- the points
seen from at least one keyframe pose of the run, inside the depth camera's image, within --max-depth, facing the camera and not
occluded by the ground-truth mesh itself (DirectBA.MeshVisibility; surface_eval.evaluate(visible_from=...)); the report then also
holds completeness_all and visibility.  --surface-visibility-margin M: the segment to a point ends M metres before it, default 0.02.
The ground truth has to be a mesh.
--mesh-deviation: how far the --mesh-* operators moved the surface -- the mesh as written against the mesh as extracted, both ways and
without a radius (surface_eval.deviation: mean, rmse and max per direction, the Hausdorff distance, and the operators that ran); at
the vertices, or at samples when --surface-sample-spacing is given.
--surface-report FILE.json: what was printed, as JSON.  Either option fuses with the --mesh-* options whether or not --mesh is given.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from badslam_amd import abi, ate, bad_slam, png, surface_eval     # noqa: E402
from badslam_amd import direct_ba as dba            # noqa: E402


def camera_from(params, width, height):
    cam = abi.Camera4f()
    cam.fx, cam.fy, cam.cx, cam.cy = [float(v) for v in params]
    cam.width, cam.height = int(width), int(height)
    return cam


def scaled_camera(params, width, height, level):
    """The camera of pyramid level `level`: Camera::Scaled(2^-level) (LV/camera.h:1696-1705, BS/main.cc:421-424).  In the
    pixel-corner convention fx, fy, cx, cy are all multiplied by the factor (pinhole ScaleParameters, LV/camera.h:1086-1096)
    and the size is int(factor * size + 0.5)."""
    factor = 1.0 / (1 << level)
    return camera_from([factor * float(v) for v in params], int(factor * width + 0.5), int(factor * height + 0.5))


def check_level_fits(width, height, level):
    """A level halves the image exactly `level` times: the kernels take 2^level x 2^level blocks, so the size must divide."""
    if not 0 <= level <= 3 or width % (1 << level) or height % (1 << level):
        raise ValueError(f"pyramid level {level} does not fit a {width}x{height} dataset: levels are 0 ... 3 and the size must be divisible by 2^level")


def render_keyframes(ba, keyframes, render_dir, every=1, radius_scale=1.0, source="surfels", max_depth=50.0, min_count=1, mesh=None):
    """Writes the model views from the poses of keyframes[::every] -- (keyframe id, timestamp string) pairs -- as a TUM-style
    directory; deleted keyframes are left out.  source "surfels": RenderModel; "volume": RenderVolume of the fused volume, up to
    max_depth and over the samples at least min_count keyframes saw; "mesh": RenderMesh of the mesh dict `mesh`, up to max_depth.
    Returns the (keyframe id, timestamp) pairs written."""
    if source not in ("surfels", "volume", "mesh"):
        raise ValueError("--render-source must be surfels, volume or mesh")
    if source == "mesh" and mesh is None:
        raise ValueError("--render-source mesh needs a mesh")
    if every < 1:
        raise ValueError("--render-every must be at least 1")
    os.makedirs(os.path.join(str(render_dir), "depth"), exist_ok=True)
    os.makedirs(os.path.join(str(render_dir), "rgb"), exist_ok=True)
    _, depth4, _ = ba.intrinsics()
    written, associated, trajectory = [], [], ["# timestamp tx ty tz qx qy qz qw"]
    for kf_id, ts in keyframes[::every]:
        if ba.keyframe_is_deleted(kf_id):
            continue
        pose = ba.keyframe_pose(kf_id)
        if source == "volume":
            views = ba.RenderVolume(pose, max_depth=max_depth, min_count=min_count, views=("depth", "color"))
        elif source == "mesh":
            views = ba.RenderMesh(mesh, pose, max_depth=max_depth, views=("depth", "color"))
        else:
            views = ba.RenderModel(pose, radius_scale=radius_scale, views=("depth", "color"))
        png.write_png(os.path.join(str(render_dir), "depth", f"{ts}.png"), views["depth"])
        png.write_png(os.path.join(str(render_dir), "rgb", f"{ts}.png"), np.ascontiguousarray(views["color"][:, :, :3]))
        associated.append(f"{ts} rgb/{ts}.png {ts} depth/{ts}.png")
        q = dba.pose7(pose)
        trajectory.append(f"{ts} {q[4]:.9g} {q[5]:.9g} {q[6]:.9g} {q[0]:.9g} {q[1]:.9g} {q[2]:.9g} {q[3]:.9g}")
        written.append((kf_id, ts))
    with open(os.path.join(str(render_dir), "associated.txt"), "w") as f:
        f.write("\n".join(associated) + "\n")
    with open(os.path.join(str(render_dir), "calibration.txt"), "w") as f:    # pixel-centre convention on disk
        f.write(f"{depth4[0]:.9g} {depth4[1]:.9g} {depth4[2] - 0.5:.9g} {depth4[3] - 0.5:.9g}\n")
    with open(os.path.join(str(render_dir), "groundtruth.txt"), "w") as f:
        f.write("\n".join(trajectory) + "\n")
    return written


MAX_VOXELS = 1 << 30


def mesh_volume(bounds_min, bounds_max, voxel_size, truncation):
    """The volume over the box [bounds_min, bounds_max] padded by the truncation: (origin (3,) float32, (nx, ny, nz)); every
    dimension at least 2.  Raises ValueError, naming the voxel size, beyond 2^30 samples."""
    if not (voxel_size > 0 and truncation > 0):
        raise ValueError("--mesh-voxel-size and --mesh-truncation must be positive")
    lo = np.asarray(bounds_min, np.float64) - truncation
    hi = np.asarray(bounds_max, np.float64) + truncation
    dims = tuple(max(2, int(np.ceil((hi[i] - lo[i]) / voxel_size))) for i in range(3))
    if dims[0] * dims[1] * dims[2] > MAX_VOXELS:
        raise ValueError(f"a volume of {dims[0]} x {dims[1]} x {dims[2]} samples at --mesh-voxel-size {voxel_size:g} m exceeds 2^30: "
                         f"use a voxel size of at least {voxel_size * (dims[0] * dims[1] * dims[2] / MAX_VOXELS) ** (1 / 3) * 1.01:.3g} m")
    return lo.astype(np.float32), dims


def fuse_model(ba, voxel_size=0.01, truncation=None):
    """FuseKeyframes over the padded ModelBounds -> (origin, dims)."""
    truncation = 4 * voxel_size if truncation is None else truncation
    bounds = ba.ModelBounds()
    if bounds is None:
        raise ValueError("--mesh / --render-source volume: the model has no surfels to take the volume's bounds from")
    origin, dims = mesh_volume(bounds[0], bounds[1], voxel_size, truncation)
    ba.FuseKeyframes(origin, voxel_size, dims, truncation)
    return origin, dims


def fuse_and_mesh(ba, path, voxel_size=0.01, truncation=None, min_count=1, fused=None, min_component=0):
    """FuseKeyframes over the padded ModelBounds (unless `fused`, the (origin, dims) of fuse_model, says it was done), ExtractMesh,
    SaveMeshAsPLY (unless path is None) -> (mesh dict, origin, dims, component report or None).  min_component >= 2: the components of fewer vertices are
    removed before the file is written, and the report says what was found and removed."""
    origin, dims = fused if fused is not None else fuse_model(ba, voxel_size, truncation)
    report = None
    if min_component >= 2:
        mesh, report = ba.ExtractMesh(min_count, min_component_vertices=min_component, report=True)
    else:
        mesh = ba.ExtractMesh(min_count)
    if path:
        dba.SaveMeshAsPLY(path, mesh)
    return mesh, origin, dims, report


def run(dataset_dir, trajectory=None, out=None, keyframe_interval=10, ba_iterations=10, max_depth=3.0, end_frame=None, raw_to_float_depth=1.0 / 5000,
        num_scales=5, max_surfel_count=25 * 1000 * 1000, ba_cost=False, pyramid_level_for_depth=0, pyramid_level_for_color=0,
        median_filter_and_densify_iterations=0, render_dir=None, render_every=1, render_radius_scale=None, inspect=None,
        place_recognition=False, place_min_gap=10, mesh=None, mesh_voxel_size=0.01, mesh_truncation=None, mesh_min_count=1, point_cloud=None,
        render_source="surfels", mesh_min_component=0, ground_truth_surface=None, surface_max_distance=0.1, surface_thresholds=(0.01, 0.02, 0.05),
        surfel_mesh_distance=False, surface_report=None, register_surface=False, surface_sample_spacing=None, mesh_simplify_cell=None,
        mesh_deviation=False, mesh_decimate_ratio=None, mesh_decimate_vertices=None, mesh_smooth_iterations=0, mesh_smooth_lambda=0.5, mesh_smooth_mu=-0.53,
        mesh_smooth_boundary="fixed", mesh_fill_holes=None, mesh_clean=False, mesh_orient=None, surface_visible_only=False, surface_visibility_margin=0.02):
    """inspect: called with the BadSlam object and the result dict before the run returns, while the model is still alive."""
    if mesh_decimate_ratio is not None and mesh_decimate_vertices is not None:
        raise ValueError("give at most one of --mesh-decimate-ratio and --mesh-decimate-vertices")
    decimate = mesh_decimate_ratio is not None or mesh_decimate_vertices is not None
    if render_dir and render_source == "mesh" and not mesh:
        raise ValueError("--render-source mesh renders the mesh that --mesh writes: give --mesh PATH")
    if mesh_smooth_iterations < 0:
        raise ValueError("--mesh-smooth-iterations must be >= 0")
    smooth = mesh_smooth_iterations > 0
    if mesh_orient is not None and mesh_orient not in abi.ORIENT_MODES:
        raise ValueError("--mesh-orient must be majority, normals or volume")
    repair = mesh_fill_holes is not None or bool(mesh_clean) or mesh_orient is not None
    if not surface_max_distance > 0:
        raise ValueError("--surface-max-distance must be > 0 (inf: no search radius)")
    radius = None if np.isinf(surface_max_distance) else float(surface_max_distance)      # None: the tree of DirectBA.NearestTriangle, no grid
    if register_surface and radius is None:
        raise ValueError("--register-surface needs a finite --surface-max-distance: it is the registration's search radius")
    ds = dba.read_tum_dataset(dataset_dir, trajectory or "")
    frames = ds["frames"] if end_frame is None else ds["frames"][:end_frame]
    check_level_fits(ds["width"], ds["height"], pyramid_level_for_color)
    check_level_fits(ds["width"], ds["height"], pyramid_level_for_depth)
    color_cam = scaled_camera(ds["camera"], ds["width"], ds["height"], pyramid_level_for_color)
    depth_cam = scaled_camera(ds["camera"], ds["width"], ds["height"], pyramid_level_for_depth)
    cell = 4                # sparse surfel cell size of the front end
    slam = bad_slam.BadSlam(color_cam, depth_cam, sparse_surfel_cell_size=cell, keyframe_interval=keyframe_interval, max_num_ba_iterations_per_keyframe=ba_iterations,
                            num_scales=num_scales, max_surfel_count=max_surfel_count, raw_to_float_depth=raw_to_float_depth, max_depth=max_depth,
                            pyramid_level_for_depth=pyramid_level_for_depth, pyramid_level_for_color=pyramid_level_for_color,
                            median_filter_and_densify_iterations=median_filter_and_densify_iterations)
    if place_recognition:
        if pyramid_level_for_depth != pyramid_level_for_color:
            raise ValueError("--place-recognition needs colour and depth images of one size: use the same pyramid level for both streams")
        slam.set_place_recognition(True, min_keyframe_gap=place_min_gap)
    keyframes = []          # (keyframe id, timestamp string) in the order of creation
    for k, fr in enumerate(frames):
        slam.ProcessFrame(k, dba.read_png(fr["depth_path"]), dba.read_png(fr["rgb_path"]))
        if render_dir and slam.state()["keyframe_created"]:
            keyframes.append((slam.state()["base_kf_id"], fr["depth_timestamp"]))
    result = {}
    if ba_cost:
        before = slam.ba().ComputeCost()
        n = slam.ba().keyframe_count()
        slam.RunBundleAdjustment(len(frames) - 1, False, False, True, True, 1, ba_iterations, 0, n - 1, True)
        after = slam.ba().ComputeCost()
        result["ba_cost"] = (before["total"], after["total"], int(after["counts"].sum()))
    poses = slam.frame_poses()
    out = out or os.path.join(str(dataset_dir), "poses_badslam_amd.txt")
    dba.save_poses([f["depth_timestamp"] for f in frames], poses, 0, out)
    result.update({"frames": len(frames), "keyframes": slam.ba().keyframe_count(), "surfels": slam.ba().surfels_size(), "poses_file": out})
    if place_recognition:
        result["place_recognition"] = slam.place_recognition_log()
    fused = None
    if render_dir and render_source != "mesh":
        if render_source == "volume":
            fused = fuse_model(slam.ba(), mesh_voxel_size, mesh_truncation)
            result["volume"] = {"origin": fused[0], "dims": fused[1]}
        result["rendered"] = render_keyframes(slam.ba(), keyframes, render_dir, render_every, float(render_radius_scale or cell), render_source, max_depth,
                                              mesh_min_count)
        result["render_dir"] = str(render_dir)
    if point_cloud:
        positions, colors, normals = slam.ba().ExportToPointCloud()
        dba.SavePointCloudAsPLY(point_cloud, positions, colors, normals)
        result["point_cloud"] = (str(point_cloud), len(positions))
    if mesh or ground_truth_surface or surfel_mesh_distance or mesh_deviation:
        m, origin, dims, report = fuse_and_mesh(slam.ba(), None if smooth or mesh_simplify_cell or decimate or repair else mesh, mesh_voxel_size, mesh_truncation, mesh_min_count, fused,
                                                mesh_min_component)
        surface, smoothed, simplified, decimated, filled, cleaned, oriented = {}, None, None, None, None, [], None
        as_extracted = m

        def clean(before, after_what):
            c = slam.ba().CleanMesh(before)
            cleaned.append(dict(c["report"], after=after_what, vertices_before=len(before["positions"]), triangles_before=len(before["triangles"]),
                                vertices=len(c["positions"]), triangles=len(c["triangles"])))
            return c

        if mesh_orient is not None:
            o = slam.ba().OrientMesh(m, mode=mesh_orient, recompute_normals=True, report=True)
            oriented = dict(o["report"], mode=mesh_orient)
            m = {k: o[k] for k in ("positions", "normals", "colors", "triangles")}
        if mesh_fill_holes is not None:
            before = m
            m = slam.ba().FillHoles(before, int(mesh_fill_holes))
            filled = {"max_hole_edges": int(mesh_fill_holes), "filled_holes": int(m["filled_holes"]), "vertices_before": len(before["positions"]),
                      "triangles_before": len(before["triangles"]), "vertices": len(m["positions"]), "triangles": len(m["triangles"])}
        if smooth:
            m = slam.ba().SmoothMesh(m, iterations=int(mesh_smooth_iterations), lambda_=float(mesh_smooth_lambda), mu=float(mesh_smooth_mu), boundary=mesh_smooth_boundary)
            smoothed = {"iterations": int(mesh_smooth_iterations), "lambda": float(mesh_smooth_lambda), "mu": float(mesh_smooth_mu), "boundary": mesh_smooth_boundary}
        if mesh_simplify_cell:
            extracted = m
            m = slam.ba().SimplifyMesh(extracted, float(mesh_simplify_cell))
            simplified = {"cell": float(mesh_simplify_cell), "vertices_before": len(extracted["positions"]), "triangles_before": len(extracted["triangles"]),
                          "vertices": len(m["positions"]), "triangles": len(m["triangles"])}
            if mesh_clean:
                m = clean(m, "simplification")
        if decimate:
            before = m
            m = slam.ba().DecimateMesh(before, target_vertices=mesh_decimate_vertices, ratio=mesh_decimate_ratio)
            decimated = {"target_vertices": mesh_decimate_vertices, "ratio": mesh_decimate_ratio, "vertices_before": len(before["positions"]),
                         "triangles_before": len(before["triangles"]), "vertices": len(m["positions"]), "triangles": len(m["triangles"]), "rounds": int(m["rounds"])}
            if mesh_clean:
                m = clean(m, "decimation")
        if mesh and (smooth or mesh_simplify_cell or decimate or repair):
            dba.SaveMeshAsPLY(mesh, m)
        if repair:
            surface["mesh_topology"] = slam.ba().MeshTopology(m)
            if oriented:
                surface["mesh_orientation"] = oriented
            if filled:
                surface["mesh_hole_filling"] = filled
            if cleaned:
                surface["mesh_cleaning"] = cleaned
        if ground_truth_surface:
            surface["ground_truth"] = str(ground_truth_surface)
            start = None
            if register_surface and trajectory:       # the rigid alignment of the trajectories (estimate -> ground truth) is the start
                aligned = ate.ate_files(os.path.join(str(dataset_dir), trajectory), out)
                start = np.eye(4)
                start[:3, :3], start[:3, 3] = aligned["R"], aligned["t"]
            visible = {}
            if surface_visible_only:    # completeness over what the keyframes could have observed: their poses, the depth camera, the run's depth range
                ba = slam.ba()
                kf_poses = [ba.keyframe_pose(k) for k in range(ba.keyframe_count()) if not ba.keyframe_is_deleted(k)]
                visible = dict(visible_from=dict(poses=kf_poses, max_depth=float(max_depth), margin=float(surface_visibility_margin)))
            surface.update(surface_eval.evaluate(slam.ba(), m, dba.LoadPLY(ground_truth_surface), radius, tuple(surface_thresholds),
                                                 register=bool(register_surface), initial=start,
                                                 sample_density=None if surface_sample_spacing is None else 1.0 / (float(surface_sample_spacing) ** 2), **visible))
        if surfel_mesh_distance:
            if radius is None:      # the centres of ExportToPointCloud, in its order, against the mesh as extracted
                centre_distance = slam.ba().NearestTriangle(slam.ba().ExportToPointCloud()[0], as_extracted)["distance"]
            else:
                centre_distance = slam.ba().SurfelMeshDistance(radius)["distance"]
            surface["surfel_mesh_distance"] = surface_eval.distance_summary(centre_distance, tuple(surface_thresholds))
        if mesh_deviation:
            operators = ([f"orient ({mesh_orient})"] if oriented else []) + (["fill holes"] if filled else []) + (["smooth"] if smoothed else []) + \
                        (["simplify"] if simplified else []) + (["decimate"] if decimated else []) + (["clean"] if cleaned else [])
            surface["mesh_deviation"] = dict(surface_eval.deviation(slam.ba(), m, as_extracted,
                                                                    sample_density=None if surface_sample_spacing is None else 1.0 / (float(surface_sample_spacing) ** 2)),
                                             operators=operators)
        if surface:
            surface["max_distance"] = radius
            if smoothed:
                surface["mesh_smoothing"] = smoothed
            if simplified:
                surface["mesh_simplification"] = simplified
            if decimated:
                surface["mesh_decimation"] = decimated
            result["surface"] = surface
            if surface_report:
                with open(surface_report, "w") as f:
                    json.dump(surface, f, indent=1)
    if render_dir and render_source == "mesh":      # the mesh as written: after the clean-up, smoothing, simplification and decimation
        result["rendered"] = render_keyframes(slam.ba(), keyframes, render_dir, render_every, source="mesh", max_depth=max_depth, mesh=m)
        result["render_dir"] = str(render_dir)
    if mesh:
        result["mesh"] = {"path": str(mesh), "vertices": len(m["positions"]), "triangles": len(m["triangles"]), "origin": origin, "dims": dims}
        if report is not None:
            result["mesh"].update(components=report["components"], removed_vertices=report["removed_vertices"], removed_triangles=report["removed_triangles"])
        if smoothed:
            result["mesh"]["smoothing"] = smoothed
        if simplified:
            result["mesh"]["simplification"] = simplified
        if decimated:
            result["mesh"]["decimation"] = decimated
        if oriented:
            result["mesh"]["orientation"] = oriented
        if filled:
            result["mesh"]["hole_filling"] = filled
        if cleaned:
            result["mesh"]["cleaning"] = cleaned
    if inspect:
        inspect(slam, result)
    if trajectory:
        result["ate"] = ate.ate_files(os.path.join(str(dataset_dir), trajectory), out)
    return result


def arg_parser():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("dataset_dir")
    ap.add_argument("--trajectory", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--keyframe-interval", type=int, default=10)
    ap.add_argument("--ba-iterations", type=int, default=10)
    ap.add_argument("--max-depth", type=float, default=3.0)
    ap.add_argument("--end-frame", type=int, default=None)
    ap.add_argument("--ba-cost", action="store_true")
    ap.add_argument("--pyramid-level-for-depth", type=int, default=0)
    ap.add_argument("--pyramid-level-for-color", type=int, default=0)
    ap.add_argument("--median-filter-and-densify-iterations", type=int, default=0)
    ap.add_argument("--render-dir", default=None)
    ap.add_argument("--render-every", type=int, default=1)
    ap.add_argument("--render-radius-scale", type=float, default=None)
    ap.add_argument("--render-source", choices=("surfels", "volume", "mesh"), default="surfels")
    ap.add_argument("--place-recognition", action="store_true")
    ap.add_argument("--place-min-gap", type=int, default=10)
    ap.add_argument("--mesh", default=None)
    ap.add_argument("--mesh-voxel-size", type=float, default=0.01)
    ap.add_argument("--mesh-truncation", type=float, default=None)
    ap.add_argument("--mesh-min-count", type=int, default=1)
    ap.add_argument("--mesh-min-component", type=int, default=0)
    ap.add_argument("--mesh-smooth-iterations", type=int, default=0)
    ap.add_argument("--mesh-smooth-lambda", type=float, default=0.5)
    ap.add_argument("--mesh-smooth-mu", type=float, default=-0.53)
    ap.add_argument("--mesh-smooth-boundary", choices=("fixed", "rim", "free"), default="fixed")
    ap.add_argument("--mesh-simplify-cell", type=float, default=None)
    ap.add_argument("--mesh-decimate-ratio", type=float, default=None)
    ap.add_argument("--mesh-decimate-vertices", type=int, default=None)
    ap.add_argument("--mesh-fill-holes", type=int, default=None)
    ap.add_argument("--mesh-clean", action="store_true")
    ap.add_argument("--mesh-orient", choices=tuple(abi.ORIENT_MODES), default=None)
    ap.add_argument("--point-cloud", default=None)
    ap.add_argument("--ground-truth-surface", default=None)
    ap.add_argument("--surface-max-distance", type=float, default=0.1)      # "inf": no search radius
    ap.add_argument("--mesh-deviation", action="store_true")
    ap.add_argument("--surface-thresholds", type=lambda text: tuple(float(v) for v in text.split(",")), default=(0.01, 0.02, 0.05))
    ap.add_argument("--surfel-mesh-distance", action="store_true")
    ap.add_argument("--surface-report", default=None)
    ap.add_argument("--register-surface", action="store_true")
    ap.add_argument("--surface-sample-spacing", type=float, default=None)
    ap.add_argument("--surface-visible-only", action="store_true")
    ap.add_argument("--surface-visibility-margin", type=float, default=0.02)
    return ap


def main():
    a = arg_parser().parse_args()
    r = run(a.dataset_dir, a.trajectory, a.out, a.keyframe_interval, a.ba_iterations, a.max_depth, a.end_frame, ba_cost=a.ba_cost,
            pyramid_level_for_depth=a.pyramid_level_for_depth, pyramid_level_for_color=a.pyramid_level_for_color,
            median_filter_and_densify_iterations=a.median_filter_and_densify_iterations, render_dir=a.render_dir, render_every=a.render_every,
            render_radius_scale=a.render_radius_scale, place_recognition=a.place_recognition, place_min_gap=a.place_min_gap, mesh=a.mesh,
            mesh_voxel_size=a.mesh_voxel_size, mesh_truncation=a.mesh_truncation, mesh_min_count=a.mesh_min_count, point_cloud=a.point_cloud,
            render_source=a.render_source, mesh_min_component=a.mesh_min_component, ground_truth_surface=a.ground_truth_surface,
            surface_max_distance=a.surface_max_distance, surface_thresholds=a.surface_thresholds, surfel_mesh_distance=a.surfel_mesh_distance,
            surface_report=a.surface_report, register_surface=a.register_surface, surface_sample_spacing=a.surface_sample_spacing,
            surface_visible_only=a.surface_visible_only, surface_visibility_margin=a.surface_visibility_margin,
            mesh_deviation=a.mesh_deviation, mesh_simplify_cell=a.mesh_simplify_cell, mesh_decimate_ratio=a.mesh_decimate_ratio, mesh_decimate_vertices=a.mesh_decimate_vertices,
            mesh_smooth_iterations=a.mesh_smooth_iterations, mesh_smooth_lambda=a.mesh_smooth_lambda, mesh_smooth_mu=a.mesh_smooth_mu,
            mesh_smooth_boundary=a.mesh_smooth_boundary, mesh_fill_holes=a.mesh_fill_holes, mesh_clean=a.mesh_clean, mesh_orient=a.mesh_orient)
    if "ba_cost" in r:
        print(f"BA objective before the final BA {r['ba_cost'][0]:.6e}, after {r['ba_cost'][1]:.6e} ({r['ba_cost'][2]} residual pairs)")
    print(f"{r['frames']} frames, {r['keyframes']} keyframes, {r['surfels']} surfels -> {r['poses_file']}")
    for e in r.get("place_recognition", []):
        if e["candidate"] >= 0:
            print(f"keyframe {e['keyframe']}: place of keyframe {e['candidate']} ({e['match_count']} matches, {e['inlier_count']} inliers) -> "
                  f"{e['status'] if e['loop_attempted'] else 'no start pose'}")
    if "rendered" in r:
        print(f"{len(r['rendered'])} model views -> {r['render_dir']}")
    if "point_cloud" in r:
        print(f"{r['point_cloud'][1]} points -> {r['point_cloud'][0]}")
    if "mesh" in r:
        cleaned = ""
        if "components" in r["mesh"]:
            cleaned = (f" ({r['mesh']['components']} components before clean-up, {r['mesh']['removed_vertices']} vertices and "
                       f"{r['mesh']['removed_triangles']} triangles removed)")
        if "smoothing" in r["mesh"]:
            sm = r["mesh"]["smoothing"]
            cleaned += f" (smoothed by {sm['iterations']} iterations of lambda {sm['lambda']:g}, mu {sm['mu']:g}, boundary {sm['boundary']})"
        if "simplification" in r["mesh"]:
            sp = r["mesh"]["simplification"]
            cleaned += f" (simplified at {sp['cell']:g} m from {sp['vertices_before']} vertices, {sp['triangles_before']} triangles)"
        if "decimation" in r["mesh"]:
            dc = r["mesh"]["decimation"]
            cleaned += f" (decimated in {dc['rounds']} rounds from {dc['vertices_before']} vertices, {dc['triangles_before']} triangles)"
        print(f"mesh of {r['mesh']['vertices']} vertices, {r['mesh']['triangles']} triangles from {r['mesh']['dims']} samples{cleaned} -> {r['mesh']['path']}")
    if "surface" in r:
        sf = r["surface"]
        if "mesh_smoothing" in sf and "mesh" not in r:
            sm = sf["mesh_smoothing"]
            print(f"mesh smoothed by {sm['iterations']} iterations of lambda {sm['lambda']:g}, mu {sm['mu']:g}, boundary {sm['boundary']}")
        if "mesh_simplification" in sf and "mesh" not in r:
            sp = sf["mesh_simplification"]
            print(f"mesh simplified at {sp['cell']:g} m: {sp['vertices_before']} vertices, {sp['triangles_before']} triangles -> {sp['vertices']}, {sp['triangles']}")
        if "mesh_decimation" in sf and "mesh" not in r:
            dc = sf["mesh_decimation"]
            print(f"mesh decimated in {dc['rounds']} rounds: {dc['vertices_before']} vertices, {dc['triangles_before']} triangles -> {dc['vertices']}, {dc['triangles']}")
        if "mesh_orientation" in sf:
            mo = sf["mesh_orientation"]
            print(f"mesh oriented by {mo['mode']}: {mo['patches']} patches ({mo['nonorientable_patches']} not orientable, {mo['closed_patches']} closed), "
                  f"{mo['disagreeing_seams_before']} of {mo['seams']} seams disagreed, {mo['disagreeing_seams_after']} do; {mo['flipped_triangles']} triangles flipped, "
                  f"{mo['inverted_patches']} patches inverted, {mo['fallback_patches']} by the majority for want of a vote")
        if "mesh_hole_filling" in sf:
            fh = sf["mesh_hole_filling"]
            print(f"{fh['filled_holes']} holes of at most {fh['max_hole_edges']} edges filled: {fh['vertices_before']} vertices, {fh['triangles_before']} triangles -> "
                  f"{fh['vertices']}, {fh['triangles']}")
        for cl in sf.get("mesh_cleaning", []):
            print(f"mesh cleaned after the {cl['after']}: {cl['duplicate_triangles']} duplicate and {cl['degenerate_triangles']} degenerate triangles, "
                  f"{cl['welded_vertices']} welded and {cl['unreferenced_vertices']} unreferenced vertices removed -> {cl['vertices']} vertices, {cl['triangles']} triangles")
        if "mesh_topology" in sf:
            tp = sf["mesh_topology"]
            print(f"mesh topology: {tp['components']} components, {tp['unique_edges']} edges ({tp['boundary_edges']} boundary, {tp['nonmanifold_edges']} non-manifold, "
                  f"{tp['inconsistent_edges']} inconsistently oriented), {tp['loops']} boundary loops (longest {tp['longest_loop']}), {tp['blocked_vertices']} blocked "
                  f"vertices, Euler characteristic {tp['euler']}; closed: {tp['closed']}, oriented: {tp['oriented']}")
        if "registration" in sf:
            reg = sf["registration"]
            print(f"registration to the ground truth: {reg['reason']} after {reg['iterations']} steps; ground_truth_T_mesh =")
            for row in reg["target_T_source"][:3]:
                print("  " + " ".join(f"{v: .9f}" for v in row))
            print(surface_eval.format_summary("accuracy before registration", reg["before"]["accuracy"]))
            print(surface_eval.format_summary("completeness before registration", reg["before"]["completeness"]))
        if "sampling" in sf:
            sm = sf["sampling"]
            at = lambda n: "its vertices" if n is None else f"{n} samples"
            print(f"measured at {sm['density']:g} samples per square metre: the mesh at {at(sm['reconstruction_samples'])}, the ground truth at {at(sm['ground_truth_samples'])}")
        if "accuracy" in sf:
            within = "no search radius" if sf["max_distance"] is None else f"within {sf['max_distance']:g} m"
            print(surface_eval.format_summary(f"accuracy (mesh -> {sf['ground_truth']}, {within})", sf["accuracy"]))
            if "visibility" in sf:
                vs = sf["visibility"]
                print(f"visible from the {vs['views']} keyframes (margin {vs['margin']:g} m): {vs['visible_points']} of {vs['points']} ground-truth points "
                      f"({100 * vs['visible_fraction']:.1f} %); completeness and recall are over these")
                print(surface_eval.format_summary("completeness over all points", sf["completeness_all"]))
            print(surface_eval.format_summary("completeness (ground truth -> mesh)", sf["completeness"]))
            for row in sf["f_scores"]:
                print(f"  at {row['threshold']:g} m: precision {row['precision']:.4f}, recall {row['recall']:.4f}, F-score {row['f_score']:.4f}")
        if "surfel_mesh_distance" in sf:
            print(surface_eval.format_summary("surfel centres -> mesh", sf["surfel_mesh_distance"]))
        if "mesh_deviation" in sf:
            dv = sf["mesh_deviation"]
            side = lambda s: f"mean {s['mean']:.5f}, rmse {s['rmse']:.5f}, max {s['max']:.5f} m over {s['count']} points"
            print(f"mesh as written against the mesh as extracted (operators: {', '.join(dv['operators']) or 'none'}): written -> extracted {side(dv['mesh_to_reference'])}; "
                  f"extracted -> written {side(dv['reference_to_mesh'])}; Hausdorff {dv['hausdorff']:.5f} m")
    if "ate" in r:
        print(f"ATE RMSE {r['ate']['rmse']:.6f} m over {r['ate']['pairs']} poses")


if __name__ == "__main__":
    main()
