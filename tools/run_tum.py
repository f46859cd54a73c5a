#!/usr/bin/env python3
"""Runs the sequential BadSlam front end over a TUM RGB-D directory (associated.txt + calibration.txt, as the reference's
dataset reader expects, LV/rgbd_video_io_tum_dataset.h:128-240), writes the trajectory in TUM format and, if the directory
has a ground truth, prints the ATE RMSE.

    python tools/run_tum.py <dataset_dir> [--trajectory groundtruth.txt] [--out poses.txt] [--keyframe-interval 10]
                            [--ba-iterations 10] [--max-depth 3.0] [--end-frame N] [--ba-cost]
                            [--pyramid-level-for-depth L] [--pyramid-level-for-color L]
                            [--median-filter-and-densify-iterations N]

--pyramid-level-for-depth / --pyramid-level-for-color (0 ... 3): the stream is halved L times on the GPU before anything else
sees it and its camera is scaled to match (level 1 runs a 640x480 dataset at 320x240).  --median-filter-and-densify-iterations:
3x3 depth median that also fills holes, for noisy sensors; not together with a depth level.

--ba-cost: after the last frame, one more BA over the whole window (poses + geometry), with the BA objective printed before and
after it (DirectBA.ComputeCost: Tukey depth terms + weighted Huber descriptor terms over all surfel / keyframe pairs).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from badslam_amd import abi, ate, bad_slam          # noqa: E402
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


def run(dataset_dir, trajectory=None, out=None, keyframe_interval=10, ba_iterations=10, max_depth=3.0, end_frame=None, raw_to_float_depth=1.0 / 5000,
        num_scales=5, max_surfel_count=25 * 1000 * 1000, ba_cost=False, pyramid_level_for_depth=0, pyramid_level_for_color=0,
        median_filter_and_densify_iterations=0):
    ds = dba.read_tum_dataset(dataset_dir, trajectory or "")
    frames = ds["frames"] if end_frame is None else ds["frames"][:end_frame]
    check_level_fits(ds["width"], ds["height"], pyramid_level_for_color)
    check_level_fits(ds["width"], ds["height"], pyramid_level_for_depth)
    color_cam = scaled_camera(ds["camera"], ds["width"], ds["height"], pyramid_level_for_color)
    depth_cam = scaled_camera(ds["camera"], ds["width"], ds["height"], pyramid_level_for_depth)
    slam = bad_slam.BadSlam(color_cam, depth_cam, keyframe_interval=keyframe_interval, max_num_ba_iterations_per_keyframe=ba_iterations,
                            num_scales=num_scales, max_surfel_count=max_surfel_count, raw_to_float_depth=raw_to_float_depth, max_depth=max_depth,
                            pyramid_level_for_depth=pyramid_level_for_depth, pyramid_level_for_color=pyramid_level_for_color,
                            median_filter_and_densify_iterations=median_filter_and_densify_iterations)
    for k, fr in enumerate(frames):
        slam.ProcessFrame(k, dba.read_png(fr["depth_path"]), dba.read_png(fr["rgb_path"]))
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
    return ap


def main():
    a = arg_parser().parse_args()
    r = run(a.dataset_dir, a.trajectory, a.out, a.keyframe_interval, a.ba_iterations, a.max_depth, a.end_frame, ba_cost=a.ba_cost,
            pyramid_level_for_depth=a.pyramid_level_for_depth, pyramid_level_for_color=a.pyramid_level_for_color,
            median_filter_and_densify_iterations=a.median_filter_and_densify_iterations)
    if "ba_cost" in r:
        print(f"BA objective before the final BA {r['ba_cost'][0]:.6e}, after {r['ba_cost'][1]:.6e} ({r['ba_cost'][2]} residual pairs)")
    print(f"{r['frames']} frames, {r['keyframes']} keyframes, {r['surfels']} surfels -> {r['poses_file']}")
    if "ate" in r:
        print(f"ATE RMSE {r['ate']['rmse']:.6f} m over {r['ate']['pairs']} poses")


if __name__ == "__main__":
    main()
