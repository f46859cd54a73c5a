"""-m gpu: BadSlam with the sensor rectification on.  The 13-frame plane sequence of tests/test_gpu_bad_slam.py (same planes,
poses, 320 x 240 target, keyframe every 4th frame) is ray-cast as a RAW sensor would see it -- a distorted 308 x 235 colour
camera and a differently distorted 320 x 240 depth camera 25 mm beside it -- and goes through set_sensor_rectification and
ProcessFrame.  The baseline is the same scene rendered as ideal frames of the undistorted camera through a plain instance."""
import numpy as np
import pytest

from badslam_amd import ate, bad_slam
from badslam_amd import direct_ba as dba
from badslam_amd import rectification as rect
from tests import bso, scenes
from tests import rectify_util as ru
from tests.test_gpu_bad_slam import trajectory_dict

pytestmark = pytest.mark.gpu

N_FRAMES = 13
RAW_TO_FLOAT = float(np.float32(1.0 / 5000))
BASELINE = 0.025

# ATE RMSE of the two runs as measured on an MI355X (DESIGN.md section 8 "Sensor rectification"): plain 0.1327 mm, rectified
# 0.1474 mm.  The gap of 0.0147 mm is what one bilinear resampling of the colour image and the re-rounding of the reprojected
# depth to whole units cost the tracker; the rectified run may exceed the plain run of the same test by twice that gap.
MEASURED_PLAIN_ATE = 1.327e-4
MEASURED_RECTIFIED_ATE = 1.474e-4
ATE_MARGIN = 2 * (MEASURED_RECTIFIED_ATE - MEASURED_PLAIN_ATE)     # 2.9e-5 m


def sensor():
    color = rect.radtan_camera(308, 235, 262.5, 262.5, 154.8, 116.2, -0.12, 0.03, 0.0, 4e-4, -3e-4)
    depth = rect.radtan_camera(320, 240, 230.0, 231.0, 158.1, 121.3, -0.08, 0.015, 0.0, -3e-4, 5e-4)
    color_T_depth = np.eye(4)[:3].copy()
    color_T_depth[0, 3] = BASELINE
    return color, depth, color_T_depth


def quantise(z):
    valid = np.isfinite(z) & (z < 6.0)
    depth = np.where(valid, z / RAW_TO_FLOAT + 0.5, 0).astype(np.uint32)
    return np.where(depth >= 32768, 0, depth).astype(np.uint16), valid


def shade(z, plane, dg, o, valid):
    points = o[None, None, :] + dg * np.where(valid, z, 0.0)[..., None]
    lum = scenes.texture_at(points, plane, 0.37)
    return np.ascontiguousarray(np.repeat(lum[:, :, None], 3, axis=2))


@pytest.fixture(scope="module")
def sequence(oracle):
    """(target camera, ideal frames, raw frames, ground truth): planes and poses exactly as tests/test_gpu_bad_slam.render_sequence."""
    color, depth_cam, color_T_depth = sensor()
    target = rect.decide_undistorted_camera(color, True)
    assert (target.width, target.height) == (320, 240)
    rng = np.random.default_rng(3)
    planes = scenes.random_planes(rng, 20)
    step = np.array([0.010, -0.004, 0.006, 0.004, -0.006, 0.003], np.float32)
    ideal_rays, color_rays, depth_rays = ru.pinhole_rays(target), rect.make_unprojection_map(color), rect.make_unprojection_map(depth_cam)
    ideal, raw, gt = [], [], []
    T = bso.se3_identity()
    for k in range(N_FRAMES):
        if k:
            wobble = (0.15 * np.sin(0.9 * k + np.arange(6))).astype(np.float32)
            T = bso.se3_mul(T, bso.se3_exp(step * (1 + wobble)))
        M = np.array(list(bso.se3_matrix3x4(T).m), np.float64).reshape(3, 4)
        R, t = M[:, :3], M[:, 3]
        z, plane, dg, o = ru.cast_planes(ideal_rays, R, t, planes)
        d, valid = quantise(z)
        ideal.append((d, shade(z, plane, dg, o, valid)))
        z, plane, dg, o = ru.cast_planes(color_rays, R, t, planes)
        raw_rgb = shade(z, plane, dg, o, np.isfinite(z) & (z < 6.0))
        z, _, _, _ = ru.cast_planes(depth_rays, R @ color_T_depth[:, :3], t + R @ color_T_depth[:, 3], planes)
        raw.append((quantise(z)[0], raw_rgb))
        gt.append(T)
    return target, ideal, raw, gt


def make_slam(target):
    return bad_slam.BadSlam(target, target, keyframe_interval=4, max_num_ba_iterations_per_keyframe=5, num_scales=4, max_surfel_count=400000,
                            raw_to_float_depth=RAW_TO_FLOAT, max_depth=6.0, baseline_fx=40.0)


def run(slam, frames):
    schedule = []
    for k, (depth, rgb) in enumerate(frames):
        slam.ProcessFrame(k, depth, rgb)
        schedule.append(slam.state()["keyframe_created"])
    return schedule, slam.frame_poses()


@pytest.fixture(scope="module")
def plain_run(sequence):
    target, ideal, raw, gt = sequence
    slam = make_slam(target)
    schedule, poses = run(slam, ideal)
    slam.close()
    return schedule, poses


def test_raw_sensor_frames_through_the_front_end(oracle, sequence, plain_run):
    target, ideal, raw, gt = sequence
    color, depth_cam, color_T_depth = sensor()
    plain_schedule, plain_poses = plain_run
    slam = make_slam(target)
    with pytest.raises(ValueError):
        slam.ProcessFrame(0, *raw[0])                                   # rectification is off: raw sizes are refused
    slam.set_sensor_rectification(color, depth_cam, color_T_depth, depth_difference_threshold=0.05, raw_depth_to_metres=RAW_TO_FLOAT)
    with pytest.raises(ValueError):
        slam.ProcessFrame(0, *ideal[0])                                 # now the raw sizes are expected
    schedule, poses = run(slam, raw)
    assert slam.ba().keyframe_count() == 4 and slam.ba().surfels_size() > 5000
    slam.close()
    assert schedule == plain_schedule == [k % 4 == 0 for k in range(N_FRAMES)]

    gt7 = np.array([dba.pose7(T) for T in gt], np.float32)
    plain_ate = ate.ate(trajectory_dict(gt7), trajectory_dict(plain_poses))["rmse"]
    rectified_ate = ate.ate(trajectory_dict(gt7), trajectory_dict(poses))["rmse"]
    print(f"ATE RMSE: plain {plain_ate:.6g} m, rectified {rectified_ate:.6g} m, gap {rectified_ate - plain_ate:.3g} m, margin {ATE_MARGIN}")
    assert plain_ate < 2e-3                                             # the bound of tests/test_gpu_bad_slam.py on the baseline
    assert rectified_ate <= plain_ate + ATE_MARGIN


def test_a_wrong_target_size_is_rejected(oracle, sequence):
    target, ideal, raw, gt = sequence
    color, depth_cam, color_T_depth = sensor()
    slam = make_slam(target)
    smaller = rect.radtan_camera(300, 235, 262.5, 262.5, 150.8, 116.2, -0.12, 0.03, 0.0, 4e-4, -3e-4)
    with pytest.raises(dba.DirectBAError, match="2\\^level"):
        slam.set_sensor_rectification(smaller, depth_cam, color_T_depth)
    with pytest.raises(dba.DirectBAError):
        slam.set_sensor_rectification(color, depth_cam, color_T_depth, depth_difference_threshold=0.0)
    slam.close()


def test_switching_it_off_again_reproduces_the_plain_run(oracle, sequence, plain_run):
    target, ideal, raw, gt = sequence
    color, depth_cam, color_T_depth = sensor()
    slam = make_slam(target)
    slam.set_sensor_rectification(color, depth_cam, color_T_depth, raw_depth_to_metres=RAW_TO_FLOAT)
    slam.PreprocessFrame(*raw[0])                                       # the staging buffers have been used
    slam.set_sensor_rectification(None)
    schedule, poses = run(slam, ideal)
    slam.close()
    assert schedule == plain_run[0]
    assert np.array_equal(poses.view(np.uint32), plain_run[1].view(np.uint32))
