"""-m gpu: the three input-conditioning switches of the BadSlam front end (pyramid_level_for_depth, pyramid_level_for_color,
median_filter_and_densify_iterations; BS/bad_slam.cc:645-685).  A 640x480 rendered sequence goes through an instance
with a switch on, and through a plain instance that is fed the frames conditioned on the host by the NumPy restatements
of tests/test_gpu_input_conditioning.py.  Everything after the conditioning stage is deterministic and sees the same
bytes, so poses, surfel count and keyframe count must be bit-identical."""
import numpy as np
import pytest

from badslam_amd import ate, bad_slam
from badslam_amd import direct_ba as dba
from tests import bso, scenes
from tests.test_gpu_input_conditioning import np_downscale_depth_median, np_downscale_rgb, np_median_filter_and_densify

pytestmark = pytest.mark.gpu

W, H = 640, 480
N_FRAMES = 9
SETTINGS = dict(keyframe_interval=4, max_num_ba_iterations_per_keyframe=5, num_scales=4, max_surfel_count=1000000, max_depth=6.0, baseline_fx=40.0)


def render_sequence(n_frames, seed=3):
    """tests/test_gpu_bad_slam.py::render_sequence at 640x480 with doubled intrinsics."""
    rng = np.random.default_rng(seed)
    cam = bso.make_camera(525.0, 525.0, 320.0, 240.0, W, H)
    raw_to_float = np.float32(1.0 / 5000)
    planes = scenes.random_planes(rng, 20)
    step = np.array([0.010, -0.004, 0.006, 0.004, -0.006, 0.003], np.float32)     # per frame: ~1.2 cm, ~0.45 degrees
    frames, gt = [], []
    T = bso.se3_identity()
    for k in range(n_frames):
        if k:
            wobble = (0.15 * np.sin(0.9 * k + np.arange(6))).astype(np.float32)   # not exactly constant motion
            T = bso.se3_mul(T, bso.se3_exp(step * (1 + wobble)))
        M = np.array(list(bso.se3_matrix3x4(T).m), np.float64).reshape(3, 4)
        tt, pidx, dg, o = scenes.render_planes(cam, W, H, M[:, :3], M[:, 3], planes)
        valid = np.isfinite(tt) & (tt < 6.0)
        depth = np.where(valid, tt / float(raw_to_float) + 0.5, 0).astype(np.uint32)
        depth = np.where(depth >= 32768, 0, depth).astype(np.uint16)              # 0 = no measurement, as in the dataset PNGs
        pts = o[None, None, :] + dg * np.where(valid, tt, 0.0)[..., None]
        lum = scenes.texture_at(pts, pidx, 0.37)
        frames.append((depth, np.ascontiguousarray(np.repeat(lum[:, :, None], 3, axis=2))))
        gt.append(T)
    return cam, float(raw_to_float), frames, gt


@pytest.fixture(scope="module")
def sequence(oracle):
    full_cam, raw_to_float, frames, gt = render_sequence(N_FRAMES)
    half_cam = bso.make_camera(262.5, 262.5, 160.0, 120.0, W // 2, H // 2)
    return dict(full_cam=full_cam, half_cam=half_cam, raw_to_float=raw_to_float, frames=frames, gt=gt)


def run(color_cam, depth_cam, raw_to_float, frames, **switches):
    """The whole sequence through one BadSlam: (frame poses, surfel count, keyframe count)."""
    slam = bad_slam.BadSlam(color_cam, depth_cam, raw_to_float_depth=raw_to_float, **SETTINGS, **switches)
    for k, (depth, rgb) in enumerate(frames):
        slam.ProcessFrame(k, depth, rgb)
    result = (slam.frame_poses().copy(), slam.ba().surfels_size(), slam.ba().keyframe_count())
    slam.close()
    assert result[0].shape == (len(frames), 7) and np.isfinite(result[0]).all()
    assert result[1] > 5000 and result[2] == (len(frames) + 3) // 4
    assert np.abs(result[0][-1, 4:7] - result[0][0, 4:7]).max() > 0.01          # the camera was tracked, not left where it started
    return result


def assert_same(got, want):
    assert got[1] == want[1] and got[2] == want[2], (got[1:], want[1:])
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), np.abs(got[0] - want[0]).max()


@pytest.fixture(scope="module")
def half_size_run(sequence):
    """A plain instance (no new keywords) with the half-size cameras on frames downscaled on the host."""
    s = sequence
    frames = [(np_downscale_depth_median(d, 1), np_downscale_rgb(rgb, 1)) for d, rgb in s["frames"]]
    return frames, run(s["half_cam"], s["half_cam"], s["raw_to_float"], frames)


def test_pyramid_level_1_for_both_streams(sequence, half_size_run):
    s = sequence
    got = run(s["half_cam"], s["half_cam"], s["raw_to_float"], s["frames"], pyramid_level_for_depth=1, pyramid_level_for_color=1)
    assert_same(got, half_size_run[1])


def test_default_path_is_unchanged(sequence, half_size_run):
    frames, want = half_size_run
    s = sequence
    got = run(s["half_cam"], s["half_cam"], s["raw_to_float"], frames, pyramid_level_for_depth=0, pyramid_level_for_color=0,
              median_filter_and_densify_iterations=0)
    assert_same(got, want)


def test_median_filter_and_densify(sequence):
    s = sequence
    got = run(s["full_cam"], s["full_cam"], s["raw_to_float"], s["frames"], median_filter_and_densify_iterations=2)
    filtered = [(np_median_filter_and_densify(d, 2), rgb) for d, rgb in s["frames"]]
    assert all((f[0] != n[0]).any() for f, n in zip(filtered, s["frames"]))       # the filter does change these frames
    want = run(s["full_cam"], s["full_cam"], s["raw_to_float"], filtered)
    assert_same(got, want)


def test_colour_level_only_with_cameras_of_different_sizes(sequence):
    """Colour level 1, depth level 0: a 320x240 colour camera next to a 640x480 depth camera."""
    s = sequence
    got = run(s["half_cam"], s["full_cam"], s["raw_to_float"], s["frames"], pyramid_level_for_color=1)
    frames = [(d, np_downscale_rgb(rgb, 1)) for d, rgb in s["frames"]]
    want = run(s["half_cam"], s["full_cam"], s["raw_to_float"], frames)
    assert_same(got, want)
    # Both runs share the tracker, so agreement alone would not notice a wrong colour pyramid: the trajectory must also follow
    # the rendered one.  The bounds are those tests/test_gpu_bad_slam.py sets for this sequence with both streams at 320x240;
    # here the depth stream has twice that resolution and the colour stream the same, so the run has no reason to do worse.
    gt7 = np.array([dba.pose7(T) for T in s["gt"]], np.float32)
    err_t = np.linalg.norm(got[0][:, 4:7] - gt7[:, 4:7], axis=1)
    stamps = lambda poses: {100.0 + 0.1 * i: poses[i, 4:7].astype(np.float64) for i in range(len(poses))}
    r = ate.ate(stamps(gt7), stamps(got[0]))
    print("mixed sizes: max translation error", float(err_t.max()), "ATE RMSE", r["rmse"])
    assert err_t.max() < 4e-3, err_t
    assert r["pairs"] == N_FRAMES and r["rmse"] < 2e-3, r["rmse"]


def test_frames_of_the_wrong_size_are_refused_by_the_binding(sequence):
    """ProcessFrame reads (height << level) x (width << level) host elements: camera-sized frames at level 1 must not get through."""
    s = sequence
    slam = bad_slam.BadSlam(s["half_cam"], s["half_cam"], pyramid_level_for_depth=1, pyramid_level_for_color=1, **SETTINGS)
    depth, rgb = s["frames"][0]
    with pytest.raises(ValueError):
        slam.ProcessFrame(0, np_downscale_depth_median(depth, 1), rgb)
    with pytest.raises(ValueError):
        slam.ProcessFrame(0, depth, np_downscale_rgb(rgb, 1))
    with pytest.raises(ValueError):
        slam.PreprocessFrame(depth[:-1], rgb)
    slam.ProcessFrame(0, depth, rgb)
    slam.close()


def test_rejected_configurations(sequence):
    s = sequence
    with pytest.raises(dba.DirectBAError):                                      # as in the reference (BS/bad_slam.cc:667-669)
        bad_slam.BadSlam(s["half_cam"], s["half_cam"], median_filter_and_densify_iterations=2, pyramid_level_for_depth=1, **SETTINGS)
    with pytest.raises(dba.DirectBAError):
        bad_slam.BadSlam(s["half_cam"], s["half_cam"], pyramid_level_for_depth=4, **SETTINGS)
    with pytest.raises(dba.DirectBAError):
        bad_slam.BadSlam(s["half_cam"], s["half_cam"], pyramid_level_for_color=4, **SETTINGS)
