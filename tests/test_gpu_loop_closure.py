"""-m gpu: loop closure (BS/loop_detector.cc:440-712 after the RANSAC step): the batched image-pair accumulation and the
lockstep tracking it verifies with are bit-identical to their single-pair forms, and a rendered closed path with injected
drift is closed by CloseLoop (verification, averaging, the pixel-distance test, the keyframe pose graph)."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi, bad_slam
from badslam_amd import direct_ba as dba
from tests import bso, scenes

pytestmark = pytest.mark.gpu
P = C.POINTER
W, H = 320, 240
RAW_TO_FLOAT = float(np.float32(1.0 / 5000))


def circle_path(n, radius=0.12):
    """Closed camera path: a circle in the image plane with a small rotation wobble; keyframe n would equal keyframe 0."""
    poses = []
    for k in range(n):
        a = 2 * np.pi * k / n
        xi = np.array([radius * np.sin(a), radius * (1 - np.cos(a)), 0.03 * np.sin(a), 0.02 * np.sin(a), 0.03 * (1 - np.cos(a)), 0.01 * np.sin(2 * a)],
                      np.float32)
        poses.append(bso.se3_exp(xi))
    return poses


def render(poses, seed=5):
    rng = np.random.default_rng(seed)
    cam = bso.make_camera(262.5, 262.5, 160.0, 120.0, W, H)
    planes = scenes.random_planes(rng, 20)
    frames = []
    for T in poses:
        M = np.array(list(bso.se3_matrix3x4(T).m), np.float64).reshape(3, 4)
        tt, pidx, dg, o = scenes.render_planes(cam, W, H, M[:, :3], M[:, 3], planes)
        valid = np.isfinite(tt) & (tt < 6.0)
        depth = np.where(valid, tt / RAW_TO_FLOAT + 0.5, 0).astype(np.uint32)
        depth = np.where(depth >= 32768, 0, depth).astype(np.uint16)
        pts = o[None, None, :] + dg * np.where(valid, tt, 0.0)[..., None]
        lum = scenes.texture_at(pts, pidx, 0.37)
        frames.append((depth, np.ascontiguousarray(np.repeat(lum[:, :, None], 3, axis=2))))
    return cam, frames


def make_ba(cam, frames, poses, use_depth=True, use_desc=True):
    ba = dba.DirectBA(200000, RAW_TO_FLOAT, 40.0, 4, 0.8, 1, 1, 1, cam, cam, 0, use_depth, use_desc)
    for k, ((depth, rgb), T) in enumerate(zip(frames, poses)):
        ba.AddKeyframeFromImages(k, depth, rgb, T)
    return ba


def drifted(poses, end=(0.03, -0.02, 0.025, 0.02, -0.015, 0.012)):
    """Drift that grows along the path: keyframe k is moved by (k / (n-1)) * end (keyframe 0 untouched)."""
    n = len(poses)
    return [poses[0]] + [bso.se3_mul(T, bso.se3_exp((np.array(end, np.float32) * (k / (n - 1))).astype(np.float32))) for k, T in enumerate(poses) if k]


def p7(T):
    return bso.se3_to_np(T)


def rel_err(A, B):
    d = bso.se3_log(bso.se3_mul(bso.se3_inverse(A), B))
    return float(np.linalg.norm(d[:3])), float(np.degrees(np.linalg.norm(d[3:])))


def keyframe_rmse(ba, truth, ids):
    return float(np.sqrt(np.mean([np.sum((p7(ba.keyframe_pose(i))[4:] - p7(truth[i])[4:]) ** 2) for i in ids])))


N_KF = 12
_cache = {}


def loop_scene():
    if "scene" not in _cache:
        gt = circle_path(N_KF)
        cam, frames = render(gt)
        _cache["scene"] = (gt, cam, frames)
    return _cache["scene"]


def perturbed_old_T_cur(gt, cur, old):
    truth = bso.se3_mul(bso.se3_inverse(gt[old]), gt[cur])
    return bso.se3_mul(truth, bso.se3_exp(np.array([0.004, -0.003, 0.003, 0.003, -0.002, 0.002], np.float32)))


# ---- batched accumulation: bit-identical rows -----------------------------------------------------------------
def _buf(t):
    return abi.Buffer2D(t.data_ptr(), t.shape[0], t.shape[1], t.stride(0) * t.element_size())


@pytest.mark.parametrize("use_depth,use_desc", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("pair_count", [1, 3, 5])
def test_batched_accumulation_rows_are_bit_identical(use_depth, use_desc, pair_count):
    import torch
    gt, cam, frames = loop_scene()
    ba = make_ba(cam, frames[:6], gt[:6], use_depth, use_desc)
    L = badslam_amd.lib()
    ctx = ba.context_handle()
    stream = C.c_void_p(None)
    imgs = []
    for k in range(6):
        d16, n16, _, col, _, _ = ba.keyframe_images(k, H, W)
        valid = (d16 != 0) & ((d16 & 0x8000) == 0)
        d = torch.from_numpy(np.where(valid, d16.astype(np.float32) * np.float32(RAW_TO_FLOAT), 0).astype(np.float32)).cuda()
        n = torch.from_numpy(n16.view(np.int16).copy()).cuda()
        c = torch.from_numpy(np.ascontiguousarray(col[:, :, 0])).cuda()
        imgs.append((d, n, c))
    torch.cuda.synchronize()
    base = imgs[0]
    tracked = [imgs[1 + (p % 5)] for p in range(pair_count)]
    Ms = []
    for p in range(pair_count):
        T = bso.se3_mul(bso.se3_inverse(gt[0]), gt[1 + (p % 5)])
        T = bso.se3_mul(T, bso.se3_exp(np.array([0.002 * p, -0.001, 0.001 * p, 0.0005, -0.0003 * p, 0.0002], np.float32)))
        if p == pair_count - 1 and pair_count > 1:
            T = bso.se3_exp(np.array([0, 0, 50.0, 0, 0, 0], np.float32))       # the base scene lies behind this tracked camera: nothing visible
        Ms.append(bso.se3_matrix3x4(bso.se3_inverse(T)))
    tcc = tdc = cam
    BufArr = abi.Buffer2D * pair_count
    td = BufArr(*[_buf(t[0]) for t in tracked])
    tn = BufArr(*[_buf(t[1]) for t in tracked])
    tc = BufArr(*[_buf(t[2]) for t in tracked])
    Marr = (abi.Mat3x4 * pair_count)(*Ms)
    bd, bn, bc = _buf(base[0]), _buf(base[1]), _buf(base[2])
    Hb, bb, vb = np.zeros(21 * pair_count, np.float32), np.zeros(6 * pair_count, np.float32), np.zeros(pair_count, np.uint32)
    for threshold in (1.0, 4.0):
        badslam_amd.check(L.bslam_accumulate_pose_coeffs_from_images_batched(
            ctx, stream, int(use_depth), int(use_desc), C.byref(tcc), C.byref(tdc), 40.0, threshold, pair_count, td, tn, tc, Marr,
            C.byref(bd), C.byref(bn), C.byref(bc), vb.ctypes.data_as(P(C.c_uint32)), Hb.ctypes.data_as(P(C.c_float)), bb.ctypes.data_as(P(C.c_float))))
        for p in range(pair_count):
            Hs, bs, vs = np.zeros(21, np.float32), np.zeros(6, np.float32), C.c_uint32()
            a1, a2, a3 = _buf(tracked[p][0]), _buf(tracked[p][1]), _buf(tracked[p][2])
            badslam_amd.check(L.bslam_accumulate_pose_coeffs_from_images(
                ctx, stream, int(use_depth), int(use_desc), C.byref(tcc), C.byref(tdc), 40.0, threshold, C.byref(a1), C.byref(a2), C.byref(a3),
                C.byref(Ms[p]), C.byref(bd), C.byref(bn), C.byref(bc), C.byref(vs), Hs.ctypes.data_as(P(C.c_float)), bs.ctypes.data_as(P(C.c_float))))
            assert np.array_equal(Hb[21 * p:21 * p + 21].view(np.uint32), Hs.view(np.uint32)), (p, threshold)
            assert np.array_equal(bb[6 * p:6 * p + 6].view(np.uint32), bs.view(np.uint32)), (p, threshold)
            assert vb[p] == vs.value, (p, vb[p], vs.value)
            if p == pair_count - 1 and pair_count > 1:
                assert vs.value == 0
            else:
                assert vs.value > 1000
    # argument checks
    for bad in (0, 9):
        assert L.bslam_accumulate_pose_coeffs_from_images_batched(
            ctx, stream, 1, 1, C.byref(tcc), C.byref(tdc), 40.0, 1.0, bad, td, tn, tc, Marr, C.byref(bd), C.byref(bn), C.byref(bc), None,
            Hb.ctypes.data_as(P(C.c_float)), bb.ctypes.data_as(P(C.c_float))) == -1
    ba.close()


def test_batched_tracking_is_bit_identical_to_single_pair_tracking():
    gt, cam, frames = loop_scene()
    ba = make_ba(cam, frames[:5], gt[:5])
    inits = [bso.se3_mul(bso.se3_mul(bso.se3_inverse(gt[0]), gt[k]), bso.se3_exp(np.array([0.003, -0.002, 0.002, 0.002, 0.001, -0.001], np.float32)))
             for k in (1, 2, 4)]
    poses, its = ba.TrackKeyframesBatched(0, [1, 2, 4], inits, num_scales=5)
    for (k, init), pose, it in zip(zip((1, 2, 4), inits), poses, its):
        ref, ref_its = ba.TrackKeyframePair(k, 0, init, num_scales=5)
        assert np.array_equal(p7(pose).view(np.uint32), p7(ref).view(np.uint32)), (k, p7(pose), p7(ref))
        assert list(it) == list(ref_its), (k, it, ref_its)
        t_err, r_err = rel_err(pose, bso.se3_mul(bso.se3_inverse(gt[0]), gt[k]))
        assert t_err < 2e-3 and r_err < 0.1, (k, t_err, r_err)
    ba.close()


# ---- CloseLoop ------------------------------------------------------------------------------------------------
def test_close_loop_on_a_drifted_closed_path():
    gt, cam, frames = loop_scene()
    drift = drifted(gt)
    ba = make_ba(cam, frames, drift)
    last = N_KF - 1
    kf0_before = p7(ba.keyframe_pose(0)).copy()
    rmse_before = keyframe_rmse(ba, gt, range(N_KF))
    res = ba.CloseLoop(last, 0, perturbed_old_T_cur(gt, last, 0), num_scales=5)
    print("close loop:", res["status"], "pixel distance", res["mean_pixel_distance"], "points", res["pixel_count"], "chi2", res["chi2"][:1], res["chi2"][-1:],
          "iterations", res["tracking_iterations"])
    assert res["status"] == "closed", res
    assert res["old_keyframe_ids"] == [0, 1, 2]
    assert res["pixel_count"] >= 5 and res["mean_pixel_distance"] > 1.0
    assert len(res["chi2"]) == 20 and res["chi2"][-1] <= res["chi2"][0]
    assert np.array_equal(p7(ba.keyframe_pose(0)), kf0_before), "the gauge keyframe must not move"
    rmse_after = keyframe_rmse(ba, gt, range(N_KF))
    t_err, r_err = rel_err(bso.se3_mul(bso.se3_inverse(ba.keyframe_pose(last)), ba.keyframe_pose(0)), bso.se3_mul(bso.se3_inverse(gt[last]), gt[0]))
    print(f"keyframe position RMSE {rmse_before * 1e3:.2f} mm -> {rmse_after * 1e3:.2f} mm; last-to-first error {t_err * 1e3:.2f} mm, {r_err:.3f} deg")
    assert rmse_after * 3 <= rmse_before, (rmse_before, rmse_after)
    assert t_err < 1e-2 and r_err < 0.5, (t_err, r_err)     # the loop edge is one of 12 equally weighted edges around the cycle
    ba.close()


def test_close_loop_without_drift_is_ignored_and_changes_nothing():
    gt, cam, frames = loop_scene()
    ba = make_ba(cam, frames, gt)
    before = [p7(ba.keyframe_pose(k)).copy() for k in range(N_KF)]
    res = ba.CloseLoop(N_KF - 1, 0, perturbed_old_T_cur(gt, N_KF - 1, 0), num_scales=5)
    print("no drift:", res["status"], res["mean_pixel_distance"], res["pixel_count"])
    assert res["status"] == "ignored_small", res
    assert res["pixel_count"] >= 5 and res["mean_pixel_distance"] <= 1.0
    for k in range(N_KF):
        assert np.array_equal(p7(ba.keyframe_pose(k)), before[k]), k
    ba.close()


def test_close_loop_with_two_keyframes_is_rejected():
    gt, cam, frames = loop_scene()
    ba = make_ba(cam, [frames[0], frames[-1]], [gt[0], gt[-1]])
    res = ba.CloseLoop(1, 0, perturbed_old_T_cur(gt, N_KF - 1, 0), num_scales=5)
    assert res["status"] == "rejected_no_neighbours", res
    ba.close()


def test_close_loop_with_an_inconsistent_neighbour_is_rejected():
    gt, cam, frames = loop_scene()
    poses = list(gt)
    poses[1] = bso.se3_mul(gt[1], bso.se3_exp(np.array([0.05, 0, 0, 0, 0, 0], np.float32)))   # the next keyframe's stored pose 5 cm off
    ba = make_ba(cam, frames, poses)
    before = [p7(ba.keyframe_pose(k)).copy() for k in range(N_KF)]
    res = ba.CloseLoop(N_KF - 1, 0, perturbed_old_T_cur(gt, N_KF - 1, 0), num_scales=5)
    assert res["status"] == "rejected_inconsistent", res
    for k in range(N_KF):
        assert np.array_equal(p7(ba.keyframe_pose(k)), before[k]), k
    ba.close()


# ---- BadSlam ----------------------------------------------------------------------------------------------------
def _run_slam(frames, search, close_at_end=None):
    cam = bso.make_camera(262.5, 262.5, 160.0, 120.0, W, H)
    slam = bad_slam.BadSlam(cam, cam, keyframe_interval=2, max_num_ba_iterations_per_keyframe=2, num_scales=4, max_surfel_count=400000,
                            raw_to_float_depth=RAW_TO_FLOAT, max_depth=6.0, baseline_fx=40.0)
    if search:
        slam.set_loop_candidate_search(True, 4)
    for k, (depth, rgb) in enumerate(frames):
        slam.ProcessFrame(k, depth, rgb)
    return slam


def test_bad_slam_candidate_search_and_close_loop():
    n = 20
    gt = circle_path(n)
    _, frames = render(gt)
    off = _run_slam(frames, False)
    on = _run_slam(frames, True)
    log = on.loop_closure_log()
    print("candidate log:", log)
    assert off.loop_closure_log() == []
    kf_ids = [e["keyframe"] for e in log]
    assert kf_ids == sorted(kf_ids) and all(e["keyframe"] - e["candidate"] >= 4 for e in log)
    assert log and log[-1]["candidate"] in (0, 1), log          # the last keyframe (frame 18) is next to the start of the circle
    if all(e["status"] == "ignored_small" for e in log):
        assert np.array_equal(on.frame_poses(), off.frame_poses())
    # CloseLoop of the newest keyframe moves the non-keyframe frames with their keyframes
    ba = off.ba()
    last = ba.keyframe_count() - 1
    before_frames = off.frame_poses().copy()
    ba.set_keyframe_pose(last, bso.se3_mul(ba.keyframe_pose(last), bso.se3_exp(np.array([0.03, 0.02, -0.02, 0.01, 0.015, -0.01], np.float32))))
    moved_kf = ba.keyframe_pose(last)
    res = off.CloseLoop(0, bso.se3_mul(bso.se3_inverse(gt[0]), gt[2 * last]))
    print("BadSlam.CloseLoop:", res["status"], res["mean_pixel_distance"])
    assert res["status"] == "closed", res
    after_frames = off.frame_poses()
    kf_after = ba.keyframe_pose(last)
    # frame 2 * last is the keyframe's frame; frame 2 * last + 1 comes after it and follows the keyframe's change
    delta_kf = bso.se3_mul(kf_after, bso.se3_inverse(moved_kf))
    expected = bso.se3_mul(delta_kf, dba.se3f_from7(before_frames[2 * last + 1]))
    assert np.abs(after_frames[2 * last + 1] - p7(expected)).max() < 1e-4
    assert not np.array_equal(after_frames, before_frames)
