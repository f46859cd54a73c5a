"""-m gpu: place recognition.  bslam_extract_keyframe_features and bslam_match_features bit for bit against the NumPy
restatement (tests/place_util.py), then DirectBA.RecognizePlace on a leave-and-return path whose poses drifted far outside
the tracker's basin, and BadSlam with place recognition on."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi, bad_slam
from badslam_amd import direct_ba as dba
from tests import bso, place_util as pu

pytestmark = pytest.mark.gpu
INVALID = -1   # BSLAM_ERR_INVALID_ARGUMENT


def _ctx():
    return badslam_amd.Context()


def _ptr(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


class DeviceImages:
    """A colour (uchar4, intensity in byte 3) and a depth (u16) image on the device with padded pitches."""

    def __init__(self, L, depth, color_pad=64, depth_pad=6):
        import torch
        h, w = L.shape
        color = np.zeros((h, w * 4 + color_pad), np.uint8)
        rgba = np.zeros((h, w, 4), np.uint8)
        rgba[:, :, 0], rgba[:, :, 1], rgba[:, :, 2], rgba[:, :, 3] = 7, 9, 11, L   # only byte 3 may matter
        color[:, :w * 4] = rgba.reshape(h, w * 4)
        color[:, w * 4:] = 0xA5
        dep = np.full((h, w * 2 + depth_pad), 0xFF, np.uint8)
        dep[:, :w * 2] = np.ascontiguousarray(depth, np.uint16).view(np.uint8).reshape(h, w * 2)
        self.color_t, self.depth_t = torch.from_numpy(color).cuda(), torch.from_numpy(dep).cuda()
        self.color = abi.Buffer2D(self.color_t.data_ptr(), h, w, color.shape[1])
        self.depth = abi.Buffer2D(self.depth_t.data_ptr(), h, w, dep.shape[1])
        self.cells = (h // 16) * (w // 16)


def gpu_extract(ctx, images, score_threshold):
    import torch
    L = badslam_amd.lib()
    xy = torch.full((images.cells,), 0x12345678, dtype=torch.int32, device="cuda")
    desc = torch.full((images.cells, 8), 0x12345678, dtype=torch.int32, device="cuda")
    badslam_amd.check(L.bslam_extract_keyframe_features(ctx.handle, None, C.byref(images.color), C.byref(images.depth), score_threshold, _ptr(xy), _ptr(desc)))
    torch.cuda.synchronize()
    return xy.cpu().numpy().view(np.uint32), desc.cpu().numpy().view(np.uint32)


def make_image(w, h, seed):
    """Intensity and depth with every case of the rule: random 4 x 4 blocks; a constant region (empty slots); a 0 / 255
    checker of 4-pixel squares (the extreme of the score); a texture of period 8 (equal scores inside a cell)."""
    rng = np.random.default_rng(seed)
    L = np.kron(rng.integers(0, 256, ((h + 3) // 4, (w + 3) // 4)), np.ones((4, 4), np.int64))[:h, :w].astype(np.uint8)
    L[12:52, 12:54] = 93                                                   # constant with a halo of 3: cells (1, 1) and (1, 2) see no gradient
    ys, xs = np.mgrid[0:h, 0:w]
    checker = (((ys // 4) + (xs // 4)) % 2 * 255).astype(np.uint8)
    L[:, 58:w - 8][16:60] = checker[:, 58:w - 8][16:60]
    period = rng.integers(0, 256, (8, 8)).astype(np.uint8)
    L[h - 44:h - 4, 4:64] = np.tile(period, (6, 9))[:40, :60]              # covers cell rows h/16 - 2 with a halo of >= 3 pixels
    depth = rng.integers(500, 30000, (h, w)).astype(np.uint16)
    return L, depth


@pytest.mark.parametrize("w,h", [(112, 80), (200, 136)])
def test_extraction_equals_the_restatement(w, h):
    L, depth = make_image(w, h, seed=w)
    threshold = 10 ** 9
    # depth holes of both kinds over would-be winners: the restatement's winners with the full depth lose their pixel
    xy_full, _ = pu.extract(L, depth, threshold)
    winners = np.flatnonzero(xy_full != pu.EMPTY)
    assert len(winners) >= 6
    for n, c in enumerate(winners[::2]):
        x, y = int(xy_full[c] & 0xFFFF), int(xy_full[c] >> 16)
        depth[y, x] = 0 if n % 2 == 0 else (0x8000 | 1234)
    ref_xy, ref_desc = pu.extract(L, depth, threshold)
    changed = int((ref_xy != xy_full).sum())
    # the cases are present
    cells_x = w // 16
    score = pu.corner_score(L)
    assert changed >= 3, "the holes must move winners"
    assert (ref_xy[[cells_x + 1, cells_x + 2]] == pu.EMPTY).all(), "the constant region must leave interior slots empty"
    assert score[16:60, 58:w - 8].max() > 10 ** 14, "the checker must reach the top of the score's range"
    tie_cell = (h // 16 - 2) * cells_x + 1
    cy0, cx0 = (tie_cell // cells_x) * 16, (tie_cell % cells_x) * 16
    cell_scores = score[cy0:cy0 + 16, cx0:cx0 + 16]
    assert (cell_scores == cell_scores.max()).sum() >= 2 and cell_scores.max() > threshold, "the periodic texture must tie inside a cell"
    ctx = _ctx()
    images = DeviceImages(L, depth)
    xy, desc = gpu_extract(ctx, images, threshold)
    assert np.array_equal(xy, ref_xy), np.flatnonzero(xy != ref_xy)
    assert np.array_equal(desc, ref_desc), np.flatnonzero((desc != ref_desc).any(axis=1))
    assert (desc[ref_xy == pu.EMPTY] == 0).all()
    xy2, desc2 = gpu_extract(ctx, images, threshold)
    assert np.array_equal(xy, xy2) and np.array_equal(desc, desc2)
    # a threshold nothing exceeds empties every slot; a negative one is legal
    xy3, desc3 = gpu_extract(ctx, images, 2 ** 62)
    assert (xy3 == pu.EMPTY).all() and (desc3 == 0).all()
    ref4 = pu.extract(L, depth, -(2 ** 62))
    xy4, desc4 = gpu_extract(ctx, images, -(2 ** 62))
    assert np.array_equal(xy4, ref4[0]) and np.array_equal(desc4, ref4[1])
    ctx.close()


def test_extraction_rejects_bad_arguments():
    import torch
    L, depth = make_image(112, 80, seed=1)
    ctx = _ctx()
    lib = badslam_amd.lib()
    im = DeviceImages(L, depth)
    xy = torch.zeros(im.cells + 4, dtype=torch.int32, device="cuda")
    desc = torch.zeros((im.cells + 4) * 8, dtype=torch.int32, device="cuda")
    call = lambda ctx_, col, dep, oxy, odesc: lib.bslam_extract_keyframe_features(ctx_, None, col, dep, 0, oxy, odesc)
    good = (ctx.handle, C.byref(im.color), C.byref(im.depth), _ptr(xy), _ptr(desc))
    assert call(*good) == 0
    assert call(None, *good[1:]) == INVALID
    assert call(good[0], None, *good[2:]) == INVALID
    assert call(*good[:2], None, *good[3:]) == INVALID
    assert call(*good[:3], None, good[4]) == INVALID
    assert call(*good[:4], None) == INVALID
    def buf(b, **kw):
        c = abi.Buffer2D(b.address, b.height, b.width, b.pitch)
        for k, v in kw.items():
            setattr(c, k, v)
        return C.byref(c)
    assert call(good[0], buf(im.color, address=None), *good[2:]) == INVALID
    assert call(good[0], buf(im.color, width=im.color.width - 16), *good[2:]) == INVALID          # sizes differ
    assert call(*good[:2], buf(im.depth, height=im.depth.height - 16), *good[3:]) == INVALID
    assert call(good[0], buf(im.color, pitch=im.color.pitch - 2), *good[2:]) == INVALID          # colour rows not 4 byte aligned
    assert call(good[0], buf(im.color, pitch=im.color.width * 4 - 4), *good[2:]) == INVALID      # pitch too small
    assert call(good[0], buf(im.color, address=im.color.address + 2), *good[2:]) == INVALID
    assert call(*good[:2], buf(im.depth, pitch=im.depth.pitch - 1), *good[3:]) == INVALID        # depth rows not 2 byte aligned
    assert call(*good[:3], _ptr(xy, 2), good[4]) == INVALID                                       # outputs not 4 byte aligned
    assert call(*good[:4], _ptr(desc, 1)) == INVALID
    assert call(*good[:3], _ptr(desc, 4 * 8), good[4]) == INVALID                                 # out_xy inside out_desc
    assert call(*good[:3], C.c_void_p(im.color.address + 64), good[4]) == INVALID                 # an output inside an input image
    assert call(*good[:4], C.c_void_p(im.depth.address)) == INVALID
    assert b"overlap" in lib.bslam_last_error()
    torch.cuda.synchronize()
    ctx.close()


# ---- matching on synthetic records --------------------------------------------------------------------------------
MAX_DISTANCE = 64
N_DB = 70


def flipped(rng, desc, count):
    out = desc.copy()
    for b in rng.permutation(256)[:count]:
        out[b // 32] ^= np.uint32(1 << (b % 32))
    return out


_records = {}


def synthetic_records(cells):
    """Query and 70 database keyframes of random descriptors with the cases of the rule planted in database keyframe 0,
    and the restatement's answer; built once per `cells`."""
    if cells in _records:
        return _records[cells]
    rng = np.random.default_rng(cells)
    rand = lambda *shape: rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)
    q_desc = rand(cells, 8)
    q_xy = rng.integers(0, 2 ** 31, cells).astype(np.uint32)
    db_desc = rand(N_DB, cells, 8)
    db_xy = rng.integers(0, 2 ** 31, (N_DB, cells)).astype(np.uint32)
    db_xy[rng.random((N_DB, cells)) < 0.2] = pu.EMPTY                      # empty database slots (their descriptors stay: they must be ignored)
    q_xy[20:24] = pu.EMPTY                                                  # empty query slots
    db_xy[1] = pu.EMPTY                                                     # a keyframe without features
    db_xy[2, :] = pu.EMPTY
    db_xy[2, cells - 1] = 5                                                 # a keyframe with a single feature: second = 257
    db_desc[2, cells - 1] = flipped(rng, q_desc[6], 60)
    plant = {3: (0, 5), 7: (0, 5),        # a duplicate of the best descriptor: second == best, rejected
             4: (1, 6), 9: (1, 6),        # equal best distances at two slots (different descriptors)
             11: (2, MAX_DISTANCE),       # exactly max_distance: accepted
             12: (3, MAX_DISTANCE + 1),   # one more: rejected
             14: (4, 30), 15: (4, 40),    # 4 best == 3 second: rejected
             17: (5, 30), 18: (5, 41)}    # 4 best < 3 second: accepted
    for slot, (q, d) in plant.items():
        db_desc[0, slot] = flipped(rng, q_desc[q], d)
        db_xy[0, slot] = slot
    db_desc[0, 7] = db_desc[0, 3]
    q_xy[:7] = np.arange(7)
    match, count = pu.match(q_xy, q_desc, db_xy, db_desc, MAX_DISTANCE)
    # the planted cases do what they were planted for
    assert match[0, 0] == -1 and match[0, 1] == -1 and match[0, 2] == 11 and match[0, 3] == -1 and match[0, 4] == -1 and match[0, 5] == 17
    assert (match[1] == -1).all() and count[1] == 0 and match[2, 6] == cells - 1 and (match[:, 20:24] == -1).all()
    _records[cells] = (q_xy, q_desc, db_xy, db_desc, match, count)
    return _records[cells]


@pytest.mark.parametrize("n_db", [0, 1, 5, N_DB])
@pytest.mark.parametrize("cells", [35, 1200])
def test_matching_equals_the_restatement(cells, n_db):
    import torch
    q_xy, q_desc, db_xy, db_desc, ref_match, ref_count = synthetic_records(cells)
    ctx = _ctx()
    lib = badslam_amd.lib()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()
    database = np.concatenate([np.concatenate([db_xy[k], db_desc[k].reshape(-1)]) for k in range(N_DB)])   # per keyframe: xy[cells], desc[cells][8]
    d_qxy, d_qdesc, d_db = dev(q_xy), dev(q_desc), dev(database)
    d_match = torch.full((max(n_db, 1), cells), 77, dtype=torch.int32, device="cuda")
    d_count = torch.full((max(n_db, 1),), 77, dtype=torch.int32, device="cuda")
    for _ in range(2):   # the second call must not add to the first one's counts
        rc = lib.bslam_match_features(ctx.handle, None, _ptr(d_qxy), _ptr(d_qdesc), cells, _ptr(d_db) if n_db else None, n_db, MAX_DISTANCE,
                                      _ptr(d_match) if n_db else None, _ptr(d_count) if n_db else None)
        badslam_amd.check(rc)
        torch.cuda.synchronize()
        match, count = d_match.cpu().numpy(), d_count.cpu().numpy().view(np.uint32)
        if n_db == 0:
            assert (match == 77).all() and (count == 77).all()   # nothing was launched
            continue
        assert np.array_equal(match, ref_match[:n_db]), np.argwhere(match != ref_match[:n_db])[:10]
        assert np.array_equal(count, ref_count[:n_db])
    ctx.close()


def test_matching_rejects_bad_arguments():
    import torch
    cells = 35
    q_xy, q_desc, db_xy, db_desc, _, _ = synthetic_records(cells)
    ctx = _ctx()
    lib = badslam_amd.lib()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()
    d_qxy, d_qdesc = dev(q_xy), dev(q_desc)
    d_db = dev(np.concatenate([np.concatenate([db_xy[k], db_desc[k].reshape(-1)]) for k in range(2)]))
    d_match = torch.zeros(2 * cells + 8, dtype=torch.int32, device="cuda")
    d_count = torch.zeros(8, dtype=torch.int32, device="cuda")
    def call(ctx_=ctx.handle, qxy=_ptr(d_qxy), qdesc=_ptr(d_qdesc), cells_=cells, db=_ptr(d_db), n_db=2, max_distance=MAX_DISTANCE, match=_ptr(d_match),
             count=_ptr(d_count)):
        return lib.bslam_match_features(ctx_, None, qxy, qdesc, cells_, db, n_db, max_distance, match, count)
    assert call() == 0
    for bad in (dict(ctx_=None), dict(qxy=None), dict(qdesc=None), dict(db=None), dict(match=None), dict(count=None), dict(cells_=0), dict(cells_=-3),
                dict(n_db=-1), dict(n_db=65536), dict(max_distance=-1), dict(max_distance=257), dict(qxy=_ptr(d_qxy, 2)), dict(qdesc=_ptr(d_qdesc, 1)),
                dict(db=_ptr(d_db, 2)), dict(match=_ptr(d_match, 3)), dict(count=_ptr(d_count, 2)),
                dict(match=_ptr(d_db, 16)), dict(count=_ptr(d_qdesc, 8)), dict(count=_ptr(d_qxy)), dict(count=_ptr(d_match, 4 * cells))):
        assert call(**bad) == INVALID, bad
    assert call(max_distance=0) == 0 and call(max_distance=256) == 0
    assert call(n_db=0, db=None, match=None, count=None) == 0
    torch.cuda.synchronize()
    ctx.close()


# ---- through DirectBA ---------------------------------------------------------------------------------------------
# old_T_cur of the host RANSAC against the restatement's: the two differ in the eigen-solver of Horn's 4 x 4 matrix (cyclic
# Jacobi vs LAPACK) and in summation order.  Measured on the nine returning / home pairs of the scene: at most 1.2e-16 in
# any of the seven entries (magnitude <= 1, double epsilon 2.2e-16).  Ten times that:
POSE_TOLERANCE = 10 * 1.2e-16


def make_ba(cam, frames, poses):
    ba = dba.DirectBA(200000, pu.RAW_TO_FLOAT, 40.0, 4, 0.8, 1, 1, 1, cam, cam, 0, True, True)
    for k, ((depth, rgb), T) in enumerate(zip(frames, poses)):
        ba.AddKeyframeFromImages(k, depth, rgb, T)
    return ba


def p7(T):
    return bso.se3_to_np(T)


def test_recognize_place_through_direct_ba():
    gt, cam, frames = pu.path_scene()
    poses = pu.drifted_poses(gt)
    end_t, end_r = pu.pose_difference(p7(poses[-1]), p7(gt[-1]))
    print(f"drift of the last keyframe: {end_t * 100:.1f} cm, {end_r:.1f} deg")
    assert end_t > 0.15 and end_r > 6.0
    ba = make_ba(cam, frames, poses)
    n = len(gt)
    # features of the keyframe images as the device holds them
    images, ref = [], []
    for k in range(n):
        depth, _, _, color, _, _ = ba.keyframe_images(k, pu.H, pu.W)
        images.append(depth)
        ref.append(pu.extract(np.ascontiguousarray(color[:, :, 3]), depth))
        xy, desc = ba.ExtractKeyframeFeatures(k)
        assert np.array_equal(xy, ref[k][0]) and np.array_equal(desc, ref[k][1]), k
        assert (xy != pu.EMPTY).sum() >= 200
    ids = [0, 1, 2, 3]
    ref_match, ref_count = pu.match(ref[9][0], ref[9][1], np.stack([ref[k][0] for k in ids]), np.stack([ref[k][1] for k in ids]))
    match, count = ba.MatchKeyframeFeatures(9, ids)
    assert np.array_equal(match, ref_match) and np.array_equal(count, ref_count)
    match, count = ba.MatchKeyframeFeatures(9, [2, 0])
    assert np.array_equal(match, ref_match[[2, 0]]) and np.array_equal(count, ref_count[[2, 0]])

    # a turned-away keyframe: no candidate, nothing changes
    before = [p7(ba.keyframe_pose(k)).copy() for k in range(n)]
    away = ba.RecognizePlace(6, min_keyframe_gap=4)
    _, away_count = pu.match(ref[6][0], ref[6][1], np.stack([ref[k][0] for k in (0, 1, 2)]), np.stack([ref[k][1] for k in (0, 1, 2)]))
    print("turned away:", away, "restatement counts", away_count.tolist())
    assert pu.query(away_count, [True] * 3) == -1
    assert away["candidate"] == -1 and away["match_count"] == 0 and not away["pose_found"] and not away["loop_attempted"] and away["loop"] is None
    assert all(np.array_equal(p7(ba.keyframe_pose(k)), before[k]) for k in range(n))

    # the last keyframe: a home keyframe, the restatement's counts and start pose, and a closed loop
    candidate = pu.query(ref_count, [True] * 4)
    pc, po = pu.matched_points(ref[9][0], images[9], ref[candidate][0], images[candidate], ref_match[candidate], cam)
    ref_pose = pu.ransac(9, candidate, pc, po)
    res = ba.RecognizePlace(9, min_keyframe_gap=6)
    difference = float(np.abs(res["old_T_cur"] - ref_pose["old_T_cur"]).max())
    truth = p7(bso.se3_mul(bso.se3_inverse(gt[candidate]), gt[9])).astype(np.float64)
    print("returned:", {k: v for k, v in res.items() if k != "loop"}, "restatement:", candidate, int(ref_count[candidate]), ref_pose["inlier_count"],
          "pose difference", difference, "error against the truth", pu.pose_difference(res["old_T_cur"], truth))
    print("loop:", res["loop"]["status"], res["loop"]["mean_pixel_distance"], res["loop"]["old_keyframe_ids"])
    assert candidate in pu.HOME and res["candidate"] == candidate
    assert res["match_count"] == int(ref_count[candidate])
    assert ref_pose["found"] and res["pose_found"] and res["inlier_count"] == ref_pose["inlier_count"]
    assert difference <= POSE_TOLERANCE, difference
    assert res["loop_attempted"] and res["loop"]["status"] == "closed", res["loop"]
    assert np.array_equal(p7(ba.keyframe_pose(0)), before[0]), "the gauge keyframe must not move"
    t_err, r_err = pu.pose_difference(p7(bso.se3_mul(bso.se3_inverse(ba.keyframe_pose(candidate)), ba.keyframe_pose(9))).astype(np.float64), truth)
    print(f"after closing: last-to-home error {t_err * 1e3:.2f} mm, {r_err:.3f} deg")
    assert t_err < end_t / 3 and r_err < end_r / 3
    # a deleted keyframe is no candidate any more
    ba.DeleteKeyframe(candidate)
    again = ba.RecognizePlace(9, min_keyframe_gap=6)
    assert again["candidate"] not in (-1, candidate) and again["candidate"] == pu.query(ref_count, [k != candidate for k in range(4)])
    ba.close()


# ---- through BadSlam ----------------------------------------------------------------------------------------------
SLAM_FRAMES, SLAM_INTERVAL, SLAM_GAP = 49, 4, 6


def slam_path():
    """49 frames, a keyframe every fourth one: the camera turns away by 1 rad in 24 frames and comes back."""
    poses = []
    for k in range(SLAM_FRAMES):
        a = 1.0 - abs(k - 24) / 24.0          # 0 -> 1 -> 0
        poses.append(bso.se3_exp(np.array([0.25 * a, 0.02 * a, 0.03 * a, 0.02 * a, 1.0 * a, 0.0], np.float32)))
    return poses


def run_slam(frames, mode):
    cam = pu.camera()
    slam = bad_slam.BadSlam(cam, cam, keyframe_interval=SLAM_INTERVAL, max_num_ba_iterations_per_keyframe=2, num_scales=4, max_surfel_count=400000,
                            raw_to_float_depth=pu.RAW_TO_FLOAT, max_depth=6.0, baseline_fx=40.0)
    if mode in ("on", "off again"):
        slam.set_place_recognition(True, min_keyframe_gap=SLAM_GAP)
    if mode == "off again":
        slam.set_place_recognition(False)
    for k, (depth, rgb) in enumerate(frames):
        slam.ProcessFrame(k, depth, rgb)
    return slam


def test_bad_slam_place_recognition():
    gt = slam_path()
    _, frames = pu.render(gt)
    plain, on, off_again = run_slam(frames, "plain"), run_slam(frames, "on"), run_slam(frames, "off again")
    assert plain.place_recognition_log() == [] and off_again.place_recognition_log() == []
    assert np.array_equal(plain.frame_poses().view(np.uint32), off_again.frame_poses().view(np.uint32))
    assert np.array_equal(plain.ba().GetSurfels().view(np.uint32), off_again.ba().GetSurfels().view(np.uint32))
    log = on.place_recognition_log()
    for e in log:
        print({k: (v if k != "old_T_cur" else np.round(v, 4).tolist()) for k, v in e.items()})
    assert [e["keyframe"] for e in log] == list(range(13))
    assert all(e["candidate"] == -1 for e in log[:SLAM_GAP])                       # nothing old enough yet
    assert all(e["candidate"] <= e["keyframe"] - SLAM_GAP for e in log if e["candidate"] >= 0)
    assert log[6]["candidate"] == -1 and not log[6]["loop_attempted"]               # turned away by 1 rad: nothing in common with home
    last = log[-1]                                                                  # the last frame stands where frame 0 stood
    assert last["candidate"] in (0, 1) and last["match_count"] >= 25 and last["pose_found"] and last["inlier_count"] >= 10
    assert last["loop_attempted"] and last["status"] is not None
    truth = p7(bso.se3_mul(bso.se3_inverse(gt[SLAM_INTERVAL * last["candidate"]]), gt[SLAM_FRAMES - 1])).astype(np.float64)
    t_err, r_err = pu.pose_difference(last["old_T_cur"], truth)
    print(f"start pose of the last keyframe against the truth: {t_err * 1e3:.2f} mm, {r_err:.3f} deg")
    assert t_err < 0.02 and r_err < 1.0                                            # well inside the tracker's basin (centimetres, degrees)
    # the two searches exclude each other, in either order
    with pytest.raises(dba.DirectBAError):
        on.set_loop_candidate_search(True, 4)
    plain.set_loop_candidate_search(True, 4)
    with pytest.raises(dba.DirectBAError):
        plain.set_place_recognition(True)
    for s in (plain, on, off_again):
        s.close()
