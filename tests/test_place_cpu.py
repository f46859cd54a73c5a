"""Place recognition without a GPU: the point-pair table, the NumPy restatement (tests/place_util.py) on the
leave-and-return scene, and the host RANSAC of badslam_amd/host/place_recognition.cpp through the C API."""
import numpy as np
import pytest

import badslam_amd
from badslam_amd import build
from badslam_amd import direct_ba as dba
from tests import bso, place_util as pu


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()
    bso.build_oracle()


# ---- the point pairs ----------------------------------------------------------------------------------------------
def test_pattern_table():
    pairs = pu.pattern()
    assert pairs.shape == (256, 4)
    assert pairs.min() >= -13 and pairs.max() <= 13
    assert not np.any((pairs[:, 0] == pairs[:, 2]) & (pairs[:, 1] == pairs[:, 3]))
    # by hand from the rule: s1 = 0x0BAD51A4 * 1664525 + 1013904223 mod 2^32 = 0xDBC770B3; 0xDBC7 = 56263 = 27 * 2083 + 22 -> 22 - 13 = 9
    assert (0x0BAD51A4 * 1664525 + 1013904223) % 2 ** 32 == 0xDBC770B3 and pairs[0, 0] == 9
    assert pairs[:2].tolist() == [[9, -4, -5, -1], [1, 7, 8, -12]]
    weights = np.arange(1, 1025, dtype=np.int64).reshape(256, 4)
    assert int(((pairs + 13) * weights).sum()) == PATTERN_CHECKSUM
    # the library generates the same table (host code, no GPU)
    import ctypes as C
    native = np.zeros((256, 4), np.int8)
    assert badslam_amd.lib().bslam_place_pattern(native.ctypes.data_as(C.POINTER(C.c_int8))) == 0
    assert np.array_equal(native.astype(np.int64), pairs)


PATTERN_CHECKSUM = 6849071   # sum of (value + 13) * (1-based position in the flattened table), from a run of the rule


# ---- the restatement on the scene ---------------------------------------------------------------------------------
# Measured with this restatement on path_scene() (20 planes, 320 x 240, f = 262.5, blocky texture):
#   features per frame   231 ... 234 of the 234 cells that can hold one
#   returning vs home    128 ... 174 accepted matches;  turned away vs home  3 ... 20
#   RANSAC, returning    137 / 170 / 153 inliers, pose error 0.6 ... 1.8 mm and 0.02 ... 0.09 degrees
# The asserts sit at half the gap between the figure and what it must stay clear of.
def test_restatement_feature_count():
    counts = [int((xy != pu.EMPTY).sum()) for xy, _ in pu.path_features()]
    print("features per frame:", counts)
    possible = (pu.W // 16 - 2) * (pu.H // 16 - 2)
    assert possible == 234
    assert all(c <= possible for c in counts)
    assert min(counts) >= 231 - 231 // 2   # measured minimum 231; a scene without corners gives 0


def test_restatement_separates_returning_from_turned_away():
    feats = pu.path_features()
    home_xy, home_desc = np.stack([feats[k][0] for k in pu.HOME]), np.stack([feats[k][1] for k in pu.HOME])
    min_matches = pu.DEFAULTS["min_matches"]
    back = [pu.match(feats[q][0], feats[q][1], home_xy, home_desc)[1] for q in pu.BACK]
    away = [pu.match(feats[q][0], feats[q][1], home_xy, home_desc)[1] for q in pu.AWAY]
    print("returning vs home:", [c.tolist() for c in back], "away vs home:", [c.tolist() for c in away])
    # measured: returning >= 128, away <= 20; min_matches = 25 lies between.  Half the gaps: (128 - 25) / 2 and (25 - 20) / 2.
    assert min(int(c.min()) for c in back) >= min_matches + (128 - min_matches) // 2
    assert max(int(c.max()) for c in away) <= min_matches - (min_matches - 20 + 1) // 2


def test_restatement_ransac_recovers_the_returning_poses():
    gt, cam, frames = pu.path_scene()
    feats = pu.path_features()
    for q in pu.BACK:
        m, c = pu.match(feats[q][0], feats[q][1], np.stack([feats[k][0] for k in pu.HOME]), np.stack([feats[k][1] for k in pu.HOME]))
        best = pu.query(c, [True] * 3)
        pc, po = pu.matched_points(feats[q][0], frames[q][0], feats[best][0], frames[best][0], m[best], cam)
        r = pu.ransac(q, best, pc, po)
        truth = bso.se3_to_np(bso.se3_mul(bso.se3_inverse(gt[best]), gt[q])).astype(np.float64)
        t_err, r_err = pu.pose_difference(r["old_T_cur"], truth)
        print(f"keyframe {q} -> {best}: {r['inlier_count']} inliers of {len(pc)}, {t_err * 1e3:.2f} mm, {r_err:.3f} deg")
        # measured: >= 137 inliers, <= 1.8 mm, <= 0.09 degrees; the tracker's basin is centimetres and degrees wide
        assert r["found"] and r["inlier_count"] >= 10 + (137 - 10) // 2
        assert t_err <= 0.005 and r_err <= 0.25


# ---- the host RANSAC ----------------------------------------------------------------------------------------------
def _rotation(w):
    from tests import scenes
    return scenes.rotation_from_log(np.asarray(w, np.float64))


def _rotation_of(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _pose_error(pose7, R, t):
    """Largest entry-wise difference of the rotation matrix and of the translation."""
    return float(np.abs(_rotation_of(pose7[:4]) - R).max()), float(np.abs(pose7[4:] - t).max())


def _pose7(R, t):
    # quaternion of R by the same formula as the restatement's output, via Horn on a tetrahedron
    _, _, q = pu.absolute_orientation(np.eye(4, 3), np.eye(4, 3) @ R.T)
    return np.concatenate([q, t])


def _cloud(n, seed):
    rng = np.random.default_rng(seed)
    pc = rng.uniform(-1, 1, (n, 3)) * np.array([1.5, 1.0, 0.8]) + np.array([0, 0, 2.5])
    R, t = _rotation([0.2, -0.35, 0.15]), np.array([0.3, -0.2, 0.1])
    return pc, pc @ R.T + t, R, t


def test_host_ransac_recovers_exact_correspondences():
    pc, po, R, t = _cloud(60, 1)
    r = dba.estimate_relative_pose(7, 2, pc, po)
    assert r["found"] and r["inlier_count"] == 60 and r["inliers"].all()
    r_err, t_err = _pose_error(r["old_T_cur"], R, t)
    assert r_err <= 1e-9 and t_err <= 1e-9, (r_err, t_err)
    assert abs(np.linalg.norm(r["old_T_cur"][:4]) - 1) <= 1e-12 and r["old_T_cur"][3] >= 0
    assert np.abs(r["old_T_cur"] - _pose7(R, t)).max() <= 1e-9


def test_host_ransac_with_gross_outliers_matches_the_restatement():
    pc, po, R, t = _cloud(100, 2)
    rng = np.random.default_rng(3)
    outliers = rng.permutation(100)[:40]
    po[outliers] += rng.uniform(0.3, 1.0, (40, 3)) * rng.choice([-1, 1], (40, 3))   # 40 % moved by at least 0.3 m per axis
    r = dba.estimate_relative_pose(11, 0, pc, po)
    expected = np.ones(100, bool)
    expected[outliers] = False
    assert r["found"] and r["inlier_count"] == 60 and np.array_equal(r["inliers"], expected)
    r_err, t_err = _pose_error(r["old_T_cur"], R, t)
    assert r_err <= 1e-9 and t_err <= 1e-9, (r_err, t_err)
    ref = pu.ransac(11, 0, pc, po)
    assert ref["found"] and np.array_equal(ref["inliers"], r["inliers"])
    assert np.abs(ref["old_T_cur"] - r["old_T_cur"]).max() <= 1e-12


def test_host_ransac_rejects_too_few_inliers():
    pc, po, _, _ = _cloud(30, 4)
    rng = np.random.default_rng(5)
    po[9:] = rng.uniform(-3, 3, (21, 3)) + np.array([0, 0, 10.0])   # 9 consistent correspondences, 21 unrelated points
    r = dba.estimate_relative_pose(5, 1, pc, po)
    assert not r["found"] and r["inlier_count"] < 10
    assert np.isfinite(r["old_T_cur"]).all()
    assert not pu.ransac(5, 1, pc, po)["found"]


@pytest.mark.parametrize("n", [0, 1, 2])
def test_host_ransac_rejects_fewer_than_three_points(n):
    pc, po, _, _ = _cloud(3, 6)
    r = dba.estimate_relative_pose(4, 0, pc[:n], po[:n], min_inliers=1)
    assert not r["found"] and r["inlier_count"] == 0 and np.isfinite(r["old_T_cur"]).all()


def test_host_ransac_rejects_collinear_points():
    s = np.linspace(-1, 1, 40)[:, None]
    pc = np.array([0.1, -0.2, 2.0]) + s * np.array([0.6, 0.3, 0.2])
    R, t = _rotation([0.1, 0.2, -0.1]), np.array([0.05, 0.02, -0.03])
    po = pc @ R.T + t
    r = dba.estimate_relative_pose(9, 3, pc, po)
    assert not r["found"] and np.isfinite(r["old_T_cur"]).all() and r["inlier_count"] == 0
    assert not pu.ransac(9, 3, pc, po)["found"]
    same = np.tile(np.array([[0.3, 0.1, 2.0]]), (20, 1))       # all points equal: zero edges
    r = dba.estimate_relative_pose(9, 3, same, same)
    assert not r["found"] and np.isfinite(r["old_T_cur"]).all()


def test_host_ransac_is_deterministic_and_seeded_by_the_pair():
    pc, po, _, _ = _cloud(80, 7)
    rng = np.random.default_rng(8)
    po[rng.permutation(80)[:30]] += rng.uniform(0.2, 0.5, (30, 3))
    a, b = dba.estimate_relative_pose(12, 1, pc, po), dba.estimate_relative_pose(12, 1, pc, po)
    assert a["found"] and np.array_equal(a["old_T_cur"], b["old_T_cur"]) and np.array_equal(a["inliers"], b["inliers"])
    L = dba._place_lib()
    assert L.bsh_place_ransac_seed(12, 1) == pu.ransac_seed(12, 1) != pu.ransac_seed(1, 12)


def test_default_options_are_the_documented_ones():
    assert dba.place_recognition_options() == pu.DEFAULTS
    with pytest.raises(ValueError):
        dba.place_recognition_options(min_match=3)
