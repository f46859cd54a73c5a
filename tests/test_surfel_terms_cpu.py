"""CPU: the float64 reference of the surfel pair body and of the geometry iteration (tests/surfel_terms_util.py) on its own and
against the oracle, before a GPU is involved: the census of the hard fixture (every stage, both halves of both robust
functions, both sides of every geometry guard), the cap on undecided pairs, finite differences of every Jacobian, the recorded
symbolic Jacobians where the formulas coincide, the oracle's per-surfel probe and geometry iteration, and the measured C.

The Jacobian convention is that of tests/test_pair_terms_cpu.py: J = -d r / d delta for ls -> exp(delta) ls.
"""
import numpy as np
import pytest

from badslam_amd import abi
from tests import jacobian_fixtures
from tests import surfel_terms_util as U

MODES = {"fixed": abi.TEX_FIXED_POINT_1_8, "exact": abi.TEX_EXACT_FLOAT}
STEP = 1e-6
MIN_PAIRS = 8


def test_constants_agree_with_the_abi():
    assert (U.TEX_FIXED_POINT_1_8, U.TEX_EXACT_FLOAT) == (abi.TEX_FIXED_POINT_1_8, abi.TEX_EXACT_FLOAT)
    assert U.INVALID_DEPTH_BIT == abi.BSLAM_INVALID_DEPTH_BIT and U.SURFEL_ACTIVE_FLAG == abi.BSLAM_SURFEL_ACTIVE_FLAG
    assert (U.ROW_X, U.ROW_Y, U.ROW_Z, U.ROW_NORMAL) == (abi.SURFEL_X, abi.SURFEL_Y, abi.SURFEL_Z, abi.SURFEL_NORMAL)
    assert (U.ROW_RADIUS_SQUARED, U.ROW_COLOR, U.ROW_D1, U.ROW_D2) == (abi.SURFEL_RADIUS_SQUARED, abi.SURFEL_COLOR, abi.SURFEL_DESCRIPTOR1, abi.SURFEL_DESCRIPTOR2)


def test_fixture_has_the_shape_the_kernels_are_cut_by():
    """1317 surfels: two work slots of the geometry-only pose kernel (4 x 256 surfels each) and three of the photometric one
    (2 x 256), the last granule ragged; six keyframes: two waves of the photometric kernel take two each"""
    assert U.N_SURFELS == 1317 and U.N_KEYFRAMES == 6
    assert -(-U.N_SURFELS // 1024) == 2 and -(-U.N_SURFELS // 512) == 3 and U.N_SURFELS % 256 not in (0, 255)
    for case in U.CASES:
        fix = U.hard_fixture(case)
        assert fix.surfels.shape == (8, U.N_SURFELS) and len(fix.keyframes) == U.N_KEYFRAMES
        assert fix.keyframes[0]["depth"].shape == (23, 37)
        assert np.isnan(fix.surfels[U.ROW_X]).sum() >= 4 and (fix.active == 0).sum() >= 8
    assert U.hard_fixture("colour_19x12").keyframes[0]["luma"].shape == (12, 19)
    deformed = U.hard_fixture("deformed_depth")
    assert deformed.a != 0 and np.ptp(deformed.cfactor) > 0


@pytest.mark.parametrize("case", list(U.CASES))
def test_every_stage_and_every_robust_half_holds_pairs(case):
    for mode in MODES.values():
        terms = U.hard_terms(case, 1, 1, mode)
        counts = np.bincount(terms.stage[~terms.ambiguous], minlength=len(U.STAGES))
        for name, count in zip(U.STAGES, counts):
            if name == "associated_no_desc" and case != "colour_19x12":
                # equal cameras: the depth-to-colour map is the identity, and a position inside the depth image is inside the colour image
                assert count == 0
                continue
            assert count >= MIN_PAIRS, (case, name, count)
        assert (terms.stage[:, U.N_KEYFRAMES - 1] == 0).all(), "the last keyframe looks away"
        decided = ~terms.ambiguous
        raw = np.abs(terms.terms["depth"]["r"].v)
        assert (decided & terms.associated & (raw < 10)).sum() >= MIN_PAIRS and (decided & terms.associated & (raw >= 10)).sum() >= MIN_PAIRS, "Tukey"
        for name in ("desc1", "desc2"):
            r = np.abs(terms.terms[name]["r"].v)
            assert (decided & terms.has_desc & (r < 10)).sum() >= MIN_PAIRS and (decided & terms.has_desc & (r >= 10)).sum() >= MIN_PAIRS, name
        # the tangent samples: footprints on the image border (the gradient's second path), samples beyond the last row / column
        assert (decided & terms.has_desc & terms.border).sum() >= MIN_PAIRS and (decided & terms.has_desc & ~terms.border).sum() >= MIN_PAIRS
    assert (U.hard_terms(case, 0, 1, MODES["fixed"]).widen > 0).any() and not (U.hard_terms(case, 0, 1, MODES["exact"]).widen > 0).any()
    # a NaN position and a surfel beyond the end leave at the first stage for every keyframe
    fix = U.hard_fixture(case)
    assert (U.hard_terms(case, 1, 1, MODES["exact"]).stage[fix.groups["nan"]] == 0).all()


@pytest.mark.parametrize("case", list(U.CASES))
def test_every_geometry_guard_has_surfels_on_both_sides(case):
    fix = U.hard_fixture(case)
    for use_depth, use_desc in ((1, 0), (1, 1), (0, 1)):
        g = U.hard_geometry(case, use_depth, use_desc, MODES["exact"])
        decided = ~g.ambiguous
        assert (g.on & decided & (g.count >= 1)).sum() >= MIN_PAIRS and (g.on & decided & (g.count < 1)).sum() >= MIN_PAIRS, "a[3] >= 1"
        assert (~g.on).sum() >= MIN_PAIRS
        assert (g.code[g.updated & decided] != fix.surfels[U.ROW_NORMAL].view(np.uint32)[g.updated & decided]).sum() >= MIN_PAIRS, "normals change"
        if not use_desc:
            assert (g.moved & decided).sum() >= MIN_PAIRS and (g.on & ~g.moved & decided).sum() >= MIN_PAIRS, "H > 1e-6"
            assert (np.abs(g.step[g.moved]) > 1e-4).sum() >= MIN_PAIRS
        else:
            for i in range(3):
                assert (g.moved3[:, i] & decided).sum() >= MIN_PAIRS and (g.on & ~g.moved3[:, i] & decided).sum() >= MIN_PAIRS, ("x != 0", i)
            for i in range(2):
                assert (g.clamped[:, i] & decided).sum() >= 4 and (g.moved3[:, 1 + i] & ~g.clamped[:, i] & decided).sum() >= MIN_PAIRS, "the +-180 clamp"
            assert (g.unclamped[g.clamped & decided[:, None]] < -180).sum() >= 4 and (g.unclamped[g.clamped & decided[:, None]] > 180).sum() >= 4
            # Q2: H12 would not be zero if it were accumulated -- the sums that would form it exist
            assert (g.sums["H01"].v != 0).sum() >= MIN_PAIRS and (g.sums["H02"].v != 0).sum() >= MIN_PAIRS


@pytest.mark.parametrize("case", list(U.CASES))
def test_undecided_pairs_and_surfels_are_at_most_one_percent(case):
    for mode in MODES.values():
        for use_depth, use_desc in U.VARIANTS:
            terms = U.hard_terms(case, use_depth, use_desc, mode)
            assert 100 * terms.ambiguous.sum() <= terms.ambiguous.size, (case, mode, use_depth, use_desc, int(terms.ambiguous.sum()))
            g = U.hard_geometry(case, use_depth, use_desc, mode)
            assert 100 * g.normal_ambiguous.sum() <= U.N_SURFELS and 100 * g.ambiguous.sum() <= U.N_SURFELS, (case, int(g.normal_ambiguous.sum()), int(g.ambiguous.sum()))


# ---- finite differences ------------------------------------------------------------------------------------------------
def moved(delta, points, normals=None):
    R = U.rodrigues(delta[3:])
    return points @ R.T + delta[:3] if normals is None else (points @ R.T + delta[:3], normals @ R.T)


def central_difference(function, count):
    out = np.zeros((count, 6))
    for i in range(6):
        delta = np.zeros(6)
        delta[i] = STEP
        out[:, i] = (function(delta) - function(-delta)) / (2 * STEP)
    return out


@pytest.mark.parametrize("case", list(U.CASES))
def test_jacobians_are_derivatives_of_the_residuals(case):
    """Central differences in float64 of the residuals as functions of the pose (6), of the position along the normal and of the two
    descriptors, with what the Jacobians hold fixed held fixed: the pixel, the depth stddev, and the image gradient of the
    descriptor residual (all three samples move with the centre's projection, BS/cost_function.cuh:187-190)."""
    inp = U.hard_inputs(case)
    terms = U.hard_terms(case, 1, 1, MODES["exact"])
    (cfx, cfy, _, _, _, _), _ = inp.cameras
    pick = terms.has_desc & ~terms.ambiguous
    assert pick.sum() > 1000
    ls, n = terms.local[pick], terms.n_local[pick]
    d = terms.terms["depth"]
    inv = terms.inv_stddev.v[pick]
    J = np.stack([j.v[pick] for j in d["J"]], -1)
    def depth_residual(delta, lu):
        p, nn = moved(delta, ls, n)
        return inv * (nn * (lu - p)).sum(1)
    lu = _unprojected_pixels(inp, terms)[pick]
    assert np.allclose(depth_residual(np.zeros(6), lu), d["r"].v[pick], rtol=0, atol=1e-9 * d["r"].a[pick].max())
    fd = -central_difference(lambda delta: depth_residual(delta, lu), len(ls))
    assert (np.abs(fd - J) <= 1e-6 * np.abs(J).max(1, keepdims=True) + 8 * 2.0 ** -53 * d["r"].a[pick][:, None] / STEP).all()
    # position along the normal: depth (-inv |n|^2, the normal being a unit vector up to roundings) and descriptor
    t_fd = (inv * (n * (lu - (ls + STEP * n))).sum(1) - inv * (n * (lu - (ls - STEP * n))).sum(1)) / (2 * STEP)
    assert (np.abs(t_fd + inv) <= 1e-6 * inv).all()
    for name in ("desc1", "desc2"):
        t = terms.terms[name]
        gx, gy = t["gx"].v[pick], t["gy"].v[pick]
        J = np.stack([j.v[pick] for j in t["J"]], -1)

        def image_term(p):
            return gx * cfx * p[:, 0] / p[:, 2] + gy * cfy * p[:, 1] / p[:, 2]
        fd = -central_difference(lambda delta: image_term(moved(delta, ls)), len(ls))
        scale = np.abs(J).max(1, keepdims=True)
        assert (np.abs(fd - J) <= 1e-6 * scale + 1e-9).all(), name
        jp = U.descriptor_position_jacobian(*[U.V(a) for a in (gx, gy)], cfx, cfy, [U.V(n[:, i]) for i in range(3)], [U.V(ls[:, i]) for i in range(3)]).v
        fd = (image_term(ls + STEP * n) - image_term(ls - STEP * n)) / (2 * STEP)
        assert (np.abs(fd - jp) <= 1e-6 * np.maximum(np.abs(jp), (np.abs(gx) * cfx + np.abs(gy) * cfy) / ls[:, 2])).all(), name
    # the descriptors: the whole reference run again with d1, d2 moved -- d r / d d = -1, and nothing else of the pair changes
    for row, name in ((U.ROW_D1, "desc1"), (U.ROW_D2, "desc2")):
        values, stored = [], []
        for sign in (1, -1):
            surfels = np.array(inp.surfels)
            surfels[row] = (surfels[row].astype(np.float64) + sign * 0.25).astype(np.float32)
            stored.append(surfels[row].astype(np.float64)[np.nonzero(pick)[0]])
            shifted = U.Inputs(surfels, inp.active, inp.keyframes, inp.cameras, inp.baseline_fx, inp.raw_to_float_depth, inp.a, inp.cfactor, inp.cell)
            values.append(U.surfel_terms(shifted, 1, 1, MODES["exact"], np.float64).terms[name]["r"].v[pick])
        small = np.abs(inp.surfels[row])[np.nonzero(pick)[0]] < 1000            # next to 1e5 a quarter is below the spacing of fp32
        assert (np.abs((values[0] - values[1])[small] / (stored[0] - stored[1])[small] + 1) <= 1e-9).all(), name


def _unprojected_pixels(inp, terms):
    """[N, K, 3]: the associated pixel's unprojection, from the fixture's images alone (float64)"""
    _, (fx, fy, cx, cy, w, h) = inp.cameras
    fx, fy, cx, cy = (float(np.float32(v)) for v in (fx, fy, cx, cy))
    out = np.zeros(terms.local.shape)
    for k, kf in enumerate(inp.keyframes):
        ls = terms.local[:, k]
        with np.errstate(invalid="ignore", divide="ignore"):
            px = np.clip(np.nan_to_num(np.trunc(fx * ls[:, 0] / ls[:, 2] + cx)), 0, w - 1).astype(int)
            py = np.clip(np.nan_to_num(np.trunc(fy * ls[:, 1] / ls[:, 2] + cy)), 0, h - 1).astype(int)
        depth = U.calibrated_depth(kf["depth"], inp.cfactor, inp.cell, inp.a, inp.raw_to_float_depth, np.float64).v[py, px]
        out[:, k] = np.stack([depth * (px - (cx - 0.5)) / fx, depth * (py - (cy - 0.5)) / fy, depth], -1)
    return out


def test_position_jacobians_match_the_symbolic_fixtures():
    """tests/golden/jacobian_golden.npz (the reference project's own symbolic derivation): the rows whose formulas coincide with
    this module's -- the descriptor residual by a move along the normal, and the depth residual's -|n|^2"""
    K = jacobian_fixtures.load()
    k = K["desc_position"]
    R, t = k.rigid("ftg")
    ls = np.einsum("nij,nj->ni", R, k.vec("s")) + t
    rn = np.einsum("nij,nj->ni", R, k.vec("n"))
    u, v = k.v["fx"] * ls[:, 0] / ls[:, 2] + k.v["cx"], k.v["fy"] * ls[:, 1] / ls[:, 2] + k.v["cy"]
    tl, tr, bl, br = k.v["top_left"], k.v["top_right"], k.v["bottom_left"], k.v["bottom_right"]
    fu, fv = jacobian_fixtures.frac(u), jacobian_fixtures.frac(v)
    gx, gy = (br - bl) * fv + (tr - tl) * (1 - fv), (br - tr) * fu + (bl - tl) * (1 - fu)
    jp = U.descriptor_position_jacobian(U.V(gx), U.V(gy), U.V(k.v["fx"]), U.V(k.v["fy"]), [U.V(rn[:, i]) for i in range(3)], [U.V(ls[:, i]) for i in range(3)])
    assert (np.abs(jp.v - k.jacobian[:, 0]) <= 1e-9 * jp.a).all()
    k = K["depth_position"]
    assert (np.abs(k.jacobian[:, 0] + (k.vec("n") ** 2).sum(1)) <= 1e-12).all()


# ---- the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(U.CASES))
def test_reference_agrees_with_the_oracles_per_surfel_probe(case, mode):
    """HostScene.accumulate_pose(per_surfel=True) of every keyframe: the flags equal the reference's off the ambiguous pairs, residuals
    and weights lie within 4 C 2^-24 of their scales (plus the fixed-point jump), and H64 / b64 within the summed row tolerances."""
    terms = U.hard_terms(case, 1, 1, MODES[mode])
    scene = U.scene_copy(case, 1, 1, MODES[mode])
    tolerance = U.pair_tolerance(terms)
    # a NaN position: the oracle follows the reference's `if (z <= 0) return false`, which lets a NaN pass; the pose and geometry
    # kernels test z > 0 (csrc/device_math.hpp: project_to_pixel), and so does the reference.  The oracle runs without those surfels.
    nan = np.isnan(scene.surfels[U.ROW_X, :U.N_SURFELS])
    scene.surfels[U.ROW_X, :U.N_SURFELS][nan] = 0
    scene.surfels[U.ROW_Z, :U.N_SURFELS][nan] = -1
    for k, kf in enumerate(scene.keyframes):
        got = scene.accumulate_pose(kf, per_surfel=True)
        ps = got["per_surfel"].astype(np.float64)
        decided = ~terms.ambiguous[:, k]
        flags = terms.associated[:, k] + 2 * terms.has_desc[:, k]
        assert np.array_equal(ps[decided, 6], flags[decided]), (case, mode, k, np.nonzero(decided & (ps[:, 6] != flags))[0][:8])
        for column, name, kind, mask in ((0, "depth", "depth", terms.associated), (2, "desc1", "desc", terms.has_desc), (4, "desc2", "desc", terms.has_desc)):
            t = terms.terms[name]
            pick = decided & mask[:, k] & (ps[:, 6] == flags)
            allowed = U.KERNEL_FACTOR * U.C_MEASURED[kind] * U.EPS32 * t["r"].a[:, k] + t["jump"][:, k]
            assert (np.abs(ps[:, column] - t["r"].v[:, k])[pick] <= allowed[pick]).all(), (case, mode, k, name, "r")
            other = U.huber(U.V(ps[:, column]), U.V(np.float64(10)), np.float64)[0].v * 0.01 if kind == "desc" else U.tukey(U.V(ps[:, column]), U.V(np.float64(10)), np.float64)[0].v
            # the weight against the robust function of the oracle's OWN residual (one rounding of a few operations: 8 ulp of 1)
            assert (np.abs(ps[:, column + 1] - other)[pick] <= 8 * U.EPS32 * np.maximum(other[pick], 0.01 if kind == "desc" else 1)).all(), (case, mode, k, name, "w")
        own = np.abs(np.where(terms.ambiguous[:, k, None], terms.row[:, k], 0)).sum(0) + np.where(terms.ambiguous[:, k, None], terms.A[:, k], 0).sum(0)
        want, allowed = terms.row[:, k].sum(0), tolerance[:, k].sum(0) + own
        assert (np.abs(got["H64"] - want[:21]) <= allowed[:21]).all() and (np.abs(got["b64"] - want[21:27]) <= allowed[21:27]).all(), (case, mode, k)
        if not terms.ambiguous[:, k].any():
            assert got["count"] == want[U.COL_COUNT]
            cost_allowed = tolerance[:, k, U.COL_COST].sum() + (U.N_SURFELS + 1) * U.EPS32 * np.abs(terms.row[:, k, U.COL_COST]).sum()
            assert abs(got["cost"] - want[U.COL_COST]) <= cost_allowed, (case, mode, k, got["cost"], want[U.COL_COST])


def oracle_scene(case, use_depth, use_desc, mode):
    """the scene with its NaN positions replaced by positions behind every camera but the last (see above), inactive for it too"""
    scene = U.scene_copy(case, use_depth, use_desc, mode)
    nan = np.nonzero(np.isnan(scene.surfels[U.ROW_X, :U.N_SURFELS]))[0]
    scene.active[0, nan] = 0
    return scene


@pytest.mark.parametrize("use_depth,use_desc", [(1, 0), (1, 1), (0, 1)])
@pytest.mark.parametrize("case", list(U.CASES))
def test_reference_agrees_with_the_oracles_geometry_iteration(case, use_depth, use_desc):
    failures = []
    for mode in MODES.values():
        g = U.hard_geometry(case, use_depth, use_desc, mode)
        scene = oracle_scene(case, use_depth, use_desc, mode)
        before = np.array(scene.surfels)
        scene.update_normals()
        assert np.array_equal(scene.surfels[U.ROW_NORMAL, :U.N_SURFELS].view(np.uint32)[~g.normal_ambiguous], g.code[~g.normal_ambiguous])
        scene = oracle_scene(case, use_depth, use_desc, mode)
        scene.optimize_geometry_iteration()
        failures += U.check_geometry(g, before, scene.surfels, use_desc, (case, mode))
    assert not failures, failures


def test_measured_c():
    measured = U.measure_c()
    print({kind: round(value, 4) for kind, value in measured.items()}, "recorded", U.C_MEASURED)
    for kind, value in measured.items():
        assert 0 < value <= U.C_MEASURED[kind], (kind, value, U.C_MEASURED[kind])
        assert value >= 0.5 * U.C_MEASURED[kind], "the recorded value is stale: far above what is measured"
