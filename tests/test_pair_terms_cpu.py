"""The float64 reference of the image-pair kernel (tests/pair_terms_util.py) checked on its own, without a GPU: that the hard
fixture makes every branch decide something (census), that few of its pixels sit on a decision boundary, that every Jacobian
of the reference is the derivative of its residual and every b the derivative of its robust cost (finite differences), that
the reference reproduces the rows recorded from the kernel (tests/golden/pair_rows.npz), and how far plain fp32 strays from it (C).

The Jacobian convention, stated once: J = -d r / d delta for ls -> exp(delta) ls, delta = (translation, rotation), where ls is the
base pixel's point in the tracked frame; n_local rotates along, and the associated pixel (px, py), its unprojection lu and its
depth stddev are held fixed.  tests/golden/jacobian_golden.npz (the reference project's own symbolic derivation) holds
d r / d T for lu -> exp(T) lu (depth) and for ls -> exp(T)^-1 ls (descriptor), which is the same thing;
test_jacobian_convention_matches_the_symbolic_fixtures checks both readings on its points."""
import os

import numpy as np
import pytest

from tests import jacobian_fixtures
from tests import pair_terms_util as U

MODES = {"fixed": U.TEX_FIXED_POINT_1_8, "exact": U.TEX_EXACT_FLOAT}
KINDS = {"depth": (1, 0, False), "desc": (0, 1, False), "gradmag": (0, 1, True)}
PAIRS = (0, 1)
STEP = 1e-6


def test_texture_mode_constants_agree_with_the_abi():
    from badslam_amd import abi
    assert (U.TEX_FIXED_POINT_1_8, U.TEX_EXACT_FLOAT) == (abi.TEX_FIXED_POINT_1_8, abi.TEX_EXACT_FLOAT)


# ---- census ------------------------------------------------------------------------------------------------------------
def test_every_stage_holds_pixels_on_the_hard_fixture():
    """Every stage holds at least 8 pixels in at least one (shape, pair); no stage proved unreachable.  `visible` holds at least a
    third of the valid base pixels in every case; the depth residuals of the visible pixels spread over the Tukey radius with a
    tenth of them beyond half of it, and some lie outside it (the grazing patch: a huge inverse stddev); descriptor and gradient-magnitude residuals beyond the Huber radius occur."""
    most = {name: 0 for name in U.STAGES}
    for shape in U.HARD_SHAPES:
        valid = int((U.cached_hard_inputs(shape)["base_depth"] > 0).sum())
        for pair in PAIRS:
            for kind, (use_depth, use_desc, gradmag) in KINDS.items():
                terms = U.hard_terms(shape, pair, use_depth, use_desc, gradmag, U.TEX_EXACT_FLOAT)
                counts = np.bincount(terms.stage.ravel(), minlength=len(U.STAGES))
                for name, count in zip(U.STAGES, counts):
                    most[name] = max(most[name], int(count))
                assert 3 * int(terms.visible.sum()) >= valid, (shape, pair, kind, int(terms.visible.sum()), valid)
                for name, term in terms.terms.items():
                    r = np.abs(term["r"][terms.visible])
                    if name == "depth":
                        q = r / terms.k_depth
                        assert q.min() > 0 and (q > 0.5).mean() >= 0.1, (shape, pair, q.min(), q.max(), (q > 0.5).mean())
                        most["tukey_outside"] = max(most.get("tukey_outside", 0), int((q >= 1).sum()))     # weight 0, constant cost
                        assert all(((q >= lo) & (q < lo + 0.25)).sum() >= 8 for lo in (0, 0.25, 0.5, 0.75)), (shape, pair)
                    else:
                        assert (r >= float(U.K_DESC_HUBER)).sum() >= 8 and (r < float(U.K_DESC_HUBER)).sum() >= 8, (shape, pair, name)
    assert most.pop("tukey_outside") >= 8
    assert set(most) == set(U.COMMON_STAGES) | set(U.DESC_STAGES) | set(U.GRADMAG_STAGES) | {"visible"}
    assert all(count >= 8 for count in most.values()), {name: count for name, count in most.items() if count < 8}


def test_ambiguous_pixels_are_at_most_one_percent():
    for shape in U.HARD_SHAPES:
        valid = int((U.cached_hard_inputs(shape)["base_depth"] > 0).sum())
        for pair in PAIRS:
            for kind, (use_depth, use_desc, gradmag) in KINDS.items():
                for mode in MODES.values():
                    ambiguous = int(U.hard_terms(shape, pair, use_depth, use_desc, gradmag, mode).ambiguous.sum())
                    assert 100 * ambiguous <= valid, (shape, pair, kind, mode, ambiguous, valid)


# ---- finite differences ------------------------------------------------------------------------------------------------
def moved(delta, points, normals=None):
    """exp(delta) applied to points [n, 3] (and the rotation alone to normals); delta has one non-zero coordinate at a time, for
    which exp(delta) is the translation or the rotation itself"""
    R = U.rodrigues(delta[3:])
    return points @ R.T + delta[:3] if normals is None else (points @ R.T + delta[:3], normals @ R.T)


def central_difference(function, at_zero_shape):
    """-> [n, 6]: d function / d delta at 0 by central differences with STEP"""
    out = np.zeros(at_zero_shape + (6,))
    for i in range(6):
        delta = np.zeros(6)
        delta[i] = STEP
        out[..., i] = (function(delta) - function(-delta)) / (2 * STEP)
    return out


def test_jacobian_convention_matches_the_symbolic_fixtures():
    K = jacobian_fixtures.load()
    k = K["depth_pose"]
    R, t = k.rigid("gtf")
    n_local = np.einsum("nji,nj->ni", R, k.vec("n"))
    ls = np.einsum("nji,nj->ni", R, k.vec("s") - t)
    lu = k.vec("l")
    one = U.V(np.ones(k.n))
    J = np.stack([j.v for j in U.depth_jacobian(one, [U.V(n_local[:, i]) for i in range(3)], [U.V(lu[:, i]) for i in range(3)])], -1)
    scale = np.abs(k.jacobian).max(1, keepdims=True)
    assert (np.abs(J - k.jacobian) <= 1e-9 * scale).all()

    def residual(delta):
        p, n = moved(delta, ls, n_local)
        return (n * (lu - p)).sum(1)
    assert (np.abs(-central_difference(residual, (k.n,)) - k.jacobian) <= 1e-6 * scale).all()

    k = K["desc_pose"]
    ls = k.vec("ls")
    u, v = k.v["fx"] * ls[:, 0] / ls[:, 2] + k.v["cx"], k.v["fy"] * ls[:, 1] / ls[:, 2] + k.v["cy"]
    tl, tr, bl, br = k.v["top_left"], k.v["top_right"], k.v["bottom_left"], k.v["bottom_right"]
    fu, fv = jacobian_fixtures.frac(u), jacobian_fixtures.frac(v)
    gx, gy = (br - bl) * fv + (tr - tl) * (1 - fv), (br - tr) * fu + (bl - tl) * (1 - fu)
    J = np.stack([j.v for j in U.colour_jacobian(U.V(gx * k.v["fx"]), U.V(gy * k.v["fy"]), [U.V(ls[:, i]) for i in range(3)])], -1)
    scale = np.abs(k.jacobian).max(1, keepdims=True)
    assert (np.abs(J - k.jacobian) <= 1e-9 * scale).all()


def fd_tolerance(J, A_r):
    """A central difference of a residual whose float64 evaluation is good to 2^-53 of its scale A_r (a few roundings: 8) differs
    from the derivative by that over STEP, plus the truncation STEP^2 |r'''| / 6, far below 1e-6 of the Jacobian's largest entry"""
    return 1e-6 * np.abs(J).max(-1, keepdims=True) + 8 * 2.0 ** -53 * A_r[..., None] / STEP


class Frozen:
    """The residuals of one hard case as functions of delta with the association frozen, for the visible pixels [n]."""

    def __init__(self, shape, pair, kind):
        use_depth, use_desc, gradmag = KINDS[kind]
        self.t = t = U.hard_terms(shape, pair, use_depth, use_desc, gradmag, U.TEX_EXACT_FLOAT)
        self.cameras = U.hard_cameras(shape)
        self.margin = U.coordinate_margin(*self.cameras[1][4:])
        inputs = U.cached_hard_inputs(shape)
        self.v = v = t.visible
        self.ls = np.stack([c.v[v] for c in t.aux["local"]], -1)
        self.n = np.stack([c.v[v] for c in t.aux["n_local"]], -1)
        self.texture = U.Texture(inputs["color"][pair], U.TEX_EXACT_FLOAT, np.float64)
        self.crossed = np.zeros(self.ls.shape[0], bool)
        if kind == "depth":
            self.lu = np.stack([c.v[v] for c in t.aux["lu"]], -1)
            self.inv_stddev = t.aux["inv_stddev"].v[v]
        else:
            self.cp = [(x.v[v], y.v[v]) for x, y in t.aux["cp"]]
            self.cp0 = U.colour_position(self.cameras, self.ls)
            assert np.allclose(self.cp0[0], self.cp[0][0], rtol=0, atol=1e-9) and np.allclose(self.cp0[1], self.cp[0][1], rtol=0, atol=1e-9)
            ys, xs = np.nonzero(v)
            self.base = inputs["base_color"][ys, xs].astype(np.float64)
            if kind == "desc":
                self.d = [d.v[v] for d in t.aux["d"]]

    def sample(self, x, y, x0, y0):
        self.crossed |= (np.floor(x - 0.5) != np.floor(x0 - 0.5)) | (np.floor(y - 0.5) != np.floor(y0 - 0.5))
        return self.texture.value(U.V(x), U.V(y), self.margin)[0].v

    def depth(self, delta):
        p, n = moved(delta, self.ls, self.n)
        return self.inv_stddev * (n * (self.lu - p)).sum(1)

    def gradmag(self, delta):
        x, y = U.colour_position(self.cameras, moved(delta, self.ls))
        return self.sample(x, y, *self.cp[0]) - self.base

    def desc(self, k):
        """what the reference differentiates (BS/kernel_opt_pose.cu:122-190): the three sample points move together, by the
        centre's motion in the colour image"""
        def residual(delta):
            x, y = U.colour_position(self.cameras, moved(delta, self.ls))
            dx, dy = x - self.cp0[0], y - self.cp0[1]
            centre = self.sample(self.cp[0][0] + dx, self.cp[0][1] + dy, *self.cp[0])
            return float(U.K_DESC_SCALE) * (self.sample(self.cp[k][0] + dx, self.cp[k][1] + dy, *self.cp[k]) - centre) - self.d[k - 1]
        return residual

    def residuals(self, kind):
        return {"depth": {"depth": self.depth}, "gradmag": {"gradmag": self.gradmag}, "desc": {"desc1": self.desc(1), "desc2": self.desc(2)}}[kind]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("shape", list(U.HARD_SHAPES))
def test_jacobians_and_b_are_derivatives_of_the_residuals_and_the_robust_cost(shape, pair, kind):
    f = Frozen(shape, pair, kind)
    t, v = f.t, f.v
    n = int(v.sum())
    found, cost_derivative, b, scale_b = {}, np.zeros((n, 6)), np.zeros((n, 6)), np.zeros((n, 1))
    weight_scale = 1.0 if kind == "depth" else t.desc_weight
    for name, residual in f.residuals(kind).items():
        term = {key: value[v] for key, value in t.terms[name].items()}
        assert np.allclose(residual(np.zeros(6)), term["r"], rtol=0, atol=1e-9 * (1 + term["A_r"])), name
        found[name] = (-central_difference(residual, (n,)), term)

        def robust_cost(delta, residual=residual):
            r = U.V(residual(delta))
            if kind == "depth":
                return U.tukey(r, U.V(np.float64(t.k_depth)), np.float64)[1].v
            return weight_scale * U.huber(r, U.V(np.float64(U.K_DESC_HUBER)), np.float64)[1].v
        cost_derivative += central_difference(robust_cost, (n,))
        b += (term["w"] * term["r"])[:, None] * term["J"]
        # the cost is good to 2^-53 of |w r| A_r to first order; its second derivative jumps at the Huber radius: a pixel within
        # STEP |J| of it is skipped with the texel crossings
        scale_b += 1e-6 * np.abs(term["w"] * term["r"])[:, None] * np.abs(term["J"]).max(-1, keepdims=True) + \
            8 * 2.0 ** -53 * (np.abs(term["w"]) * (np.abs(term["r"]) + 1e-3) * term["A_r"])[:, None] / STEP
        if kind == "depth":
            # the truncation of the central difference, STEP^2 / 6 |d^3 cost / d delta^3|: r is linear or quadratic in delta, and
            # the Tukey cost's third derivative by r, (20 q^3 - 12 q) / k, is at most 12 / k
            scale_b += STEP ** 2 / 6 * 12 / t.k_depth * np.abs(term["J"]).max(-1, keepdims=True) ** 3
        else:
            f.crossed |= np.abs(np.abs(term["r"]) - float(U.K_DESC_HUBER)) <= 4 * STEP * np.abs(term["J"]).max(-1) * 2
    assert 50 * int(f.crossed.sum()) <= n, (int(f.crossed.sum()), n)                     # at most 2 % skipped
    # Where a sample's footprint is clamped at the image border the reference's gradient (BS/cost_function.cuh:200-239) is a
    # difference of the two nearest texels, not the derivative of the clamped value: those pixels' Jacobians are what the
    # operation defines them to be (the GPU test compares them), and no derivative.
    # They lie in a strip along the border of the colour image: half a texel wide at the left and the top, and up to one and a half
    # at the right and the bottom (the footprint's second texel, and the descriptor's samples one depth pixel further on): two
    # texels per axis, so at most the share 2 (cw + ch) / (cw ch) of the image -- the cap on what this exclusion may take.
    interior = t.stage[v] == U.S["visible"]
    cw, ch = f.cameras[0][4:]
    print(f"{shape} pair {pair} {kind}: {n} visible, {int((~interior).sum())} in the border strip, {int(f.crossed.sum())} crossings or Huber edges")
    assert int((~interior).sum()) * cw * ch <= 2 * (cw + ch) * n, (int((~interior).sum()), n)
    keep = ~f.crossed & interior
    assert keep.sum() >= 50
    for name, (J_fd, term) in found.items():
        excess = np.abs(J_fd - term["J"]) - fd_tolerance(term["J"], term["A_r"])
        assert (excess[keep] <= 0).all(), (name, float(excess[keep].max()), int((excess[keep] > 0).sum()))
    excess = np.abs(-cost_derivative - b) - scale_b
    assert (excess[keep] <= 0).all(), (float(excess[keep].max()), int((excess[keep] > 0).sum()))
    # and b of the assembled row is that b
    assert np.allclose(t.coeffs[v][:, 21:27], b, rtol=1e-12, atol=0)


# ---- the reference against the recorded rows ---------------------------------------------------------------------------
def full_row_tolerance(terms, coeffs, width, height):
    """The "full-row tolerance": the per-pixel tolerances summed, plus the reduction's (n_add + 1) 2^-24 sum |pixel rows|."""
    row, _, _ = terms.row(coeffs)
    return U.pixel_tolerance(terms, coeffs).sum((0, 1)) + U.reduction_bound(width, height, np.abs(row).sum((0, 1)))


# What tests/test_gpu_pair_rows_recorded.py recorded tests/golden/pair_rows.npz with (stated again here so that this module imports
# nothing of a GPU module): name -> (depth size, colour size, depth camera fx fy cx cy, threshold factor); the colour camera is
# the depth camera scaled; depth = u16 * f32(1 / 5000); a shape may share all inputs but the tracked colour with another.
RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_rows.npz")
RECORDED_SHAPES = {
    "20x12": ((20, 12), (20, 12), (40.0, 40.0, 10.0, 6.0), 4.0),
    "84x60": ((84, 60), (84, 60), (100.0, 100.0, 42.3, 29.6), 1.0),
    "84x60_color42x30": ((84, 60), (42, 30), (100.0, 100.0, 42.3, 29.6), 1.0),
}
RECORDED_STORED_WITH = {"84x60_color42x30": "84x60"}
RECORDED_RAW_TO_FLOAT, RECORDED_BASELINE_FX = np.float32(1.0 / 5000), 40.0
RECORDED_RESIDUAL_SETS = {"depth": (1, 0), "desc": (0, 1), "both": (1, 1)}


def test_reference_reproduces_the_recorded_rows():
    """Every variant/* and single/* row of tests/golden/pair_rows.npz against the float64 sum of the reference's per-pixel rows:
    every value within the full-row tolerance and nothing more, ambiguous pixels or not, and the count exactly -- in all 222
    cases, which is more than is owed where a case has ambiguous pixels (112 of them do; none of their decisions fell the
    other way in the recorded rows, and the rows are fixed)."""
    with np.load(RECORDED) as f:
        recorded = {key: f[key] for key in f.files}
    checked = unambiguous = 0
    for shape, ((dw, dh), (cw, ch), (fx, fy, cx, cy), threshold) in RECORDED_SHAPES.items():
        stored = RECORDED_STORED_WITH.get(shape, shape)
        inputs = {key: recorded[f"{shape if key == 'color' else stored}/{key}"] for key in ("depth", "normals", "color_depth", "color", "M")}
        s = cw / dw
        cameras = ((fx * s, fy * s, cx * s, cy * s, cw, ch), (fx, fy, cx, cy, dw, dh))
        depth = inputs["depth"].astype(np.float32) * RECORDED_RAW_TO_FLOAT
        for mode_name, mode in MODES.items():
            for label, row in zip(recorded[f"{shape}/{mode_name}/labels"], recorded[f"{shape}/{mode_name}/rows"]):
                part = str(label).split("/")
                if part[0] == "variant":
                    frame, m, coeffs, gradmag = 1, 0, part[2] == "coeffs", len(part) > 3
                elif part[0] == "single":
                    frame, m, coeffs, gradmag = int(part[2][5:]), int(part[3][1:]), True, False
                else:
                    continue                                   # batched rows equal single rows bit for bit (the recorded test)
                use_depth, use_desc = RECORDED_RESIDUAL_SETS[part[1]]
                images = {"base_depth": depth[0], "base_normals": inputs["normals"][0], "base_color": inputs["color_depth"][0],
                          "depth": depth[frame], "normals": inputs["normals"][frame], "color": inputs["color"][frame]}
                terms = U.pair_terms(images, cameras, inputs["M"][m], RECORDED_BASELINE_FX, threshold, use_depth, use_desc, gradmag, mode, np.float64)
                want, _, _ = U.summed_row(terms, coeffs)
                got = row.view(np.float32).astype(np.float64)
                got[U.COL_COUNT] = row[U.COL_COUNT]
                assert got[U.COL_COUNT] == want[U.COL_COUNT], (shape, mode_name, label, got[U.COL_COUNT], want[U.COL_COUNT])
                unambiguous += not terms.ambiguous.any()
                tolerance = full_row_tolerance(terms, coeffs, dw, dh)
                columns = list(range(27)) if coeffs else [U.COL_COST]
                excess = np.abs(got - want)[columns] - tolerance[columns]
                assert (excess <= 0).all(), (shape, mode_name, label, np.nonzero(excess > 0)[0].tolist(), float(excess.max()))
                checked += 1
    assert checked == 2 * 3 * (10 + 27) and unambiguous >= 2 * (10 + 27), (checked, unambiguous)


# ---- C -----------------------------------------------------------------------------------------------------------------
def measure_c(kind):
    """The largest |row32 - row64| / (2^-24 A) over all columns of both output kinds and all non-ambiguous pixels of the hard
    fixture that both precisions see (both texture modes; in the fixed-point mode less the widening of an undecided weight).
    Also: a pixel that is not flagged ambiguous leaves the kernel at the same stage in fp32 as in float64."""
    use_depth, use_desc, gradmag = KINDS[kind]
    worst = 0.0
    for shape in U.HARD_SHAPES:
        for pair in PAIRS:
            for mode in MODES.values():
                t64 = U.hard_terms(shape, pair, use_depth, use_desc, gradmag, mode)
                t32 = U.hard_terms(shape, pair, use_depth, use_desc, gradmag, mode, "float32")
                decided = ~(t64.ambiguous | t32.ambiguous)
                assert np.array_equal(t64.stage[decided], t32.stage[decided]), (shape, pair, kind, mode)
                both = decided & t64.visible
                for coeffs in (True, False):
                    row64, A, widen = t64.row(coeffs)
                    row32 = t32.row(coeffs)[0].astype(np.float64)
                    live = A[both] > 0
                    ratio = np.maximum(np.abs(row32 - row64)[both] - widen[both], 0)[live] / (U.EPS32 * A[both][live])
                    worst = max(worst, float(ratio.max()))
    return worst


@pytest.mark.parametrize("kind", list(KINDS))
def test_measured_c(kind):
    measured = measure_c(kind)
    print(f"C[{kind}] = {measured:.4f} (recorded {U.C_MEASURED[kind]})")
    assert 0 < measured <= U.C_MEASURED[kind], (kind, measured, U.C_MEASURED[kind])
    assert measured >= 0.5 * U.C_MEASURED[kind], "the recorded value is stale: far above what is measured"
