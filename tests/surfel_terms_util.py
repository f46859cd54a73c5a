"""A plain NumPy restatement of one surfel against one keyframe -- the pair body of pose_accumulate_kernel (csrc/pose_kernels.hpp)
and of the geometry iteration (csrc/geometry_kernels.hpp) -- vectorised over (surfel, keyframe), and the deterministic "hard"
fixture the per-pair tests run on.  The reference itself (surfel_terms, geometry_terms) calls neither the library nor the oracle.

Written from the formulas of the operation in the reference project (BS/ = applications/badslam/src/badslam): cost_function.cuh
(depth residual :56-98, tangent points :115-136, descriptor residual :140-156, its image gradient :191-260), surfel_projection*.cuh
(projection, association, depth-to-colour map), robust_weighting.cuh, kernel_opt_pose.cu (Jacobians, accumulation :251-383),
kernel_opt_geometry.cu (normals :527-597, position :417-507, position + descriptors :118-361), gauss_newton.cuh, util.cuh
(depth calibration :46-53, normal codes).  Values, scales, the texture, the robust functions and the pose Jacobians are those of
tests/pair_terms_util.py (imported, not copied); see its docstring for what a scale `A` is.  Generic in the dtype: np.float64 is
the reference, np.float32 only MEASURES how far plain fp32 strays from it (C_MEASURED).

Two quirks of the operation are kept: Q1 -- the cost column counts only the FIRST descriptor residual of a pair; Q2 -- the joint
position + descriptor system never accumulates H12, it is solved with H12 = 0.

The Tukey zero-weight half CAN be reached by an associated pair: association bounds |z_surfel - z_pixel| by 10 sigma, the residual
is n . (unprojected pixel - surfel) / sigma.  For a tilted normal the residual's numerator is the offset ALONG THE NORMAL, of
which the z difference is only the share n.z, and the lateral offset of the pixel centre from the surfel's projection adds to it;
so a surfel offset 10 .. 11 sigma along a normal tilted by 15 .. 25 degrees associates with |r| >= 10.  The fixture holds such
surfels (HardFixture: `near_ten`), and the census of tests/test_surfel_terms_cpu.py requires the half to be live in the pose rows.
In the geometry iteration's position pass the normal is the NEW one, the mean of the associated pixels' normals: it is the
measured surface's own normal, for which the offset along the normal and the z difference nearly coincide, so there an
associated pair with weight zero is a matter of the last tenth of a sigma and cannot be placed on purpose.  The guards H > 1e-6
and x0 != 0 are therefore closed in the fixture by active surfels that no keyframe associates (H = b = 0: the 0 / 0 they guard
against); an associated surfel whose every weight is zero occurs by chance only (three surfels of `deformed_depth`).
"""
import ctypes
import functools

import numpy as np

from tests.pair_terms_util import (COL_COST, COL_COUNT, EPS32, KERNEL_FACTOR, K_COS_NORMAL_COMPAT, K_DEPTH_TUKEY, K_DEPTH_UNCERTAINTY,
                                   K_DESC_HUBER, K_DESC_SCALE, K_DESC_WEIGHT, ROW, TEX_EXACT_FLOAT, TEX_FIXED_POINT_1_8, Texture, V,
                                   colour_jacobian, coordinate_margin, decode_normal, depth_jacobian, dot3, encode_normal, huber,
                                   near_integer, rodrigues, tukey)

INVALID_DEPTH_BIT = 1 << 15                       # abi.BSLAM_INVALID_DEPTH_BIT (the tests assert that they agree)
SURFEL_ACTIVE_FLAG = 1
# rows of the surfel buffer (abi.SURFEL_*)
ROW_X, ROW_Y, ROW_Z, ROW_NORMAL, ROW_RADIUS_SQUARED, ROW_COLOR, ROW_D1, ROW_D2 = range(8)

# The stage at which a pair leaves the kernel, in the kernel's order; the last two are "associated".
STAGES = ("z_nonpositive_or_nan", "out_left", "out_top", "out_right", "out_bottom", "record_depth_0", "depth_far", "depth_near",
          "back_facing", "normal_incompatible", "associated_no_desc", "associated")
S = {name: i for i, name in enumerate(STAGES)}
FIRST_ASSOCIATED = S["associated_no_desc"]


# ---- pieces of the operation -------------------------------------------------------------------------------------------
def unpack_surfel_normal(code, dtype):
    """SurfelGetNormal (BS/util_nvcc_only.cuh): three signed 10-bit fields / 511, normalised"""
    code = np.asarray(code, np.uint32)
    fields = [(((code >> shift) & 0x3ff).astype(np.int64) ^ 0x200) - 0x200 for shift in (0, 10, 20)]
    n = [V(f.astype(dtype)) / dtype(511) for f in fields]
    length = dot3(n, n).sqrt_clamped()
    return [c / length for c in n]


def pack_surfel_normal(n):
    """SurfelSetNormal: every component to a signed 10-bit field, int16(v * 511 +- 0.5) truncated -> (uint32 code, the three
    numbers v * 511 +- 0.5 whose truncation decides the fields)"""
    code, decided = np.zeros(np.shape(n[0]), np.uint32), []
    for shift, v in zip((0, 10, 20), n):
        with np.errstate(invalid="ignore"):
            q = v * 511 + np.where(v > 0, 0.5, -0.5)
            field = np.nan_to_num(np.trunc(q), nan=0.0).astype(np.int64)
        code |= ((field & 0x3ff) << shift).astype(np.uint32)
        decided.append(q)
    return code, decided


def calibrated_depth(raw_u16, cfactor, cell, a, raw_to_float_depth, dtype):
    """RawToCalibratedDepth BS/util.cuh:46-53 for every pixel; 0 where the pixel holds no measurement (invalid bit, or raw 0)"""
    h, w = raw_u16.shape
    ys, xs = np.mgrid[0:h, 0:w]
    valid = ((raw_u16 & INVALID_DEPTH_BIT) == 0) & (raw_u16 != 0)
    raw = V(np.where(valid, raw_u16, 1).astype(dtype))
    inv_depth = dtype(1) / (dtype(np.float32(raw_to_float_depth)) * raw)
    cf = V(cfactor[ys // cell, xs // cell].astype(dtype))
    exponent = -(dtype(np.float32(a)) * inv_depth)
    e = V(np.exp(exponent.v), np.exp(exponent.v) * (1 + exponent.a))
    depth = dtype(1) / (inv_depth + cf * e)
    return depth.where(valid, dtype(0))


def tangent_points(gp, gn, radius_squared, dtype):
    """ComputeTangentProjections BS/cost_function.cuh:115-136, the part that depends on the surfel only -> (p1, p2, whether the
    choice of the helper axis |n.x| > 0.9 is undecided)"""
    use_y = np.abs(gn[0].v) > 0.9
    zero, one = V(np.zeros_like(gn[0].v)), V(np.ones_like(gn[0].v))
    helper = [zero.where(use_y, one), one.where(use_y, zero), zero]
    cross = lambda a, b: [a[1] * b[2] - b[1] * a[2], b[0] * a[2] - a[0] * b[2], a[0] * b[1] - b[0] * a[1]]

    def scaled(t):
        sq = dot3(t, t)
        sq = sq.where(sq.v > 1e-12, dtype(1e-12))
        factor = dtype(2) * (radius_squared / sq).sqrt_clamped()
        return [c * factor for c in t]
    t1 = scaled(cross(gn, helper))
    t2 = scaled(cross(gn, t1))
    return [gp[i] + t1[i] for i in range(3)], [gp[i] + t2[i] for i in range(3)], np.abs(np.abs(gn[0].v) - 0.9) < 1e-5


def descriptor_position_jacobian(gx, gy, cfx, cfy, rn, ls):
    """BS/kernel_opt_geometry.cu:188-192: d r / d t for a surfel move of t along its normal; gx, gy = image gradient of the residual"""
    term1 = -(cfx * (rn[0] * ls[2] - rn[2] * ls[0]))
    term2 = -(cfy * (rn[1] * ls[2] - rn[2] * ls[1]))
    return -((gx * term1 + gy * term2) / (ls[2] * ls[2]))


class Inputs:
    """Host arrays of one problem.  surfels: float32 [8, N] (row 3 holds the uint32 normal codes' bits); active: uint8 [N];
    keyframes: list of {"depth" u16 [h, w], "normals" u16 [h, w], "luma" u8 [ch, cw], "M" frame_T_global 12 floats,
    "R" global_R_frame 9 floats}; cameras: (colour, depth), each (fx, fy, cx, cy, width, height), pixel-corner convention."""

    def __init__(self, surfels, active, keyframes, cameras, baseline_fx, raw_to_float_depth, a, cfactor, cell):
        self.surfels, self.active, self.keyframes, self.cameras = surfels, active, keyframes, cameras
        self.baseline_fx, self.raw_to_float_depth, self.a, self.cfactor, self.cell = baseline_fx, raw_to_float_depth, a, cfactor, cell


class SurfelTerms:
    """What surfel_terms returns; every array is per pair [N, K, ...].
    stage: index into STAGES; associated; has_desc; ambiguous: a discrete decision of the pair lies within its margin.
    terms: {"depth" | "desc1" | "desc2": {"r", "J" (six), "w", "cost" as V (value and scale), for the descriptors "gx", "gy" (image
    gradient of the residual, no focal length), and "jump" (how far the residual may move in the fixed-point mode)}} -- garbage
    where the residual does not exist.
    row, A, widen: the 32-column row (H 0..20, b 21..26, cost 27 with Q1, count 28), its scale and the fixed-point widening;
    A_depth, A_desc: the two kinds' shares of A.  pixel_normal [N, K, 3], n_local, local, inv_stddev: for the geometry reference."""


def stack_v(per_k, key, part):
    return np.stack([getattr(o[key], part) for o in per_k], 1)


def surfel_terms(inp, use_depth, use_desc, tex_mode, dtype, normal_codes=None):
    """Every (surfel, keyframe) pair of `inp`.  normal_codes: in place of the surfels' (the geometry iteration's second pass)."""
    dtype = np.dtype(dtype).type
    f = lambda value: dtype(np.float32(value))
    (cfx, cfy, ccx, ccy, cw, ch), (fx, fy, cx, cy, w, h) = inp.cameras
    cfx, cfy, ccx, ccy, fx, fy, cx, cy = (V(f(v)) for v in (cfx, cfy, ccx, ccy, fx, fy, cx, cy))
    bfx = V(f(inp.baseline_fx))
    half = dtype(0.5)
    margin = coordinate_margin(max(w, cw), max(h, ch))
    rows = inp.surfels
    N = rows.shape[1]
    gp = [V(rows[r].astype(dtype)) for r in (ROW_X, ROW_Y, ROW_Z)]
    codes = rows[ROW_NORMAL].view(np.uint32) if normal_codes is None else normal_codes
    gn = unpack_surfel_normal(codes, dtype)
    d_surfel = [V(rows[ROW_D1].astype(dtype)), V(rows[ROW_D2].astype(dtype))]
    p1, p2, helper_undecided = tangent_points(gp, gn, V(rows[ROW_RADIUS_SQUARED].astype(dtype)), dtype)
    ray_x = lambda x: (V(np.asarray(x).astype(dtype)) - (cx - half)) / fx          # PixelCenterUnprojector
    ray_y = lambda y: (V(np.asarray(y).astype(dtype)) - (cy - half)) / fy
    d2c_fx, d2c_fy = cfx / fx, cfy / fy                                           # DepthToColorPixelCorner
    d2c_cx, d2c_cy = -(cfx * cx / fx) + ccx, -(cfy * cy / fy) + ccy
    k_depth, k_huber, desc_weight = V(dtype(K_DEPTH_TUKEY)), V(dtype(K_DESC_HUBER)), V(dtype(K_DESC_WEIGHT))
    scale = V(dtype(K_DESC_SCALE))
    per_k = []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k, kf in enumerate(inp.keyframes):
            M = [V(f(v)) for v in np.asarray(kf["M"]).reshape(12)]
            transform = lambda p: [M[4 * i] * p[0] + M[4 * i + 1] * p[1] + M[4 * i + 2] * p[2] + M[4 * i + 3] for i in range(3)]
            rotate = lambda p: [M[4 * i] * p[0] + M[4 * i + 1] * p[1] + M[4 * i + 2] * p[2] for i in range(3)]
            stage = np.full(N, S["associated"], np.int64)
            alive, ambiguous = np.ones(N, bool), np.zeros(N, bool)

            def leave(mask, name):
                nonlocal alive
                stage[alive & mask] = S[name]
                alive = alive & ~mask
            local = transform(gp)
            leave(~(local[2].v > 0), "z_nonpositive_or_nan")
            pxy = (fx * (local[0] / local[2]) + cx, fy * (local[1] / local[2]) + cy)
            ambiguous |= alive & (near_integer(pxy[0].v, margin) | near_integer(pxy[1].v, margin))
            leave(pxy[0].v < 0, "out_left")
            leave(pxy[1].v < 0, "out_top")
            leave(np.trunc(pxy[0].v) >= w, "out_right")
            leave(np.trunc(pxy[1].v) >= h, "out_bottom")
            px = np.clip(np.nan_to_num(np.trunc(pxy[0].v), nan=0.0, posinf=0.0, neginf=0.0), 0, w - 1).astype(np.int64)
            py = np.clip(np.nan_to_num(np.trunc(pxy[1].v), nan=0.0, posinf=0.0, neginf=0.0), 0, h - 1).astype(np.int64)
            image_depth = calibrated_depth(kf["depth"], inp.cfactor, inp.cell, inp.a, inp.raw_to_float_depth, dtype)
            pixel_depth = V(image_depth.v[py, px], image_depth.a[py, px])
            leave(~(pixel_depth.v > 0), "record_depth_0")
            pixel_depth = pixel_depth.where(pixel_depth.v > 0, dtype(1))
            # IsAssociatedWithPixel BS/surfel_projection_nvcc_only.cuh:49-127
            n_local = rotate(gn)
            tnx, tny = ray_x(px), ray_y(py)
            slant = (n_local[0] * tnx + n_local[1] * tny + n_local[2]).abs()
            variance_part = V(dtype(K_DEPTH_UNCERTAINTY)) * slant * pixel_depth * pixel_depth
            bound = k_depth * (variance_part / bfx)
            difference = local[2] - pixel_depth
            ambiguous |= alive & (np.abs(np.abs(difference.v) - bound.v) <= 1e-5 * bound.v)
            leave(difference.v > bound.v, "depth_far")
            leave(-difference.v > bound.v, "depth_near")
            facing = dot3(local, n_local)
            ambiguous |= alive & (np.abs(facing.v) <= 1e-5 * facing.a)
            leave(facing.v > 0, "back_facing")
            pixel_normal = decode_normal(kf["normals"][py, px], dtype)
            compat = dot3(n_local, pixel_normal)
            ambiguous |= alive & (np.abs(compat.v - dtype(K_COS_NORMAL_COMPAT)) <= 1e-5 * float(K_COS_NORMAL_COMPAT))
            leave(compat.v < dtype(K_COS_NORMAL_COMPAT), "normal_incompatible")
            associated = alive.copy()

            out = {"local": local, "n_local": n_local, "pixel_normal": pixel_normal}
            # depth residual BS/cost_function.cuh:56-98
            inv_stddev = bfx / variance_part
            lu = [pixel_depth * tnx, pixel_depth * tny, pixel_depth]
            raw = inv_stddev * dot3(n_local, [lu[i] - local[i] for i in range(3)])
            weight, cost = tukey(raw, k_depth, dtype)
            out["depth"] = (raw, depth_jacobian(inv_stddev, n_local, lu), weight, cost, None, None, np.zeros(N))
            out["inv_stddev"] = inv_stddev
            # descriptor residuals BS/cost_function.cuh:115-260, BS/kernel_opt_pose.cu:320-382
            cp = (d2c_fx * pxy[0] + d2c_cx, d2c_fy * pxy[1] + d2c_cy)
            outside = (cp[0].v < 0) | (cp[1].v < 0) | (np.trunc(cp[0].v) >= cw) | (np.trunc(cp[1].v) >= ch)
            has_desc = associated & ~outside
            if use_desc:
                ambiguous |= associated & (near_integer(cp[0].v, margin) | near_integer(cp[1].v, margin))
                stage[associated & outside] = S["associated_no_desc"]
                texture = Texture(kf["luma"], tex_mode, dtype)
                positions = [cp]
                for point in (p1, p2):
                    ls = transform(point)
                    positions.append((cfx * (ls[0] / ls[2]) + ccx, cfy * (ls[1] / ls[2]) + ccy))
                sampled = [texture.value(p[0], p[1], margin) for p in positions]
                gradients = [texture.gradient(p[0], p[1]) for p in positions]
                ambiguous |= has_desc & (sampled[0][3] | sampled[1][3] | sampled[2][3] | helper_undecided)
                out["border"] = sampled[0][2] | sampled[1][2] | sampled[2][2]
                for i, name in ((1, "desc1"), (2, "desc2")):
                    r = scale * (sampled[i][0] - sampled[0][0]) - d_surfel[i - 1]
                    gx, gy = scale * (gradients[i][0] - gradients[0][0]), scale * (gradients[i][1] - gradients[0][1])
                    hw, hc = huber(r, k_huber, dtype)
                    out[name] = (r, colour_jacobian(gx * cfx, gy * cfy, local), desc_weight * hw, desc_weight * hc, gx, gy,
                                 float(K_DESC_SCALE) * (sampled[i][1] + sampled[0][1]))
            else:
                stage[associated] = S["associated"]
            out.update(stage=stage, associated=associated, has_desc=has_desc, ambiguous=ambiguous & ~(stage == 0))
            per_k.append(out)

    res = SurfelTerms()
    stack = lambda key: np.stack([o[key] for o in per_k], 1)
    res.stage, res.associated, res.has_desc, res.ambiguous = stack("stage"), stack("associated"), stack("has_desc"), stack("ambiguous")
    if use_desc:
        res.border = stack("border")
    vec = lambda key: (np.stack([np.stack([c.v for c in o[key]], -1) for o in per_k], 1), np.stack([np.stack([c.a for c in o[key]], -1) for o in per_k], 1))
    res.pixel_normal, _ = vec("pixel_normal")
    res.n_local, res.n_local_a = vec("n_local")
    res.local, res.local_a = vec("local")
    res.inv_stddev = V(stack_v(per_k, "inv_stddev", "v"), stack_v(per_k, "inv_stddev", "a"))
    res.use_depth, res.use_desc = use_depth, use_desc
    names = ["depth"] + (["desc1", "desc2"] if use_desc else [])
    res.terms = {}
    for name in names:
        r = V(np.stack([o[name][0].v for o in per_k], 1), np.stack([o[name][0].a for o in per_k], 1))
        J = [V(np.stack([o[name][1][i].v for o in per_k], 1), np.stack([o[name][1][i].a for o in per_k], 1)) for i in range(6)]
        wt = V(np.stack([o[name][2].v for o in per_k], 1), np.stack([o[name][2].a for o in per_k], 1))
        cost = V(np.stack([o[name][3].v for o in per_k], 1), np.stack([o[name][3].a for o in per_k], 1))
        g = [None if per_k[0][name][i] is None else V(np.stack([o[name][i].v for o in per_k], 1), np.stack([o[name][i].a for o in per_k], 1)) for i in (4, 5)]
        res.terms[name] = {"r": r, "J": J, "w": wt, "cost": cost, "gx": g[0], "gy": g[1], "jump": np.stack([o[name][6] for o in per_k], 1)}
    _assemble(res, dtype)
    return res


def _row_of(terms, shape, dtype):
    """[(r, J, w, cost or None, mask)] -> V [.., 32] with zeros where a term's mask is false"""
    v, a = np.zeros(shape + (ROW,), dtype), np.zeros(shape + (ROW,), dtype)

    def add(col, value, mask):
        with np.errstate(invalid="ignore"):
            v[..., col] += np.where(mask, value.v, 0)
            a[..., col] += np.where(mask, value.a, 0)
    for r, J, w, cost, mask in terms:
        idx = 0
        for i in range(6):
            wj = w * J[i]
            for j in range(i, 6):
                add(idx, wj * J[j], mask)
                idx += 1
        wr = w * r
        for i in range(6):
            add(21 + i, wr * J[i], mask)
        if cost is not None:
            add(COL_COST, cost, mask)
        v[..., COL_COUNT] += mask
    return V(v, a)


def _assemble(res, dtype):
    shape = res.stage.shape
    t = res.terms
    depth = [(t["depth"]["r"], t["depth"]["J"], t["depth"]["w"], t["depth"]["cost"], res.associated)] if res.use_depth else []
    desc = []
    if res.use_desc:
        desc.append((t["desc1"]["r"], t["desc1"]["J"], t["desc1"]["w"], t["desc1"]["cost"], res.has_desc))        # Q1: only this cost
        desc.append((t["desc2"]["r"], t["desc2"]["J"], t["desc2"]["w"], None, res.has_desc))
    row_depth, row_desc = _row_of(depth, shape, dtype), _row_of(desc, shape, dtype)
    row_desc.v[..., COL_COUNT] = res.has_desc if res.use_desc else 0          # the two residuals of a pair count once
    res.row = row_depth.v + row_desc.v
    res.A_depth, res.A_desc = row_depth.a.astype(np.float64), row_desc.a.astype(np.float64)
    res.A = res.A_depth + res.A_desc
    widen = np.zeros(shape + (ROW,))
    if res.use_desc and any(np.any(t[n]["jump"][res.has_desc] > 0) for n in ("desc1", "desc2")):
        k_huber, desc_weight = V(dtype(K_DESC_HUBER)), V(dtype(K_DESC_WEIGHT))
        for s1 in (-1, 1):
            for s2 in (-1, 1):
                moved = []
                for sign, name, cost in ((s1, "desc1", True), (s2, "desc2", False)):
                    r = V((t[name]["r"].v.astype(np.float64) + sign * t[name]["jump"]).astype(dtype))
                    hw, hc = huber(r, k_huber, dtype)
                    moved.append((r, t[name]["J"], desc_weight * hw, desc_weight * hc if cost else None, res.has_desc))
                other = _row_of(moved, shape, dtype)
                other.v[..., COL_COUNT] = res.has_desc
                widen = np.maximum(widen, np.abs(other.v.astype(np.float64) - row_desc.v.astype(np.float64)))
    res.widen = widen


# C: the largest |value32 - value64| / (2^-24 A) over the decided pairs (surfels) of the hard fixture, value32 being the same
# formulas in np.float32 -- measured on the CPU from the reference alone; tests/test_surfel_terms_cpu.py::test_measured_c recomputes
# it and fails if it grows.  The measured values, rounded up.
C_MEASURED = {"depth": 6.8, "desc": 1.4, "normals": 2.2, "position": 1.4, "joint": 2.5}


def pair_tolerance(terms):
    """[N, K, 32]: KERNEL_FACTOR 2^-24 (C[depth] A[depth] + C[desc] A[desc]) + the fixed-point mode's widening"""
    return KERNEL_FACTOR * EPS32 * (C_MEASURED["depth"] * terms.A_depth + C_MEASURED["desc"] * terms.A_desc) + terms.widen


# ---- the geometry iteration --------------------------------------------------------------------------------------------
class GeometryTerms:
    """Per surfel [N]: on (exists and active), count (associated keyframes with the OLD normal), mean [N, 3] and A_mean, code (uint32,
    the old code where count < 1 or the surfel is off), normal_ambiguous (an s10 field within its margin of a rounding boundary, or
    an ambiguous pair in the normals pass), step / A_step (geometry-only: -b / H along the new normal; 0 where the guard is closed),
    H, moved (H > 1e-6 and on), joint: x [N, 3] (guard_undecided [N, 3]: |x| below its tolerance) / A_x [N, 3] (x0 position, x1, x2 descriptors), new_d [N, 2] (clamped), clamped [N, 2],
    ambiguous (some pair of the second pass, or the normal)."""


def geometry_terms(inp, use_depth, use_desc, tex_mode, dtype):
    """UpdateSurfelNormals + one OptimizeGeometryIteration (BS/kernel_opt_geometry.cc:39-78, 137-169), per surfel"""
    dt = np.dtype(dtype).type
    N, K = inp.surfels.shape[1], len(inp.keyframes)
    on = (inp.active & SURFEL_ACTIVE_FLAG) != 0
    first = surfel_terms(inp, True, False, tex_mode, dtype)
    g = GeometryTerms()
    g.on = on
    take = first.associated & on[:, None]
    total, total_a = np.zeros((N, 3), dt), np.zeros((N, 3), dt)
    count = np.zeros(N, dt)
    for k, kf in enumerate(inp.keyframes):                                      # in keyframe order, as the kernels add
        R = [V(dt(np.float32(v))) for v in np.asarray(kf["R"]).reshape(9)]
        pn = [V(first.pixel_normal[:, k, i]) for i in range(3)]
        for i in range(3):
            c = R[3 * i] * pn[0] + R[3 * i + 1] * pn[1] + R[3 * i + 2] * pn[2]
            total[:, i] += np.where(take[:, k], c.v, 0)
            total_a[:, i] += np.where(take[:, k], c.a, 0)
        count += take[:, k]
    g.count = count
    updated = on & (count >= 1)
    inv = dt(1) / np.where(updated, count, 1)
    g.mean, g.A_mean = inv[:, None] * total, (inv[:, None] * total_a).astype(np.float64)
    code, decided = pack_surfel_normal([g.mean[:, i] for i in range(3)])
    old = inp.surfels[ROW_NORMAL].view(np.uint32)
    g.code = np.where(updated, code, old).astype(np.uint32)
    boundary = np.zeros(N, bool)
    for i, q in enumerate(decided):
        boundary |= np.abs(q - np.rint(q)) <= np.maximum(1e-4, 511 * 8 * EPS32 * g.A_mean[:, i])
    g.normal_ambiguous = (updated & boundary) | (first.ambiguous & on[:, None]).any(1)
    g.updated = updated

    second = surfel_terms(inp, use_depth, use_desc, tex_mode, dtype, normal_codes=g.code)
    g.second = second
    g.ambiguous = g.normal_ambiguous | (second.ambiguous & on[:, None]).any(1)
    take = second.associated & on[:, None]
    t = second.terms
    zero = V(np.zeros(N, dt))

    def total_of(value, mask):
        out = zero
        for k in range(K):
            with np.errstate(invalid="ignore"):
                out = out + V(np.where(mask[:, k], value.v[:, k], 0), np.where(mask[:, k], value.a[:, k], 0))
        return out
    dj = -second.inv_stddev
    dw, dr = t["depth"]["w"], t["depth"]["r"]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if not use_desc:
            H = total_of(dw * dj * dj, take)
            b = total_of(dw * dj * dr, take)
            g.H, g.moved = H.v, on & (H.v > 1e-6)
            step = -(b / H.where(g.moved, dt(1)))
            g.step, g.A_step = np.where(g.moved, step.v, 0), np.where(g.moved, step.a, 0).astype(np.float64)
            g.associated_any = take.any(1)
            return g
        has = second.has_desc & on[:, None]
        (cfx, cfy, _, _, _, _), _ = inp.cameras
        cfx, cfy = V(dt(np.float32(cfx))), V(dt(np.float32(cfy)))
        rn = [V(second.n_local[..., i], second.n_local_a[..., i]) for i in range(3)]
        ls = [V(second.local[..., i], second.local_a[..., i]) for i in range(3)]
        jp = [descriptor_position_jacobian(t[n]["gx"], t[n]["gy"], cfx, cfy, rn, ls) for n in ("desc1", "desc2")]
        k_huber, desc_weight = V(dt(K_DESC_HUBER)), V(dt(K_DESC_WEIGHT))
        depth_H, depth_b = (total_of(dw * dj * dj, take), total_of(dw * dr * dj, take)) if use_depth else (zero, zero)

        def solve(r1, r2):
            """the sums and the 3 x 3 solve for given descriptor residuals -> (x0, x1, x2, the sums)"""
            w1, w2 = desc_weight * huber(r1, k_huber, dt)[0], desc_weight * huber(r2, k_huber, dt)[0]
            H00 = total_of(w1 * jp[0] * jp[0] + w2 * jp[1] * jp[1], has) + depth_H
            b0 = total_of(w1 * r1 * jp[0] + w2 * r2 * jp[1], has) + depth_b
            H01, H02 = -total_of(w1 * jp[0], has), -total_of(w2 * jp[1], has)
            H11, H22 = total_of(w1, has), total_of(w2, has)
            b1, b2 = -total_of(w1 * r1, has), -total_of(w2 * r2, has)
            # UpdateSurfelPositionAndDescriptorCUDAKernel BS/kernel_opt_geometry.cu:273-361 (Q2: H12 = 0)
            eps = dt(1e-6)
            L00 = (H00 + eps).sqrt_clamped()
            L01 = H01 / L00
            L11 = ((H11 + eps) - L01 * L01).sqrt_clamped()
            L02 = H02 / L00
            L12 = (zero - L02 * L01) / L11
            L22 = ((H22 + eps) - L02 * L02 - L12 * L12).sqrt_clamped()
            y0 = b0 / L00
            y1 = (b1 - L01 * y0) / L11
            y2 = (b2 - L02 * y0 - L12 * y1) / L22
            x2 = y2 / L22
            x1 = (y1 - L12 * x2) / L11
            x0 = (y0 - L02 * x2 - L01 * x1) / L00
            return x0, x1, x2, {"H00": H00, "H01": H01, "H02": H02, "H11": H11, "H22": H22, "b0": b0, "b1": b1, "b2": b2}
        r1, r2 = t["desc1"]["r"], t["desc2"]["r"]
        x0, x1, x2, g.sums = solve(r1, r2)
        # fixed-point texture mode: a residual whose filter weight sits on a rounding boundary may move by its jump; to first order
        # the step moves by the sum over those residuals of what each one's move does, taken twice
        widen = np.zeros((N, 3))
        for name, which in (("desc1", 0), ("desc2", 1)):
            jump = np.where(has, t[name]["jump"], 0)
            for k in np.nonzero((jump > 0).any(0))[0]:
                shift = np.zeros(jump.shape)
                shift[:, k] = jump[:, k]
                moved_r = [r1, r2]
                moved_r[which] = V((moved_r[which].v.astype(np.float64) + shift).astype(dt), moved_r[which].a)
                other = solve(*moved_r)
                widen += 2 * np.abs(np.stack([o.v.astype(np.float64) - x.v.astype(np.float64) for o, x in zip(other[:3], (x0, x1, x2))], 1))
    g.widen_x = np.nan_to_num(widen, nan=np.inf)
    g.x = np.stack([x0.v, x1.v, x2.v], 1)
    g.A_x = np.stack([x0.a, x1.a, x2.a], 1).astype(np.float64)
    g.moved3 = on[:, None] & (g.x != 0)
    # x != 0 is undecided where the float64 step is smaller than the fp32 evaluation's error (two Huber-limited residuals of opposite
    # sign cancel exactly in b: the reference gets 0, fp32 a last-bit remainder)
    g.guard_undecided = on[:, None] & (g.A_x > 0) & (np.abs(g.x) <= KERNEL_FACTOR * C_MEASURED["joint"] * EPS32 * g.A_x + g.widen_x)
    d_old = np.stack([inp.surfels[ROW_D1], inp.surfels[ROW_D2]], 1).astype(dt)
    unclamped = d_old - g.x[:, 1:]
    g.new_d = np.where(g.moved3[:, 1:], np.clip(unclamped, -180, 180), d_old)
    g.clamped = g.moved3[:, 1:] & (np.abs(unclamped) > 180)
    g.unclamped = unclamped
    g.associated_any = take.any(1)
    return g


# ---- the hard fixture --------------------------------------------------------------------------------------------------
N_SURFELS, N_KEYFRAMES = 1317, 6
DEPTH_SIZE = (37, 23)
DEPTH_CAMERA = (45.0, 44.0, 18.2, 11.7)
BASELINE_FX = 40.0
RAW_TO_FLOAT_DEPTH = float(np.float32(1.0 / 5000.0))
CELL = 4
# name -> (colour size, colour camera, a, whether the cfactor image is non-constant)
CASES = {
    "same_camera": ((37, 23), (45.0, 44.0, 18.2, 11.7), 0.0, False),
    "colour_19x12": ((19, 12), (23.5, 22.1, 10.6, 7.0), 0.0, False),
    "deformed_depth": ((37, 23), (45.0, 44.0, 18.2, 11.7), 0.45, True),
}
# global_T_frame of the keyframes: rotation vector, translation.  Keyframe 4 stands 0.45 m to the right: what lies right of its column
# 30 nobody else sees, so a surfel there has one pair.  Keyframe 5 looks away from the surface.
_POSES = [((0.004, -0.006, 0.010), (0.010, -0.005, 0.000)), ((0.030, -0.040, 0.020), (-0.060, 0.030, 0.020)),
          ((-0.035, 0.030, -0.050), (0.050, 0.050, -0.050)), ((0.020, 0.050, 0.080), (0.020, -0.070, 0.040)),
          ((-0.010, 0.020, -0.015), (0.450, 0.010, 0.000)), ((0.020, np.pi - 0.03, 0.010), (0.000, 0.000, 0.100))]


def _surface(x, y):
    """the scene: z = S(x, y) in the global frame, and its gradient"""
    z = 1.6 + 0.10 * np.sin(1.1 * x + 0.2) * np.cos(0.9 * y) + 0.05 * x
    return z, 0.11 * np.cos(1.1 * x + 0.2) * np.cos(0.9 * y) + 0.05, -0.09 * np.sin(1.1 * x + 0.2) * np.sin(0.9 * y)


def _cast(R, t, rays):
    """depth along rays [.., 3] (z = 1) of a camera global_T_frame = (R, t) to the surface, by Newton's method"""
    d = np.full(rays.shape[:-1], 1.6)
    direction = rays @ R.T
    for _ in range(12):
        p = d[..., None] * direction + t
        z, sx, sy = _surface(p[..., 0], p[..., 1])
        d = d - (p[..., 2] - z) / (direction[..., 2] - sx * direction[..., 0] - sy * direction[..., 1])
    return d


def _surface_normal(p):
    _, sx, sy = _surface(p[..., 0], p[..., 1])
    n = np.stack([sx, sy, -np.ones_like(sx)], -1)
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def _luma(u, v, phase):
    base = 128 + 55 * np.sin(0.9 * u + 0.3 + phase) * np.cos(0.7 * v - 0.2) + 45 * np.sin(0.5 * (u + v) + 2 * phase)
    base = np.where((u >= 24) & (u < 27), 255.0, base)                            # a hard edge: 255 next to 0
    return np.where((u >= 27) & (u < 30), 0.0, base)


def pose_quaternions():
    """[K, 7] float32: unit quaternion (x, y, z, w) and translation of every keyframe's global_T_frame"""
    out = []
    for w, t in _POSES:
        w = np.asarray(w, np.float64)
        angle = np.linalg.norm(w)
        out.append(np.concatenate([np.sin(angle / 2) * w / angle, [np.cos(angle / 2)], t]))
    return np.asarray(out, np.float32)


def _frac(v):
    return v - np.floor(v)


class HardFixture:
    """Deterministic inputs of one case: surfels float32 [8, N], active uint8 [N], keyframes (depth u16, normals u16, luma u8,
    rgba u8 [ch, cw, 4] with the luma in .w), cameras, cfactor, a; groups: {name: surfel indices} of the surfels placed on purpose."""


@functools.lru_cache(maxsize=None)
def hard_fixture(case, size=DEPTH_SIZE, cell=CELL, n_surfels=N_SURFELS):
    """size, cell, n_surfels: the variants of tests/lifecycle_util.py (another image size, cell size and surfel count over the same
    scene, poses and groups); the defaults are the fixture every other module uses."""
    (cw, ch), color_cam, a, vary_cfactor = CASES[case]
    w, h = size
    CELL, N_SURFELS = cell, n_surfels
    fx, fy, cx, cy = DEPTH_CAMERA
    fix = HardFixture()
    fix.case, fix.a = case, a
    fix.cameras = (color_cam + (cw, ch), DEPTH_CAMERA + (w, h))
    gy_, gx_ = np.mgrid[0:(h - 1) // CELL + 1, 0:(w - 1) // CELL + 1]
    fix.cfactor = ((0.0020 + 0.0012 * np.sin(0.8 * gx_ + 0.5 * gy_)) if vary_cfactor else np.zeros(gx_.shape)).astype(np.float32)
    poses = [(rodrigues(wv), np.asarray(t, np.float64)) for wv, t in _POSES]
    fix.quaternions = pose_quaternions()
    ys, xs = np.mgrid[0:h, 0:w]
    centre_rays = np.stack([(xs - (cx - 0.5)) / fx, (ys - (cy - 0.5)) / fy, np.ones(xs.shape)], -1)
    fix.keyframes = []
    for k, (R, t) in enumerate(poses):
        if k == N_KEYFRAMES - 1:
            d, normal = np.full((h, w), 1.5), np.zeros((h, w, 3))
        else:
            d = _cast(R, t, centre_rays)
            normal = _surface_normal(d[..., None] * (centre_rays @ R.T) + t) @ R
        raw = np.clip(np.rint(d / RAW_TO_FLOAT_DEPTH), 1, INVALID_DEPTH_BIT - 1).astype(np.uint16)
        hole = ((xs * 5 + ys * 11 + k) % 29 == 3) | ((ys >= h // 2) & (ys < h // 2 + 2) & (xs >= 3 + k) & (xs < 6 + k))
        # no measurement: the invalid bit alone, or on top of a depth that would associate (a raw 0 WITHOUT the bit is outside the
        # operation's domain -- the preprocessing never writes one, and at a = 0 the calibration formula is 0 * inf for it)
        raw[hole & ((xs + ys) % 2 == 0)] = INVALID_DEPTH_BIT
        raw[hole & ((xs + ys) % 2 == 1)] |= INVALID_DEPTH_BIT
        cys, cxs = np.mgrid[0:ch, 0:cw]
        s = w / cw
        luma = np.clip(_luma(s * (cxs + 0.5), s * (cys + 0.5), 0.4 * k) + 0.5, 0, 255).astype(np.uint8)
        rgba = np.stack([np.full_like(luma, 0x55), 255 - luma, np.full_like(luma, 0xaa), luma], -1)
        # squared point radii as half-float bits, another number at every pixel of every keyframe (the lifecycle reads them)
        radius = 0.010 + 0.012 * _frac(0.37 * xs + 0.61 * ys + 0.29 * k)
        fix.keyframes.append({"depth": raw, "normals": encode_normal(normal).astype(np.uint16), "luma": luma, "rgba": np.ascontiguousarray(rgba),
                              "radius": (radius * radius).astype(np.float16).view(np.uint16)})

    i = np.arange(N_SURFELS)
    g1, g2, g3, g4 = (_frac((i + 1) * c) for c in (0.7548776662466927, 0.5698402909980532, 0.3819660112501051, 0.2360679774997897))
    home = i % 5
    u, v = g1 * (w + 5) - 2.5, g2 * (h + 5) - 2.5
    rays = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones(N_SURFELS)], -1)
    position, normal, sigma = np.zeros((N_SURFELS, 3)), np.zeros((N_SURFELS, 3)), np.zeros(N_SURFELS)
    for k in range(5):
        R, t = poses[k]
        sel = home == k
        d = _cast(R, t, rays[sel])
        position[sel] = d[:, None] * (rays[sel] @ R.T) + t
        normal[sel] = _surface_normal(position[sel])
        sigma[sel] = 0.1 * d * d / BASELINE_FX
    groups = {"tilt_40": i % 7 == 3, "tilt_90": i % 17 == 5, "flipped": i % 23 == 7, "beyond_10_sigma": i % 11 == 4, "near_ten": i % 13 == 6,
              "wide": i % 5 == 2, "huge_descriptor": i % 83 == 10, "nan": i % 167 == 20, "inactive": i % 101 == 50}
    theta = np.radians(12.0 * g4)
    theta = np.where(groups["near_ten"], np.radians(15 + 10 * g4), theta)
    theta = np.where(groups["tilt_40"], np.radians(33 + 14 * g4), theta)
    theta = np.where(groups["tilt_90"], np.radians(78 + 24 * g4), theta)
    theta = np.where(groups["flipped"], np.radians(170 + 10 * g4), theta)
    e1 = np.cross(normal, [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(normal, e1)
    phi = 2 * np.pi * g3
    tilted = np.cos(theta)[:, None] * normal + np.sin(theta)[:, None] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
    codes, _ = pack_surfel_normal([tilted[:, c] for c in range(3)])
    decoded = np.stack([c.v for c in unpack_surfel_normal(codes, np.float64)], 1)
    sign = np.where(i % 2 == 0, 1.0, -1.0)
    offset = 16 * (g3 - 0.5)
    offset = np.where(groups["near_ten"], sign * (9.6 + 1.6 * g2), offset)
    offset = np.where(groups["beyond_10_sigma"], sign * (10.6 + 4 * g2), offset)
    slant = np.maximum(np.abs((decoded * (position / position[:, 2:3])).sum(1)), 0.2)
    position = position + (offset * sigma * slant)[:, None] * decoded
    radius = np.where(groups["wide"], 0.06 + 0.05 * g4, 0.012 + 0.012 * g4)
    d1, d2 = 15 * np.sin(1.7 * i), 15 * np.cos(2.3 * i)
    d1, d2 = np.where(groups["huge_descriptor"], 1e5, d1), np.where(groups["huge_descriptor"], -1e5, d2)
    position[groups["nan"], 0] = np.nan
    surfels = np.zeros((8, N_SURFELS), np.float32)
    surfels[ROW_X:ROW_Z + 1] = position.T
    surfels[ROW_NORMAL] = codes.view(np.float32)
    surfels[ROW_RADIUS_SQUARED] = radius * radius
    surfels[ROW_COLOR] = np.full(N_SURFELS, 0x80808080, np.uint32).view(np.float32)
    surfels[ROW_D1], surfels[ROW_D2] = d1, d2
    fix.surfels = surfels
    fix.active = np.where(groups["inactive"], 0, SURFEL_ACTIVE_FLAG).astype(np.uint8)
    fix.groups = {name: np.nonzero(mask)[0] for name, mask in groups.items()}
    for array in (fix.surfels, fix.active, fix.cfactor, fix.quaternions):
        array.setflags(write=False)
    for kf in fix.keyframes:
        for array in kf.values():
            array.setflags(write=False)
    return fix


# ---- what the tests share ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_scene(case):
    """The fixture as a tests.bso.HostScene (the containers the library's and the oracle's entry points read; the one place of this
    module that touches the oracle's binding, for the keyframe views' matrices: frame_T_global and global_R_frame are formed
    from the quaternion in fp32 there, and the reference takes them from the views, so that it reads what the kernels read)."""
    from badslam_amd import abi
    from tests import bso
    fix = hard_fixture(case)
    color_cam, depth_cam = (bso.make_camera(*c) for c in fix.cameras)
    scene = bso.HostScene(color_cam, depth_cam, RAW_TO_FLOAT_DEPTH, BASELINE_FX, CELL, N_SURFELS + 59)
    scene.cfactor[:] = fix.cfactor
    scene.a = fix.a
    for k, kf in enumerate(fix.keyframes):
        pose = abi.SE3f((ctypes.c_float * 4)(*[float(x) for x in fix.quaternions[k, :4]]), (ctypes.c_float * 3)(*[float(x) for x in fix.quaternions[k, 4:]]))
        scene.keyframes.append(bso.HostKeyframe(np.array(kf["depth"]), np.array(kf["normals"]), np.zeros(kf["depth"].shape, np.uint16),
                                                np.array(kf["rgba"]), pose, kf_id=k))
    scene.surfels[:8, :N_SURFELS] = fix.surfels
    scene.active[0, :N_SURFELS] = fix.active
    scene.surfels_size = N_SURFELS
    return scene


@functools.lru_cache(maxsize=None)
def hard_inputs(case):
    """Inputs of a case, with the matrices of the scene's keyframe views"""
    fix, scene = hard_fixture(case), host_scene(case)
    keyframes = []
    for kf, host in zip(fix.keyframes, scene.keyframes):
        view = host.view()
        keyframes.append(dict(kf, M=np.array(view.frame_T_global.m, np.float32), R=np.array(view.global_R_frame.m, np.float32)))
    return Inputs(fix.surfels, fix.active, keyframes, fix.cameras, BASELINE_FX, RAW_TO_FLOAT_DEPTH, fix.a, fix.cfactor, CELL)


@functools.lru_cache(maxsize=None)
def hard_terms(case, use_depth, use_desc, tex_mode, dtype_name="float64"):
    return surfel_terms(hard_inputs(case), bool(use_depth), bool(use_desc), tex_mode, np.dtype(dtype_name))


@functools.lru_cache(maxsize=None)
def hard_geometry(case, use_depth, use_desc, tex_mode, dtype_name="float64"):
    return geometry_terms(hard_inputs(case), bool(use_depth), bool(use_desc), tex_mode, np.dtype(dtype_name))


def scene_copy(case, use_depth, use_desc, tex_mode):
    """A HostScene of the case with surfel rows and flags of its own (the geometry entry points write them)"""
    from tests import bso
    base = host_scene(case)
    scene = bso.HostScene(base.color_camera, base.depth_camera, RAW_TO_FLOAT_DEPTH, BASELINE_FX, CELL, base.max_surfels, bool(use_depth), bool(use_desc), tex_mode)
    scene.cfactor[:], scene.a, scene.keyframes = base.cfactor, base.a, base.keyframes
    scene.surfels[:], scene.active[:], scene.surfels_size = base.surfels, base.active, base.surfels_size
    return scene


def measure_c():
    """{kind: the largest |value32 - value64| / (2^-24 A)} over the decided pairs and surfels of all cases (exact texture mode: the
    fixed-point mode's flips are widening, not rounding)"""
    def ratio(d, A, mask):
        with np.errstate(invalid="ignore", divide="ignore"):
            return float(np.nanmax(np.where(mask & (A > 0), np.abs(d) / (EPS32 * np.where(A > 0, A, 1)), 0)))
    out = {kind: 0.0 for kind in C_MEASURED}
    for case in CASES:
        for kind, (use_depth, use_desc) in (("depth", (1, 0)), ("desc", (0, 1))):
            t64, t32 = hard_terms(case, use_depth, use_desc, TEX_EXACT_FLOAT), hard_terms(case, use_depth, use_desc, TEX_EXACT_FLOAT, "float32")
            decided = ~(t64.ambiguous | t32.ambiguous)
            assert np.array_equal(t64.stage[decided], t32.stage[decided]), (case, kind)
            out[kind] = max(out[kind], ratio(t32.row.astype(np.float64) - t64.row, t64.A, decided[..., None]))
        for use_depth, use_desc in ((1, 0), (1, 1), (0, 1)):
            g64, g32 = hard_geometry(case, use_depth, use_desc, TEX_EXACT_FLOAT), hard_geometry(case, use_depth, use_desc, TEX_EXACT_FLOAT, "float32")
            decided = ~(g64.ambiguous | g32.ambiguous) & g64.on
            assert np.array_equal(g64.code[decided], g32.code[decided]), (case, use_depth, use_desc)
            out["normals"] = max(out["normals"], ratio(g32.mean.astype(np.float64) - g64.mean, g64.A_mean, (decided & g64.updated)[:, None]))
            if use_desc:
                out["joint"] = max(out["joint"], ratio(g32.x.astype(np.float64) - g64.x, g64.A_x, decided[:, None] & g64.moved3 & g32.moved3))
            else:
                out["position"] = max(out["position"], ratio(g32.step.astype(np.float64) - g64.step, g64.A_step, decided & g64.moved & g32.moved))
    return out


def geometry_step_tolerances(g, old, kind):
    """how far a stored fp32 result may lie from the float64 step: 4 C 2^-24 A of the step, and the rounding of the stored number
    itself (a position component next to `old`, which is what limits a step of millimetres on coordinates of metres)"""
    if kind == "position":
        return KERNEL_FACTOR * C_MEASURED["position"] * EPS32 * g.A_step
    return KERNEL_FACTOR * C_MEASURED["joint"] * EPS32 * g.A_x + g.widen_x


def check_geometry(g, before, after, use_desc, label):
    """The checks both the oracle and the kernels must pass: before / after = surfel rows [8, N].  Returns the failures."""
    failures = []
    N = len(g.code)
    bits = lambda rows: np.ascontiguousarray(rows[:8, :N]).view(np.uint32)
    b, a = bits(before), bits(after)
    decided = ~g.ambiguous
    wrong_code = ~g.normal_ambiguous & (a[ROW_NORMAL] != g.code)
    if wrong_code.any():
        failures.append((label, "normal code", int(wrong_code.sum()), np.nonzero(wrong_code)[0][:5].tolist()))
    for row in (ROW_RADIUS_SQUARED, ROW_COLOR):
        if not np.array_equal(a[row], b[row]):
            failures.append((label, "row written", row))
    moved = g.moved3[:, 0] if use_desc else g.moved
    undecided = g.guard_undecided if use_desc else np.zeros((N, 3), bool)
    keeps = decided & ~(g.updated | moved | (g.moved3[:, 1:].any(1) if use_desc else False)) & ~undecided.any(1)
    changed = keeps & (a != b).any(0)
    if changed.any():
        failures.append((label, "a surfel that keeps its rows changed", int(changed.sum()), np.nonzero(changed)[0][:5].tolist()))
    n = np.stack([c.v for c in unpack_surfel_normal(g.code, np.float64)], 1)
    old, new = before[:3, :N].T.astype(np.float64), after[:3, :N].T.astype(np.float64)
    with np.errstate(invalid="ignore"):
        move = new - old
        along = (move * n).sum(1)
        across = np.linalg.norm(move - along[:, None] * n, axis=1)
        stored = EPS32 * (np.abs(n) * np.maximum(np.abs(old), np.abs(new))).sum(1)          # half an ulp per stored component
        want = -g.x[:, 0] if use_desc else g.step
        allowed = (geometry_step_tolerances(g, old, "joint")[:, 0] if use_desc else geometry_step_tolerances(g, old, "position")) + 2 * stored
        pick = decided & moved
        bad = pick & ~(np.abs(along - want) <= allowed)
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            failures.append((label, "step along the normal", int(bad.sum()), i, float(along[i]), float(want[i]), float(allowed[i])))
        bad = pick & ~(across <= 4 * EPS32 * np.linalg.norm(np.maximum(np.abs(old), np.abs(new)), axis=1) + 4 * EPS32 * np.abs(want))
        if bad.any():
            failures.append((label, "move across the normal", int(bad.sum()), int(np.nonzero(bad)[0][0])))
        still = decided & ~moved & ~undecided[:, 0] & (a[:3] != b[:3]).any(0)
        if still.any():
            failures.append((label, "position written behind a closed guard", int(still.sum())))
    if use_desc:
        tol = geometry_step_tolerances(g, old, "joint")
        for i, row in ((0, ROW_D1), (1, ROW_D2)):
            d_old, d_new = before[row, :N].astype(np.float64), after[row, :N].astype(np.float64)
            pick = decided & g.moved3[:, 1 + i]
            allowed = tol[:, 1 + i] + EPS32 * (np.abs(d_old) + np.abs(g.new_d[:, i]))
            bad = pick & ~(np.abs(d_new - g.new_d[:, i]) <= allowed)
            if bad.any():
                j = int(np.nonzero(bad)[0][0])
                failures.append((label, "descriptor %d" % (i + 1), int(bad.sum()), j, float(d_new[j]), float(g.new_d[j, i]), float(allowed[j])))
            sure = pick & g.clamped[:, i] & (np.abs(np.abs(g.unclamped[:, i]) - 180) > allowed)
            if not (np.abs(d_new[sure]) == 180).all() or not np.array_equal(np.sign(d_new[sure]), np.sign(g.unclamped[sure, i])):
                failures.append((label, "clamped descriptors are exactly +-180", i))
            if not (np.abs(d_new[np.isfinite(d_new)]) <= 180).all() and not (np.abs(d_old[np.abs(d_new) > 180]) > 180).all():
                failures.append((label, "descriptor beyond the clamp", i))
            still = decided & ~g.moved3[:, 1 + i] & ~undecided[:, 1 + i] & (a[row] != b[row])
            if still.any():
                failures.append((label, "descriptor written behind a closed guard", i, int(still.sum())))
    else:
        if not np.array_equal(a[ROW_D1:], b[ROW_D1:]):
            failures.append((label, "descriptors written by the geometry-only iteration"))
    return failures


VARIANTS = ((1, 0), (0, 1), (1, 1))               # (use_depth, use_desc)


def variant_name(use_depth, use_desc):
    return "both" if use_depth and use_desc else "depth" if use_depth else "desc"
