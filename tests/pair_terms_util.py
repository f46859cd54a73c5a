"""A plain NumPy restatement of pair_accumulate_kernel (csrc/odometry_kernels.hpp), one image pair at a time and pixel by pixel,
and the deterministic "hard" inputs the per-pixel tests run on.  Nothing here calls the library or the oracle.

`pair_terms(...)` is written from the formulas of the operation (BS/kernel_opt_pose.cu, BS/cost_function.cuh,
BS/surfel_projection*.cuh), generic in the dtype (np.float64: the reference; np.float32: the same formulas in the kernel's
precision, used only to MEASURE how far plain fp32 strays from float64).  No fused multiply-adds are imitated and every division
is NumPy's correctly rounded one.

Every number is carried as a pair (value, scale): `V.v` is the value and `V.a` the same expression evaluated with absolute
values, to first order: |x| + |y| for x +- y, and for a product, a quotient or a square root the scales of the operands
carried through the operation's derivative -- a(x y) = |x| a(y) + |y| a(x) - |x y|, which IS |x| |y| evaluated on the absolute
values whenever one of the two factors is free of cancellation (a = |.|), and which grows by the sum, not the product, of the
two amplifications where both carry some (q * q in the Tukey weight: squaring the scale of q there would claim an error no
rounding of q can cause, and would leave the tolerance of w a million times wider than the kernel's error).  The scale of
a row entry, `A`, is what every tolerance of the tests is taken against: 2^-24 * A is one rounding of the largest term
that entered the entry, carried to the entry.
"""
import functools

import numpy as np

ROW, COL_COST, COL_COUNT = 32, 27, 28
TEX_FIXED_POINT_1_8, TEX_EXACT_FLOAT = 0, 1            # abi.TEX_* (the tests assert that they agree)
EPS32 = 2.0 ** -24

# constants of the operation as the library holds them: fp32 numbers (BS/cost_function.cuh:44-98, BS/kernels.cuh:58)
K_DEPTH_TUKEY = np.float32(10.0)
K_DEPTH_UNCERTAINTY = np.float32(0.1)
K_COS_NORMAL_COMPAT = np.float32(0.76604)
K_DESC_WEIGHT = np.float32(1e-2)
K_DESC_HUBER = np.float32(10.0)
K_DESC_SCALE = np.float32(180.0) / np.float32(255.0)

# The stage at which a pixel leaves the kernel, in the kernel's order.  The last three are all "visible": the two after VISIBLE
# name a path the visible pixel took through the gradient code.
STAGES = ("base_depth_0", "local_z_nonpositive", "out_left", "out_top", "out_right", "out_bottom", "tracked_depth_0",
          "depth_far", "depth_near", "back_facing", "normal_incompatible",
          "desc_last_column_or_row", "desc_sample_outside", "desc_sample_z_nonpositive", "desc_d2c_centre", "desc_d2c_sample1",
          "desc_d2c_sample2", "gradmag_d2c",
          "visible", "visible_desc_border_gradient", "visible_gradmag_footprint_clamped")
S = {name: i for i, name in enumerate(STAGES)}
FIRST_VISIBLE = S["visible"]
COMMON_STAGES = STAGES[:11] + ("visible",)
DESC_STAGES = STAGES[11:17] + ("visible_desc_border_gradient",)
GRADMAG_STAGES = ("gradmag_d2c", "visible_gradmag_footprint_clamped")


def coordinate_margin(w, h):
    """How close to an integer a projected coordinate may lie before a truncation of it is not decided by the inputs alone:
    16 spacings of fp32 at the image's larger side (1.2e-4 px up to 128)."""
    return 16.0 * float(np.spacing(np.float32(max(w, h))))


class V:
    """value and absolute-value scale, elementwise (see the module's docstring)"""
    __slots__ = ("v", "a")
    __array_ufunc__ = None                     # NumPy operands defer to the reflected operators below

    def __init__(self, v, a=None):
        self.v = v
        self.a = np.abs(v) if a is None else a

    @staticmethod
    def of(o, like):
        return o if isinstance(o, V) else V(np.asarray(o, dtype=like.v.dtype))

    def __add__(self, o):
        o = V.of(o, self)
        return V(self.v + o.v, self.a + o.a)
    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o, self)
        return V(self.v - o.v, self.a + o.a)

    def __rsub__(self, o):
        return V.of(o, self) - self

    def __mul__(self, o):
        o = V.of(o, self)
        return V(self.v * o.v, np.abs(self.v) * o.a + np.abs(o.v) * self.a - np.abs(self.v * o.v))
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o, self)
        return V(self.v / o.v, self.a / np.abs(o.v) + np.abs(self.v) * o.a / (o.v * o.v) - np.abs(self.v / o.v))

    def __rtruediv__(self, o):
        return V.of(o, self) / self

    def __neg__(self):
        return V(-self.v, self.a)

    def abs(self):
        return V(np.abs(self.v), self.a)

    def sqrt_clamped(self):
        """sqrt(max(s, 0)); at s <= 0 the scale is sqrt of the scale (a value this close to 0 has no relative accuracy)"""
        s = np.maximum(self.v, 0)
        root = np.sqrt(s)
        return V(root, np.where(s > 0, 0.5 * self.a / np.where(s > 0, root, 1) + 0.5 * root, np.sqrt(self.a)))

    def where(self, mask, other):
        other = V.of(other, self)
        return V(np.where(mask, self.v, other.v), np.where(mask, self.a, other.a))


def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def near_integer(v, margin):
    return np.abs(v - np.rint(v)) < margin


def decode_normal(code, dtype):
    """U16ToImageSpaceNormal BS/util.cuh:107-130: two signed bytes / 127, z = -sqrt(1 - x^2 - y^2)"""
    code = code.astype(np.uint16)
    x = V((code & 0xff).astype(np.uint8).view(np.int8).astype(dtype)) / dtype(127)
    y = V((code >> 8).astype(np.uint8).view(np.int8).astype(dtype)) / dtype(127)
    return [x, y, -((dtype(1) - x * x - y * y).sqrt_clamped())]


class Texture:
    """A single-channel u8 image behind the reference's texture: clamp addressing, pixel-corner coordinates (the texel centres lie
    at i + 0.5), bilinear filtering.  Values and gradients are in byte units."""

    def __init__(self, image, tex_mode, dtype):
        self.image, self.tex_mode, self.dtype = image, tex_mode, dtype
        self.h, self.w = image.shape

    def texel(self, ix, iy):
        return V(self.image[np.clip(iy, 0, self.h - 1), np.clip(ix, 0, self.w - 1)].astype(self.dtype))

    def quad(self, i, j):
        return self.texel(i, j), self.texel(i + 1, j), self.texel(i, j + 1), self.texel(i + 1, j + 1)

    def value(self, x, y, margin):
        """tex_footprint / tex_u8_direct: the filtered value at (x, y), how far it may jump in the fixed-point mode when a filter
        weight sits on a rounding boundary of the 1/256 grid (0 where none does), whether the footprint's base texel lies outside
        [0, w - 2] x [0, h - 2], and whether x - 0.5 or y - 0.5 is within the margin of an integer (the footprint is undecided)."""
        dtype = self.dtype
        xb, yb = x - dtype(0.5), y - dtype(0.5)
        with np.errstate(invalid="ignore"):
            fx, fy = np.floor(xb.v), np.floor(yb.v)
        ua, ub = xb - fx, yb - fy
        fx, fy = np.nan_to_num(fx, nan=0.0, posinf=1e9, neginf=-1e9), np.nan_to_num(fy, nan=0.0, posinf=1e9, neginf=-1e9)
        i = np.clip(fx, -1, self.w - 1).astype(np.int64)
        j = np.clip(fy, -1, self.h - 1).astype(np.int64)
        tl, tr, bl, br = self.quad(i, j)
        a, b = ua, ub
        jump = np.zeros(xb.v.shape)
        if self.tex_mode == TEX_FIXED_POINT_1_8:
            dtop, dleft, dmix = np.abs(tr.v - tl.v), np.abs(bl.v - tl.v), np.abs((br.v - bl.v) - (tr.v - tl.v))
            step = (dtop + dleft + dmix).astype(np.float64) / 256
            for frac in (ua, ub):
                jump = jump + np.where(near_integer(frac.v * dtype(256) + dtype(0.5), margin * 256), step, 0.0)
            a = V(np.floor(ua.v * dtype(256) + dtype(0.5)) / dtype(256))      # a number of the 1/256 grid: exact
            b = V(np.floor(ub.v * dtype(256) + dtype(0.5)) / dtype(256))
        one = dtype(1)
        value = (one - a) * (one - b) * tl + a * (one - b) * tr + (one - a) * b * bl + a * b * br
        border = (i < 0) | (i > self.w - 2) | (j < 0) | (j > self.h - 2)
        undecided = near_integer(xb.v, margin) | near_integer(yb.v, margin)
        return value, jump, border, undecided

    def gradient(self, x, y):
        """grad_footprint / grad_filter (BS/cost_function.cuh:200-239): d value / d x, d value / d y at (x, y) with unquantised
        weights, and whether anything of the footprint was clamped."""
        dtype = self.dtype
        xb, yb = x - dtype(0.5), y - dtype(0.5)
        with np.errstate(invalid="ignore"):
            ix = np.nan_to_num(np.trunc(np.maximum(xb.v, 0)), nan=0.0, posinf=1e9).astype(np.int64)
            iy = np.nan_to_num(np.trunc(np.maximum(yb.v, 0)), nan=0.0, posinf=1e9).astype(np.int64)
        tx, ty = xb - ix.astype(dtype), yb - iy.astype(dtype)
        lo_x, lo_y, hi_x, hi_y = tx.v < 0, ty.v < 0, tx.v > 1, ty.v > 1
        tx = tx.where(~lo_x, dtype(0)).where(~hi_x, dtype(1))
        ty = ty.where(~lo_y, dtype(0)).where(~hi_y, dtype(1))
        clamped = lo_x | lo_y | hi_x | hi_y | (ix + 1 > self.w - 1) | (iy + 1 > self.h - 1)
        tl, tr, bl, br = self.quad(np.minimum(ix, self.w - 1), np.minimum(iy, self.h - 1))
        one = dtype(1)
        gx = (br - bl) * ty + (tr - tl) * (one - ty)
        gy = (br - tr) * tx + (bl - tl) * (one - tx)
        return gx, gy, clamped


def tukey(r, k, dtype):
    """BS/robust_weighting.cuh: weight (1 - (r/k)^2)^2 inside k, 0 outside; cost k^2/6 (1 - (1 - (r/k)^2)^3) inside, k^2/6 outside"""
    inside = np.abs(r.v) < k.v
    q = r / k
    t = dtype(1) - q * q
    sixth = k * k / dtype(6)
    return (t * t).where(inside, dtype(0)), (sixth * (dtype(1) - t * t * t)).where(inside, sixth)


def huber(r, k, dtype):
    """weight 1 inside k, k / |r| outside; cost r^2 / 2 inside, k (|r| - k / 2) outside"""
    inside = np.abs(r.v) < k.v
    with np.errstate(divide="ignore", invalid="ignore"):
        outer_w = k / r.abs()
    return V(np.ones_like(r.v)).where(inside, outer_w), (dtype(0.5) * r * r).where(inside, k * (r.abs() - dtype(0.5) * k))


def depth_jacobian(inv_stddev, n, lu):
    """BS/kernel_opt_pose.cu:45-94"""
    return [inv_stddev * n[0], inv_stddev * n[1], inv_stddev * n[2],
            inv_stddev * (n[2] * lu[1] - n[1] * lu[2]), inv_stddev * (n[0] * lu[2] - n[2] * lu[0]), inv_stddev * (n[1] * lu[0] - n[0] * lu[1])]


def colour_jacobian(gx, gy, ls):
    """BS/kernel_opt_pose.cu:122-141: gx, gy = d r / d (colour pixel) times the colour camera's fx, fy"""
    x, y, z = ls
    zz = z * z
    return [-(gx / z), -(gy / z), (x * gx + y * gy) / zz, ((y * y + zz) * gy + x * y * gx) / zz, -(((x * x + zz) * gx + x * y * gy) / zz),
            -((x * gy - y * gx) / z)]


def assemble_rows(terms, visible, shape, dtype):
    """terms: [(r, J[6], weight, cost)] as V -> the coefficient row and the cost row of every pixel, as V [h, w, 32]: H 0..20
    (upper triangle, row-major), b 21..26, cost 27, count 28; zero where the pixel is not visible."""
    zero = V(np.zeros(shape, dtype))
    coeffs, cost = [zero] * ROW, [zero] * ROW
    for r, J, w, c in terms:
        idx = 0
        for i in range(6):
            for j in range(i, 6):
                coeffs[idx] = coeffs[idx] + w * J[i] * J[j]
                idx += 1
        for i in range(6):
            coeffs[21 + i] = coeffs[21 + i] + w * r * J[i]
        cost[COL_COST] = cost[COL_COST] + c
    coeffs[COL_COUNT] = V(np.ones(shape, dtype))
    cost[COL_COUNT] = V(np.full(shape, len(terms), dtype))
    out = []
    for row in (coeffs, cost):
        with np.errstate(invalid="ignore"):
            v = np.stack([np.where(visible, np.broadcast_to(e.v, shape), 0) for e in row], -1)
            a = np.stack([np.where(visible, np.broadcast_to(e.a, shape), 0) for e in row], -1)
        out.append(V(v, a))
    return out


class PairTerms:
    """What pair_terms returns; every array is per base pixel [h, w, ...] in the dtype asked for.
    stage: index into STAGES; visible: stage >= FIRST_VISIBLE; ambiguous: a discrete decision of this pixel lies within its margin.
    terms: {"depth" | "desc1" | "desc2" | "gradmag": {"r", "A_r" (its scale), "J" [.., 6], "w", "cost"}} (values; garbage where not visible).
    coeffs, cost: the pixel's 32-column row in the two output kinds; A_coeffs, A_cost: the same rows evaluated with absolute
    values; widen_coeffs, widen_cost: what a flip of a quantised filter weight (fixed-point texture mode) may add on top.
    A_by_kind: {"depth" | "desc" | "gradmag": (A_coeffs, A_cost) of that kind's residuals alone}.
    aux: intermediate values of the visible pixels for tests that re-derive a residual on their own."""

    def row(self, coeffs):
        return (self.coeffs, self.A_coeffs, self.widen_coeffs) if coeffs else (self.cost, self.A_cost, self.widen_cost)


def pair_terms(images, cameras, M, baseline_fx, threshold_factor, use_depth, use_desc, gradmag, tex_mode, dtype):
    """images: {"base_depth" f32, "base_normals" u16, "base_color" u8 (depth-sized); "depth" f32, "normals" u16 (tracked frame,
    depth-sized), "color" u8 (tracked frame, colour-sized)}; cameras: (colour, depth), each (fx, fy, cx, cy, width, height) with
    the projection's pixel-corner convention; M: frame_T_base, 12 numbers row-major; everything is taken as the fp32 numbers
    the library receives and promoted to `dtype`."""
    assert use_depth or use_desc
    dtype = np.dtype(dtype).type
    f = lambda value: dtype(np.float32(value))
    (cfx, cfy, ccx, ccy, cw, ch), (fx, fy, cx, cy, w, h) = cameras
    cfx, cfy, ccx, ccy, fx, fy, cx, cy = (V(f(v)) for v in (cfx, cfy, ccx, ccy, fx, fy, cx, cy))
    M = [V(f(v)) for v in np.asarray(M).reshape(12)]
    bfx, thr = V(f(baseline_fx)), V(f(threshold_factor))
    half, one = dtype(0.5), dtype(1)
    margin = coordinate_margin(w, h)
    shape = (h, w)
    ys, xs = np.mgrid[0:h, 0:w]
    out = PairTerms()
    stage = np.full(shape, S["visible"], np.int64)
    alive = np.ones(shape, bool)
    ambiguous = np.zeros(shape, bool)

    def leave(mask, name):
        nonlocal alive
        stage[alive & mask] = S[name]
        alive = alive & ~mask

    def transform(p):
        return [M[4 * i] * p[0] + M[4 * i + 1] * p[1] + M[4 * i + 2] * p[2] + M[4 * i + 3] for i in range(3)]

    def rotate(p):
        return [M[4 * i] * p[0] + M[4 * i + 1] * p[1] + M[4 * i + 2] * p[2] for i in range(3)]

    # PixelCenterUnprojector (BS/surfel_projection.h:42-124): the ray through the centre of pixel (x, y)
    ray_x = lambda x: (V(np.asarray(x).astype(dtype)) - (cx - half)) / fx
    ray_y = lambda y: (V(np.asarray(y).astype(dtype)) - (cy - half)) / fy
    unproject = lambda x, y, depth: [depth * ray_x(x), depth * ray_y(y), depth]
    project = lambda p: (fx * (p[0] / p[2]) + cx, fy * (p[1] / p[2]) + cy)     # pixel-corner projector

    def outside(p, width, height):
        with np.errstate(invalid="ignore"):
            return p[0].v < 0, p[1].v < 0, np.trunc(p[0].v) >= width, np.trunc(p[1].v) >= height

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        depth = V(images["base_depth"].astype(dtype))
        leave(~(depth.v > 0), "base_depth_0")
        nx, ny = ray_x(xs), ray_y(ys)
        local = transform([depth * nx, depth * ny, depth])
        leave(~(local[2].v > 0), "local_z_nonpositive")
        pxy = project(local)
        ambiguous |= alive & (near_integer(pxy[0].v, margin) | near_integer(pxy[1].v, margin))
        for side, name in zip(outside(pxy, w, h), ("out_left", "out_top", "out_right", "out_bottom")):
            leave(side, name)
        px = np.clip(np.nan_to_num(np.trunc(pxy[0].v), nan=0.0, posinf=0.0, neginf=0.0), 0, w - 1).astype(np.int64)
        py = np.clip(np.nan_to_num(np.trunc(pxy[1].v), nan=0.0, posinf=0.0, neginf=0.0), 0, h - 1).astype(np.int64)
        pixel_depth = V(images["depth"][py, px].astype(dtype))
        leave(~(pixel_depth.v > 0), "tracked_depth_0")
        # IsAssociatedWithPixel BS/surfel_projection_nvcc_only.cuh:168-215
        base_normal = decode_normal(images["base_normals"], dtype)
        n_local = rotate(base_normal)
        tnx, tny = ray_x(px), ray_y(py)
        slant = (n_local[0] * tnx + n_local[1] * tny + n_local[2]).abs()
        variance_part = V(dtype(K_DEPTH_UNCERTAINTY)) * slant * pixel_depth * pixel_depth
        stddev = variance_part / bfx
        k_depth = thr * dtype(K_DEPTH_TUKEY)
        difference, bound = local[2] - pixel_depth, k_depth * stddev
        ambiguous |= alive & (np.abs(np.abs(difference.v) - bound.v) <= 1e-5 * bound.v)
        leave(difference.v > bound.v, "depth_far")
        leave(-difference.v > bound.v, "depth_near")
        facing = dot3(local, n_local)
        ambiguous |= alive & (np.abs(facing.v) <= 1e-5 * facing.a)
        leave(facing.v > 0, "back_facing")
        compat = dot3(n_local, decode_normal(images["normals"][py, px], dtype))
        ambiguous |= alive & (np.abs(compat.v - dtype(K_COS_NORMAL_COMPAT)) <= 1e-5 * float(K_COS_NORMAL_COMPAT))
        leave(compat.v < dtype(K_COS_NORMAL_COMPAT), "normal_incompatible")

        terms, names, jumps = [], [], []
        aux = {"local": local, "n_local": n_local, "px": px, "py": py, "pxy": pxy}
        if use_depth:                                                   # BS/cost_function.cuh:56-98
            inv_stddev = bfx / variance_part
            lu = [pixel_depth * tnx, pixel_depth * tny, pixel_depth]
            raw = inv_stddev * dot3(n_local, [lu[i] - local[i] for i in range(3)])
            weight, cost = tukey(raw, k_depth, dtype)
            terms.append((raw, depth_jacobian(inv_stddev, n_local, lu), weight, cost))
            names.append("depth")
            jumps.append(np.zeros(shape))
            aux.update(inv_stddev=inv_stddev, lu=lu)

        # DepthToColorPixelCorner BS/surfel_projection.cuh:196-207
        d2c_fx, d2c_fy = cfx / fx, cfy / fy
        d2c_cx, d2c_cy = -(cfx * cx / fx) + ccx, -(cfy * cy / fy) + ccy
        to_colour = lambda p: (d2c_fx * p[0] + d2c_cx, d2c_fy * p[1] + d2c_cy)
        texture = Texture(images["color"], tex_mode, dtype)
        desc_weight = thr * dtype(K_DESC_WEIGHT)
        k_huber = V(dtype(K_DESC_HUBER))
        base_color = lambda x, y: V(images["base_color"][np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(dtype))

        def colour_term(name, r, gx, gy, jump):
            ambiguous_r = np.abs(np.abs(r.v) - dtype(K_DESC_HUBER)) <= 1e-5
            weight, cost = huber(r, k_huber, dtype)
            terms.append((r, colour_jacobian(gx * cfx, gy * cfy, local), desc_weight * weight, desc_weight * cost))
            names.append(name)
            jumps.append(jump)
            return ambiguous_r

        if use_desc and gradmag:                                        # BS/cost_function.cuh:324-352
            cp = to_colour(pxy)
            ambiguous |= alive & (near_integer(cp[0].v, margin) | near_integer(cp[1].v, margin))
            leave(np.logical_or.reduce(outside(cp, cw, ch)), "gradmag_d2c")
            value, jump, _, undecided = texture.value(cp[0], cp[1], margin)
            gx, gy, clamped = texture.gradient(cp[0], cp[1])
            r = value - base_color(xs, ys)
            ambiguous |= alive & (undecided | colour_term("gradmag", r, gx, gy, jump))
            stage[alive & clamped] = S["visible_gradmag_footprint_clamped"]
            aux.update(cp=[cp])
        elif use_desc:                                                  # BS/kernel_opt_pose.cu:939-1171, BS/cost_function.cuh:115-239
            leave((xs >= w - 1) | (ys >= h - 1), "desc_last_column_or_row")
            intensity = lambda x, y: base_color(x, y) / dtype(255)
            d1 = dtype(180) * (intensity(xs + 1, ys) - intensity(xs, ys))
            d2 = dtype(180) * (intensity(xs, ys + 1) - intensity(xs, ys))
            plane_d = dot3([nx * depth, ny * depth, depth], base_normal)
            samples = []
            for sx, sy in ((xs + 1, ys), (xs, ys + 1)):                 # the neighbour pixels' rays, cut with the base pixel's tangent plane
                sample_depth = plane_d / (ray_x(sx) * base_normal[0] + ray_y(sy) * base_normal[1] + base_normal[2])
                samples.append(transform(unproject(sx, sy, sample_depth)))
            sample_pxy = [project(p) for p in samples]
            for p in sample_pxy:
                ambiguous |= alive & (near_integer(p[0].v, margin) | near_integer(p[1].v, margin))
            leave(np.logical_or.reduce(outside(sample_pxy[0], w, h) + outside(sample_pxy[1], w, h)), "desc_sample_outside")
            leave(~(samples[0][2].v > 0) | ~(samples[1][2].v > 0), "desc_sample_z_nonpositive")
            cps = [to_colour(p) for p in [pxy] + sample_pxy]
            for cp, name in zip(cps, ("desc_d2c_centre", "desc_d2c_sample1", "desc_d2c_sample2")):
                ambiguous |= alive & (near_integer(cp[0].v, margin) | near_integer(cp[1].v, margin))
                leave(np.logical_or.reduce(outside(cp, cw, ch)), name)
            sampled = [texture.value(cp[0], cp[1], margin) for cp in cps]
            gradients = [texture.gradient(cp[0], cp[1]) for cp in cps]
            scale = V(dtype(K_DESC_SCALE))
            for k, name, d in ((1, "desc1", d1), (2, "desc2", d2)):
                r = scale * (sampled[k][0] - sampled[0][0]) - d
                gx, gy = scale * (gradients[k][0] - gradients[0][0]), scale * (gradients[k][1] - gradients[0][1])
                ambiguous |= alive & colour_term(name, r, gx, gy, float(K_DESC_SCALE) * (sampled[k][1] + sampled[0][1]))
            ambiguous |= alive & (sampled[0][3] | sampled[1][3] | sampled[2][3])
            stage[alive & (sampled[0][2] | sampled[1][2] | sampled[2][2])] = S["visible_desc_border_gradient"]
            aux.update(cp=cps, d=[d1, d2])

        visible = alive
        rows = assemble_rows(terms, visible, shape, dtype)
        out.coeffs, out.A_coeffs = rows[0].v, rows[0].a.astype(np.float64)
        out.cost, out.A_cost = rows[1].v, rows[1].a.astype(np.float64)
        # the scales of each residual kind's share of the rows (they add up to A, but for the count column, which is exact)
        out.A_by_kind = {}
        for kind in ("depth", "desc", "gradmag"):
            share = [term for name, term in zip(names, terms) if name.rstrip("12") == kind]
            if share:
                part = assemble_rows(share, visible, shape, dtype)
                out.A_by_kind[kind] = (part[0].a.astype(np.float64), part[1].a.astype(np.float64))
        # fixed-point texture mode: a filter weight on a rounding boundary may land on either side; the residual moves by up to
        # `jump`, and the row by what that does through the weight and J
        widen = [np.zeros(shape + (ROW,)), np.zeros(shape + (ROW,))]
        moving = [i for i, jump in enumerate(jumps) if np.any(jump[visible] > 0)]
        if moving:
            for signs in np.ndindex(*(2,) * len(moving)):
                moved = list(terms)
                for sign, i in zip(signs, moving):
                    r, J, _, _ = terms[i]
                    r = V((r.v.astype(np.float64) + (2 * sign - 1) * jumps[i]).astype(dtype))
                    weight, cost = huber(r, k_huber, dtype)
                    moved[i] = (r, J, desc_weight * weight, desc_weight * cost)
                for kind, row in enumerate(assemble_rows(moved, visible, shape, dtype)):
                    widen[kind] = np.maximum(widen[kind], np.abs(row.v.astype(np.float64) - rows[kind].v.astype(np.float64)))
        out.widen_coeffs, out.widen_cost = widen

    out.stage, out.visible, out.ambiguous = stage, stage >= FIRST_VISIBLE, ambiguous & (images["base_depth"] > 0)
    out.terms = {name: {"r": r.v, "A_r": r.a, "J": np.stack([j.v for j in J], -1), "w": wt.v, "cost": c.v} for name, (r, J, wt, c) in zip(names, terms)}
    out.aux = aux
    out.k_depth = float(k_depth.v)
    out.desc_weight = float(desc_weight.v)
    return out


def colour_position(cameras, p):
    """Float64, no scales: where a point p [..., 3] of the tracked frame lies in the colour image (pixel-corner projection into
    the depth image, then the depth-to-colour map), from the fp32 camera numbers."""
    (cfx, cfy, ccx, ccy, _, _), (fx, fy, cx, cy, _, _) = [[float(np.float32(v)) for v in cam] for cam in cameras]
    x, y = fx * (p[..., 0] / p[..., 2]) + cx, fy * (p[..., 1] / p[..., 2]) + cy
    return cfx / fx * x + (-(cfx * cx / fx) + ccx), cfy / fy * y + (-(cfy * cy / fy) + ccy)


def summed_row(terms, coeffs):
    """The float64 sum of the per-pixel rows, of their scales and of their widenings: what a full-image call returns."""
    row, A, widen = terms.row(coeffs)
    return (row.astype(np.float64).sum((0, 1)), A.sum((0, 1)), widen.sum((0, 1)))


# ---- the hard fixture ---------------------------------------------------------------------------------------------------
# name -> (depth size, colour size, depth camera fx fy cx cy, colour camera fx fy cx cy, threshold factor)
HARD_SHAPES = {
    "20x12": ((20, 12), (20, 12), (40.0, 40.0, 10.0, 6.0), (40.0, 40.0, 10.0, 6.0), 4.0),
    "37x23": ((37, 23), (37, 23), (45.0, 44.0, 18.2, 11.7), (45.0, 44.0, 18.2, 11.7), 2.0),
    # a colour camera that is no clean scaling of the depth camera: the right and the bottom of the depth image map outside it
    "37x23_color19x12": ((37, 23), (19, 12), (45.0, 44.0, 18.2, 11.7), (23.5, 22.1, 10.6, 7.0), 2.0),
}
HARD_BASELINE_FX = 40.0
HARD_PAIRS = 8                                   # pairs 0 and 1 go through the per-pixel tests, all eight through the batch test


def rodrigues(w):
    w = np.asarray(w, np.float64)
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) if a == 0 else np.eye(3) + np.sin(a) / a * K + (1 - np.cos(a)) / (a * a) * K @ K


def hard_cameras(shape):
    (dw, dh), (cw, ch), depth_cam, color_cam, _ = HARD_SHAPES[shape]
    return color_cam + (cw, ch), depth_cam + (dw, dh)


def encode_normal(n):
    """the u16 code of the nearest representable image-space normal (x, y as signed bytes of 127ths)"""
    q = np.clip(np.rint(np.asarray(n)[..., :2] * 127), -127, 127).astype(np.int8).view(np.uint8).astype(np.uint16)
    return q[..., 0] | (q[..., 1] << 8)


def _pick_code(ray, low, high, min_x=-1.0):
    """The normal code (a, b) with |z| >= 0.12 whose normal n has n.x >= min_x and low < ray . n < high, nearest the middle of that window."""
    a, b = np.meshgrid(np.arange(-127, 128), np.arange(-127, 128), indexing="ij")
    s = 1 - (a * a + b * b) / 127.0 ** 2
    z = -np.sqrt(np.maximum(s, 0))
    value = (a * ray[0] + b * ray[1]) / 127.0 + z * ray[2]
    score = np.where((s >= 0.12 ** 2) & (a >= 127 * min_x) & (value > low) & (value < high), np.abs(value - 0.5 * (low + high)), np.inf)
    best = np.unravel_index(np.argmin(score), score.shape)
    assert np.isfinite(score[best]), (ray, low, high)
    return int(np.array(a[best], np.int8).view(np.uint8)) | (int(np.array(b[best], np.int8).view(np.uint8)) << 8)


def _texture(u, v, phase):
    return 128 + 55 * np.sin(0.9 * u + 0.3 + phase) * np.cos(0.7 * v - 0.2) + 45 * np.sin(0.5 * (u + v) + 2 * phase)


def _pair_motion(p):
    """frame_T_base of pair p.  Pair 0 zooms in (negative t_z: the near block of base depths ends up behind the camera and
    pixels leave through all four sides) and rolls a little; pair 1 shifts towards the bottom and the left (the last column stays inside, and the
    grazing patch's normals still face the camera); the others vary both."""
    if p % 2 == 0:
        w = np.array([0.010, -0.014, 0.050]) * (1 + 0.11 * (p // 2))
        t = np.array([0.012, -0.009, -0.30 + 0.013 * (p // 2)])
    else:
        w = np.array([-0.020, -0.030, -0.020]) * (1 + 0.09 * (p // 2))
        t = np.array([-0.030, 0.040, -0.12 - 0.011 * (p // 2)])
    return np.concatenate([rodrigues(w), t[:, None]], 1).astype(np.float32).reshape(12)


def hard_inputs(shape):
    """Deterministic inputs of one hard shape: {"base_depth", "base_normals", "base_color", "depth" [P], "normals" [P], "color" [P],
    "M" [P, 12]} for HARD_PAIRS pairs, each with tracked images and a transform of its own.  The images are not a rendering of
    any scene: the tracked depth, normals and colour of pair p are written where the base pixels land under M[p], with the
    offsets that make every branch of the kernel decide something (see tests/test_pair_terms_cpu.py for the census)."""
    color_cam, depth_cam = hard_cameras(shape)
    (cfx, cfy, ccx, ccy, cw, ch), (fx, fy, cx, cy, w, h) = color_cam, depth_cam
    threshold = HARD_SHAPES[shape][4]
    ys, xs = np.mgrid[0:h, 0:w]
    rx, ry = (xs - (cx - 0.5)) / fx, (ys - (cy - 0.5)) / fy                                  # the pixel centre's ray
    # base depth: a gently curved surface around 1.6 m; a block of very near depths; scattered holes and a block of them
    base_depth = 1.6 + 0.12 * np.sin(0.31 * xs + 0.2) * np.cos(0.23 * ys) + 0.004 * xs
    near = (xs >= w // 2 + 1) & (xs < w // 2 + 5) & (ys >= 1) & (ys < 4)
    base_depth[near] = 0.05 + 0.002 * (xs + ys)[near]
    base_depth[(xs * 5 + ys * 11) % 29 == 3] = 0
    base_depth[h - 4:h - 2, 2:5] = 0
    base_depth = base_depth.astype(np.float32)
    # base normals: near the optical axis, tilted smoothly
    normal = np.stack([0.25 * np.sin(0.4 * ys + 0.1), 0.2 * np.cos(0.3 * xs), np.zeros(xs.shape)], -1)
    base_normals = encode_normal(normal)
    # a patch of normals that look away from the camera: ray . n > 0 by a clear margin
    away = (xs < 4) & (ys < 3)
    # a patch whose tangent plane passes between the pixel's ray and its right neighbour's: the first tangent sample's depth is negative
    grazing = (rx >= 0.13) & (rx <= 0.21) & (ys >= 5) & (ys < 9)
    for y, x in zip(*np.nonzero(away)):
        base_normals[y, x] = _pick_code((rx[y, x], ry[y, x], 1.0), 0.02, 0.12)
    for y, x in zip(*np.nonzero(grazing)):
        base_normals[y, x] = _pick_code((rx[y, x], ry[y, x], 1.0), -0.8 / fx, -0.2 / fx, min_x=0.9)
        a = np.array(base_normals[y, x] & 0xff, np.uint8).view(np.int8) / 127.0
        assert a > 0.9, "the grazing normals tilt towards +x, so that the right neighbour's ray lies behind the plane"
    out = {"base_depth": base_depth, "base_normals": base_normals, "depth": [], "normals": [], "color": [], "M": []}
    base_color = None
    for p in range(HARD_PAIRS):
        M = _pair_motion(p)
        geometry = pair_terms({"base_depth": base_depth, "base_normals": base_normals, "base_color": np.zeros((h, w), np.uint8),
                               "depth": np.ones((h, w), np.float32), "normals": np.zeros((h, w), np.uint16), "color": np.zeros((ch, cw), np.uint8)},
                              (color_cam, depth_cam), M, HARD_BASELINE_FX, threshold, True, False, False, TEX_EXACT_FLOAT, np.float64)
        local, n_local, px, py = [c.v for c in geometry.aux["local"]], [c.v for c in geometry.aux["n_local"]], geometry.aux["px"], geometry.aux["py"]
        lands = (base_depth > 0) & (local[2] > 0) & np.isin(geometry.stage, [S[n] for n in STAGES[6:]])
        depth, normals = np.zeros((h, w), np.float32), np.zeros((h, w), np.uint16)
        # the fraction u of the Tukey radius that the pixel's depth residual shall have: a quarter of the pixels beyond 0.5
        u = ((xs * 7 + ys * 3 + p) % 16 + 0.5) / 16.0
        u = np.where((xs + 2 * ys + p) % 4 == 0, 0.5 + 0.45 * u, 0.5 * u) * np.where((xs + ys) % 2 == 0, 1.0, -1.0)
        # a step in depth: left of it the tracked surface lies far behind the base pixel, right of it far in front
        far, nearer = (ys >= h - 5) & (xs >= w // 2 - 4) & (xs < w // 2), (ys >= h - 5) & (xs >= w // 2) & (xs < w // 2 + 4)
        u = np.where(far, -6.0, np.where(nearer, 6.0, u))
        u = np.where(grazing, 0.0, u)                       # these reach the descriptor code only at an exact depth
        k = threshold * 10.0
        for y, x in zip(*np.nonzero(lands)):
            tx, ty = (px[y, x] - (cx - 0.5)) / fx, (py[y, x] - (cy - 0.5)) / fy
            n = np.array([n_local[0][y, x], n_local[1][y, x], n_local[2][y, x]])
            slant = n @ np.array([tx, ty, 1.0])
            ls = np.array([local[0][y, x], local[1][y, x], local[2][y, x]])
            d = ls[2]
            for _ in range(3):                              # raw = (n . (d ray - ls)) / stddev(d) = u k, solved for d
                stddev = 0.1 * abs(slant) * d * d / HARD_BASELINE_FX
                d = (u[y, x] * k * stddev + n @ ls) / slant if abs(slant) > 1e-3 else ls[2]
            depth[py[y, x], px[y, x]] = d if u[y, x] != 0 else ls[2]
            normals[py[y, x], px[y, x]] = encode_normal(n)
        depth[~(depth > 0.02)] = 0                          # a solve that ran away is a hole
        # tracked normals more than 40 degrees off, over a patch; holes: scattered and a block
        normals[1:5, w - 12:w - 4] = encode_normal(np.array([0.75, 0.1, 0.0]))
        depth[(xs * 3 + ys * 7 + p) % 23 == 5] = 0
        depth[h // 2:h // 2 + 2, 1:4] = 0
        # colour: a texture given in colour pixel coordinates; the base pixel holds it where it lands, so that most residuals are
        # small; in the right third of the tracked image its phase is shifted
        cys, cxs = np.mgrid[0:ch, 0:cw]
        scale = w / cw
        phase = np.where(cxs >= (2 * cw) // 3, 1.3, 0.0)
        color = np.clip(_texture(scale * (cxs + 0.5), scale * (cys + 0.5), phase) + 0.5, 0, 255).astype(np.uint8)
        if base_color is None:                              # pair 0's landing positions; the other pairs see larger residuals
            pxy = [c.v for c in geometry.aux["pxy"]]
            u_c = (cfx / fx * (pxy[0] - cx) + ccx) * scale
            v_c = (cfy / fy * (pxy[1] - cy) + ccy) * scale
            u_c, v_c = np.where(lands, u_c, xs + 0.5), np.where(lands, v_c, ys + 0.5)
            base_color = np.clip(_texture(u_c, v_c, 0.0) + ((xs * 13 + ys * 5) % 7 - 3) + 0.5, 0, 255).astype(np.uint8)
        out["depth"].append(depth)
        out["normals"].append(normals)
        out["color"].append(color)
        out["M"].append(M)
    out["base_color"] = base_color
    for key in ("depth", "normals", "color", "M"):
        out[key] = np.stack(out[key])
    return out


def pair_images(inputs, p):
    return {"base_depth": inputs["base_depth"], "base_normals": inputs["base_normals"], "base_color": inputs["base_color"],
            "depth": inputs["depth"][p], "normals": inputs["normals"][p], "color": inputs["color"][p]}


# (use_depth, use_desc, gradmag, coeffs) of the ten variants of the four single-pair entry points
VARIANTS = [(d, s, g, c) for d, s in ((1, 0), (0, 1), (1, 1)) for g in ((False, True) if s else (False,)) for c in (True, False)]


def variant_name(use_depth, use_desc, gradmag, coeffs):
    return f"{'both' if use_depth and use_desc else 'depth' if use_depth else 'desc'}/{'coeffs' if coeffs else 'cost'}{'/gradmag' if gradmag else ''}"


# ---- what the tests share -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cached_hard_inputs(shape):
    """hard_inputs(shape), built once per process; nobody writes into it."""
    inputs = hard_inputs(shape)
    for value in inputs.values():
        value.setflags(write=False)
    return inputs


@functools.lru_cache(maxsize=None)
def hard_terms(shape, pair, use_depth, use_desc, gradmag, tex_mode, dtype_name="float64"):
    inputs = cached_hard_inputs(shape)
    return pair_terms(pair_images(inputs, pair), hard_cameras(shape), inputs["M"][pair], HARD_BASELINE_FX, HARD_SHAPES[shape][4],
                      bool(use_depth), bool(use_desc), bool(gradmag), tex_mode, np.dtype(dtype_name))


# C: the largest |row32 - row64| / (2^-24 A) over the non-ambiguous pixels of the hard fixture and all columns, row32 being
# pair_terms in np.float32 -- measured on the CPU from the reference alone (tests/test_pair_terms_cpu.py::test_measured_c
# recomputes it and fails if it grows), per residual kind.  The measured values, rounded up to two digits.
C_MEASURED = {"depth": 3.6, "desc": 0.37, "gradmag": 0.88}
KERNEL_FACTOR = 4.0                     # what the kernel's fused multiply-adds, its 1-ulp reciprocal and its own association may add


def pixel_tolerance(terms, coeffs):
    """[h, w, 32]: KERNEL_FACTOR * 2^-24 * sum over the residual kinds of the row of C[kind] * A[kind], plus the fixed-point mode's
    widening where a filter weight is undecided"""
    _, _, widen = terms.row(coeffs)
    scaled = sum(C_MEASURED[kind] * A[0 if coeffs else 1] for kind, A in terms.A_by_kind.items())
    return KERNEL_FACTOR * EPS32 * scaled + widen


# n_add: the longest chain of fp32 additions a pixel's term passes through between its lane and the returned row --
#   wave_transpose_sum32 (csrc/device_math.hpp:1130-1159): one addition in each of its six exchange steps             6
#   pose_reduce_kernel (csrc/pose_kernels.hpp:452): `v += ...` once per eighth row of the part; a part holds
#     ceil(rows / 8) rows, rows = 4 * blocks: 1 row at 20x12 (4 rows), 2 rows at 37x23 (16 rows) -> one addition    1
#   pose_reduce_kernel (csrc/pose_kernels.hpp:457): the eight sub-sums of a part                                      8
#   pose_reduce_final_kernel (csrc/pose_kernels.hpp:474): the eight parts                                             8
def n_add(width, height):
    rows = 4 * ((width * height + 255) // 256)
    per_part = (rows + 7) // 8
    return 6 + (per_part + 7) // 8 + 8 + 8


def reduction_bound(width, height, abs_sum):
    """(n_add + 1) 2^-24 sum |pixel rows|"""
    return (n_add(width, height) + 1) * EPS32 * abs_sum
