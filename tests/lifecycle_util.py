"""A plain NumPy restatement of the surfel lifecycle (csrc/lifecycle_kernels.hpp, csrc/lifecycle_abi.inc) and of activation_kernel
(csrc/geometry_kernels.hpp), one decision at a time, and the fixtures the lifecycle tests run on.  The reference calls neither the
library nor the oracle.  As in surfel_terms_util.host_scene, the fixtures do touch the oracle's binding for INPUTS: frame_T_global,
global_R_frame, global_T_frame and the covis_T_frame matrices (covis frame_T_global * global_T_frame, BS/direct_ba.cc:365-370) are
formed in fp32 by tests/bso.py and handed to the reference as the numbers the calls receive, so that it reads what the kernels
read; how covis_T_frame is composed is therefore not restated independently here.

Written from the reference project (BS/ = applications/badslam/src/badslam): surfel_projection_nvcc_only.cuh (the association of a
surfel :49-127 and of a surfel that a pixel defines :131-236, SurfelProjectsToAssociatedPixel :302-328 and its free-space form
:482-511), kernel_supporting_surfels.cu (:45-97), kernel_create_surfels.cu (the serialising kernel :41-72, CreateNewSurfel :96-161,
the observation counts :213-276, the filter :314-332, the append :357-385), kernel_delete_surfels.cu (counts :84-102, marking
:132-164), kernel_compact_surfels.cu (:97-281) and kernel_surfel_activation.cu (:38-79).  Calibrated depth, normal codes, tangent
points, the texture, the value-and-scale type V, coordinate_margin and near_integer are those of tests/surfel_terms_util.py and
tests/pair_terms_util.py (imported, not copied).  Generic in the dtype: np.float64 is the reference, np.float32 only MEASURES C.

The project fixes what the reference project leaves to a race (the top of csrc/lifecycle_kernels.hpp): the holders of a cell are its
three smallest associated surfel indices, surfels are met in index order, and the new surfel of a free cell is its first valid
pixel in raster order.

Three things the lifecycle's association does that the BA association (surfel_terms) does not: a NaN position passes the test
`z <= 0` and lands on pixel (0, 0), where every later comparison with NaN is false, so that only the normal test can refuse it; it
reads the pixel's RAW depth with the invalid bit; and its free-space form tells a violation (pixel_depth - z > 10 sigma) from "neither".

Activation (BS/kernel_surfel_activation.cu): `active &= ~flag` for every surfel (:44), then, for every ACTIVE keyframe, a surfel
whose flag is not set and that the keyframe associates gets `active = flag` (:76) -- the whole byte.  So the other bits of the byte
survive exactly where the surfel stays inactive, and an activated surfel's byte is the flag alone.  The oracle and the kernel do the
same; the reference here follows the file.

Every discrete decision carries its margin; what lies within it is `ambiguous` and left out of the comparisons (the tests bound the
share that may be).  MUTATION names one deliberate misreading of the operation; tests/test_lifecycle_cpu.py switches each on and
demands that the comparison with the oracle fails, which shows that the decision is live in the fixture.

C: the largest |value32 - value64| / (2^-24 A) over the created surfels of all fixtures, value32 being the same formulas in
np.float32 (test_lifecycle_cpu.py::test_measured_c recomputes them and fails if they grow).  Measured: position 3.28 (recorded 3.3), d1 / d2 0.18 (recorded 0.2).
"""
import copy
import ctypes
import functools

import numpy as np

from tests import surfel_terms_util as ST
from tests.pair_terms_util import (EPS32, KERNEL_FACTOR, K_COS_NORMAL_COMPAT, K_DEPTH_TUKEY, K_DEPTH_UNCERTAINTY, K_DESC_SCALE, TEX_EXACT_FLOAT,
                                   TEX_FIXED_POINT_1_8, Texture, V, coordinate_margin, decode_normal, dot3, near_integer)
from tests.surfel_terms_util import (INVALID_DEPTH_BIT, ROW_COLOR, ROW_D1, ROW_D2, ROW_NORMAL, ROW_RADIUS_SQUARED, ROW_X, ROW_Y, ROW_Z,
                                     SURFEL_ACTIVE_FLAG, calibrated_depth, pack_surfel_normal, tangent_points, unpack_surfel_normal)

INVALID_INDEX = 0xFFFFFFFF
NAN_BITS = 0x7FFFFFFF                                  # CUDART_NAN_F marks a merged or deleted surfel (BS/kernel_delete_surfels.cu:145-146)
KF_ACTIVE, KF_COVISIBLE_ACTIVE, KF_INACTIVE = 0, 1, 2  # abi.KF_* (the tests assert that they agree)
C_MEASURED = {"position": 3.3, "descriptor": 0.2}
MUTATIONS = ("holders_largest", "skip_holder_1_vs_2", "viol_ge_obs", "radius_first_keyframe", "border_0", "scan_carry", "cells_floor")
MUTATION = None                                        # one of MUTATIONS while a test shows that a decision is live


def nan_x():
    return np.array([NAN_BITS], np.uint32).view(np.float32)[0]


def is_deleted(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32) == NAN_BITS


def cells_of(w, h, cell):
    """the cell grid of an image: ((w - 1) / cell + 1, (h - 1) / cell + 1), a partial cell counting (BS/direct_ba.cc: supporting
    surfel buffers)"""
    if MUTATION == "cells_floor":
        return max(1, w // cell), max(1, h // cell)
    return (w - 1) // cell + 1, (h - 1) // cell + 1


# ---- the lifecycle association ------------------------------------------------------------------------------------------
class Association:
    """Per point [N]: associated, violation (free-space form only), px, py (the pixel, meaningless where the point left before it had
    one), ambiguous (a decision the point reached lies within its margin), margins: {name: signed distance to the decision, NaN where
    not reached}."""


def image_depth(inp, kf, dtype):
    """the calibrated depth of every pixel of a keyframe of `inp`, computed once (kept with the inputs, next to the keyframe itself)"""
    cache = inp.__dict__.setdefault("_image_depth", {})
    key = (id(kf), np.dtype(dtype).name)
    if key not in cache:
        cache[key] = (kf, calibrated_depth(kf["depth"], inp.cfactor, inp.cell, inp.a, inp.raw_to_float_depth, np.dtype(dtype).type))
    return cache[key][1]


def associate(inp, kf, M, gp, gn, free_space, dtype):
    """The point gp with normal gn (three V [N] each, in the frame that M = target_T_that_frame, 12 fp32 numbers, maps from) against the
    images of keyframe `kf`: IsAssociatedWithPixel BS/surfel_projection_nvcc_only.cuh:49-127 (= :178-236 for a point that a pixel
    defines) behind MultiplyIfResultZIsPositive and ProjectSurfelToImage (:302-328, :482-511)."""
    dtype = np.dtype(dtype).type
    f = lambda value: dtype(np.float32(value))
    fx, fy, cx, cy, w, h = inp.cameras[1]
    fx, fy, cx, cy = (V(f(v)) for v in (fx, fy, cx, cy))
    bfx, half = V(f(inp.baseline_fx)), dtype(0.5)
    margin = coordinate_margin(w, h)
    M = [V(f(v)) for v in np.asarray(M).reshape(12)]
    N = gp[0].v.shape[0]
    out = Association()
    margins = {}
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        local = [M[4 * i] * gp[0] + M[4 * i + 1] * gp[1] + M[4 * i + 2] * gp[2] + M[4 * i + 3] for i in range(3)]
        alive = ~(local[2].v <= 0)                                     # a NaN passes
        ambiguous = np.zeros(N, bool)
        pxy = (fx * (local[0] / local[2]) + cx, fy * (local[1] / local[2]) + cy)
        margins["column"], margins["row"] = pxy[0].v - np.rint(pxy[0].v), pxy[1].v - np.rint(pxy[1].v)
        near = near_integer(pxy[0].v, margin) | near_integer(pxy[1].v, margin)
        ambiguous |= alive & near
        alive &= ~((pxy[0].v < 0) | (pxy[1].v < 0) | (np.trunc(pxy[0].v) >= w) | (np.trunc(pxy[1].v) >= h))
        px = np.clip(np.nan_to_num(np.trunc(pxy[0].v), nan=0.0, posinf=0.0, neginf=0.0), 0, w - 1).astype(np.int64)   # float -> int of a NaN: 0
        py = np.clip(np.nan_to_num(np.trunc(pxy[1].v), nan=0.0, posinf=0.0, neginf=0.0), 0, h - 1).astype(np.int64)
        alive &= (kf["depth"][py, px] & INVALID_DEPTH_BIT) == 0
        depth = image_depth(inp, kf, dtype)
        pixel_depth = V(depth.v[py, px], depth.a[py, px])
        pixel_depth = pixel_depth.where(pixel_depth.v > 0, dtype(1))
        n_local = [M[4 * i] * gn[0] + M[4 * i + 1] * gn[1] + M[4 * i + 2] * gn[2] for i in range(3)]
        tnx = (V(px.astype(dtype)) - (cx - half)) / fx                 # PixelCenterUnprojector
        tny = (V(py.astype(dtype)) - (cy - half)) / fy
        slant = (n_local[0] * tnx + n_local[1] * tny + n_local[2]).abs()
        bound = V(dtype(K_DEPTH_TUKEY)) * (V(dtype(K_DEPTH_UNCERTAINTY)) * slant * pixel_depth * pixel_depth / bfx)
        difference = pixel_depth - local[2]
        margins["depth_far"], margins["depth_near"] = difference.v - bound.v, -difference.v - bound.v
        ambiguous |= alive & (np.abs(np.abs(difference.v) - bound.v) <= 1e-5 * bound.v)
        violation = alive & (difference.v > bound.v)                    # the surfel lies in front of the measured surface: free space
        alive &= ~(difference.v > bound.v) & ~(difference.v < -bound.v)
        facing = dot3(local, n_local)                                   # the sign of (1 / |local|) * dot
        margins["facing"] = np.where(facing.a > 0, facing.v / np.where(facing.a > 0, facing.a, 1), 0)
        ambiguous |= alive & (np.abs(facing.v) <= 1e-5 * facing.a)
        alive &= ~(facing.v > 0)
        compat = dot3(n_local, decode_normal(kf["normals"][py, px], dtype))
        margins["normal"] = compat.v - dtype(K_COS_NORMAL_COMPAT)
        ambiguous |= alive & (np.abs(compat.v - dtype(K_COS_NORMAL_COMPAT)) <= 1e-5 * float(K_COS_NORMAL_COMPAT))
        alive &= ~(compat.v < dtype(K_COS_NORMAL_COMPAT))
    out.associated, out.violation, out.px, out.py, out.ambiguous, out.margins = alive, violation & bool(free_space), px, py, ambiguous, margins
    out.near_column, out.near_row = near_integer(pxy[0].v, margin), near_integer(pxy[1].v, margin)
    # the pixel next door that an undecided coordinate may fall into: the one below when the coordinate lies just above an integer
    out.other_dx, out.other_dy = np.where(margins["column"] >= 0, -1, 1), np.where(margins["row"] >= 0, -1, 1)
    return out


def surfel_vectors(surfels, x, dtype):
    """position (with `x` as the first row: the state of the deletions so far) and unpacked normal of every column, as V"""
    dtype = np.dtype(dtype).type
    gp = [V(np.asarray(x).astype(dtype)), V(surfels[ROW_Y].astype(dtype)), V(surfels[ROW_Z].astype(dtype))]
    return gp, unpack_surfel_normal(surfels[ROW_NORMAL].view(np.uint32), dtype)


# ---- supporting surfels and merge ---------------------------------------------------------------------------------------
class Support:
    """cell_of [N] (INVALID_INDEX: not associated), holders [3, cells], cell_ambiguous [cells], cells_w, cells_h, association"""


def supporting_surfels(inp, k, surfels, x, dtype, drop=None):
    """DetermineSupportingSurfelsCUDAKernel BS/kernel_supporting_surfels.cu:51-63 in the project's order.  drop [N]: surfels taken as
    not associated (merge_step: the other reading of an undecided association)."""
    kf = inp.keyframes[k]
    _, _, _, _, w, h = inp.cameras[1]
    cell = inp.cell
    cells_w, cells_h = cells_of(w, h, cell)
    gp, gn = surfel_vectors(surfels, x, dtype)
    a = associate(inp, kf, kf["M"], gp, gn, False, dtype)
    s = Support()
    s.association, s.cells_w, s.cells_h = a, cells_w, cells_h
    cell_index = lambda px, py: np.minimum(py // cell, cells_h - 1) * cells_w + np.minimum(px // cell, cells_w - 1)
    associated = a.associated if drop is None else a.associated & ~drop
    s.cell_of = np.where(associated, cell_index(a.px, a.py), INVALID_INDEX).astype(np.int64)
    s.holders = np.full((3, cells_w * cells_h), INVALID_INDEX, np.int64)
    order = np.argsort(s.cell_of, kind="stable")
    order = order[s.cell_of[order] != INVALID_INDEX]
    starts = np.flatnonzero(np.r_[True, np.diff(s.cell_of[order]) != 0])[:len(order)]
    s.members = {}
    for begin, end in zip(starts, np.r_[starts[1:], len(order)]):
        members = order[begin:end]                                      # ascending: the sort is stable
        s.members[int(s.cell_of[members[0]])] = members
        pick = members[-3:][::-1] if MUTATION == "holders_largest" else members[:3]
        s.holders[:len(pick), s.cell_of[members[0]]] = pick
    # a cell is ambiguous if the association of one of its surfels is: the surfel's own cell and, where a pixel coordinate is
    # undecided, the cell of the pixel next door
    s.cell_ambiguous = np.zeros(cells_w * cells_h, bool)
    for i in np.flatnonzero(a.ambiguous):
        for dx in (0, a.other_dx[i]) if a.near_column[i] else (0,):
            for dy in (0, a.other_dy[i]) if a.near_row[i] else (0,):
                s.cell_ambiguous[cell_index(np.clip(a.px[i] + dx, 0, w - 1), np.clip(a.py[i] + dy, 0, h - 1))] = True
    return s


def merge_close(surfels, x, sup, this, cell_merge_dist_squared, dtype):
    """BS/kernel_supporting_surfels.cu:68-83 for the pairs (sup[j], this[j]) -> (close, ambiguous, the normal test alone, the distance
    test alone); all false where sup is INVALID_INDEX"""
    dtype = np.dtype(dtype).type
    there = sup != INVALID_INDEX
    sup = np.where(there, sup, 0)
    gp, gn = surfel_vectors(surfels, x, dtype)
    at = lambda vec, idx: [V(c.v[idx], c.a[idx]) for c in vec]
    with np.errstate(invalid="ignore"):
        normal_dot = dot3(at(gn, sup), at(gn, this))
        d = [a - b for a, b in zip(at(gp, sup), at(gp, this))]
        squared = dot3(d, d)
        radius = surfels[ROW_RADIUS_SQUARED].astype(dtype)
        limit = np.minimum(radius[sup], radius[this]) * dtype(np.float32(cell_merge_dist_squared))
        normal_ok = normal_dot.v > dtype(K_COS_NORMAL_COMPAT)
        near_ok = squared.v < limit                                     # false when either x is NaN: already merged away
        ambiguous = (np.abs(normal_dot.v - dtype(K_COS_NORMAL_COMPAT)) <= 1e-5) | (normal_ok & (np.abs(squared.v - limit) <= 1e-5 * np.maximum(squared.a, limit)))
    return there & normal_ok & near_ok, there & ambiguous, there & normal_ok, there & near_ok


class Merge:
    """deleted [N] (by this step, decided), ambiguous [N] (whether this step deleted it is undecided), support, rank [N] (0..2: a holder;
    3: another surfel of a cell; -1: none), close [3, N] (the test against holder b of the surfel's cell with the surfel's own position
    as it was BEFORE the step; false where the surfel never meets that holder), normal_ok / near_ok [3, N]: the two halves of that
    test, kept_by_order [N]: holder 2, close to holder 1 alone, kept because holder 1 was merged away first"""


def _merge_outcome(inp, k, surfels, x, merge_dist_factor, dtype, drop=None):
    N = len(x)
    s = supporting_surfels(inp, k, surfels, x, dtype, drop)
    cell = np.float32(inp.cell)
    cell_merge_dist_squared = cell * cell * np.float32(merge_dist_factor) * np.float32(merge_dist_factor)      # BS/kernel_supporting_surfels.cc:74-76
    idx = np.arange(N)
    has = s.cell_of != INVALID_INDEX
    own = np.where(has, s.cell_of, 0)
    holder = [np.where(has, s.holders[b, own], INVALID_INDEX) for b in range(3)]
    rank = np.where(~has, -1, np.where(holder[0] == idx, 0, np.where(holder[1] == idx, 1, np.where(holder[2] == idx, 2, 3))))
    m = Merge()
    m.support, m.rank = s, rank
    tests = [merge_close(surfels, x, np.where(rank > b, holder[b], INVALID_INDEX), idx, cell_merge_dist_squared, dtype) for b in range(3)]
    m.close, m.normal_ok, m.near_ok = (np.stack([t[j] for t in tests]) for j in (0, 2, 3))
    undecided = np.stack([t[1] for t in tests])
    # in arrival order: a surfel merged away is NaN for everyone after it
    gone, doubt = np.zeros(N, bool), np.zeros(N, bool)
    h1, h2 = s.holders[1], s.holders[2]
    c1, c2 = h1[h1 != INVALID_INDEX], h2[h2 != INVALID_INDEX]
    gone[c1], doubt[c1] = m.close[0, c1], undecided[0, c1]
    first_gone, first_doubt = np.zeros(N, bool), np.zeros(N, bool)     # per surfel: what became of its cell's holder 1
    ok = has & (holder[1] != INVALID_INDEX)
    first_gone[ok], first_doubt[ok] = gone[holder[1][ok]], doubt[holder[1][ok]]
    by_first = m.close[1] & ~first_gone
    if MUTATION == "skip_holder_1_vs_2":
        by_first = by_first & (rank != 2)
    gone[c2] = m.close[0, c2] | by_first[c2]
    doubt[c2] = undecided[0, c2] | undecided[1, c2] | (first_doubt[c2] & m.close[1, c2])
    second_gone, second_doubt = np.zeros(N, bool), np.zeros(N, bool)
    ok = has & (holder[2] != INVALID_INDEX)
    second_gone[ok], second_doubt[ok] = gone[holder[2][ok]], doubt[holder[2][ok]]
    others = rank == 3
    gone[others] = (m.close[0] | by_first | (m.close[2] & ~second_gone))[others]
    doubt[others] = (undecided.any(0) | (first_doubt & m.close[1]) | (second_doubt & m.close[2]))[others]
    m.gone, m.doubt = gone, doubt
    m.kept_by_order = (rank == 2) & ~m.close[0] & m.close[1] & first_gone
    return m


def merge_step(inp, k, surfels, x, merge_dist_factor, dtype, unknown=None):
    """One bslam_determine_supporting_surfels_and_merge: x [N] float32 is the first row as the decided deletions so far left it.
    unknown [N]: surfels of which nobody knows whether an earlier step deleted them.  Where anything is undecided -- such a surfel, an
    association within its margin -- the step is evaluated in both readings (the surfel there, or gone and, a NaN, on pixel
    (0, 0); the association made, or not); what comes out differently is ambiguous, and so is every surfel of a cell into which an
    undecided pixel coordinate may move a surfel."""
    m = _merge_outcome(inp, k, surfels, x, merge_dist_factor, dtype)
    doubt = m.doubt | m.support.association.ambiguous
    if unknown is not None:
        doubt = doubt | unknown
    if doubt.any():
        other = _merge_outcome(inp, k, surfels, np.where(unknown, nan_x(), x) if unknown is not None else x, merge_dist_factor, dtype,
                               drop=m.support.association.ambiguous)
        doubt = doubt | other.doubt | (other.gone != m.gone)
        s = m.support
        moved = s.association.ambiguous & (s.association.near_column | s.association.near_row)
        if moved.any():
            has = s.cell_of != INVALID_INDEX
            doubt = doubt | (has & _cells_next_to(s, inp, moved)[np.where(has, s.cell_of, 0)])
    m.deleted, m.ambiguous = m.gone & ~doubt, doubt
    m.count = int(m.deleted.sum())                                      # what the call takes off surfel_count, the ambiguous aside
    return m


def _cells_next_to(s, inp, which):
    """the cells a surfel of `which` may lie in when its undecided pixel coordinate falls the other way"""
    _, _, _, _, w, h = inp.cameras[1]
    a, cell = s.association, inp.cell
    out = np.zeros(s.cells_w * s.cells_h, bool)
    for i in np.flatnonzero(which):
        for dx in (0, a.other_dx[i]) if a.near_column[i] else (0,):
            for dy in (0, a.other_dy[i]) if a.near_row[i] else (0,):
                px, py = np.clip(a.px[i] + dx, 0, w - 1), np.clip(a.py[i] + dy, 0, h - 1)
                out[min(py // cell, s.cells_h - 1) * s.cells_w + min(px // cell, s.cells_w - 1)] = True
    return out


# ---- creation -----------------------------------------------------------------------------------------------------------
class Creation:
    """candidates: pixel indices (y * w + x, ascending = the order of the new columns) of the free cells' first valid pixels;
    candidate_ambiguous (the cell's occupancy is undecided); observations, violations [n] (filtered only); kept [n];
    kept_ambiguous [n] (a co-visible pair within its margin); support; columns (new_columns of the kept candidates)"""


def first_valid_pixels(depth, occupied, cell, cells_w, cells_h):
    """CreateSurfelsForKeyframeCUDASerializingKernel BS/kernel_create_surfels.cu:53-70 with raster order winning the cell: the
    first pixel of every free cell, in raster order inside the cell, that has a measurement and lies inside the 1-pixel border"""
    h, w = depth.shape
    border = 0 if MUTATION == "border_0" else 1
    ys, xs = np.mgrid[0:h, 0:w]
    valid = (xs >= border) & (ys >= border) & (xs < w - border) & (ys < h - border) & ((depth & INVALID_DEPTH_BIT) == 0)
    cx, cy = np.minimum(xs // cell, cells_w - 1), np.minimum(ys // cell, cells_h - 1)
    if MUTATION == "cells_floor":                                       # the pixels past the last whole cell have none
        valid &= (xs // cell < cells_w) & (ys // cell < cells_h)
    cell_id = cy * cells_w + cx
    valid &= ~occupied[cell_id]
    key = (ys % cell) * cell + (xs % cell)
    best = np.full(cells_w * cells_h, cell * cell, np.int64)
    np.minimum.at(best, cell_id[valid], key[valid])
    chosen = valid & (key == best[cell_id])
    return np.flatnonzero(chosen.ravel())


def new_columns(inp, k, pixels, tex_mode, dtype):
    """CreateNewSurfel BS/kernel_create_surfels.cu:96-161 for the pixels (y * w + x) of keyframe k -> dict of
    position V [n, 3] (.v, .a), normal code + ambiguous, radius bits (float32), colour bytes [n, 3] with the margin of the truncation,
    d V [n, 2], d_widen [n, 2], d_ambiguous [n]"""
    dtype = np.dtype(dtype).type
    f = lambda value: dtype(np.float32(value))
    kf = inp.keyframes[k]
    (cfx, cfy, ccx, ccy, cw, ch), (fx, fy, cx, cy, w, h) = inp.cameras
    cfx, cfy, ccx, ccy, fx, fy, cx, cy = (V(f(v)) for v in (cfx, cfy, ccx, ccy, fx, fy, cx, cy))
    half = dtype(0.5)
    y, x = pixels // w, pixels % w
    G = [V(f(v)) for v in np.asarray(kf["G"]).reshape(12)]
    M = [V(f(v)) for v in np.asarray(kf["M"]).reshape(12)]
    image = image_depth(inp, kf, dtype)
    depth = V(image.v[y, x], image.a[y, x])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        frame_point = [depth * ((V(x.astype(dtype)) - (cx - half)) / fx), depth * ((V(y.astype(dtype)) - (cy - half)) / fy), depth]
        gp = [G[4 * i] * frame_point[0] + G[4 * i + 1] * frame_point[1] + G[4 * i + 2] * frame_point[2] + G[4 * i + 3] for i in range(3)]
        image_normal = decode_normal(kf["normals"][y, x], dtype)
        gn = [G[4 * i] * image_normal[0] + G[4 * i + 1] * image_normal[1] + G[4 * i + 2] * image_normal[2] for i in range(3)]
        code, decided = pack_surfel_normal([c.v for c in gn])
        normal_ambiguous = np.zeros(len(pixels), bool)
        for q, c in zip(decided, gn):
            normal_ambiguous |= np.abs(q - np.rint(q)) <= np.maximum(1e-4, 511 * 8 * EPS32 * c.a)
        radius = kf["radius"][y, x].view(np.float16).astype(np.float32)   # __half2float: exact
        # TransformDepthToColorPixelCorner of the pixel's centre (BS/surfel_projection.cuh:196-207)
        colour_xy = ((cfx / fx) * V(x.astype(dtype) + half) + (-(cfx * cx / fx) + ccx), (cfy / fy) * V(y.astype(dtype) + half) + (-(cfy * cy / fy) + ccy))
        margin = coordinate_margin(max(w, cw), max(h, ch))
        colour, colour_margin = [], []
        for channel in range(3):                                        # make_uchar4(255.f * color.x, ...): truncation (:153-157)
            value, jump, _, undecided = Texture(kf["rgba"][..., channel], tex_mode, dtype).value(colour_xy[0], colour_xy[1], margin)
            colour.append(value.v.astype(np.float64))
            colour_margin.append(np.where(undecided, 256.0, 16 * EPS32 * 255.0 + jump))
        p1, p2, helper_undecided = tangent_points(gp, gn, V(radius.astype(dtype)), dtype)     # the unquantised normal (:132-139)
        luma = Texture(kf["rgba"][..., 3], tex_mode, dtype)
        positions = [colour_xy]
        for point in (p1, p2):
            ls = [M[4 * i] * point[0] + M[4 * i + 1] * point[1] + M[4 * i + 2] * point[2] + M[4 * i + 3] for i in range(3)]
            positions.append((cfx * (ls[0] / ls[2]) + ccx, cfy * (ls[1] / ls[2]) + ccy))
        sampled = [luma.value(p[0], p[1], margin) for p in positions]
        scale = V(dtype(K_DESC_SCALE))                                   # ComputeRawDescriptorResidual with a zero descriptor (:141-151)
        d = [scale * (sampled[i][0] - sampled[0][0]) for i in (1, 2)]
        widen = [float(K_DESC_SCALE) * (sampled[i][1] + sampled[0][1]) for i in (1, 2)]
    return {"position": gp, "code": code, "normal_ambiguous": normal_ambiguous, "radius": radius, "colour": np.stack(colour, 1),
            "colour_margin": np.stack(colour_margin, 1), "d": d, "d_widen": np.stack(widen, 1),
            "d_ambiguous": sampled[0][3] | sampled[1][3] | sampled[2][3] | helper_undecided, "pixels": pixels}


def u16(v):
    return np.asarray(v).astype(np.int64) & 0xFFFF


def creation(inp, k, surfels, x, filtered, min_observation_count, covis, tex_mode, dtype, with_columns=True):
    """bslam_create_surfels_for_keyframe.  surfels / x: the columns below surfels_size; covis: [(keyframe index, covis_T_frame as 12
    fp32 numbers)] in the caller's order (BS/direct_ba.cc:365-370)."""
    dtype = np.dtype(dtype).type
    kf = inp.keyframes[k]
    _, _, _, _, w, h = inp.cameras[1]
    c = Creation()
    s = supporting_surfels(inp, k, surfels, x, dtype)                   # occupancy: holder 0 (BS/direct_ba.cc:349-358)
    c.support = s
    # a cell that a surfel with a decided association holds is occupied whatever the undecided ones do
    sure = s.association.associated & ~s.association.ambiguous
    occupied = np.zeros(s.cells_w * s.cells_h, bool)
    occupied[s.cell_of[sure & (s.cell_of != INVALID_INDEX)]] = True
    undecided = (s.cell_ambiguous | (s.holders[0] != INVALID_INDEX)) & ~occupied
    c.candidates = first_valid_pixels(kf["depth"], occupied, inp.cell, s.cells_w, s.cells_h)
    y, x_ = c.candidates // w, c.candidates % w
    cell_id = np.minimum(y // inp.cell, s.cells_h - 1) * s.cells_w + np.minimum(x_ // inp.cell, s.cells_w - 1)
    c.candidate_ambiguous = undecided[cell_id]
    c.occupied, c.cell_undecided = occupied, undecided
    n = len(c.candidates)
    c.observations, c.violations = np.ones(n, np.int64), np.zeros(n, np.int64)
    c.kept, c.kept_ambiguous = np.ones(n, bool), np.zeros(n, bool)
    if filtered:
        f = lambda value: dtype(np.float32(value))
        fx, fy, cx, cy = (V(f(v)) for v in inp.cameras[1][:4])
        image = image_depth(inp, kf, dtype)
        depth = V(image.v[y, x_], image.a[y, x_])
        point = [depth * ((V(x_.astype(dtype)) - (cx - dtype(0.5))) / fx), depth * ((V(y.astype(dtype)) - (cy - dtype(0.5))) / fy), depth]
        normal = decode_normal(kf["normals"][y, x_], dtype)
        flips = np.zeros(n, np.int64)
        for index, matrix in covis:                                     # CountObservationsForNewSurfelsCUDAKernel :226-275
            a = associate(inp, inp.keyframes[index], matrix, point, normal, True, dtype)
            c.observations += a.associated
            c.violations += a.violation
            flips += a.ambiguous
        remove = lambda obs, viol: (u16(obs) < u16(min_observation_count)) | (u16(viol) > u16(obs))     # FilterNewSurfelsCUDAKernel :323-326
        c.kept = ~remove(c.observations, c.violations)
        c.kept_ambiguous = flips > 0
    c.columns = new_columns(inp, k, c.candidates[c.kept | c.kept_ambiguous], tex_mode, dtype) if with_columns else None
    return c


# ---- deletion and radius update -----------------------------------------------------------------------------------------
class Deletion:
    """observations, violations [N]; deleted [N] (newly: an already-NaN surfel is not counted again); survives [N] (its radius is
    written); radius [N] float32 (the minimum, where survives); ambiguous [N]; associated, violation [N, K]; px, py [N, K]"""


def deletion(inp, surfels, x, min_observation_count, dtype, keyframes=None):
    """bslam_delete_surfels_and_update_radii: BS/kernel_delete_surfels.cu:84-102 once per keyframe, then :132-151"""
    N = len(x)
    keyframes = list(range(len(inp.keyframes))) if keyframes is None else keyframes
    gp, gn = surfel_vectors(surfels, x, dtype)
    per_k = [associate(inp, inp.keyframes[k], inp.keyframes[k]["M"], gp, gn, True, dtype) for k in keyframes]
    d = Deletion()
    stack = lambda name: np.stack([getattr(a, name) for a in per_k], 1) if per_k else np.zeros((N, 0), bool)
    d.associated, d.violation, d.px, d.py = stack("associated"), stack("violation"), stack("px"), stack("py")
    d.ambiguous = stack("ambiguous").any(1)
    d.observations, d.violations = d.associated.sum(1), d.violation.sum(1)
    too_many = d.violations >= d.observations if MUTATION == "viol_ge_obs" else d.violations > d.observations
    remove = (d.observations < min_observation_count) | too_many
    d.deleted = remove & ~is_deleted(x)
    d.survives = ~remove
    radius = np.full(N, np.inf, np.float32)
    first = np.full(N, np.inf, np.float32)
    for j, k in enumerate(keyframes):
        seen = inp.keyframes[k]["radius"][d.py[:, j], d.px[:, j]].view(np.float16).astype(np.float32)
        radius = np.where(d.associated[:, j], np.minimum(radius, seen), radius)
        first = np.where(d.associated[:, j] & np.isinf(first), seen, first)
    d.radius = first if MUTATION == "radius_first_keyframe" else radius
    d.radius_of_first = first
    return d


# ---- compaction ---------------------------------------------------------------------------------------------------------
def exclusive_scan(flags):
    """the exclusive prefix sum the three scan kernels compute: tiles of 1024 values, their totals carried in blocks of 256 tiles"""
    flags = np.asarray(flags, np.int64)
    out = np.cumsum(flags) - flags
    if MUTATION == "scan_carry" and len(flags) > 256 * 1024:            # the second block of tile totals starts one tile short
        out[256 * 1024:] -= flags[255 * 1024:256 * 1024].sum()
    return out


def compaction(rows, active, size, surfel_count):
    """bslam_compact_surfels, pure integers (BS/kernel_compact_surfels.cu:97-281): rows uint32 [8, >= size], active uint8 [>= size] or
    None -> (new rows, new active, new size, the moves as (from, to))"""
    rows = rows.copy()
    active = None if active is None else active.copy()
    if size == surfel_count:                                            # :186-188
        return rows, active, size, (np.zeros(0, np.int64),) * 2
    free_spot_count = size - surfel_count
    invalid = rows[ROW_X, :size] == NAN_BITS
    ordinal = exclusive_scan(invalid)                                   # free spots before i
    free_list = np.full(free_spot_count, -1, np.int64)
    listed = invalid & (ordinal < free_spot_count)
    free_list[ordinal[listed]] = np.flatnonzero(listed)
    behind = exclusive_scan(~invalid[::-1])[::-1]                       # valid surfels behind i
    moving = np.flatnonzero(~invalid & (behind < free_spot_count))
    spot = free_list[behind[moving]]
    go = (spot >= 0) & (spot < moving)
    source, target = moving[go], spot[go]
    rows[:, target] = rows[:, source]
    if active is not None:
        active[target] = active[source]
    return rows, active, surfel_count, (source, target)


def compaction_brute_force(rows, active, size, surfel_count):
    """the same by a sequential loop: the last valid surfels fill the first free spots, each only if the spot lies before it"""
    rows = rows.copy()
    active = None if active is None else active.copy()
    if size == surfel_count:
        return rows, active, size
    free_spots = [i for i in range(size) if rows[ROW_X, i] == NAN_BITS][:size - surfel_count]
    valid_from_back = [i for i in range(size - 1, -1, -1) if rows[ROW_X, i] != NAN_BITS][:size - surfel_count]
    for spot, i in zip(free_spots, valid_from_back):
        if spot < i:
            rows[:, spot] = rows[:, i]
            if active is not None:
                active[spot] = active[i]
    return rows, active, surfel_count


# ---- activation ---------------------------------------------------------------------------------------------------------
def activation(associated, pair_ambiguous, keyframe_activation, active):
    """UpdateSurfelActivationCUDA (BS/kernel_surfel_activation.cc:38-77, .cu:38-79) from the association of every pair [N, K]
    (surfel_terms: associated, ambiguous) -> (the new bytes [N], ambiguous [N])"""
    on = np.asarray(keyframe_activation) == KF_ACTIVE
    decided = (associated & ~pair_ambiguous)[:, on].any(1)
    any_associated = associated[:, on].any(1)
    new = np.where(any_associated, SURFEL_ACTIVE_FLAG, active & ~np.uint8(SURFEL_ACTIVE_FLAG)).astype(np.uint8)
    return new, ~decided & pair_ambiguous[:, on].any(1)


def nan_surfel_association(inputs, keyframes):
    """[N, K] (associated, ambiguous): where a surfel with a NaN x lands by the reference project's own association, which the
    activation pass calls like every lifecycle pass (BS/kernel_surfel_activation.cu:75 -> surfel_projection_nvcc_only.cuh:302-328): on
    pixel (0, 0) of every keyframe.  False for every other surfel.

    The project's activation_kernel uses the BA association instead, which refuses a NaN position (csrc/device_math.hpp:
    project_with<false>), so a deleted surfel that has not been compacted away stays inactive there, while the reference project and
    the oracle set its flag when pixel (0, 0) of an active keyframe has a measurement with a compatible normal.  No kernel reads the
    flag of a surfel with a NaN position and compaction drops it, so the two readings differ in that byte alone; the tests pin both:
    the oracle to this function, the kernel to the BA association."""
    gp, gn = surfel_vectors(inputs.surfels, inputs.surfels[ROW_X], np.float64)
    lost = np.isnan(inputs.surfels[ROW_X])
    per_k = [associate(inputs, kf, kf["M"], gp, gn, False, np.float64) for kf in keyframes]
    return np.stack([a.associated & lost for a in per_k], 1), np.stack([a.ambiguous & lost for a in per_k], 1)


# ---- the fixtures -------------------------------------------------------------------------------------------------------
# name -> (depth image size, cell, surfels): the hard fixture of surfel_terms_util with radius images, and two smaller variants over the
# same scene: 38 x 25 at cell 3 (partial cells of two columns and one row), and cell 1 (every pixel a cell)
VARIANTS = {"cell4": (ST.DEPTH_SIZE, ST.CELL, ST.N_SURFELS), "cell3": ((38, 25), 3, 520), "cell1": ((21, 14), 1, 330)}
SPARE_COLUMNS = 700                                    # room behind the surfels for what creation appends, and then some


class LifecycleInputs(ST.Inputs):
    """ST.Inputs whose keyframes also carry "radius" (u16 half bits), "rgba" and "G" (global_T_frame, 12 fp32 numbers)"""


def placed_surfels(fix, cell):
    """The fixture's surfel rows with the groups the merge census needs, written over surfels of the upper two thirds of the index
    range that belong to none of the fixture's own groups.  Every placed surfel copies a surfel of the lowest third (`twin`: its
    own index modulo a third of the count), which lies in the same cell, comes earlier, and is often one of the cell's holders:
      merge_twins: the twin moved by 4 mm -- close to it in position and normal, merged by whichever holder of the cell is as close;
      turned_twins: the twin's position, its normal turned by 35 degrees -- still associated, and against a holder tilted the other
        way refused by the normal test alone;
      wide_twins: the twin moved by 3 cm with a radius of 9 cm -- the distance test turns on the smaller radius of the pair, so it
        is merged by the wide holders only."""
    surfels = fix.surfels.copy()
    N = surfels.shape[1]
    i = np.arange(N)
    taken = np.zeros(N, bool)
    for members in fix.groups.values():
        taken[members] = True
    free = np.flatnonzero(~taken & (i > N // 3))
    groups = {}
    third = len(free) // 12
    for name, members in (("merge_twins", free[:third]), ("turned_twins", free[third:2 * third]), ("wide_twins", free[2 * third:3 * third])):
        twin = members % (N // 3)
        twin = np.where(taken[twin], (twin + 1) % (N // 3), twin)
        surfels[:, members] = fix.surfels[:, twin]
        if name == "merge_twins":
            surfels[ROW_X, members] += np.float32(0.004)
        elif name == "wide_twins":
            surfels[ROW_Y, members] += np.float32(0.03)
            surfels[ROW_RADIUS_SQUARED, members] = np.float32(0.09 ** 2)
        else:
            n = np.stack([c.v for c in unpack_surfel_normal(fix.surfels[ROW_NORMAL, twin].view(np.uint32), np.float64)], 1)
            axis = np.cross(n, [0.0, 1.0, 0.0])
            axis /= np.linalg.norm(axis, axis=1, keepdims=True)
            turned = np.cos(np.radians(35)) * n + np.sin(np.radians(35)) * axis
            surfels[ROW_NORMAL, members] = pack_surfel_normal([turned[:, c] for c in range(3)])[0].view(np.float32)
        groups[name] = members
    return surfels, groups


FLOATER_KEYFRAMES = (0, 1)
FLOATER = (1.22, (-0.16, 0.02), (-0.12, 0.04))          # a patch of the plane z = 1.22 (global), x and y range


def floater(k, depth, normals, camera):
    """The keyframe's depth and normal images with, in keyframes 0 and 1 only, a small plane patch in front of the surface: a new
    surfel made from it is seen again by the other of the two and is a free-space violation for every keyframe that looks through
    where it would be, so the creation filter's `violations > observations` has both outcomes, turned by one co-visible keyframe."""
    from tests.pair_terms_util import encode_normal, rodrigues
    depth, normals = np.array(depth), np.array(normals)
    if k not in FLOATER_KEYFRAMES:
        return depth, normals
    fx, fy, cx, cy, w, h = camera
    R, t = rodrigues(ST._POSES[k][0]), np.asarray(ST._POSES[k][1], np.float64)
    ys, xs = np.mgrid[0:h, 0:w]
    direction = np.stack([(xs - (cx - 0.5)) / fx, (ys - (cy - 0.5)) / fy, np.ones(xs.shape)], -1) @ R.T
    z, (x0, x1), (y0, y1) = FLOATER
    d = (z - t[2]) / direction[..., 2]
    p = d[..., None] * direction + t
    on = (p[..., 0] >= x0) & (p[..., 0] <= x1) & (p[..., 1] >= y0) & (p[..., 1] <= y1) & ((depth & INVALID_DEPTH_BIT) == 0)
    depth[on] = np.rint(d[on] / ST.RAW_TO_FLOAT_DEPTH).astype(np.uint16)
    normals[on] = encode_normal(np.broadcast_to(np.array([0.0, 0.0, -1.0]) @ R, xs.shape + (3,)))[on]
    return depth, normals


class LifecycleFixture:
    """case, variant, cell, inputs (LifecycleInputs, the reference's view), scene (tests.bso.HostScene with SPARE_COLUMNS columns of
    0xA5 behind the surfels), N, groups"""


@functools.lru_cache(maxsize=None)
def lifecycle_fixture(case, variant="cell4"):
    from badslam_amd import abi
    from tests import bso
    size, cell, n = VARIANTS[variant]
    fix = ST.hard_fixture(case, size, cell, n)
    surfels, placed = placed_surfels(fix, cell)
    # a deleted surfel carries CUDART_NAN_F's bits; the last of the fixture's NaN surfels keeps another NaN, which is no deletion mark
    dead = fix.groups["nan"][:-1]
    surfels[ROW_X, dead] = nan_x()
    color_cam, depth_cam = (bso.make_camera(*c) for c in fix.cameras)
    scene = bso.HostScene(color_cam, depth_cam, ST.RAW_TO_FLOAT_DEPTH, ST.BASELINE_FX, cell, n + SPARE_COLUMNS, True, True, abi.TEX_EXACT_FLOAT)
    scene.cfactor[:] = fix.cfactor
    scene.a = fix.a
    keyframes = []
    for k, kf in enumerate(fix.keyframes):
        depth, normals = floater(k, kf["depth"], kf["normals"], fix.cameras[1])
        pose = abi.SE3f((ctypes.c_float * 4)(*[float(v) for v in fix.quaternions[k, :4]]), (ctypes.c_float * 3)(*[float(v) for v in fix.quaternions[k, 4:]]))
        host = bso.HostKeyframe(depth, normals, np.array(kf["radius"]), np.array(kf["rgba"]), pose, kf_id=k)
        scene.keyframes.append(host)
        view = host.view()
        keyframes.append(dict(kf, depth=depth, normals=normals, M=np.array(view.frame_T_global.m, np.float32), R=np.array(view.global_R_frame.m, np.float32),
                              G=np.array(bso.se3_matrix3x4(pose).m, np.float32)))
    scene.surfels.view(np.uint32)[:] = 0xA5A5A5A5
    scene.surfels[:8, :n] = surfels
    scene.active[:] = 0xA5
    # flag bytes with other bits set: the activation pass must keep them where the surfel stays inactive
    scene.active[0, :n] = (fix.active | ((np.arange(n) * 37) & 0xFE)).astype(np.uint8)
    scene.surfels_size = n
    out = LifecycleFixture()
    out.case, out.variant, out.cell, out.N, out.scene = case, variant, cell, n, scene
    out.inputs = LifecycleInputs(surfels, scene.active[0, :n].copy(), keyframes, fix.cameras, ST.BASELINE_FX, ST.RAW_TO_FLOAT_DEPTH, fix.a, fix.cfactor, cell)
    out.groups = dict(fix.groups, **placed)
    for array in (out.inputs.surfels, out.inputs.active):
        array.setflags(write=False)
    return out


def scene_of(fixture, tex_mode=None, surfels_size=None, keyframes=None, max_surfels=None):
    """A HostScene of the fixture with rows, flags and keyframe list of its own (the entry points write the rows); keyframes: indices"""
    from tests import bso
    base = fixture.scene
    scene = bso.HostScene(base.color_camera, base.depth_camera, base.raw_to_float_depth, base.baseline_fx, base.cell, max(base.max_surfels, max_surfels or 0),
                          True, True, base.tex_mode if tex_mode is None else tex_mode)
    scene.cfactor[:], scene.a = base.cfactor, base.a
    scene.keyframes = list(base.keyframes) if keyframes is None else [base.keyframes[k] for k in keyframes]
    scene.surfels.view(np.uint32)[:] = 0xA5A5A5A5
    scene.active[:] = 0xA5
    scene.surfels[:, :base.max_surfels], scene.active[:, :base.max_surfels] = base.surfels, base.active
    scene.surfels_size = base.surfels_size if surfels_size is None else surfels_size
    if surfels_size is not None:
        scene.surfels.view(np.uint32)[:, surfels_size:] = 0xA5A5A5A5
    return scene


def covis_list(fixture, k, indices):
    """[(index, covis_T_frame)] of keyframe k's co-visible keyframes `indices`, the matrices as the call receives them"""
    scene = fixture.scene
    _, _, mats = scene.covis_args(scene.keyframes[k], [scene.keyframes[i] for i in indices])
    return [(index, np.array(mats[j].m, np.float32)) for j, index in enumerate(indices)]


# ---- the synthetic keyframe of the pixel scan past 256 tiles ---------------------------------------------------------------
LARGE_SIZE, LARGE_CELL = (640, 410), 16                 # 262400 pixels: 257 tiles of 1024, so scan_sums_kernel takes its second pass


@functools.lru_cache(maxsize=None)
def large_fixture():
    """One 640 x 410 keyframe at cell 16 (a partial bottom row of cells), images written directly: a tilted plane with scattered holes
    and whole rows of holes at the top of some cells, so the chosen pixel of a cell varies; a few surfels that hold some cells."""
    from badslam_amd import abi
    from tests import bso
    w, h = LARGE_SIZE
    camera = (520.0, 515.0, 322.3, 203.9)
    ys, xs = np.mgrid[0:h, 0:w]
    depth = 1.4 + 0.0004 * xs + 0.0003 * ys
    raw = np.rint(depth / ST.RAW_TO_FLOAT_DEPTH).astype(np.uint16)
    hole = ((xs * 7 + ys * 13) % 31 < 9) | ((ys % 16 < (xs // 16) % 5) & ((xs // 16 + ys // 16) % 3 == 0))
    # the last, partial row of cells: in every fourth cell the rows above image row 408 are holes, so that the cell's pixel lies
    # in row 408 -- tile 255 of the pixel scan, the last of its first block of tile totals, whose sum the returned count carries
    hole |= (ys >= 400) & (ys < 408) & ((xs // 16) % 4 == 1)
    raw[hole] |= INVALID_DEPTH_BIT
    normal = np.stack([np.full(xs.shape, 0.12), np.full(xs.shape, -0.08), np.zeros(xs.shape)], -1)
    from tests.pair_terms_util import encode_normal
    normals = encode_normal(normal).astype(np.uint16)
    radius = (0.004 + 0.003 * ST._frac(0.137 * xs + 0.291 * ys)) ** 2
    luma = np.clip(128 + 90 * np.sin(0.05 * xs + 0.3) * np.cos(0.07 * ys) + 0.5, 0, 255).astype(np.uint8)
    rgba = np.ascontiguousarray(np.stack([(xs * 3 + ys) % 251, 255 - luma, (xs + ys * 5) % 241, luma], -1).astype(np.uint8))
    cam = bso.make_camera(*camera, w, h)
    n = 300
    scene = bso.HostScene(cam, cam, ST.RAW_TO_FLOAT_DEPTH, ST.BASELINE_FX * 10, LARGE_CELL, n + 1200, True, True, abi.TEX_EXACT_FLOAT)
    pose = abi.SE3f((ctypes.c_float * 4)(0.01, -0.02, 0.015, 0.9996), (ctypes.c_float * 3)(0.1, -0.05, 0.02))
    q = np.array(list(pose.q), np.float64)
    q /= np.linalg.norm(q)
    pose = abi.SE3f((ctypes.c_float * 4)(*[float(v) for v in q]), (ctypes.c_float * 3)(0.1, -0.05, 0.02))
    host = bso.HostKeyframe(raw, normals, radius.astype(np.float16).view(np.uint16), rgba, pose, kf_id=0)
    scene.keyframes.append(host)
    view = host.view()
    G = np.array(bso.se3_matrix3x4(pose).m, np.float32)
    kf = {"depth": raw, "normals": normals, "radius": host.radius, "rgba": rgba, "luma": luma, "M": np.array(view.frame_T_global.m, np.float32),
          "R": np.array(view.global_R_frame.m, np.float32), "G": G}
    inputs = LifecycleInputs(None, None, [kf], ((camera + (w, h)), (camera + (w, h))), ST.BASELINE_FX * 10, ST.RAW_TO_FLOAT_DEPTH, 0.0, scene.cfactor, LARGE_CELL)
    # surfels: what the reference itself creates at every seventh cell's pixel
    cells_w, cells_h = cells_of(w, h, LARGE_CELL)
    pixels = first_valid_pixels(raw, np.zeros(cells_w * cells_h, bool), LARGE_CELL, cells_w, cells_h)[::7][:n]
    columns = new_columns(inputs, 0, pixels, TEX_EXACT_FLOAT, np.float64)
    n = len(pixels)
    scene.surfels.view(np.uint32)[:] = 0xA5A5A5A5
    scene.surfels[ROW_X:ROW_Z + 1, :n] = np.stack([c.v for c in columns["position"]])
    scene.surfels[ROW_NORMAL, :n] = columns["code"].view(np.float32)
    scene.surfels[ROW_RADIUS_SQUARED, :n] = columns["radius"]
    scene.surfels[ROW_COLOR, :n] = 0
    scene.surfels[ROW_D1, :n], scene.surfels[ROW_D2, :n] = columns["d"][0].v, columns["d"][1].v
    scene.surfels_size = n
    inputs.surfels = scene.surfels[:8, :n].copy()
    out = LifecycleFixture()
    out.case, out.variant, out.cell, out.N, out.scene, out.inputs, out.groups = "large", "cell16", LARGE_CELL, n, scene, inputs, {}
    return out


# ---- what the tests share -----------------------------------------------------------------------------------------------
def column_tolerances(columns):
    """how far a created column's position [n, 3] and descriptors [n, 2] may lie from the float64 values: KERNEL_FACTOR C 2^-24 A,
    plus the fixed-point texture mode's widening"""
    position = KERNEL_FACTOR * C_MEASURED["position"] * EPS32 * np.stack([c.a for c in columns["position"]], 1).astype(np.float64)
    d = KERNEL_FACTOR * C_MEASURED["descriptor"] * EPS32 * np.stack([c.a for c in columns["d"]], 1).astype(np.float64) + columns["d_widen"]
    return position, d


def check_columns(columns, got, label):
    """got: float32 [8, n] columns in the order of columns["pixels"] -> the failures"""
    failures = []
    n = len(columns["pixels"])
    bits = np.ascontiguousarray(got[:8, :n]).view(np.uint32)
    tol_p, tol_d = column_tolerances(columns)
    want = np.stack([c.v for c in columns["position"]], 1).astype(np.float64)
    bad = ~(np.abs(got[ROW_X:ROW_Z + 1, :n].T.astype(np.float64) - want) <= tol_p)
    if bad.any():
        j = np.argwhere(bad)[0]
        failures.append((label, "position", int(bad.sum()), j.tolist(), float(got[j[1], j[0]]), float(want[j[0], j[1]]), float(tol_p[j[0], j[1]])))
    wrong = ~columns["normal_ambiguous"] & (bits[ROW_NORMAL] != columns["code"])
    if wrong.any():
        failures.append((label, "normal code", int(wrong.sum()), np.flatnonzero(wrong)[:5].tolist()))
    if not np.array_equal(bits[ROW_RADIUS_SQUARED], columns["radius"].view(np.uint32)):
        failures.append((label, "radius bits", int((bits[ROW_RADIUS_SQUARED] != columns["radius"].view(np.uint32)).sum())))
    for channel in range(3):
        byte = ((bits[ROW_COLOR] >> (8 * channel)) & 0xFF).astype(np.int64)
        low = np.floor(columns["colour"][:, channel] - columns["colour_margin"][:, channel])
        high = np.floor(columns["colour"][:, channel] + columns["colour_margin"][:, channel])
        bad = ~((byte >= low) & (byte <= high))                          # outside the margin of the truncation: one value, exact
        if bad.any():
            j = int(np.flatnonzero(bad)[0])
            failures.append((label, "colour byte", channel, int(bad.sum()), j, int(byte[j]), float(columns["colour"][j, channel])))
    if ((bits[ROW_COLOR] >> 24) != 0).any():
        failures.append((label, "colour .w is 0"))
    want_d = np.stack([c.v for c in columns["d"]], 1).astype(np.float64)
    bad = ~columns["d_ambiguous"][:, None] & ~(np.abs(np.stack([got[ROW_D1, :n], got[ROW_D2, :n]], 1).astype(np.float64) - want_d) <= tol_d)
    if bad.any():
        j = np.argwhere(bad)[0]
        failures.append((label, "descriptor", int(bad.sum()), j.tolist(), float(got[ROW_D1 + j[1], j[0]]), float(want_d[j[0], j[1]]), float(tol_d[j[0], j[1]])))
    return failures


def match_created(c, got, created, label):
    """The created columns got [8, created] against the reference's candidates in pixel order: every decided kept candidate must be
    there, in order; an ambiguous one may be.  -> failures"""
    sure = c.kept & ~c.kept_ambiguous & ~c.candidate_ambiguous
    maybe = (c.kept_ambiguous | (c.candidate_ambiguous & c.kept))
    listed = np.flatnonzero(c.kept | c.kept_ambiguous)                   # the rows of c.columns
    position = np.stack([v.v for v in c.columns["position"]], 1).astype(np.float64)
    tol = column_tolerances(c.columns)[0]
    take, j = [], 0
    for row, candidate in enumerate(listed):
        here = j < created and bool((np.abs(got[ROW_X:ROW_Z + 1, j].astype(np.float64) - position[row]) <= tol[row]).all())
        if sure[candidate] and not here:
            return [(label, "a decided new surfel is missing or out of order", int(c.candidates[candidate]), j)]
        if here and (sure[candidate] or maybe[candidate]):
            take.append(row)
            j += 1
    if j != created:
        return [(label, "created count", created, j, int(sure.sum()), int(maybe.sum()))]
    take = np.array(take, np.int64)
    pick = lambda value: [V(v.v[take], v.a[take]) for v in value] if isinstance(value, list) else value[take]
    return check_columns({name: pick(value) for name, value in c.columns.items()}, got[:, :created], label)


class OracleBackend:
    """The oracle's lifecycle on a tests.bso.HostScene, behind the calls the checks below make (the GPU tests put the library on a
    device scene behind the same calls)."""

    def __init__(self, scene):
        self.scene = scene

    def rows(self):
        return self.scene.surfels

    def active(self):
        return self.scene.active[0]

    def size(self):
        return self.scene.surfels_size

    def merge(self, k, factor, count):
        return self.scene.merge_surfels(self.scene.keyframes[k], factor, count)

    def create(self, k, filtered, min_observation_count, covis):
        return self.scene.create_surfels_for_keyframe_ex(self.scene.keyframes[k], filtered, min_observation_count, [self.scene.keyframes[i] for i in covis])

    def delete(self, min_observation_count, count):
        return self.scene.delete_surfels_and_update_radii(min_observation_count, count)

    def compact(self, count, with_active):
        self.scene.compact_surfels(count, with_active)

    def activate(self):
        self.scene.update_activation()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_merge(fixture, factor, backend, stats=None):
    """Merge against every keyframe in turn without compaction (BS/direct_ba.cc:578-597): after every keyframe the deleted set and the
    returned count against the reference.  -> failures; stats: list that receives (keyframe, Merge)"""
    inp, N = fixture.inputs, fixture.N
    x, unknown = inp.surfels[ROW_X].copy(), np.zeros(N, bool)
    count = int(N - is_deleted(x).sum())
    failures = []
    for k in range(len(inp.keyframes)):
        m = merge_step(inp, k, inp.surfels, x, factor, np.float64, unknown)
        before = is_deleted(backend.rows()[ROW_X, :N])
        got_count = backend.merge(k, factor, count)
        rows = backend.rows()
        after = is_deleted(rows[ROW_X, :N])
        newly = after & ~before
        if got_count != count - int(newly.sum()):
            failures.append((k, "returned count", got_count, count, int(newly.sum())))
        wrong = ~m.ambiguous & (newly != m.deleted)
        if wrong.any():
            failures.append((k, "deleted set", int(wrong.sum()), np.flatnonzero(wrong)[:6].tolist(), m.rank[wrong][:6].tolist()))
        if (before & ~after).any() or not np.array_equal(_bits(rows[ROW_X, :N])[~after], _bits(inp.surfels[ROW_X])[~after]) \
                or not np.array_equal(_bits(rows[1:8, :N]), _bits(inp.surfels[1:8])):
            failures.append((k, "something other than the merged surfels' x was written"))
        count = got_count
        x[m.deleted] = nan_x()
        unknown |= m.ambiguous
        if stats is not None:
            stats.append((k, m))
    return failures


def check_creation(fixture, backend_of, k, size, filtered, min_observation_count, covis, tex_mode, label=""):
    """One creation call on the first `size` surfels of the fixture.  backend_of(scene) -> backend.  -> (failures, Creation)"""
    inp = fixture.inputs
    scene = scene_of(fixture, tex_mode, surfels_size=size)
    backend = backend_of(scene)
    c = creation(inp, k, inp.surfels[:, :size], inp.surfels[ROW_X, :size], filtered, min_observation_count, covis_list(fixture, k, covis), tex_mode, np.float64)
    before = _bits(backend.rows()).copy()
    created = backend.create(k, filtered, min_observation_count, covis)
    after = _bits(backend.rows())
    failures = match_created(c, np.ascontiguousarray(after[:, size:size + created]).view(np.float32), created, label)
    if not np.array_equal(after[:, :size], before[:, :size]):
        failures.append((label, "an existing surfel was written"))
    if not np.array_equal(after[:, size + created:], before[:, size + created:]):
        failures.append((label, "a column at or beyond surfels_size + created was written"))
    return failures, c


def check_deletion(fixture, backend_of, min_observation_count, keyframes=None, order=None, copies=1, label=""):
    """One deletion + radius update.  keyframes: indices of the keyframes handed in; order: the scene's column j holds the fixture's
    surfel order[j]; copies: the (ordered) surfels that many times side by side.  -> (failures, Deletion)"""
    inp, N = fixture.inputs, fixture.N
    order = np.arange(N) if order is None else np.asarray(order)
    order = np.tile(order, copies)
    n = len(order)
    scene = scene_of(fixture, keyframes=keyframes, max_surfels=n + 64)
    scene.surfels[:8, :n] = inp.surfels[:, order]
    scene.surfels_size = n
    backend = backend_of(scene)
    d = deletion(inp, inp.surfels, inp.surfels[ROW_X], min_observation_count, np.float64, keyframes)
    before = _bits(backend.rows()).copy()
    count = int(n - is_deleted(before[ROW_X, :n].view(np.float32)).sum())
    got_count = backend.delete(min_observation_count, count)
    after = _bits(backend.rows())
    failures = []
    was, now = before[ROW_X, :n] == NAN_BITS, after[ROW_X, :n] == NAN_BITS
    newly = now & ~was
    if got_count != count - int(newly.sum()):
        failures.append((label, "returned count", got_count, count, int(newly.sum())))
    decided = ~d.ambiguous[order]
    wrong = decided & (newly != d.deleted[order])
    if wrong.any():
        j = np.flatnonzero(wrong)
        failures.append((label, "deleted set", len(j), order[j][:6].tolist(), d.observations[order[j]][:6].tolist(), d.violations[order[j]][:6].tolist()))
    survives = decided & d.survives[order]
    wrong = survives & (after[ROW_RADIUS_SQUARED, :n] != d.radius[order].view(np.uint32))
    if wrong.any():
        failures.append((label, "radius of a survivor", int(wrong.sum()), order[np.flatnonzero(wrong)][:6].tolist()))
    wrong = decided & ~d.survives[order] & (after[ROW_RADIUS_SQUARED, :n] != before[ROW_RADIUS_SQUARED, :n])
    if wrong.any():
        failures.append((label, "radius of a deleted surfel written", int(wrong.sum())))
    others = [r for r in range(8) if r not in (ROW_X, ROW_RADIUS_SQUARED)]
    if not np.array_equal(after[others], before[others]) or not np.array_equal(after[:, n:], before[:, n:]) \
            or not np.array_equal(after[ROW_X, :n][~newly], before[ROW_X, :n][~newly]):
        failures.append((label, "something else was written"))
    return failures, d


def compaction_case(n, pattern, seed=0):
    """rows uint32 [8, n] with distinguishable bits in all eight rows, flag bytes [n], the number of valid surfels"""
    i = np.arange(n, dtype=np.uint32)
    rows = np.stack([(np.uint32(r + 1) << np.uint32(27)) | i for r in range(8)])
    rng = np.random.default_rng(seed + n)
    half = rng.random(n) < 0.5
    # late: holes only among the last 4096 surfels, early: survivors only among the first 4096 -- at n > 262144 what fills a hole,
    # or where a survivor goes, then hangs on a prefix sum of the scan's second block of tile totals, forward or from the back
    dead = {"thirds": rng.random(n) < 1 / 3, "prefix": i < (n + 2) // 3, "tail": i >= n - (n + 2) // 3, "all": np.ones(n, bool),
            "late": half & (i + 4096 >= n), "early": ~(half & (i < 4096))}[pattern]
    rows[ROW_X, dead] = NAN_BITS
    return rows, ((i * 7 + 3) & 0xFF).astype(np.uint8), int(n - dead.sum())


def check_compaction(backend_of_rows, n, pattern, with_active):
    """backend_of_rows(rows, active) -> a backend on a scene of n surfels with these rows and flag bytes.  -> failures"""
    rows, active, count = compaction_case(n, pattern)
    want_rows, want_active, want_size, moves = compaction(rows, active if with_active else None, n, count)
    backend = backend_of_rows(rows, active)
    backend.compact(count, with_active)
    failures = []
    label = (n, pattern, with_active)
    if backend.size() != want_size:
        failures.append((label, "size", backend.size(), want_size))
    if pattern == "tail" and len(moves[0]):
        failures.append((label, "a deleted tail moves nothing"))
    got = _bits(backend.rows())[:8, :n]
    if not np.array_equal(got, want_rows):
        bad = np.argwhere(got != want_rows)
        failures.append((label, "rows", len(bad), bad[:4].tolist()))
    got_active = np.asarray(backend.active())[:n]
    if not np.array_equal(got_active, want_active if with_active else active):
        failures.append((label, "flag bytes", int((got_active != (want_active if with_active else active)).sum())))
    return failures


def check_activation(backend, associated, pair_ambiguous, keyframe_activation, label=""):
    """backend: on a scene whose keyframes carry keyframe_activation.  -> (failures, new bytes, ambiguous)"""
    n = associated.shape[0]
    before, behind = np.array(backend.active()[:n]), np.array(backend.active()[n:])
    rows_before = _bits(backend.rows()).copy()
    backend.activate()
    got = np.asarray(backend.active())[:n]
    want, ambiguous = activation(associated, pair_ambiguous, keyframe_activation, before)
    failures = []
    wrong = ~ambiguous & (got != want)
    if wrong.any():
        j = np.flatnonzero(wrong)
        failures.append((label, "flag bytes", len(j), j[:6].tolist(), got[j][:6].tolist(), want[j][:6].tolist(), before[j][:6].tolist()))
    if not np.array_equal(np.asarray(backend.active())[n:], behind) or not np.array_equal(_bits(backend.rows()), rows_before):
        failures.append((label, "something else was written"))
    return failures, want, ambiguous


def measure_c():
    """{kind: the largest |value32 - value64| / (2^-24 A)} over the created columns (exact texture mode) of every fixture"""
    out = {"position": 0.0, "descriptor": 0.0}
    runs = [(lifecycle_fixture(case, "cell4"), k) for case in ST.CASES for k in range(5)] + [(lifecycle_fixture("same_camera", v), 1) for v in ("cell3", "cell1")]
    runs.append((large_fixture(), 0))
    for fixture, k in runs:
        inp = fixture.inputs
        w, h = inp.cameras[1][4:]
        cells_w, cells_h = cells_of(w, h, inp.cell)
        pixels = first_valid_pixels(inp.keyframes[k]["depth"], np.zeros(cells_w * cells_h, bool), inp.cell, cells_w, cells_h)
        c64, c32 = (new_columns(inp, k, pixels, TEX_EXACT_FLOAT, dt) for dt in (np.float64, np.float32))
        for kind, name, skip in (("position", "position", np.zeros(len(pixels), bool)), ("descriptor", "d", c64["d_ambiguous"] | c32["d_ambiguous"])):
            for v64, v32 in zip(c64[name], c32[name]):
                ok = ~skip & (v64.a > 0)
                ratio = np.abs(v32.v.astype(np.float64) - v64.v)[ok] / (EPS32 * v64.a[ok])
                out[kind] = max(out[kind], float(ratio.max()) if ratio.size else 0.0)
    return out


# ---- the runs of tests/test_lifecycle_cpu.py (the oracle) and tests/test_gpu_lifecycle_reference.py (the kernels) ----------------
RUNS = [(case, "cell4") for case in ST.CASES] + [("same_camera", "cell3"), ("same_camera", "cell1")]
FACTORS = (0.8, 2.0)
MODES = {"fixed": TEX_FIXED_POINT_1_8, "exact": TEX_EXACT_FLOAT}
MAX_AMBIGUOUS_SHARE = 0.02
# (keyframe, surfels below surfels_size as a share of the fixture's, filtered, min_observation_count, co-visible keyframes, mode):
# unfiltered and filtered, the three counts and one that only the u16 cast brings into range (65538 -> 2), the list in both orders
# and one keyframe shorter (the outcome of a candidate turns on that keyframe), both texture modes
CREATION_RUNS = [(0, 0.0, False, 2, (), "exact"), (1, 0.15, False, 2, (), "fixed"), (4, 1.0, False, 2, (), "exact"),
                 (0, 0.0, True, 1, (1, 2, 3, 4, 5), "exact"), (0, 0.0, True, 2, (1, 2, 3, 4, 5), "fixed"), (0, 0.0, True, 3, (5, 4, 3, 2, 1), "exact"),
                 (0, 0.0, True, 1, (1, 2, 3), "exact"), (0, 0.0, True, 1, (1, 2), "exact"), (1, 0.15, True, 2, (0, 2, 3, 4), "exact"),
                 (1, 0.15, True, 2, (4, 3, 2, 0), "fixed"), (1, 0.15, True, 65538, (0, 2, 3, 4), "exact"), (4, 0.15, True, 3, (0, 1, 2, 3), "fixed"),
                 (2, 0.15, True, 2, (), "exact")]


def size_of(fixture, share):
    return int(round(share * fixture.N))


ACTIVITY_MASKS = {"all": (0, 0, 0, 0, 0, 0), "one": (2, 2, 0, 2, 2, 2), "none": (2, 1, 2, 1, 2, 1), "alternating": (0, 2, 0, 1, 0, 2)}


def ba_terms(inputs):
    terms = ST.surfel_terms(inputs, True, False, TEX_EXACT_FLOAT, np.float64)
    return terms.associated, terms.ambiguous


SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 262145, 264200)
PATTERNS = ("thirds", "prefix", "tail", "all", "late", "early")


def with_nan_surfels(inputs, keyframes, associated, ambiguous):
    """the oracle's reading of a surfel with a NaN position (lifecycle_util.nan_surfel_association) on top of the BA association"""
    lands, undecided = nan_surfel_association(inputs, keyframes)
    assert lands.any()
    return associated | lands, ambiguous | undecided


def tiled_scene(fixture, copies=1):
    """scene_of(fixture) with the fixture's surfels and flag bytes `copies` times side by side: from 64 granules of 256 surfels on, the
    library may walk the surfels in its per-surfel order, through the sorted copy and with the granule boxes of the culling"""
    n = fixture.N * copies
    scene = scene_of(fixture, max_surfels=n + 64)
    scene.surfels[:8, :n] = np.tile(fixture.inputs.surfels, (1, copies))
    scene.active[0, :n] = np.tile(fixture.inputs.active, copies)
    scene.surfels_size = n
    return scene


def activity_scene(fixture, mask, copies=1, repeat=1):
    """the fixture's keyframes `repeat` times in a row, every round with the activity of `mask`"""
    scene = tiled_scene(fixture, copies)
    scene.keyframes = [copy.copy(kf) for _ in range(repeat) for kf in scene.keyframes]
    for kf, activation in zip(scene.keyframes, tuple(mask) * repeat):
        kf.activation = activation
    return scene


def stack_scene(fixture, K, copies=1):
    """K - 1 copies of the look-away keyframe in front of keyframe 0: the only associating keyframe is the last"""
    scene = tiled_scene(fixture, copies)
    scene.keyframes = [scene.keyframes[5]] * (K - 1) + [scene.keyframes[0]]
    return scene


def stack_terms(fixture, K):
    kfs = fixture.inputs.keyframes
    two = LifecycleInputs(fixture.inputs.surfels, fixture.inputs.active, [kfs[5], kfs[0]], fixture.inputs.cameras, ST.BASELINE_FX, ST.RAW_TO_FLOAT_DEPTH,
                            fixture.inputs.a, fixture.inputs.cfactor, fixture.inputs.cell)
    associated, ambiguous = ba_terms(two)
    pick = [0] * (K - 1) + [1]
    assert not associated[:, 0].any() and associated[:, 1].sum() > 300
    return associated[:, pick], ambiguous[:, pick]
