"""Shared pieces of the alternating intrinsics step's parity tests (bslam_optimize_intrinsics against bso_optimize_intrinsics):
the scenes, the entry groups and the per-entry comparators.  tests/test_intrinsics_step_cpu.py holds the oracle's side alone,
tests/test_gpu_intrinsics_step.py the device against it.

Accumulated entries -- the 40 global sums and each cell's B[5], D, b2 -- are judged as the shared PCG entries are
(tests/pcg_parity.py): |device - sum64| <= tol * abs64 per entry, sum64 / abs64 being the oracle's float64 sums of its own fp32
terms and of their absolute values (bso_intrinsics_last_shadow).  tol is four times the worst ratio measured on an MI355X over
all cases and instantiations of tests/test_gpu_intrinsics_step.py, capped at pcg_parity.TOL_CEILING: the device contracts
products that the oracle does not and divides through the hardware reciprocal, so single terms differ by a few ulps.
#                          measured worst ratio      case it came from
#   A/b1 fx fy cx cy       2.512e-07                 odd-1 <depth> (entries of one to three terms: the terms' own difference)
#   A/b1 a                 3.324e-07                 odd-1 <depth>
#   A mixed                1.359e-07                 odd-1 <depth>
#   colour H/b             7.337e-08                 odd-1 <colour>
#   cell B                 5.201e-07                 odd-1 <depth>
#   cell D                 3.982e-07                 odd-1 <depth>
#   cell b2                3.748e-07                 odd-1 <depth>
#   schur A/b1             4.417e-08                 odd-1 <depth> (the 20 sums after the Schur pass, on the pass's own inputs)
The device sums the threads' fp32 sums in float64 and rounds once, so over the cases that use all their surfels the worst
ratios are the rounding itself: 6.5e-08 (A/b1: tiny <depth>), 5.9e-08 (colour), 3.7e-09 (after the Schur pass, which stays in
float64); the cells' 4.6e-07 (even <depth>) is the difference of single terms.
"""
import copy
import functools

import numpy as np

from tests import bso, pcg_parity as pp

U = 2.0 ** -24

TOL = {
    "A/b1 fx fy cx cy": 1.01e-6,
    "A/b1 a": 1.33e-6,
    "A mixed": 5.44e-7,
    "colour H/b": 2.94e-7,
    "cell B": 2.09e-6,
    "cell D": 1.60e-6,
    "cell b2": 1.50e-6,
    "schur A/b1": 1.77e-7,
}
assert all(t <= pp.TOL_CEILING for t in TOL.values())

#               width height cell K  surfels color_scale
CASES = {
    "even":      (160, 120, 2, 3,  None, 1),   # the plain case: sizes divide evenly, 13 work slots
    "odd":       (150, 113, 4, 3,  None, 1),   # 38 x 29 grid with partial cells on both borders; the last slot is ragged
    # Depth preprocessing leaves a border of two pixels without a measurement, so the partial cells of "odd" (2 and 1 pixels
    # wide) can never be observed.  Here they are 3 pixels wide, on the same 38 x 29 grid, and are observed.
    "odd-border": (151, 115, 4, 3, None, 1),
    "odd-513":   (150, 113, 4, 3,  513,  1),   # one surfel into the second slot
    "odd-100":   (150, 113, 4, 3,  100,  1),   # most cells without an observation: D = 0 -> NaN flag -> offset 0, cfactor zeroed
    "odd-1":     (150, 113, 4, 3,  1,    1),   # one pair per keyframe at most
    "tiny":      (67,  49,  3, 2,  None, 1),   # cell 3, fewer surfels than one slot
    "k17":       (160, 120, 4, 17, None, 1),   # a second RowStash group of the keyframe walk; every cell observed
    "colour-2x": (80,  60,  2, 3,  None, 2),   # the colour camera has its own resolution (depth-to-colour map not the identity)
}
FULL_RANK = ("even", "odd", "odd-border", "tiny", "k17", "colour-2x")   # the ragged cases are rank-deficient by construction: entries only
# instantiation of intrinsics_accumulate_kernel -> (optimize_depth_intrinsics, optimize_color_intrinsics)
INSTANTIATIONS = {"depth": (True, False), "colour": (False, True), "both": (True, True)}

# the 40 sums: A[15] (upper triangle of the 5 x 5 system, row by row), b1[5], colour H[10], colour b[4], 6 unused
_A_INDEX = {(r, c): i for i, (r, c) in enumerate((r, c) for r in range(5) for c in range(r, 5))}
GLOBAL_GROUPS = {
    "A/b1 fx fy cx cy": np.array([i for (r, c), i in _A_INDEX.items() if c < 4] + [15, 16, 17, 18]),
    "A/b1 a": np.array([_A_INDEX[4, 4], 19]),
    "A mixed": np.array([_A_INDEX[r, 4] for r in range(4)]),
    "colour H/b": np.arange(20, 34),
}
assert np.array_equal(np.sort(np.concatenate(list(GLOBAL_GROUPS.values()))), np.arange(34))


def scaled_camera(width, height):
    """scenes.synthetic_scene's 640x480 camera scaled to width x height (pixel-corner convention)."""
    return bso.make_camera(525.0 * width / 640, 525.0 * height / 480, 320.0 * width / 640, 240.0 * height / 480, width, height)


@functools.lru_cache(maxsize=None)
def base_scene(width, height, cell, K, color_scale):
    """One scene per shape, with both residual types, shared by the cases and never modified."""
    return pp.variant_scene(K, cell, True, True, seed=100 + K, width=width, height=height, camera=scaled_camera(width, height),
                            color_scale=color_scale)


def case_scene(name):
    """A private copy of the case's scene: the step updates the cameras, a and the cfactor image in place."""
    width, height, cell, K, surfels, color_scale = CASES[name]
    base = base_scene(width, height, cell, K, color_scale)
    scene = copy.copy(base)   # the keyframe and surfel buffers stay shared (read only)
    scene.cfactor = base.cfactor.copy()
    if surfels is not None:
        assert base.surfels_size > surfels
        scene.surfels_size = surfels
    assert scene.a == 0.02 and scene.cfactor.all(), "the depth deformation has real values"
    return scene


@functools.lru_cache(maxsize=None)
def oracle_step(name, inst, pad=(0, 0), sentinel=-7.25):
    """The oracle's step on case `name` with its global blocks summed in float64 (bso_set_intrinsics_sum64), once per case and
    instantiation: dict(scene = the scene after the step, shadow = its float64 shadow, buffer = the cfactor buffer after the
    step).  pad = (columns, rows): the cfactor image is the top-left of a buffer that much larger, filled with `sentinel`."""
    scene = case_scene(name)
    depth, colour = INSTANTIATIONS[inst]
    h, w = scene.cfactor.shape
    buffer = np.full((h + pad[1], w + pad[0]), sentinel, np.float32)
    buffer[:h, :w] = scene.cfactor
    bso.lib().bso_set_intrinsics_sum64(1)
    try:
        scene.optimize_intrinsics(depth, colour, cfactor=buffer)
    finally:
        bso.lib().bso_set_intrinsics_sum64(0)
    scene.cfactor = buffer[:h, :w].copy()
    return dict(scene=scene, shadow=scene.intrinsics_shadow(), buffer=buffer)


def accumulated_close(sums, cells, shadow, what, tol=None):
    """Every accumulated entry of the device (sums [40]; cells [7, n] or None without depth intrinsics) against the shadow, per
    entry; an entry without terms must be exactly 0.  Returns {group: worst ratio}."""
    got, s64, a64 = [np.asarray(sums[:34], np.float64)], [shadow["sum64"][:34]], [shadow["abs64"][:34]]
    groups = dict(GLOBAL_GROUPS)
    assert not np.asarray(sums[34:]).any(), f"{what}: the unused sums are not zero"
    if cells is not None:
        n = cells.shape[1]
        got.append(np.asarray(cells, np.float64).ravel()); s64.append(shadow["cell_sum64"].ravel()); a64.append(shadow["cell_abs64"].ravel())
        groups["cell B"] = 34 + np.arange(5 * n)
        groups["cell D"] = 34 + 5 * n + np.arange(n)
        groups["cell b2"] = 34 + 6 * n + np.arange(n)
    return pp.shared_close(np.concatenate(got), (np.concatenate(s64), np.concatenate(a64)), groups, what, tol=tol or TOL)


def schur_reference(pre):
    """The Schur pass in float64 on its own fp32 inputs pre = [7, cells] (B[5], D, b2): dict(flagged [cells], cells [6, cells]
    = D^-1 B, D^-1 b2, terms [20, cells] = B_r D^-1 B_c (upper triangle, row by row) and B_r D^-1 b2).  A cell with
    !(1 / D < 1e12) in fp32 carries the NaN flag and contributes nothing."""
    pre32 = np.asarray(pre, np.float32)
    B, D, b2 = pre32[:5].astype(np.float64), pre32[5].astype(np.float64), pre32[6].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        flagged = ~(np.float32(1) / pre32[5] < np.float32(1e12))
        Dinv = np.where(flagged, 0.0, 1.0 / D)
    cells = np.concatenate([B * Dinv, (Dinv * b2)[None]])
    terms = np.array([B[r] * Dinv * B[c] for r in range(5) for c in range(r, 5)] + [B[r] * Dinv * b2 for r in range(5)])
    return dict(flagged=flagged, cells=cells, terms=terms)


def schur_close(pre, pre_sums, post, post_sums, shadow, what, tol=None):
    """The device's Schur pass judged on its own inputs (pre, pre_sums: the tap before it; post, post_sums: after it).  Cell
    outputs: 1 / D, then one product -- each correctly rounded or through the reciprocal -- so within 4 fp32 roundings of the
    float64 value, per entry; a flagged cell has D' = NaN and keeps its B.  The 20 reduced sums: against pre_sums minus the
    float64 sum of the terms, at tol * (abs64 of the entry + sum |term|).  Returns the worst ratio of the sums."""
    ref = schur_reference(pre)
    f, ok = ref["flagged"], ~ref["flagged"]
    post = np.asarray(post, np.float32)
    assert np.isnan(post[5][f]).all() and not np.isnan(post[5][ok]).any(), f"{what}: the NaN flags are not those of !(1 / D < 1e12)"
    assert np.array_equal(post[:5][:, f].view(np.uint32), np.asarray(pre, np.float32)[:5][:, f].view(np.uint32)), f"{what}: a flagged cell's B changed"
    err = np.abs(post.astype(np.float64) - ref["cells"])[:, ok]
    bound = 4 * U * np.abs(ref["cells"])[:, ok]
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0, (f"{what}: {len(bad)} cell outputs of the Schur pass off, first row {bad[0][0]} cell {np.flatnonzero(ok)[bad[0][1]]}: "
                           f"|diff| {err[tuple(bad[0])]:.3e} > {bound[tuple(bad[0])]:.3e}")
    want = np.asarray(pre_sums[:20], np.float64) - ref["terms"].sum(axis=1)
    scale = shadow["abs64"][:20] + np.abs(ref["terms"]).sum(axis=1)
    worst = pp.shared_close(post_sums[:20], (want, scale), {"schur A/b1": np.arange(20)}, what, tol=tol or TOL)
    assert np.array_equal(np.asarray(post_sums[20:], np.float64), np.asarray(pre_sums[20:], np.float64)), \
        f"{what}: the Schur pass changed a colour sum"
    return worst


def solve_close(upper, rhs, x, what):
    """The host solve judged on its own inputs: x against the float64 solution of the symmetric system given by its upper
    triangle (row by row) and rhs.  Both sides factor in float64; with the system scaled to a unit diagonal (M' = S M S,
    S = diag(M)^-1/2, which a symmetric factorisation's error bound is invariant under) the forward error is at most
    n eps cond(M') of the largest scaled component, taken as 8 * 2^-53 * cond(M'), plus the rounding of x to fp32."""
    n = len(rhs)
    M = np.zeros((n, n))
    M[np.triu_indices(n)] = np.asarray(upper, np.float64)
    M = M + np.triu(M, 1).T
    assert (np.diag(M) > 0).all(), f"{what}: the system has an empty diagonal entry"
    d = np.sqrt(np.diag(M))
    Ms = M / np.outer(d, d)
    y = np.linalg.solve(Ms, np.asarray(rhs, np.float64) / d)   # = d * x
    bound = (8 * 2.0 ** -53 * np.linalg.cond(Ms) + U) * np.abs(y).max()
    err = np.abs(d * np.asarray(x, np.float64) - y)
    assert np.all(err <= bound), f"{what}: solve off by {err.max():.3e} > {bound:.3e} (scaled components), x {np.asarray(x)!r}, float64 {y / d!r}"
    return float(err.max() / bound)


def pixel_update_close(old, new, post, x1, obs, what):
    """The cfactor update judged on its own inputs: new = old - (D' - sum B' x1) in float64 from the tapped D', B' (post
    [6, cells]) and x1; exactly 0 where the cell has no observation, old unchanged where it is flagged.  Per cell within 1e-6 of
    the largest intermediate (the bound test_gpu_pcg_variants.entrywise_close derives for elementwise kernels)."""
    old, new = np.asarray(old, np.float32).ravel(), np.asarray(new, np.float32).ravel()
    post64, x64 = np.asarray(post, np.float64), np.asarray(x1, np.float64)
    flagged = np.isnan(post64[5])
    prod = post64[:5] * x64[:, None]
    offset = np.where(flagged, 0.0, post64[5] - prod.sum(axis=0))
    want = np.where(obs == 0, 0.0, old.astype(np.float64) - offset)
    scale = np.abs(old) + np.where(flagged, 0.0, np.abs(post64[5]) + np.abs(prod).sum(axis=0))
    exact = (obs == 0) | flagged
    assert np.array_equal(new[exact].view(np.uint32), want[exact].astype(np.float32).view(np.uint32)), \
        f"{what}: a cell without observation is not 0, or a flagged cell changed"
    err = np.abs(new.astype(np.float64) - want)
    bad = np.flatnonzero(~(err <= 1e-6 * scale))
    assert bad.size == 0, f"{what}: {bad.size} cfactor cells off, first cell {bad[0]}: got {new[bad[0]]!r}, float64 {want[bad[0]]!r}, scale {scale[bad[0]]:.3e}"
