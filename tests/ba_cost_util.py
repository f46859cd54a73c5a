"""The BA objective in float64 from the oracle's per-surfel residual probe, for the tests of bslam_compute_ba_cost.

The oracle's bso_accumulate_pose_estimation_coeffs(per_surfel=...) writes [raw, w, r1, w1, r2, w2, flags, 0] per surfel (flags
bit 0: associated, bit 1: descriptor residuals valid).  The objective is Tukey on the depth residuals and kDescWeight * Huber on
both descriptor residuals (BS/robust_weighting.cuh, BS/cost_function.cuh), summed over the associated pairs."""
import ctypes as C

import numpy as np


DEPTH_TUKEY = 10.0
DESC_HUBER = 10.0
DESC_WEIGHT = 1e-2


def tukey_residual(r, k=DEPTH_TUKEY):
    r = np.asarray(r, np.float64)
    t = 1.0 - (r / k) ** 2
    return np.where(np.abs(r) < k, (k * k / 6.0) * (1.0 - t ** 3), k * k / 6.0)


def huber_residual(r, k=DESC_HUBER):
    r = np.asarray(r, np.float64)
    a = np.abs(r)
    return np.where(a < k, 0.5 * r * r, k * (a - 0.5 * k))


def objective_from_probe(per_surfel, use_depth, use_desc, mask=None):
    """(cost[2] float64, counts[2] int) of one keyframe from the per-surfel probe; `mask`: surfels that take part (bool array)."""
    ps = np.asarray(per_surfel)
    flags = ps[:, 6].astype(np.int64)
    take = np.ones(len(ps), bool) if mask is None else np.asarray(mask, bool)
    depth = take & ((flags & 1) != 0) & bool(use_depth)
    desc = take & ((flags & 2) != 0) & bool(use_desc)
    cost = np.array([tukey_residual(ps[depth, 0]).sum(),
                     DESC_WEIGHT * (huber_residual(ps[desc, 2]) + huber_residual(ps[desc, 4])).sum()], np.float64)
    return cost, np.array([int(depth.sum()), int(desc.sum())], np.int64)


def oracle_per_surfel(color_camera, depth_camera, depth_params, depth, normals, color, frame_T_global, surfels, surfels_size, tex_mode,
                      use_depth, use_desc):
    """The oracle's per-surfel probe of one keyframe on host arrays: (per_surfel [S, 8] float32, count, cost)."""
    from tests import bso
    L = bso.lib()
    P = C.POINTER
    surfels = np.ascontiguousarray(surfels, np.float32)
    ps = np.zeros((max(1, surfels_size), 8), np.float32)
    H, b = np.zeros(21, np.float32), np.zeros(6, np.float32)
    H64, b64 = np.zeros(21, np.float64), np.zeros(6, np.float64)
    count, cost = C.c_uint32(), C.c_float()
    L.bso_accumulate_pose_estimation_coeffs(int(use_depth), int(use_desc), C.byref(color_camera), C.byref(depth_camera), C.byref(depth_params),
                                            C.byref(bso.np_buffer2d(depth)), C.byref(bso.np_buffer2d(normals)), C.byref(bso.np_buffer2d(color)),
                                            C.byref(frame_T_global), surfels_size, C.byref(bso.np_buffer2d(surfels)), tex_mode, C.byref(count),
                                            C.byref(cost), bso.fptr(H), bso.fptr(b), H64.ctypes.data_as(P(C.c_double)),
                                            b64.ctypes.data_as(P(C.c_double)), bso.fptr(ps))
    return ps[:surfels_size], count.value, cost.value


def scene_objective(scene, mask=None, surfels_size=None, use_depth=None, use_desc=None):
    """(cost [K, 2] float64, counts [K, 2]) of a tests.bso.HostScene at its keyframes' poses, from the oracle."""
    use_depth = scene.use_depth_residuals if use_depth is None else use_depth
    use_desc = scene.use_descriptor_residuals if use_desc is None else use_desc
    n = scene.surfels_size if surfels_size is None else surfels_size
    saved = scene.surfels_size
    scene.surfels_size = n
    try:
        cost, counts = [], []
        for kf in scene.keyframes:
            r = scene.accumulate_pose(kf, per_surfel=True, use_depth=use_depth, use_desc=use_desc)
            m = None if mask is None else np.asarray(mask[:n], bool)
            c, k = objective_from_probe(r["per_surfel"], use_depth, use_desc, m)
            cost.append(c)
            counts.append(k)
    finally:
        scene.surfels_size = saved
    return np.array(cost), np.array(counts)



def oracle_terms(got_cost, want_cost, want_counts):
    """[(keyframe, residual type, |device - oracle|, tolerance)] of a cost table against scene_objective's: 1e-4 relative, plus 1e-9
    per pair for sums of near-zero terms (at the true poses a depth residual is a rounding error, formed with fused multiply-adds on
    the device and without on the host)."""
    out = []
    for k in range(len(want_cost)):
        for j in range(2):
            tol = 1e-4 * abs(want_cost[k, j]) + 1e-9 * max(1, int(want_counts[k, j]))
            out.append((k, j, abs(float(got_cost[k, j]) - want_cost[k, j]), tol))
    return out
