"""Shared pieces of the PCG parity tests: small scenes with a real depth deformation, the entry groups of an unknown layout
and the per-entry comparator for the entries that every (keyframe, surfel) pair adds to."""
import numpy as np

from badslam_amd import abi
from tests import bso, scenes

WIDTH, HEIGHT = 160, 120
INVALID = abi.INVALID_INDEX


def small_camera():
    """scenes.synthetic_scene's 640x480 camera scaled to 160x120 (pixel-corner convention: everything scales by 1/4)."""
    return bso.make_camera(525.0 / 4, 525.0 / 4, 320.0 / 4, 240.0 / 4, WIDTH, HEIGHT)


def variant_scene(K, cell, use_depth, use_desc, seed, a=0.02, cfactor_range=0.01, width=WIDTH, height=HEIGHT, camera=None, color_scale=1):
    """synthetic_scene at 160x120 (or width x height with `camera`), perturbed as test_gpu_pcg.perturbed_scene does (surfel depth
    noise, keyframe poses off by a small twist), then given a depth deformation with real values: with a = 0 and cfactor = 0 the
    `a` column of the depth-intrinsics Jacobian is identically zero."""
    assert camera is not None or (width, height) == (WIDTH, HEIGHT), "another image size needs its own camera"
    scene = scenes.synthetic_scene(K, seed=seed, width=width, height=height, cell=cell, camera=camera or small_camera(),
                                   use_depth_residuals=use_depth, use_descriptor_residuals=use_desc, color_scale=color_scale)
    rng = np.random.default_rng(seed)
    n = scene.surfels_size
    scene.surfels[2, :n] += rng.uniform(-0.003, 0.003, n).astype(np.float32)
    for kf in scene.keyframes[1:]:
        x = np.concatenate([rng.uniform(-0.002, 0.002, 3), rng.uniform(-0.0005, 0.0005, 3)]).astype(np.float32)
        kf.global_T_frame = bso.se3_mul(kf.global_T_frame, bso.se3_exp(x))
    scene.a = a
    scene.cfactor[:] = rng.uniform(-cfactor_range, cfactor_range, scene.cfactor.shape).astype(np.float32)
    return scene


def entry_groups(scene, layout):
    """{group name: index array} over the unknowns of `layout`.  "surfels" are the per-surfel entries; every other group is
    shared: each of its entries is a sum over every (keyframe, surfel) pair."""
    groups = {}
    K = len(scene.keyframes)
    if layout.optimize_poses:
        groups["poses"] = np.arange(6 * (K - 1))
    if layout.optimize_geometry:
        per = 3 if layout.use_descriptor_residuals else 1
        groups["surfels"] = layout.surfel_unknown_start_index + np.arange(per * scene.surfels_size)
    if layout.optimize_depth_intrinsics:
        d0 = layout.depth_intrinsics_unknown_start_index
        groups["depth fx fy cx cy"] = d0 + np.arange(4)
        groups["depth a"] = np.array([layout.a_unknown_index])
        groups["cfactor cells"] = d0 + 5 + np.arange(scene.cfactor.size)
    if layout.optimize_color_intrinsics:
        groups["colour fx fy cx cy"] = layout.color_intrinsics_unknown_start_index + np.arange(4)
    covered = np.concatenate([np.asarray(g) for g in groups.values()]) if groups else np.zeros(0, np.int64)
    assert np.array_equal(np.sort(covered), np.arange(layout.unknown_count)), "the groups partition the unknowns"
    return groups


def shared_groups(scene, layout):
    return {name: idx for name, idx in entry_groups(scene, layout).items() if name != "surfels"}


# Shared entries: |device - sum64| <= tol * abs64 per entry, where sum64 / abs64 are the oracle's float64 sums of its own fp32
# terms and of their absolute values (bso_pcg_last_shared_sums).  The ceiling is what the project grants summed pose entries
# (tests/test_gpu_pcg.py).  The committed values are four times the worst ratio measured on an MI355X over r, M and g of every
# case of tests/test_gpu_pcg_variants.py, capped at the ceiling: the device contracts products that the oracle does not (and
# divides through the hardware reciprocal), so single terms differ by a few ulps in a data-dependent way.
#                          measured worst ratio      case it came from
#   poses                  2.417e-07                 k65-b
#   depth fx fy cx cy      1.308e-07                 a, b, d, f (K = 3, cell 2)
#   depth a                1.518e-07                 k17-b
#   cfactor cells          1.894e-06                 first100-b (cells with one to three terms: the terms' own difference)
#   colour fx fy cx cy     1.442e-07                 b-gauge-last
#   alpha_d                1.315e-06                 k65-b
TOL_CEILING = 1e-4
SHARED_TOL = {
    "poses": 9.7e-7,
    "depth fx fy cx cy": 5.3e-7,
    "depth a": 6.1e-7,
    "cfactor cells": 7.6e-6,
    "colour fx fy cx cy": 5.8e-7,
    "alpha_d": 5.3e-6,   # one more sum over every pair, against bso_pcg_last_alpha_d64 (all terms >= 0: abs64 = sum64)
}
assert all(t <= TOL_CEILING for t in SHARED_TOL.values())

measured = {}   # group -> worst ratio seen by shared_close in this process (printed by the GPU tests' report)


def shared_ratio(got, sum64, abs64):
    """Per-entry |got - sum64| / abs64; an entry with abs64 == 0 gives 0 where got is exactly 0 and inf elsewhere."""
    got, sum64, abs64 = (np.asarray(x, np.float64) for x in (got, sum64, abs64))
    err = np.abs(got - sum64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(abs64 > 0, err / abs64, np.where(got == 0, 0.0, np.inf))


def shared_close(got, sums, groups, what, tol=None):
    """Asserts every shared entry of the full-length vector `got` against sums = (sum64, abs64[, terms]), entry by entry,
    never by a group's maximum.  Returns {group: worst ratio}."""
    sum64, abs64 = sums[0], sums[1]
    worst = {}
    failures = []
    for name, idx in groups.items():
        if name == "surfels" or len(idx) == 0:
            continue
        t = (tol or SHARED_TOL)[name]
        ratio = shared_ratio(np.asarray(got)[idx], sum64[idx], abs64[idx])
        worst[name] = float(ratio.max())
        measured[name] = max(measured.get(name, 0.0), worst[name]) if np.isfinite(worst[name]) else measured.get(name, 0.0)
        bad = np.flatnonzero(~(ratio <= t))
        if bad.size:
            j = bad[np.argmax(ratio[bad])]
            failures.append(f"{what} [{name}]: {bad.size} of {len(idx)} entries off, worst at unknown {idx[j]}: got {np.asarray(got)[idx[j]]!r}, "
                            f"sum64 {sum64[idx[j]]!r}, abs64 {abs64[idx[j]]!r}, ratio {ratio[j]:.3e} > {t:g}")
    assert not failures, "\n".join(failures)
    return worst


def ulp_distance(a, b):
    """Distance in representable fp32 values between two float32 arrays."""
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(ordered(a) - ordered(b))


def rel_close(a, b, rel, what):
    """test_gpu_pcg.close: max |a - b| over the slice's largest |b| (for runs of like-scaled entries and for scalars)."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    if b.size == 0:
        return 0.0
    scale = max(np.abs(b).max(), 1e-30)
    err = np.abs(a - b).max() / scale
    assert err <= rel, f"{what}: max rel err {err:.3e} > {rel}"
    return err
