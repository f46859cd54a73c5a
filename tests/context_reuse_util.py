"""Shared pieces of the context re-use tests (test_context_reuse_cpu.py, test_gpu_context_reuse.py): a scene on which every
cached path of a bslam_context is live, mutations that change the inputs between two calls (on the host scene and, when there is
one, on the device tensors alike, so that the oracle sees what the device sees), and for each observer -- an entry point whose
output depends on what the context caches -- the reference the suite already trusts, its comparator with the committed tolerance,
and the margin by which two references differ (the precondition that a stale answer cannot pass).

    observer     entry point                                    reference                          comparator
    fuse         bslam_fuse_keyframes                           fusion_util.fuse                   bit for bit
    pose         bslam_accumulate_pose_coeffs_batched           HostScene.accumulate_pose H64/b64  counts exact, 1e-4 (test_gpu_large_configs)
    cost         bslam_compute_ba_cost                          ba_cost_util.scene_objective       test_gpu_ba_cost.check_against_oracle
    pcg, pcg_di  bslam_pcg_init + bslam_pcg_step1 (+ depth      HostPCG, float64 shadow sums       pcg_parity.shared_close at SHARED_TOL, surfel
                 intrinsics)                                                                       entries at test_gpu_pcg_variants' 1e-6 / 1e-5
    activation   bslam_update_surfel_activation                 oracle                             flags exact
    geometry     bslam_optimize_geometry_iteration              oracle                             test_gpu_parity: normals exact, rows 1e-4
    normals      bslam_update_surfel_normals                    oracle                             test_gpu_parity: every row exact
"""
import contextlib
import copy
import ctypes as C
import functools

import numpy as np

from badslam_amd import abi
from tests import ba_cost_util, bso, fusion_util as fu, pcg_parity as pp

P = C.POINTER
BASE_K = 5                    # keyframes in the list; the scene holds one more for the list to grow by
MUT_KF = 1                    # the keyframe whose images the mutations rewrite
CELL = 1
DIMS, VOXEL, TRUNCATION = (40, 32, 24), 0.02, 0.08
MIN_KEYFRAMES, MIN_SURFELS = 4, 16129          # kPermMinKeyframes; 64 granules of 256 surfels (make_schedule)


# ----------------------------------------------------------------------------- scenes

def clone_scene(s):
    """A HostScene with buffers of its own."""
    c = copy.copy(s)
    c.cfactor, c.surfels, c.active = s.cfactor.copy(), s.surfels.copy(), s.active.copy()
    c.keyframes = [clone_keyframe(kf) for kf in s.keyframes]
    if hasattr(s, "spare"):
        c.spare = [clone_keyframe(kf) for kf in s.spare]
    return c


def clone_keyframe(kf):
    return bso.HostKeyframe(kf.depth.copy(), kf.normals.copy(), kf.radius.copy(), kf.color.copy(), kf.global_T_frame, kf.id, kf.activation,
                            kf.min_depth, kf.max_depth)


def _volume_origin(scene):
    """A volume around the surface point that MUT_KF sees in the middle of its image."""
    kf = scene.keyframes[MUT_KF]
    h, w = kf.depth.shape
    cam = scene.depth_camera
    z = float(kf.depth[h // 2, w // 2] & 0x7fff) * scene.raw_to_float_depth
    local = np.array([(w / 2 - cam.cx) / cam.fx * z, (h / 2 - cam.cy) / cam.fy * z, z])
    M = np.array(list(bso.se3_matrix3x4(kf.global_T_frame).m), np.float64).reshape(3, 4)
    centre = M[:, :3] @ local + M[:, 3]
    return tuple(float(np.float32(v)) for v in centre - 0.5 * VOXEL * np.array(DIMS))


@functools.lru_cache(maxsize=None)
def _base_scene(use_desc):
    scene = pp.variant_scene(BASE_K + 1, CELL, True, use_desc, seed=41)
    scene.spare = [scene.keyframes.pop()]
    scene.origin = _volume_origin(scene)
    # the last columns hold surfels in a corner of the spare keyframe's image that no other keyframe sees; surfels from the middle of
    # keyframe 0's image take their place (the order of the columns means nothing), so that lowering surfels_size removes residuals
    n = scene.surfels_size
    tail, mid = slice(n - 64, n), slice(9600, 9664)
    scene.surfels[:, tail], scene.surfels[:, mid] = scene.surfels[:, mid].copy(), scene.surfels[:, tail].copy()
    return scene


def base_scene(use_desc):
    """pcg_parity.variant_scene at 160 x 120 with a = 0.02 and a real cfactor image: BASE_K keyframes in the list and one
    spare whose surfels are part of the cloud.  Every call returns a copy of its own."""
    return clone_scene(_base_scene(bool(use_desc)))


@functools.lru_cache(maxsize=None)
def _k65_scene():
    # the k65 recipe of test_gpu_pcg_variants (65 keyframes, seed 100 + K); at its cell size of 4 the cloud has 5556 surfels, below
    # the 64 granules from which make_schedule orders anything, so the cell is 1 here: 58039 surfels, 227 granules (about 1 s of
    # oracle time per pose reference)
    scene = pp.variant_scene(65, 1, True, True, seed=165)
    scene.spare = []
    scene.origin = _volume_origin(scene)
    return scene


def k65_scene():
    return clone_scene(_k65_scene())


def check_thresholds(scene):
    n = scene.surfels_size
    assert len(scene.keyframes) >= MIN_KEYFRAMES, "per-surfel order needs 4 keyframes"
    assert n >= MIN_SURFELS, f"{n} surfels: below 64 granules the work order is the identity"
    assert n % 256 != 0, "a ragged last granule"
    assert scene.a != 0 and scene.cfactor.any()


# ----------------------------------------------------------------------------- mutations
# mutation(h, d): h the HostScene, d its bso.DeviceScene or None.  Device tensors that a mutation replaces stay alive in d.keep,
# with their old content, so that the address is not handed out again and a stale pointer reads the old values.

def _t(d, array):
    return d.torch.from_numpy(np.ascontiguousarray(array)).to(d.device)


def _keep(d, tensor):
    if not hasattr(d, "keep"):
        d.keep = []
    d.keep.append(tensor)


def _sync_image(h, d, k, which):
    if d is not None:
        kf = h.keyframes[k]
        src = (kf.depth.view(np.int16), kf.normals.view(np.int16), kf.radius.view(np.int16), kf.color)[which]
        d.kf_tensors[k][which].copy_(_t(d, src))


def _sync_surfels(h, d):
    if d is not None:
        d.surfels.copy_(_t(d, h.surfels))
        d.surfels_size = h.surfels_size


def _shift_block(depth, raw_units):
    block = depth[30:90, 40:120]
    valid = (block & 0x8000) == 0
    block[valid] = np.minimum(block[valid].astype(np.int64) + raw_units, 0x7fff).astype(np.uint16)


def depth_shift(h, d):                        # 3 cm at 1 / 5000 m per unit
    _shift_block(h.keyframes[MUT_KF].depth, 150)
    _sync_image(h, d, MUT_KF, 0)


def depth_invalid_stripe(h, d):
    h.keyframes[MUT_KF].depth[50:70, :] ^= 0x8000
    _sync_image(h, d, MUT_KF, 0)


def normals_image(h, d):
    n = h.keyframes[MUT_KF].normals
    x = (n[20:, :] & 0xff).astype(np.uint8).view(np.int8).astype(np.int32)
    x = np.clip(x + 70, -127, 127).astype(np.int8).view(np.uint8).astype(np.uint16)
    n[20:, :] = (n[20:, :] & 0xff00) | x
    _sync_image(h, d, MUT_KF, 1)


def colour_image(h, d):
    c = h.keyframes[MUT_KF].color
    c[10:110, 10:150] = 255 - c[10:110, 10:150]       # r, g, b and the luma channel
    _sync_image(h, d, MUT_KF, 3)


def colour_moved(h, d):
    """MUT_KF's colour image in a new tensor with other content; the old tensor keeps the old content."""
    c = h.keyframes[MUT_KF].color
    c[5:115, 20:140] = 255 - c[5:115, 20:140]
    if d is not None:
        old = d.kf_tensors[MUT_KF]
        _keep(d, old[3])
        d.kf_tensors[MUT_KF] = tuple(old[:3]) + (_t(d, c),)


def _new_cfactor(h, seed):
    """Other values in the range of pcg_parity.variant_scene's, for which the committed tolerances were measured (three times that
    range puts single-term cfactor cells of the PCG 60 times over SHARED_TOL on a fresh context as well: terms near the Tukey cutoff)."""
    return np.random.default_rng(seed).uniform(-0.01, 0.01, h.cfactor.shape).astype(np.float32)


def cfactor_inplace(h, d):
    h.cfactor[:] = _new_cfactor(h, 5)
    if d is not None:
        d.cfactor.copy_(_t(d, h.cfactor))


def cfactor_moved(h, d):
    h.cfactor = _new_cfactor(h, 6)
    if d is not None:
        _keep(d, d.cfactor)
        d.cfactor = _t(d, h.cfactor)


def a_changed(h, d):
    h.a = -0.05


def raw_to_float_changed(h, d):
    h.raw_to_float_depth = float(np.float32(1.0 / 4900))


def depth_moved(h, d):
    """MUT_KF's depth in a new tensor with a shifted block; the old tensor keeps the old content."""
    _shift_block(h.keyframes[MUT_KF].depth, -140)
    if d is not None:
        old = d.kf_tensors[MUT_KF]
        _keep(d, old[0])
        d.kf_tensors[MUT_KF] = (_t(d, h.keyframes[MUT_KF].depth.view(np.int16)),) + tuple(old[1:])


def depth_repitched(h, d, pad=8):
    """MUT_KF's depth at the address of before in rows `pad` elements wider, with a shifted block.  (The same content would give
    the same records whether they are rebuilt or not: only new content shows that the pitch is looked at.)  The wider tensor
    is allocated once per device scene, so that the address stays."""
    _shift_block(h.keyframes[MUT_KF].depth, 120)
    if d is not None:
        depth = h.keyframes[MUT_KF].depth
        hh, ww = depth.shape
        big = d.pitch_store                     # make_pitch_store put MUT_KF's depth at its start
        flat = big.view(-1)
        flat[:hh * (ww + pad)].view(hh, ww + pad)[:, :ww].copy_(_t(d, depth.view(np.int16)))
        d.kf_tensors[MUT_KF] = (flat[:hh * (ww + pad)].view(hh, ww + pad)[:, :ww],) + tuple(d.kf_tensors[MUT_KF][1:])


def make_pitch_store(d, pad=8):
    """Moves MUT_KF's depth into a tensor with room for the wider rows of depth_repitched (same address before and after)."""
    t = d.kf_tensors[MUT_KF][0]
    hh, ww = t.shape
    d.pitch_store = d.torch.zeros((hh, ww + pad), dtype=t.dtype, device=d.device)
    view = d.pitch_store.view(-1)[:hh * ww].view(hh, ww)
    view.copy_(t)
    _keep(d, t)
    d.kf_tensors[MUT_KF] = (view,) + tuple(d.kf_tensors[MUT_KF][1:])


def _renumber(h):
    for i, kf in enumerate(h.keyframes):
        kf.id = i                               # the PCG path wants ids 0 .. K-1 in list order


def reorder(h, d):
    order = [3, 0, 4, 1, 2] + list(range(5, len(h.keyframes)))
    h.keyframes = [h.keyframes[i] for i in order]
    if d is not None:
        d.kf_tensors = [d.kf_tensors[i] for i in order]
    _renumber(h)


def shorten(h, d):
    h.spare.append(h.keyframes.pop())
    if d is not None:
        d.spare_tensors.append(d.kf_tensors.pop())


def lengthen(h, d):                            # restores after shorten; from the base list, grows it by the spare keyframe
    h.keyframes.append(h.spare.pop())
    if d is not None:
        d.kf_tensors.append(d.spare_tensors.pop())
    _renumber(h)


def pose_changed(h, d):
    kf = h.keyframes[MUT_KF]
    kf.global_T_frame = bso.se3_mul(kf.global_T_frame, bso.se3_exp(np.array([0.02, -0.015, 0.01, 0.004, -0.003, 0.002], np.float32)))


def surfel_normals(h, d):
    n = h.surfels_size
    h.surfels[3, :n] = np.roll(h.surfels[3, :n], 5003)
    _sync_surfels(h, d)


def surfel_descriptors(h, d):
    n = h.surfels_size
    h.surfels[6:8, :n] = h.surfels[6:8, :n][::-1] * np.float32(0.5) + np.float32(20)
    _sync_surfels(h, d)


def surfel_radii(h, d):
    h.surfels[4, :h.surfels_size] *= np.float32(9.0)
    _sync_surfels(h, d)


def surfel_positions(h, d):
    n = h.surfels_size
    rng = np.random.default_rng(77)
    h.surfels[:3, :n] += rng.uniform(-0.02, 0.02, (3, n)).astype(np.float32)
    _sync_surfels(h, d)


def size_minus_37(h, d):
    h.surfels_size -= 37
    if d is not None:
        d.surfels_size = h.surfels_size


def surfels_moved(h, d):
    """The surfel buffer in another tensor, displaced a little; the old tensor keeps the old surfels."""
    n = h.surfels_size
    h.surfels = h.surfels.copy()
    h.surfels[2, :n] += np.random.default_rng(78).uniform(-0.02, 0.02, n).astype(np.float32)
    if d is not None:
        _keep(d, d.surfels)
        d.surfels = _t(d, h.surfels)


MUTATIONS = {f.__name__: f for f in (
    depth_shift, depth_invalid_stripe, normals_image, colour_image, colour_moved, cfactor_inplace, cfactor_moved, a_changed, raw_to_float_changed,
    depth_moved, depth_repitched, reorder, shorten, lengthen, pose_changed, surfel_normals, surfel_descriptors, surfel_radii,
    surfel_positions, size_minus_37, surfels_moved)}
IN_PLACE_CONTENT = ("depth_shift", "depth_invalid_stripe", "normals_image", "colour_image", "cfactor_inplace")   # need an invalidate under the keyframe cache
NOTICED_BY_SIGNATURE = ("colour_moved", "cfactor_moved", "a_changed", "raw_to_float_changed", "depth_moved", "depth_repitched", "reorder", "shorten", "lengthen")

# The observers each mutation is paired with; "photo" observers run on the scene with descriptor residuals.  Every pair meets the
# precondition of test_context_reuse_cpu.py.
PAIRS = {
    "depth_shift": ("fuse", "pose", "cost", "pcg"),
    "depth_invalid_stripe": ("fuse", "pose", "cost", "pcg_di", "activation"),
    "normals_image": ("pose", "pcg", "normals"),
    "colour_image": ("fuse", "pose", "cost"),
    "colour_moved": ("fuse", "pose", "cost", "pcg"),
    "cfactor_inplace": ("fuse", "pose", "cost", "pcg_di"),
    "cfactor_moved": ("fuse", "pose", "pcg"),
    "a_changed": ("fuse", "pose", "cost", "pcg_di"),
    "raw_to_float_changed": ("fuse", "pose", "cost"),
    "depth_moved": ("fuse", "pose", "pcg"),
    "depth_repitched": ("fuse", "pose"),
    "reorder": ("pose", "cost", "pcg"),
    "shorten": ("fuse", "pose", "pcg"),
    "lengthen": ("fuse", "pose", "pcg"),
    "pose_changed": ("fuse", "pose", "cost", "pcg", "activation"),
    "surfel_normals": ("pose", "pcg", "activation"),
    "surfel_descriptors": ("pose", "cost", "pcg"),
    "surfel_radii": ("pose", "pcg"),
    "surfel_positions": ("pose", "cost", "pcg", "activation", "geometry"),
    "size_minus_37": ("pose", "cost", "pcg"),     # counts: 37 surfels seen by most keyframes, over 100 residuals
    "surfels_moved": ("pose", "cost", "pcg", "geometry"),
}
BOTH_SCENES = ("depth_shift", "depth_moved", "a_changed", "surfel_positions")      # run on the depth-only and on the photometric scene
PHOTO_ONLY = ("colour_image", "colour_moved", "surfel_descriptors", "surfel_radii")    # mutations that only descriptor residuals (or colour) see


def scene_kinds(mutation):
    """Whether the scenes a mutation runs on have descriptor residuals."""
    return (True,) if mutation in PHOTO_ONLY else (False, True) if mutation in BOTH_SCENES else (False,)


# ----------------------------------------------------------------------------- references

def pcg_layout_of(scene, depth_intrinsics):
    return bso.pcg_layout(scene, optimize_poses=True, optimize_geometry=True, optimize_depth_intrinsics=depth_intrinsics, gauge_keyframe_id=1)


class PcgRef:
    """The oracle's init, init2 and first step 1 on a scene: r, M, g with their float64 shadow sums, the vectors that go into
    step 1 (`loaded`), alpha_d in float64."""

    def __init__(self, scene, depth_intrinsics):
        self.layout = pcg_layout_of(scene, depth_intrinsics)
        self.n = self.layout.unknown_count
        self.groups = pp.entry_groups(scene, self.layout)
        self.shared = pp.shared_groups(scene, self.layout)
        self.surf = self.groups["surfels"]
        ref = bso.HostPCG(scene, self.layout)
        ref.init()
        self.r, self.M = ref.r.copy(), ref.M.copy()
        self.r_sums, self.M_sums = ref.shared_sums("r"), ref.shared_sums("M")
        ref.init2()
        self.loaded = copy.copy(ref)
        for nm in ref.NAMES:
            setattr(self.loaded, nm, getattr(ref, nm).copy())
        self.loaded.scalars = ref.scalars.copy()
        ref.step1(False)
        self.g, self.g_sums = ref.g.copy(), ref.shared_sums("g")
        self.alpha_d64 = bso.lib().bso_pcg_last_alpha_d64()


def _fuse_ref(s):
    kfs = [fu.Keyframe(kf.depth, kf.color, list(kf.view().frame_T_global.m)) for kf in s.keyframes]
    tsdf, count, color = fu.fuse(kfs, s.depth_camera, s.color_camera, s.cfactor, s.a, s.raw_to_float_depth, s.cell, s.origin, VOXEL, DIMS, TRUNCATION, True)
    return dict(tsdf=tsdf, count=count, color=color)


def _pose_ref(s):
    rs = [s.accumulate_pose(kf) for kf in s.keyframes]
    return dict(H=np.array([r["H64"] for r in rs]), b=np.array([r["b64"] for r in rs]), count=np.array([r["count"] for r in rs], np.int64))


def _cost_ref(s):
    cost, counts = ba_cost_util.scene_objective(s)
    return dict(cost=cost, counts=counts)


@contextlib.contextmanager
def only_mut_kf_active(s):
    """The activation observer's keyframe states on a HostScene: only the keyframe at MUT_KF is active, so a surfel's flag is its
    association with that keyframe.  The states of before come back on leaving."""
    saved = [kf.activation for kf in s.keyframes]
    try:
        for i, kf in enumerate(s.keyframes):
            kf.activation = abi.KF_ACTIVE if i == MUT_KF else abi.KF_INACTIVE
        yield
    finally:
        for kf, a in zip(s.keyframes, saved):
            kf.activation = a


def active_start(s):
    """Flags before an activation pass: bits 0 and 1 at random, so that a pass has flags to clear as well as to set."""
    return np.random.default_rng(3).integers(0, 4, s.active.shape).astype(np.uint8)


def _activation_ref(s):
    saved = s.active.copy()
    try:
        with only_mut_kf_active(s):
            s.active[:] = active_start(s)
            s.update_activation()
            return dict(flags=s.active[0, :s.surfels_size].copy())
    finally:
        s.active[:] = saved


def _writer_ref(s, which):
    saved = s.surfels.copy()
    try:
        (s.optimize_geometry_iteration if which == "geometry" else s.update_normals)()
        return dict(rows=s.surfels[:8, :s.surfels_size].copy())
    finally:
        s.surfels[:] = saved


REFERENCES = {
    "fuse": _fuse_ref, "pose": _pose_ref, "cost": _cost_ref,
    "pcg": lambda s: PcgRef(s, False), "pcg_di": lambda s: PcgRef(s, True),
    "activation": _activation_ref,
    "geometry": lambda s: _writer_ref(s, "geometry"), "normals": lambda s: _writer_ref(s, "normals"),
}


# ----------------------------------------------------------------------------- comparators and margins

def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _exact(got, ref, what):
    differ = _bits(got) != _bits(ref)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {differ.size} values differ, first at {np.argwhere(differ)[0]}"


def _pose_terms(got, ref):
    """[(error, tolerance)] per keyframe for H and b: the bar of test_gpu_large_configs (bso.pose_coeff_terms)."""
    return [t for k in range(len(ref["H"])) for t in bso.pose_coeff_terms(got["H"][k], got["b"][k], ref["H"][k], ref["b"][k])]


def _cost_terms(got, ref):
    """check_against_oracle of test_gpu_ba_cost, entry by entry (ba_cost_util.oracle_terms)."""
    return [(err, tol) for _, _, err, tol in ba_cost_util.oracle_terms(got["cost"], ref["cost"], ref["counts"])]


def _rows_terms(got, ref):
    """test_gpu_parity.test_geometry_iteration_matches_oracle: positions and descriptors at 1e-4 of max(1, largest entry)."""
    return [(np.abs(got["rows"][r].astype(np.float64) - ref["rows"][r]).max(), 1e-4 * max(1.0, float(np.abs(ref["rows"][r]).max()))) for r in (0, 1, 2, 6, 7)]


def check(observer, got, ref, what):
    """Holds an observer's device output to its reference with the comparator the suite commits to."""
    if observer == "fuse":
        for name in ("tsdf", "count", "color"):
            _exact(got[name], ref[name], f"{what}: {name}")
    elif observer == "pose":
        assert np.array_equal(got["count"], ref["count"]), f"{what}: counts {got['count']} != {ref['count']}"
        for i, (err, tol) in enumerate(_pose_terms(got, ref)):
            assert err <= tol, f"{what}: keyframe {i // 2} {'Hb'[i % 2]}: {err:.3e} > {tol:.3e}"
    elif observer == "cost":
        assert np.array_equal(np.asarray(got["counts"], np.int64), ref["counts"]), f"{what}: counts"
        for i, (err, tol) in enumerate(_cost_terms(got, ref)):
            assert err <= tol, f"{what}: entry {i}: {err:.3e} > {tol:.3e}"
    elif observer in ("pcg", "pcg_di"):
        check_pcg_init(got, ref, what)
        check_pcg_step1(got, ref, what)
    elif observer == "activation":
        _exact(got["flags"], ref["flags"], f"{what}: flags")
    elif observer == "geometry":
        _exact(got["rows"][3], ref["rows"][3], f"{what}: normals")
        for r, (err, tol) in zip((0, 1, 2, 6, 7), _rows_terms(got, ref)):
            assert err <= tol, f"{what}: row {r}: {err:.3e} > {tol:.3e}"
    elif observer == "normals":
        _exact(got["rows"], ref["rows"], f"{what}: rows")
    else:
        raise KeyError(observer)


def check_pcg_init(got, ref, what):
    n = ref.n
    pp.rel_close(got["r"][:n][ref.surf], ref.r[ref.surf], 1e-6, f"{what}: r0 [surfels]")
    pp.rel_close(got["M"][:n][ref.surf], ref.M[ref.surf], 1e-6, f"{what}: M [surfels]")
    pp.shared_close(got["r"][:n], ref.r_sums, ref.shared, f"{what}: r0")
    pp.shared_close(got["M"][:n], ref.M_sums, ref.shared, f"{what}: M")


def check_pcg_step1(got, ref, what):
    n = ref.n
    pp.shared_close([got["alpha_d"]], (np.array([ref.alpha_d64]), np.array([abs(ref.alpha_d64)])), {"alpha_d": np.array([0])}, f"{what}: alpha_d")
    pp.rel_close(got["g"][:n][ref.surf], ref.g[ref.surf], 1e-5, f"{what}: g [surfels]")
    pp.shared_close(got["g"][:n], ref.g_sums, ref.shared, f"{what}: g")


def margin(observer, old, new):
    """How far the reference on the old inputs is from passing the observer's comparator against the reference on the new ones:
    (largest error / tolerance over the asserted float entries, number of changed elements of the outputs compared exactly)."""
    if observer == "fuse":
        return 0.0, int(sum((_bits(old[k]) != _bits(new[k])).sum() for k in ("tsdf", "count", "color")))
    if observer == "pose":
        if old["H"].shape != new["H"].shape:
            return np.inf, 0
        return max(e / t for e, t in _pose_terms(old, new)), int(np.abs(old["count"] - new["count"]).sum())
    if observer == "cost":
        if old["cost"].shape != new["cost"].shape:
            return np.inf, 0
        return max(e / t for e, t in _cost_terms(old, new)), int(np.abs(old["counts"] - new["counts"]).sum())
    if observer in ("pcg", "pcg_di"):
        if old.n != new.n:
            return np.inf, 0
        worst = 0.0
        for vec, sums in ((old.r, new.r_sums), (old.M, new.M_sums), (old.g, new.g_sums)):
            for name, idx in new.shared.items():
                ratio = pp.shared_ratio(vec[:new.n][idx], sums[0][idx], sums[1][idx]) / pp.SHARED_TOL[name]
                worst = max(worst, float(ratio.max()))
        return worst, 0
    if observer == "activation":
        if old["flags"].shape != new["flags"].shape:
            return 0.0, abs(old["flags"].size - new["flags"].size)
        return 0.0, int((old["flags"] != new["flags"]).sum())
    if observer in ("geometry", "normals"):
        if old["rows"].shape != new["rows"].shape:
            return 0.0, abs(old["rows"].shape[1] - new["rows"].shape[1])
        exact = int((_bits(old["rows"][3]) != _bits(new["rows"][3])).sum())
        if observer == "normals":
            return 0.0, int((_bits(old["rows"]) != _bits(new["rows"])).sum())
        return max(e / t for e, t in _rows_terms(old, new)), exact
    raise KeyError(observer)


def stale_cannot_pass(observer, old, new):
    ratio, changed = margin(observer, old, new)
    return ratio >= 100.0 or changed >= 100


# ----------------------------------------------------------------------------- the device side

def to_device(scene):
    d = scene.to_device()
    d.keep = []
    spare = getattr(scene, "spare", [])
    t = lambda a: d.torch.from_numpy(np.ascontiguousarray(a)).to(d.device)
    d.spare_tensors = [(t(kf.depth.view(np.int16)), t(kf.normals.view(np.int16)), t(kf.radius.view(np.int16)), t(kf.color)) for kf in spare]
    return d


class Run:
    """One bslam_context on a device scene and the observers' calls through it.  The scene is read at every call, so a
    mutation applied to it is what the next call hands in."""

    def __init__(self, d, cache=False, schedule=True):
        import badslam_amd
        from tests import gpu_util
        self.bs, self.gu = badslam_amd, gpu_util
        self.d = d
        self.hip = gpu_util.Hip(d)
        self.L, self.ctx = self.hip.L, self.hip.ctx
        if cache:
            self.set_cache(1)
        if not schedule:
            self.bs.check(self.L.bslam_set_xcd_schedule(self.ctx.handle, 0))

    def set_cache(self, on):
        self.bs.check(self.L.bslam_set_keyframe_cache(self.ctx.handle, on))

    def invalidate(self):
        self.bs.check(self.L.bslam_invalidate_keyframe_cache(self.ctx.handle))

    def set_schedule(self, on):
        self.bs.check(self.L.bslam_set_xcd_schedule(self.ctx.handle, on))

    def set_culling(self, on):
        self.bs.check(self.L.bslam_set_culling(self.ctx.handle, on))

    # --- observers
    def fuse(self):
        torch, d, h = self.d.torch, self.d, self.d.host
        nx, ny, nz = DIMS
        out = [torch.full((nz * ny, nx), -1, dtype=torch.int32, device=d.device) for _ in range(3)]
        bufs = [d.tbuf(t) for t in out]
        vol = abi.Volume((C.c_float * 3)(*h.origin), VOXEL, *DIMS)
        dp = d.depth_params()
        self.bs.check(self.L.bslam_fuse_keyframes(self.ctx.handle, self.gu.stream_ptr(), C.byref(h.color_camera), C.byref(h.depth_camera), C.byref(dp),
                                                  len(h.keyframes), d.keyframe_views(), C.byref(vol), TRUNCATION, C.byref(bufs[0]), C.byref(bufs[1]), C.byref(bufs[2])))
        torch.cuda.synchronize()
        got = [t.cpu().numpy().reshape(nz, ny, nx) for t in out]
        return dict(tsdf=got[0].view(np.float32), count=got[1].view(np.uint32), color=np.ascontiguousarray(got[2]).view(np.uint8).reshape(nz, ny, nx, 4))

    def pose(self):
        Hb, counts = self.hip.accumulate_pose_batched()
        return dict(H=Hb[:, :21].copy(), b=Hb[:, 21:27].copy(), count=counts.astype(np.int64))

    def cost(self):
        d, h = self.d, self.d.host
        K = len(h.keyframes)
        cost, counts = np.zeros((K, 2), np.float32), np.zeros((K, 2), np.uint32)
        sb, dp = d.surfel_buf(), d.depth_params()
        self.bs.check(self.L.bslam_compute_ba_cost(
            self.ctx.handle, self.gu.stream_ptr(), int(h.use_depth_residuals), int(h.use_descriptor_residuals), C.byref(h.color_camera),
            C.byref(h.depth_camera), C.byref(dp), K, d.keyframe_views(), d.surfels_size, C.byref(sb), None, cost.ctypes.data_as(P(C.c_float)),
            counts.ctypes.data_as(P(C.c_uint32)), C.cast(None, abi.ALLREDUCE_FN), None))
        return dict(cost=cost, counts=counts)

    def pcg_init(self, ref):
        """bslam_pcg_init for ref's layout -> (HipPCG, {r, M})."""
        got = self.gu.HipPCG(self.hip, ref.layout)
        got.init()
        return got, dict(r=got.get("r"), M=got.get("M"))

    def pcg_step1(self, got, ref, out=None):
        """bslam_pcg_step1 on the oracle's vectors of before its own step 1 -> out + {g, alpha_d}."""
        got.load_from(ref.loaded)
        got.step1(False)
        out = {} if out is None else out
        out.update(g=got.get("g"), alpha_d=got.scalar("alpha_d"))
        return out

    def pcg(self, ref):
        got, out = self.pcg_init(ref)
        return self.pcg_step1(got, ref, out)

    def activation(self):
        d = self.d
        saved = d.active.clone()
        try:
            with only_mut_kf_active(d.host):
                d.active.copy_(_t(d, active_start(d.host)))
                self.hip.update_activation()
                return dict(flags=d.active_np()[0, :d.surfels_size].copy())
        finally:
            d.active.copy_(saved)

    def writer(self, which, restore=True):
        d = self.d
        before = d.surfels.clone()
        (self.hip.optimize_geometry_iteration if which == "geometry" else self.hip.update_normals)()
        out = dict(rows=d.surfels_np()[:8, :d.surfels_size].copy())
        if restore:
            d.surfels.copy_(before)
        return out

    def observe(self, observer, ref):
        if observer in ("pcg", "pcg_di"):
            return self.pcg(ref)
        if observer in ("geometry", "normals"):
            return self.writer(observer)
        return getattr(self, observer)()


def same_bits(observer, x, y, what, ref=None):
    """Two device outputs of one observer agree bit for bit.  With depth intrinsics among the PCG's unknowns (ref: the PcgRef)
    the cfactor cells, float64 atomic sums, may round differently once in a great while: 1 ulp, as assert_same_run of
    test_gpu_pcg_variants grants them."""
    cells = ref.shared.get("cfactor cells") if isinstance(ref, PcgRef) else None
    for key in x:
        a, b = np.atleast_1d(np.asarray(x[key])), np.atleast_1d(np.asarray(y[key]))
        assert a.shape == b.shape, f"{what}: {key}: shapes {a.shape} and {b.shape}"
        differ = _bits(a) != _bits(b)
        if cells is not None and key in ("r", "M", "g") and differ.any():
            assert pp.ulp_distance(a[cells], b[cells]).max() <= 1, f"{what}: {key}: cfactor cells differ by more than 1 ulp"
            differ[cells] = False
        assert not differ.any(), f"{what}: {key}: {int(differ.sum())} of {differ.size} values differ, first at {np.argwhere(differ)[0]}"
