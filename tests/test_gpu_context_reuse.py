"""-m gpu: what a bslam_context carries from call to call -- the keyframe table, the derived records and luma quads, the work
orders, the sorted copy of the surfel rows, the intrinsics cell scratch -- against inputs that change between the calls.

After every step the observer's output on the long-lived context A is held to the reference evaluated on the inputs as they are
now (tests/context_reuse_util.py: the references, comparators and tolerances the suite already commits to) and to the same call on
a brand-new context B.  While the surfel positions are what they were when A built its work order, A and B agree bit for bit;
after a change of positions in place A may sum in the older order, and then A and B agree bit for bit with the work order
switched off on both.  tests/test_context_reuse_cpu.py shows that no answer from the inputs of before can pass."""

import numpy as np
import pytest

from tests import bso, context_reuse_util as U, pcg_parity as pp

pytestmark = pytest.mark.gpu

MOVES_POSITIONS_IN_PLACE = ("surfel_positions",)


def cases(mutations):
    """(mutation, photometric scene?) for every scene kind a mutation runs on."""
    return [pytest.param(m, photo, id=f"{m}-{'photometric' if photo else 'geometric'}") for m in mutations for photo in U.scene_kinds(m)]


def observe_all(run, h, observers, what, fresh=True, bitwise=True):
    """Every observer on `run`, held to the reference on h as it is now and to a fresh context; returns {observer: output}."""
    out = {}
    for observer in observers:
        ref = U.REFERENCES[observer](h)
        out[observer] = got = run.observe(observer, ref)
        U.check(observer, got, ref, f"{what}: {observer} against the reference")
        if fresh:
            other = U.Run(run.d).observe(observer, ref)
            U.check(observer, other, ref, f"{what}: {observer} on a fresh context against the reference")
            if bitwise:
                U.same_bits(observer, got, other, f"{what}: {observer} against a fresh context", ref)
    return out


def warm(run, h, observers):
    """The calls that fill the context's caches from the unchanged scene (held to the reference as well)."""
    return observe_all(run, h, observers, "before the change", fresh=False)


def without_order_agree(A, h, observers, what):
    """With the work order switched off on the long-lived context and on a fresh one, outputs agree bit for bit."""
    A.set_schedule(0)
    try:
        for observer in observers:
            ref = U.REFERENCES[observer](h)
            U.same_bits(observer, A.observe(observer, ref), U.Run(A.d, schedule=False).observe(observer, ref), f"{what}: {observer} with the work order off", ref)
    finally:
        A.set_schedule(1)


# ----------------------------------------------------------------------------- 1, 2: the keyframe cache off and on

@pytest.mark.parametrize("cache", [False, True], ids=["cache-off", "cache-on"])
@pytest.mark.parametrize("mutation,photo", cases([m for m in U.MUTATIONS if m not in U.IN_PLACE_CONTENT]))
def test_change_is_picked_up_by_the_next_call(oracle, mutation, photo, cache):
    """Addresses, pitches, a, raw_to_float_depth, the list, the poses and the surfel buffer: the next call sees the change with no
    further action, whether the keyframe cache is on or off."""
    h = U.base_scene(photo)
    d = U.to_device(h)
    if mutation == "depth_repitched":
        U.make_pitch_store(d)
    observers = U.PAIRS[mutation]
    A = U.Run(d, cache=cache)
    warm(A, h, observers)
    U.MUTATIONS[mutation](h, d)
    in_place = mutation in MOVES_POSITIONS_IN_PLACE
    observe_all(A, h, observers, mutation, bitwise=not in_place)
    if in_place:
        without_order_agree(A, h, observers, mutation)
    if mutation == "shorten":
        U.lengthen(h, d)                              # ... and restored
        observe_all(A, h, observers, "restored")


@pytest.mark.parametrize("mutation,photo", cases([m for m in U.MUTATIONS if m in U.IN_PLACE_CONTENT]))
def test_content_change_with_the_cache_off(oracle, mutation, photo):
    h = U.base_scene(photo)
    d = U.to_device(h)
    A = U.Run(d)
    warm(A, h, U.PAIRS[mutation])
    U.MUTATIONS[mutation](h, d)
    observe_all(A, h, U.PAIRS[mutation], mutation)


@pytest.mark.parametrize("mutation,photo", cases([m for m in U.MUTATIONS if m in U.IN_PLACE_CONTENT]))
def test_content_change_with_the_cache_on_needs_the_invalidate(oracle, mutation, photo):
    """In-place content under the caller's promise: without the invalidate the output is that of before, bit for bit -- which
    shows that the cache was in effect, nothing more; after bslam_invalidate_keyframe_cache it is the new reference."""
    h = U.base_scene(photo)
    d = U.to_device(h)
    observers = U.PAIRS[mutation]
    A = U.Run(d, cache=True)
    before = warm(A, h, observers)
    old_refs = {o: U.REFERENCES[o](h) for o in observers}
    U.MUTATIONS[mutation](h, d)
    for o in observers:
        if (mutation == "colour_image" and o == "fuse") or o == "pcg_di":
            continue      # not from the cache alone: fusion reads the colour pixels, the depth-intrinsics terms the raw depth and cfactor images
        # the vectors of the PCG's step 1 are the oracle's of before: the call is the same call on changed images
        U.same_bits(o, A.observe(o, old_refs[o]), before[o], f"{mutation}: {o} without an invalidate", old_refs[o])
    A.invalidate()
    observe_all(A, h, observers, f"{mutation}, invalidated")


def test_cache_switched_off_and_on_starts_from_empty(oracle):
    h = U.base_scene(False)
    d = U.to_device(h)
    observers = ("fuse", "pose")
    A = U.Run(d, cache=True)
    warm(A, h, observers)
    U.depth_shift(h, d)
    A.set_cache(0)
    A.set_cache(1)
    observe_all(A, h, observers, "cache off and on again")


def _stale_cannot_pass(h_before, h, observers):
    for o in observers:
        assert U.stale_cannot_pass(o, U.REFERENCES[o](h_before), U.REFERENCES[o](h)), f"{o}: the step changed too little for the test to mean anything"


def test_intrinsics_step_drops_the_records(oracle):
    """bslam_optimize_intrinsics with depth intrinsics rewrites the cfactor image and a: the next call on the caching context
    matches the reference built from both."""
    h = U.base_scene(False)
    d = U.to_device(h)
    observers = ("fuse", "pose", "pcg")
    A = U.Run(d, cache=True)
    warm(A, h, observers)
    before = U.clone_scene(h)
    _, out_d, a = A.hip.optimize_intrinsics(True, False)
    h.cfactor[:] = d.cfactor.cpu().numpy()      # the oracle sees what the device wrote
    assert not np.array_equal(h.cfactor, before.cfactor)
    _stale_cannot_pass(before, h, observers)     # at the a and camera of before: the cfactor image alone
    observe_all(A, h, observers, "after the intrinsics step, old a")
    h.a, h.depth_camera = a, out_d
    observe_all(A, h, observers, "after the intrinsics step")


def test_cfactor_update_from_the_pcg_delta_drops_the_records(oracle):
    """bslam_update_cfactors_from_pcg_delta rewrites the cfactor image in place: the library drops the records itself, as the
    intrinsics step does, and a raw-ABI caller with the cache on needs no invalidate."""
    from tests import gpu_util
    h = U.base_scene(False)
    d = U.to_device(h)
    observers = ("fuse", "pose", "pcg_di")
    A = U.Run(d, cache=True)
    warm(A, h, observers)
    before = U.clone_scene(h)
    layout = U.pcg_layout_of(h, True)
    ref, got = bso.HostPCG(h, layout), gpu_util.HipPCG(A.hip, layout)
    ref.delta[:] = np.random.default_rng(9).uniform(-0.004, 0.004, ref.delta.size).astype(np.float32)
    got.load_from(ref)
    ref.apply_delta_to_cfactors()
    got.apply_delta_to_cfactors()
    assert np.array_equal(d.cfactor.cpu().numpy().view(np.uint32), h.cfactor.view(np.uint32))
    _stale_cannot_pass(before, h, observers)
    observe_all(A, h, observers, "after the cfactor update")


# ----------------------------------------------------------------------------- 3: the keyframe table

def _pose_loop_then_observe(h, observers):
    d = U.to_device(h)
    A = U.Run(d)
    warm(A, h, observers)
    rng = np.random.default_rng(21)
    inits = [bso.se3_mul(kf.global_T_frame, bso.se3_exp(np.concatenate([rng.uniform(-0.004, 0.004, 3), rng.uniform(-0.002, 0.002, 3)]).astype(np.float32)))
             for kf in h.keyframes]
    poses, iters, conv = A.hip.estimate_poses_batched(inits, max_iterations=3)
    assert max(iters) > 0
    moved = max(np.abs(bso.se3_to_np(p) - bso.se3_to_np(kf.global_T_frame)).max() for p, kf in zip(poses, h.keyframes))
    assert moved > 1e-5, "the loop left poses of its own in the device copy of the table"
    observe_all(A, h, observers, "after the batched pose loop, original views")


def test_pose_loop_invalidates_the_device_keyframe_table(oracle):
    """bslam_estimate_frame_poses_batched rewrites frame_T_global in the device copy of the keyframe table; a following call with
    the views of before must upload them again although the host's record of the table says nothing has changed."""
    _pose_loop_then_observe(U.base_scene(False), ("pose", "cost", "pcg"))


def test_pose_loop_invalidates_the_device_keyframe_table_65_keyframes(oracle):
    """... with 65 keyframes, where the loop walks the device-side list of unconverged keyframes and the pose grid culls."""
    _pose_loop_then_observe(U.k65_scene(), ("pose", "activation"))


# ----------------------------------------------------------------------------- 4: the sorted copy of the surfel rows

def _pcg_sequence(A, h, between, what, di=False, layout_h=None):
    """bslam_pcg_init, `between`, bslam_pcg_step1: r and M against the reference at init, g and alpha_d against the reference
    on the surfels as they are at step 1."""
    ref0 = U.PcgRef(h if layout_h is None else layout_h, di)
    got, out = A.pcg_init(ref0)
    U.check_pcg_init(out, ref0, f"{what}: init")
    between()
    ref1 = U.PcgRef(h, di)
    assert ref1.n == ref0.n
    got.layout = ref1.layout
    U.check_pcg_step1(A.pcg_step1(got, ref1), ref1, f"{what}: step 1")


def test_pcg_solve_reuses_the_sorted_copy(oracle):
    h = U.base_scene(True)
    d = U.to_device(h)
    A = U.Run(d)
    ref = U.PcgRef(h, True)
    got, out = A.pcg_init(ref)
    U.check_pcg_init(out, ref, "init")
    first = A.pcg_step1(got, ref)
    U.check_pcg_step1(first, ref, "first step 1")
    second = A.pcg_step1(got, ref)
    U.check_pcg_step1(second, ref, "second step 1")
    U.same_bits("pcg_di", first, second, "two step 1 on one copy", ref)


def _write(A, h, d, writer):
    """One writer on A: the caller's rows (or flags) equal the oracle's update, and a fresh context reads the same surfels."""
    if writer == "activation":
        h.active[:] = U.active_start(h)
        d.active.copy_(U._t(d, h.active))
        h.update_activation()
        A.hip.update_activation()
        assert np.array_equal(d.active_np()[0, :h.surfels_size], h.active[0, :h.surfels_size])
        return
    before = h.surfels.copy()
    ref = U._writer_ref(h, writer)
    got = A.writer(writer, restore=False)
    U.check(writer, got, ref, f"{writer}: the caller's rows")
    assert (before[:8, :h.surfels_size].view(np.uint32) != ref["rows"].view(np.uint32)).sum() >= 100, "the writer changed surfels"
    h.surfels[:8, :h.surfels_size] = got["rows"]      # the oracle goes on from the device's rows
    observe_all(U.Run(d), h, ("pose",), f"after {writer}, fresh context", fresh=False)


@pytest.mark.parametrize("writer", ["geometry", "normals", "activation"])
def test_writer_between_init_and_step1(oracle, writer):
    """A kernel that updates surfels writes to the sorted copy and to the caller's rows: the caller's rows equal the oracle's
    update, a fresh context reads the same surfels, and the step 1 that follows sees the updated surfels."""
    h = U.base_scene(writer == "geometry")
    d = U.to_device(h)
    A = U.Run(d)
    _pcg_sequence(A, h, lambda: _write(A, h, d, writer), writer)


def test_order_rebuilt_between_writer_and_step1(oracle):
    """bslam_set_xcd_schedule drops the cached order but not the sorted copy's key.  After pcg_init, the geometry iteration (which
    rebuilds the copy and moves positions through it) and that call, step 1 sorts a new permutation from the moved positions
    while the copy's key still matches: only the permutation's serial number tells it that the copy is laid out in another
    order, and a copy re-used with the new permutation would scatter the per-surfel entries of g to other columns."""
    h = U.base_scene(True)
    d = U.to_device(h)
    A = U.Run(d)

    def between():
        before = h.surfels[:3, :h.surfels_size].copy()
        _write(A, h, d, "geometry")
        assert (h.surfels[:3, :h.surfels_size] != before).any(axis=0).sum() > h.surfels_size // 2, "most surfels moved: another order"
        A.set_schedule(1)

    _pcg_sequence(A, h, between, "order rebuilt")


def test_short_keyframe_list_between_init_and_step1(oracle):
    """An observer with fewer than 4 keyframes runs without the per-surfel order and leaves no sorted copy to re-use."""
    h = U.base_scene(False)
    d = U.to_device(h)
    A = U.Run(d)

    def short_call():
        U.surfel_positions(h, d)                     # the copy of the init is stale now
        kept_h, kept_d = h.keyframes, d.kf_tensors
        h.keyframes, d.kf_tensors = kept_h[:3], kept_d[:3]
        try:
            observe_all(A, h, ("pose",), "three keyframes", bitwise=False)
        finally:
            h.keyframes, d.kf_tensors = kept_h, kept_d

    _pcg_sequence(A, h, short_call, "short list")


def test_other_surfel_buffer_between_init_and_step1(oracle):
    h = U.base_scene(False)
    d = U.to_device(h)
    A = U.Run(d)
    other_h = U.base_scene(False)
    U.surfels_moved(other_h, None)
    other_h.surfels_size -= 300
    other_d = U.to_device(other_h)

    def other_buffer():
        U.check("pose", _on(A, other_d).pose(), U.REFERENCES["pose"](other_h), "the other buffer")
        _on(A, d)

    _pcg_sequence(A, h, other_buffer, "other buffer")


def _on(run, d):
    """`run`'s context pointed at another device scene."""
    run.hip.d, run.hip.h, run.d = d, d.host, d
    return run


def test_geometry_only_init_then_photometric_step1(oracle):
    """The copy of a geometry-only call holds four rows; a photometric step 1 needs seven and must not re-use it."""
    h = U.base_scene(True)
    d = U.to_device(h)
    A = U.Run(d)
    h.use_descriptor_residuals = False
    ref0 = U.PcgRef(h, False)
    got, out = A.pcg_init(ref0)
    U.check_pcg_init(out, ref0, "geometry-only init")
    h.use_descriptor_residuals = True
    ref1 = U.PcgRef(h, False)
    got1 = A.gu.HipPCG(A.hip, ref1.layout)
    U.check_pcg_step1(A.pcg_step1(got1, ref1), ref1, "photometric step 1")


def test_culling_toggled_between_init_and_step1(oracle):
    h = U.base_scene(False)
    d = U.to_device(h)
    for first in (1, 0):
        A = U.Run(d)
        A.set_culling(first)
        _pcg_sequence(A, h, lambda: A.set_culling(1 - first), f"culling {first} -> {1 - first}")


# ----------------------------------------------------------------------------- 5: intr_cells between the intrinsics step and the PCG

def _intrinsics_step_matches(A, h, what):
    from tests import intrinsics_parity as ip
    ref = U.clone_scene(h)
    bso.lib().bso_set_intrinsics_sum64(1)
    try:
        ref.optimize_intrinsics(True, False)
    finally:
        bso.lib().bso_set_intrinsics_sum64(0)
    shadow = ref.intrinsics_shadow()
    scratch = A.d.cfactor.clone()                   # the step writes its cfactor image: a copy, so that the scene stays
    _, _, _, tap = A.hip.debug_optimize_intrinsics(True, False, cfactor_buf=A.d.tbuf(scratch))
    assert np.array_equal(tap["obs"], shadow["obs"]), f"{what}: observation counts"
    ip.accumulated_close(tap["sums"], tap["cells"], shadow, what)


def _pcg_cells_match(A, h, what):
    ref = U.PcgRef(h, True)
    got = A.pcg(ref)
    U.check_pcg_init(got, ref, what)
    U.check_pcg_step1(got, ref, what)
    assert len(ref.shared["cfactor cells"]) == h.cfactor.size


def test_intr_cells_alternate_between_the_intrinsics_step_and_the_pcg(oracle):
    """The intrinsics step zeroes the cell scratch per call, the PCG path keeps it zero between calls: alternating them on one
    context, and once more across a cfactor image of another size (cell size 2: a quarter of the cells)."""
    h = U.base_scene(False)
    A = U.Run(U.to_device(h))
    for round_ in range(2):
        _intrinsics_step_matches(A, h, f"round {round_}: intrinsics step")
        _pcg_cells_match(A, h, f"round {round_}: pcg")
    small = pp.variant_scene(U.BASE_K, 2, True, False, seed=41)
    _on(A, U.to_device(small))
    _pcg_cells_match(A, small, "other cell count: pcg")
    _intrinsics_step_matches(A, small, "other cell count: intrinsics step")
    _on(A, U.to_device(h))
    _pcg_cells_match(A, h, "back: pcg")
    _intrinsics_step_matches(A, h, "back: intrinsics step")
    _pcg_cells_match(A, h, "back: pcg again")


# ----------------------------------------------------------------------------- 6: the surfel-buffer keys

def test_surfel_buffer_keys_in_sequence(oracle):
    h = U.base_scene(False)
    d = U.to_device(h)
    observers = ("pose", "cost", "pcg")
    A = U.Run(d)
    warm(A, h, observers)
    U.surfel_positions(h, d)
    observe_all(A, h, observers, "positions in place", bitwise=False)
    without_order_agree(A, h, observers, "positions in place")
    U.size_minus_37(h, d)
    observe_all(A, h, observers, "size lowered")          # a new key: the order is rebuilt from the positions as they are
    U.surfels_moved(h, d)
    observe_all(A, h, observers, "buffer moved")
    # two buffers alternated call by call
    other_h = U.clone_scene(h)
    U.surfel_positions(other_h, None)
    other_h.surfels_size -= 256
    other_d = U.to_device(other_h)
    for i in range(2):
        for dd in (other_d, d):
            _on(A, dd)
            observe_all(A, dd.host, ("pose", "pcg"), f"alternating, round {i}")


# ----------------------------------------------------------------------------- 7: another stream

def test_observer_on_another_stream_gives_the_same_result(oracle):
    """The call that builds the order runs on one torch stream, the next call on another: the output is the reference's and a fresh
    context's.  Only the result is checked.  The first call has read its sums back, so the sort is complete when the second
    starts, and the library's wait for perm_ready is issued but decides nothing here: a context's scratch is ordered by one
    stream at a time, so two calls of one context may not be in flight together."""
    import torch
    h = U.base_scene(False)
    d = U.to_device(h)
    A = U.Run(d)
    ref = U.REFERENCES["pose"](h)
    side = torch.cuda.Stream()
    first = A.pose()                                       # builds the order on the current stream
    side.wait_stream(torch.cuda.current_stream())          # the inputs, on the torch side
    with torch.cuda.stream(side):
        got = A.pose()
    U.check("pose", got, ref, "on the second stream")
    U.same_bits("pose", got, first, "on the second stream against the first", ref)
    U.same_bits("pose", got, U.Run(d).pose(), "on the second stream against a fresh context", ref)


# ----------------------------------------------------------------------------- 8: through DirectBA

def _direct_ba(scene):
    from badslam_amd.direct_ba import DirectBA
    ba = DirectBA(scene.max_surfels, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, 0.8, 1, 1, 1, scene.color_camera, scene.depth_camera, 0,
                  scene.use_depth_residuals, scene.use_descriptor_residuals)
    ba.set_options(texture_mode=scene.tex_mode, scheme_end_tasks=False)
    for kf in scene.keyframes:
        ba.AddKeyframe(kf.id, max(kf.min_depth, 1e-3), max(kf.max_depth, 1e-2), kf.depth, kf.normals, kf.radius, kf.color, kf.global_T_frame)
    ba.SetSurfels(scene.surfels[:8], scene.surfels_size)
    return ba


def _ba_outputs(ba, h):
    cost = ba.ComputeCost()
    ba.FuseKeyframes(h.origin, U.VOXEL, U.DIMS, U.TRUNCATION)
    vol = ba.Volume()
    return dict(cost=cost["cost"], counts=cost["counts"]), dict(tsdf=vol["tsdf"], count=vol["count"], color=vol["color"])


def test_direct_ba_invalidates_after_its_in_place_changes(oracle, tmp_path):
    """DirectBA switches the keyframe cache on and promises to invalidate after each in-place change it makes.  After
    LoadCalibration with another cfactor image and a (UploadCFactor), upload_keyframe_depth, upload_keyframe_normals,
    bsh_set_intrinsics (SetDepthCamera and SetA, after which the host does not invalidate: a is in the records' signature and the
    cameras are not in the records) and DeleteKeyframe, ComputeCost and the fused volume equal those of a fresh DirectBA brought
    to the same state, and the references."""
    from badslam_amd import direct_ba
    target = U.base_scene(False)                       # a = 0.02 and a real cfactor image
    h = U.clone_scene(target)
    h.a = 0.0
    h.cfactor[:] = 0                                   # a DirectBA starts without a depth deformation
    ba = _direct_ba(h)
    replay = []                                        # what brings a fresh DirectBA of h's images to the state of `ba`
    cam4 = lambda c: np.array([c.fx, c.fy, c.cx, c.cy], np.float32)
    camera = lambda p, like: bso.make_camera(float(p[0]), float(p[1]), float(p[2]), float(p[3]), like.width, like.height)
    base = str(tmp_path / "calibration")

    def adopt():
        """The host scene takes the intrinsics and the cfactor image that the DirectBA holds (the file keeps 8 digits)."""
        c4, d4, a = ba.intrinsics()
        h.a, h.color_camera, h.depth_camera = a, camera(c4, h.color_camera), camera(d4, h.depth_camera)
        h.cfactor[:] = ba.cfactor(h.cfactor.shape)

    def load_calibration():
        direct_ba.save_calibration_arrays(base, cam4(h.depth_camera), cam4(h.color_camera), target.a, target.cfactor)
        ba.LoadCalibration(base)
        replay.append(lambda b: b.LoadCalibration(base))
        adopt()
        assert h.a != 0 and abs(h.a - target.a) < 1e-6 and np.abs(h.cfactor - target.cfactor).max() < 1e-6

    def set_intrinsics():
        d4, a = cam4(h.depth_camera) * np.array([1.01, 0.99, 1, 1], np.float32), -0.03
        ba.set_intrinsics(None, d4, a)
        replay.append(lambda b: b.set_intrinsics(None, d4, a))
        adopt()
        assert h.a == np.float32(a) and h.depth_camera.fx == d4[0]

    steps = [("LoadCalibration", load_calibration),
             ("upload_keyframe_depth", lambda: (U.depth_shift(h, None), ba.upload_keyframe_depth(U.MUT_KF, h.keyframes[U.MUT_KF].depth))),
             ("upload_keyframe_normals", lambda: (U.normals_image(h, None), ba.upload_keyframe_normals(U.MUT_KF, h.keyframes[U.MUT_KF].normals))),
             ("set_intrinsics", set_intrinsics),
             ("DeleteKeyframe", lambda: (ba.DeleteKeyframe(h.keyframes[-1].id), h.keyframes.pop()))]
    try:
        _ba_outputs(ba, h)
        for name, step in steps:
            before = U.clone_scene(h)
            step()
            assert U.stale_cannot_pass("cost", U.REFERENCES["cost"](before), U.REFERENCES["cost"](h)), name
            cost, vol = _ba_outputs(ba, h)
            U.check("cost", cost, U.REFERENCES["cost"](h), f"{name}: ComputeCost")
            U.check("fuse", vol, U.REFERENCES["fuse"](h), f"{name}: volume")
            fresh = _direct_ba(h)
            try:
                for action in replay:
                    action(fresh)
                fresh_cost, fresh_vol = _ba_outputs(fresh, h)
            finally:
                fresh.close()
            U.same_bits("cost", cost, fresh_cost, f"{name}: ComputeCost against a fresh DirectBA")
            U.same_bits("fuse", vol, fresh_vol, f"{name}: volume against a fresh DirectBA")
    finally:
        ba.close()
