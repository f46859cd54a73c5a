"""-m gpu parity of the surfel lifecycle entry points against the oracle: creation with and
without the observation-count filter, supporting surfels + merge, deletion + radius update, compaction.
All decisions are integer / bit-pattern outputs (which pixel creates a surfel, which surfel is merged away or
deleted, where compaction moves it): they must match exactly."""
import numpy as np
import pytest

from badslam_amd import abi
from tests import bso, scenes

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FFFFFFF


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def build_scene(K=4, seed=5, use_desc=True):
    """K keyframes preprocessed by the oracle; surfels created (unfiltered) from the first K - 1 only."""
    full = scenes.synthetic_scene(K, seed=seed, cell=4, use_depth_residuals=True, use_descriptor_residuals=use_desc,
                                  max_surfels=19200 * K * 2)
    scene = bso.HostScene(full.color_camera, full.depth_camera, full.raw_to_float_depth, full.baseline_fx, full.cell, full.max_surfels,
                          use_depth_residuals=True, use_descriptor_residuals=use_desc, tex_mode=full.tex_mode)
    scene.keyframes = full.keyframes
    for kf in scene.keyframes[:K - 1]:
        scene.create_surfels_for_keyframe(kf)
    return scene


def rows_equal(got, ref, n, what):
    for row in range(8):
        same = np.array_equal(bits(got[row, :n]), bits(ref[row, :n]))
        assert same, f"{what}: surfel row {row} differs in {(bits(got[row, :n]) != bits(ref[row, :n])).sum()} of {n} columns"


@pytest.mark.parametrize("filtered", [False, True])
def test_create_surfels_matches_oracle(oracle, filtered):
    from tests import gpu_util
    scene = build_scene()
    K = len(scene.keyframes)
    hip = gpu_util.Hip(scene.to_device())
    before = scene.surfels_size
    covis = list(range(K - 1))
    created_ref = scene.create_surfels_for_keyframe_ex(scene.keyframes[K - 1], filtered, 2, [scene.keyframes[i] for i in covis])
    created = hip.create_surfels_for_keyframe(K - 1, filtered, 2, covis)
    assert created == created_ref and created > 1000
    if filtered:
        unfiltered = build_scene()
        assert created < unfiltered.create_surfels_for_keyframe_ex(unfiltered.keyframes[K - 1], False, 2, [])
    got = hip.d.surfels_np()
    # same pixels chosen, same positions / normals / radii / colours / descriptors: identical arithmetic, identical bits
    rows_equal(got[:, before:before + created], scene.surfels[:, before:before + created], created, "created surfels")
    rows_equal(got, scene.surfels, before, "existing surfels untouched")


def nan_surfel_scene(compacted):
    """build_scene() with a handful of surfels marked deleted (x = NaN), among them the one created from the top-left cell of
    keyframe 0, and with a measurement at pixel (0, 0) of the last keyframe: a NaN position passes the lifecycle's z test
    (`z <= 0` is false) and projects to pixel (0, 0) (float -> int maps NaN to 0), where depth preprocessing leaves no
    measurement in its own images (it clears a border of two pixels), so the test gives that pixel the cell's first measured one.
    compacted: the same scene with those surfels compacted away."""
    scene = build_scene()
    width, n = scene.depth_camera.width, scene.surfels_size
    pixel = scene.association(scene.keyframes[0])
    in_corner_cell = np.flatnonzero((pixel != 0xFFFFFFFF) & (pixel % width < scene.cell) & (pixel // width < scene.cell))
    assert in_corner_cell.size and in_corner_cell[0] == 0, "keyframe 0 created no surfel from its top-left cell"
    kill = np.unique(np.concatenate([in_corner_cell[:1], np.linspace(0, n - 1, 7).astype(np.int64)]))
    scene.surfels[0, kill] = np.array([NAN_BITS], np.uint32).view(np.float32)[0]
    last = scene.keyframes[-1]
    assert not last.depth[2, 2] & abi.BSLAM_INVALID_DEPTH_BIT
    last.depth[0, 0], last.normals[0, 0] = last.depth[2, 2], last.normals[2, 2]
    if compacted:
        scene.compact_surfels(n - kill.size)
    return scene


def test_create_surfels_with_deleted_surfels_present(oracle):
    """A deleted surfel still takes part in the supporting-surfel pass of creation and may hold cell (0, 0)."""
    from tests import gpu_util
    scene = nan_surfel_scene(compacted=False)
    hip = gpu_util.Hip(scene.to_device())
    before = scene.surfels_size
    last = len(scene.keyframes) - 1
    created_ref = scene.create_surfels_for_keyframe_ex(scene.keyframes[last], False, 2, [])
    # the case is live: without the deleted surfels the top-left cell is free and creates a surfel of its own
    without = nan_surfel_scene(compacted=True)
    created_without = without.create_surfels_for_keyframe_ex(without.keyframes[last], False, 2, [])
    assert created_ref == created_without - 1, (created_ref, created_without)
    created = hip.create_surfels_for_keyframe(last, False, 2, [])
    assert created == created_ref and created > 1000
    got = hip.d.surfels_np()
    rows_equal(got[:, before:before + created], scene.surfels[:, before:before + created], created, "created surfels")
    rows_equal(got, scene.surfels, before, "existing surfels untouched")


def test_filtered_creation_with_empty_covisibility_list(oracle):
    """No co-visible keyframe: every candidate has one observation, below min_observation_count = 2."""
    from tests import gpu_util
    scene = build_scene()
    hip = gpu_util.Hip(scene.to_device())
    last = len(scene.keyframes) - 1
    untouched = scene.surfels.copy()
    created_ref = scene.create_surfels_for_keyframe_ex(scene.keyframes[last], True, 2, [])
    created = hip.create_surfels_for_keyframe(last, True, 2, [])
    assert created == created_ref == 0
    assert np.array_equal(bits(hip.d.surfels_np()), bits(untouched)) and np.array_equal(bits(scene.surfels), bits(untouched))


def test_filtered_creation_with_reversed_covisibility_list(oracle):
    from tests import gpu_util
    scene = build_scene()
    K = len(scene.keyframes)
    hip = gpu_util.Hip(scene.to_device())
    before = scene.surfels_size
    covis = list(range(K - 1))[::-1]
    created_ref = scene.create_surfels_for_keyframe_ex(scene.keyframes[K - 1], True, 2, [scene.keyframes[i] for i in covis])
    created = hip.create_surfels_for_keyframe(K - 1, True, 2, covis)
    assert created == created_ref and created > 1000
    got = hip.d.surfels_np()
    rows_equal(got[:, before:before + created], scene.surfels[:, before:before + created], created, "created surfels")
    rows_equal(got, scene.surfels, before, "existing surfels untouched")


def overlapping_scene(K=3, cell=4, **scene_args):
    """Surfels created from every keyframe independently (no occupancy test) -> plenty of duplicates to merge."""
    full = scenes.synthetic_scene(K, seed=9, cell=cell, use_depth_residuals=True, use_descriptor_residuals=False, max_surfels=19200 * 8, **scene_args)
    scene = bso.HostScene(full.color_camera, full.depth_camera, full.raw_to_float_depth, full.baseline_fx, full.cell, full.max_surfels,
                          use_depth_residuals=True, use_descriptor_residuals=False, tex_mode=full.tex_mode)
    scene.keyframes = full.keyframes
    for kf in scene.keyframes:
        single = bso.HostScene(full.color_camera, full.depth_camera, full.raw_to_float_depth, full.baseline_fx, full.cell, 19200,
                               use_depth_residuals=True, use_descriptor_residuals=False, tex_mode=full.tex_mode)
        single.keyframes = [kf]
        single.create_surfels_for_keyframe(kf)
        n = single.surfels_size
        scene.surfels[:, scene.surfels_size:scene.surfels_size + n] = single.surfels[:, :n]
        scene.surfels_size += n
    scene.active[0, :scene.surfels_size] = np.arange(scene.surfels_size, dtype=np.uint32).astype(np.uint8) | 1   # distinguishable flags
    return scene


def test_merge_delete_compact_match_oracle(oracle):
    from tests import gpu_util
    scene = overlapping_scene()
    hip = gpu_util.Hip(scene.to_device())
    n = scene.surfels_size
    count_ref = count = n
    # merge against every keyframe in turn without compaction in between (BS/direct_ba.cc:578-597)
    for k, kf in enumerate(scene.keyframes):
        count_ref = scene.merge_surfels(kf, 0.8, count_ref)
        count = hip.merge_surfels(k, 0.8, count)
        assert count == count_ref, (k, count, count_ref)
        got = hip.d.surfels_np()
        assert np.array_equal(bits(got[0, :n]) == NAN_BITS, bits(scene.surfels[0, :n]) == NAN_BITS), f"merged set differs at keyframe {k}"
    assert count < 0.8 * n, (count, n)   # the duplicates really are merged
    # deletion + radius update (BS/direct_ba.cc:616)
    count_ref = scene.delete_surfels_and_update_radii(2, count_ref)
    count = hip.delete_surfels_and_update_radii(2, count)
    assert count == count_ref
    got = hip.d.surfels_np()
    rows_equal(got, scene.surfels, n, "after merge + delete")
    assert 0 < count < n
    # compaction (BS/direct_ba.cc:620)
    scene.compact_surfels(count_ref)
    hip.compact_surfels(count)
    assert hip.d.surfels_size == scene.surfels_size == count
    got = hip.d.surfels_np()
    rows_equal(got, scene.surfels, count, "after compaction")
    assert not (bits(got[0, :count]) == NAN_BITS).any()
    assert np.array_equal(hip.d.active_np()[0, :count], scene.active[0, :count])


def test_delete_through_the_sorted_copy_matches_oracle(oracle):
    """Deletion + radius update over >= 4 keyframes and >= 64 granules of 256 surfels: the kernel reads the library's sorted
    copy of the rows through the per-surfel permutation and writes the caller's rows."""
    from tests import gpu_util
    scene = overlapping_scene(K=4, cell=1, width=160, height=120, camera=bso.make_camera(131.25, 131.25, 80.0, 60.0, 160, 120))
    n = scene.surfels_size
    assert len(scene.keyframes) >= 4 and n >= 16384
    hip = gpu_util.Hip(scene.to_device())
    count_ref = scene.delete_surfels_and_update_radii(2, n)
    count = hip.delete_surfels_and_update_radii(2, n)
    assert count == count_ref and 0 < count < n
    rows_equal(hip.d.surfels_np(), scene.surfels, n, "after delete")


def test_compaction_without_active_buffer_and_noop(oracle):
    from tests import gpu_util
    scene = build_scene(K=3, use_desc=False)
    hip = gpu_util.Hip(scene.to_device())
    n = scene.surfels_size
    hip.compact_surfels(n)                      # nothing deleted: no-op
    assert hip.d.surfels_size == n
    rng = np.random.default_rng(0)
    kill = rng.choice(n, n // 3, replace=False)
    scene.surfels[0, kill] = np.array([NAN_BITS], np.uint32).view(np.float32)[0]
    hip.d.surfels.copy_(hip.torch.from_numpy(scene.surfels))
    scene.compact_surfels(n - kill.size, with_active=False)
    hip.compact_surfels(n - kill.size, with_active=False)
    rows_equal(hip.d.surfels_np(), scene.surfels, n - kill.size, "compaction of a random third")
