"""Preconditions of test_gpu_context_reuse.py, on the references alone: the scenes are large enough for every cached path of a
context to be live, and every mutation changes every observer it is paired with by so much that an answer computed from the
inputs of before cannot pass that observer's comparator -- at least one asserted entry off by 100 times its tolerance, or at
least 100 elements changed where the comparison is exact."""
import pytest

from tests import context_reuse_util as U


@pytest.fixture(scope="module")
def references(oracle):
    """{(photometric, observer): reference on the unchanged scene}, computed once."""
    cache = {}

    def get(photo, observer):
        if (photo, observer) not in cache:
            cache[(photo, observer)] = U.REFERENCES[observer](U.base_scene(photo))
        return cache[(photo, observer)]
    return get


@pytest.mark.parametrize("use_desc", [False, True])
def test_scene_thresholds(oracle, use_desc):
    scene = U.base_scene(use_desc)
    U.check_thresholds(scene)
    assert len(scene.keyframes) == U.BASE_K and len(scene.spare) == 1
    assert len(scene.keyframes) - 1 >= U.MIN_KEYFRAMES, "the shortened list still has the per-surfel order"
    assert scene.surfels_size - 37 >= U.MIN_SURFELS
    assert scene.use_depth_residuals and scene.use_descriptor_residuals == use_desc
    assert scene.depth_camera.width == 160 and scene.depth_camera.height == 120


def test_k65_scene_thresholds(oracle):
    scene = U.k65_scene()
    U.check_thresholds(scene)
    assert len(scene.keyframes) == 65      # from 64 keyframes on: pose-grid culling, the device-side keyframe list of the pose loop


def test_every_mutation_is_paired(oracle):
    assert set(U.PAIRS) == set(U.MUTATIONS)
    assert all(set(obs) <= set(U.REFERENCES) for obs in U.PAIRS.values())
    assert set(U.IN_PLACE_CONTENT) | set(U.NOTICED_BY_SIGNATURE) <= set(U.MUTATIONS)


@pytest.mark.parametrize("mutation", list(U.MUTATIONS))
def test_a_stale_answer_cannot_pass(references, mutation):
    for photo in U.scene_kinds(mutation):
        scene = U.base_scene(photo)
        U.MUTATIONS[mutation](scene, None)
        for observer in U.PAIRS[mutation]:
            old, new = references(photo, observer), U.REFERENCES[observer](scene)
            ratio, changed = U.margin(observer, old, new)
            print(f"{mutation} / {observer} / {'photometric' if photo else 'geometric'}: {ratio:.3g} x tolerance, {changed} elements changed")
            assert ratio >= 100.0 or changed >= 100, (mutation, observer, photo, ratio, changed)
