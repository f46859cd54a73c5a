"""-m gpu: the surfel lifecycle kernels (csrc/lifecycle_kernels.hpp behind csrc/lifecycle_abi.inc) and activation_kernel
(csrc/geometry_kernels.hpp) against the float64 reference of tests/lifecycle_util.py, one decision at a time.

tests/test_gpu_lifecycle.py demands bit equality with the oracle, which is the same authors' fp32 reading of the same files.  Here the
reference is a NumPy restatement written from the reference project's kernels; tests/test_lifecycle_cpu.py holds its census, checks
it against the oracle with the very checks used here (lifecycle_util.check_*), and shows every decision live by a mutation.

Every decided decision must equal the reference: which surfels a merge deletes after every keyframe and the count it returns; which
pixels create a surfel, in which order, and which candidates the filter removes; which surfels deletion marks and the exact
minimum radius of the survivors; where compaction moves every column of all eight rows and the flag byte; the flag byte after
activation.  Floats (created position, d1, d2) are compared within KERNEL_FACTOR * C * 2^-24 * A plus the fixed-point texture
mode's widening, C measured on the CPU (position 3.28, recorded 3.3; d1 / d2 0.18, recorded 0.2); radius bits, packed normals and
colour bytes outside their margins are exact.

Which test notices which mutation of the reference (lifecycle_util.MUTATIONS), were the kernel to do the same:
  holders_largest, skip_holder_1_vs_2   test_merge
  viol_ge_obs, radius_first_keyframe    test_deletion
  border_0, cells_floor                 test_creation (cells_floor also test_merge)
  scan_carry                            test_compaction at n = 264200 ("late", "early"): there the moves read the carried prefix.
                                        In test_creation_on_640x410 no append reads it (the pixels from 262144 on are border), but the
                                        returned count is the carried total, and tile 255, the last of the first block, holds flags
                                        (test_lifecycle_cpu.py asserts it): a carry short by that tile changes the count

Two things about the cases.  At 1317 surfels neither the 6-keyframe nor the 3-keyframe deletion takes the sorted-copy path: the
per-surfel order needs 64 granules of 256 surfels as well as 4 keyframes (make_schedule, csrc/badslam_hip.hip), so test_deletion adds
a run of the fixture's surfels 13 times side by side (17121 surfels), which does, and must give every copy the fixture's own result.
And n = 262145 enters the second pass of scan_sums_kernel with one element whose prefix nobody reads (the last hole has nothing behind
it to fill it; surfel 0 has nowhere to go), so n = 264200 with holes only at the back ("late") and survivors only at the front
("early") is added: there the moves hang on the carried prefix.

The activation cases on the fixture's 1317 surfels never leave the granule order either, whatever the culling switch says: the
per-surfel order with the granule boxes needs 64 granules, 64 keyframes and culling on (bslam_update_surfel_activation,
make_schedule), so on them `culling` changes no executed code.  The two tests `..._in_the_per_surfel_order` therefore run the
K = 63 / 64 / 65 stacks and a 66-keyframe list with mixed activity on the surfels 13 times side by side: with culling on and K >= 64
the sorted, culled path is taken (the flag byte goes back through the permutation, the look-away keyframes leave the ballot of 64),
with culling off or K = 63 the granule order on the same surfels, and every copy must give the fixture's own result.

A surfel with a NaN position is refused by the kernel's activation pass (the BA association), while the reference project and the
oracle let it land on pixel (0, 0); see lifecycle_util.nan_surfel_association.  The kernel is pinned to its reading here.

keyframe_count = 0 in deletion: setup_keyframe_table uploads one zeroed entry, so the table pointer is valid, prepare_surfels takes
the identity order, and the kernel's keyframe loop runs zero times: the path is sound, and every surfel is deleted for
min_observation_count >= 1 (test_deletion, the `no keyframes` run).

Time, measured on MI355X (the module prints every case's and its own; the times include the reference and the scene's upload): the
whole module takes 2.9 s, 1.6 s of it the first context.  A merge case (6 calls) takes 0.01 to 0.04 s, a creation case (13 calls)
0.04 s, the 640 x 410 creation 0.01 s, a deletion run 2 to 4 ms (the 17121-surfel one as well), the 12 compaction calls of a size
4 to 6 ms, 80 ms at the two sizes above 262144 (17 MB of rows up and down per call), an activation case 1 ms, 6 ms on a stack of 65
keyframes, 7 ms on the same stack with 17121 surfels (0.13 s for the first, which builds the per-surfel order) and 0.02 to 0.04 s on
the 66-keyframe list with 17121 surfels.  No case comes near a second.
"""
import time

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi
from tests import bso
from tests import lifecycle_util as L
from tests import surfel_terms_util as ST
from tests.gpu_util import Hip

pytestmark = pytest.mark.gpu
PAD = 5                                                # extra elements per image row of the pitched run, filled with 0x33 bytes


class HipBackend:
    """The library on a device copy of a HostScene, behind the calls of lifecycle_util.check_*"""

    def __init__(self, scene, ctx, dev=None):
        self.dev = scene.to_device() if dev is None else dev
        self.hip = Hip(self.dev, ctx)

    def rows(self):
        return self.dev.surfels_np()

    def active(self):
        return self.dev.active_np()[0]

    def size(self):
        return self.dev.surfels_size

    def merge(self, k, factor, count):
        return self.hip.merge_surfels(k, factor, count)

    def create(self, k, filtered, min_observation_count, covis):
        return self.hip.create_surfels_for_keyframe(k, filtered, min_observation_count, list(covis))

    def delete(self, min_observation_count, count):
        return self.hip.delete_surfels_and_update_radii(min_observation_count, count)

    def compact(self, count, with_active):
        self.hip.compact_surfels(count, with_active)

    def activate(self):
        self.hip.update_activation()


class PitchedScene(bso.DeviceScene):
    """A device scene whose keyframe images all lie in rows of width + PAD elements, the padding filled with 0x33 bytes"""

    def __init__(self, host, device="cuda:0"):
        super().__init__(host, device)
        from tests.preprocess_util import pitched
        self.storage, self.bufs = [], []
        for kf in host.keyframes:
            bufs = []
            for image, fill in ((kf.depth.view(np.int16), np.int16(0x3333)), (kf.normals.view(np.int16), np.int16(0x3333)),
                                (kf.radius.view(np.int16), np.int16(0x3333)), (np.ascontiguousarray(kf.color).view(np.int32)[..., 0], np.int32(0x33333333))):
                storage, buf = pitched(self.torch, image, PAD, fill)
                self.storage.append(storage)
                bufs.append(buf)
            self.bufs.append(tuple(bufs))

    def keyframe_view(self, i):
        return self.host.keyframes[i].view(self.bufs[i])


@pytest.fixture(scope="module")
def ctx():
    start = time.perf_counter()
    context = badslam_amd.Context(0)
    print(f"\n[lifecycle reference] first context: {time.perf_counter() - start:.2f} s")
    yield context
    print(f"\n[lifecycle reference] module: {time.perf_counter() - start:.2f} s")
    context.close()


class timed:
    def __init__(self, label):
        self.label = label

    def __enter__(self):
        self.start = time.perf_counter()

    def __exit__(self, *exc):
        print(f"\n[lifecycle reference] {self.label}: {time.perf_counter() - self.start:.3f} s")


@pytest.mark.parametrize("factor", L.FACTORS)
@pytest.mark.parametrize("case,variant", L.RUNS)
def test_merge(oracle, ctx, case, variant, factor):
    fixture = L.lifecycle_fixture(case, variant)
    with timed(f"merge {case} {variant} {factor}"):
        failures = L.check_merge(fixture, factor, HipBackend(L.scene_of(fixture), ctx))
    assert not failures, failures[:5]


@pytest.mark.parametrize("case,variant", L.RUNS)
def test_creation(oracle, ctx, case, variant):
    """unfiltered and filtered, min_observation_count 1, 2, 3 and 65538, the co-visibility list in both orders, both texture modes; the
    cases bring the colour camera of another size and a non-zero `a` with a varying cfactor"""
    fixture = L.lifecycle_fixture(case, variant)
    failures, created = [], 0
    with timed(f"creation {case} {variant}, {len(L.CREATION_RUNS)} calls"):
        for k, share, filtered, min_count, covis, mode in L.CREATION_RUNS:
            f, c = L.check_creation(fixture, lambda scene: HipBackend(scene, ctx), k, L.size_of(fixture, share), filtered, min_count, list(covis), L.MODES[mode],
                                    (k, share, filtered, min_count, covis, mode))
            failures += f
            created += int(c.kept.sum())
    assert not failures, failures[:5]
    assert created > 100


@pytest.mark.parametrize("case", sorted(ST.CASES))
def test_creation_from_pitched_images(oracle, ctx, case):
    """every keyframe image in rows of width + 5 elements, the surfel buffer wider than surfels_size"""
    fixture = L.lifecycle_fixture(case)
    failures = []
    with timed(f"pitched creation {case}"):
        for k, share, filtered, min_count, covis, mode in L.CREATION_RUNS[1:2] + L.CREATION_RUNS[8:10]:
            f, _ = L.check_creation(fixture, lambda scene: HipBackend(scene, ctx, PitchedScene(scene)), k, L.size_of(fixture, share), filtered, min_count,
                                    list(covis), L.MODES[mode], ("pitched", k, share, filtered, min_count, covis, mode))
            failures += f
    assert not failures, failures[:5]


def test_creation_on_640x410(oracle, ctx):
    """262400 pixels: the pixel scan takes the second pass of scan_sums_kernel; the count it returns is the carried total"""
    fixture = L.large_fixture()
    with timed("creation 640x410 at cell 16"):
        failures, c = L.check_creation(fixture, lambda scene: HipBackend(scene, ctx), 0, fixture.N, False, 2, [], abi.TEX_EXACT_FLOAT, "640x410")
    assert not failures, failures[:5]
    assert len(c.candidates) > 600


@pytest.mark.parametrize("min_count", (1, 2, 3))
@pytest.mark.parametrize("case,variant", L.RUNS)
def test_deletion(oracle, ctx, case, variant, min_count):
    fixture = L.lifecycle_fixture(case, variant)
    runs = [("6 keyframes", None, None, 1), ("3 keyframes", [0, 1, 2], None, 1), ("reversed", None, np.arange(fixture.N)[::-1], 1), ("no keyframes", [], None, 1)]
    if variant == "cell4":
        runs.append(("13 copies: the sorted copy", None, None, 13))
    for name, keyframes, order, copies in runs:
        with timed(f"deletion {case} {variant} min {min_count} {name}"):
            failures, d = L.check_deletion(fixture, lambda scene: HipBackend(scene, ctx), min_count, keyframes, order, copies, label=name)
        assert not failures, failures[:5]
        if keyframes == []:
            assert not d.survives.any()


def rows_backend(ctx):
    def make(rows, active):
        cam = bso.make_camera(45.0, 44.0, 18.2, 11.7, 37, 23)
        scene = bso.HostScene(cam, cam, ST.RAW_TO_FLOAT_DEPTH, ST.BASELINE_FX, 4, rows.shape[1])
        scene.surfels.view(np.uint32)[:8] = rows
        scene.active[0] = active
        scene.surfels_size = rows.shape[1]
        return HipBackend(scene, ctx)
    return make


@pytest.mark.parametrize("n", L.SIZES)
def test_compaction(oracle, ctx, n):
    with timed(f"compaction n = {n}, {2 * len(L.PATTERNS)} calls"):
        for pattern in L.PATTERNS:
            for with_active in (True, False):
                assert not L.check_compaction(rows_backend(ctx), n, pattern, with_active)


def set_culling(ctx, on):
    badslam_amd.check(badslam_amd.lib().bslam_set_culling(ctx.handle, int(on)))


@pytest.mark.parametrize("culling", (True, False))
@pytest.mark.parametrize("mask", sorted(L.ACTIVITY_MASKS))
@pytest.mark.parametrize("case", sorted(ST.CASES))
def test_activation(oracle, ctx, case, mask, culling):
    fixture = L.lifecycle_fixture(case)
    associated, ambiguous = L.ba_terms(fixture.inputs)
    set_culling(ctx, culling)
    try:
        with timed(f"activation {case} {mask} culling {culling}"):
            failures, want, undecided = L.check_activation(HipBackend(L.activity_scene(fixture, L.ACTIVITY_MASKS[mask]), ctx), associated, ambiguous, L.ACTIVITY_MASKS[mask])
    finally:
        set_culling(ctx, True)
    assert not failures, failures
    assert undecided.mean() <= L.MAX_AMBIGUOUS_SHARE
    assert ((want & 0xFE) != 0).sum() > 100 or mask == "all"        # flag bytes with other bits that must survive


@pytest.mark.parametrize("culling", (True, False))
@pytest.mark.parametrize("K", (63, 64, 65))
def test_activation_of_a_long_stack(oracle, ctx, K, culling):
    """K - 1 look-away keyframes in front of one that sees the surfels: it is the last of the first batch of 64, or the first of the next"""
    fixture = L.lifecycle_fixture("same_camera")
    associated, ambiguous = L.stack_terms(fixture, K)
    set_culling(ctx, culling)
    try:
        with timed(f"activation stack K = {K} culling {culling}"):
            failures, want, _ = L.check_activation(HipBackend(L.stack_scene(fixture, K), ctx), associated, ambiguous, [L.KF_ACTIVE] * K)
    finally:
        set_culling(ctx, True)
    assert not failures, failures
    assert (want & 1).sum() > 300


COPIES = 13                                            # 17121 surfels: 67 granules of 256


def test_tiled_scene_reaches_the_per_surfel_order():
    assert COPIES * ST.N_SURFELS >= 64 * 256


@pytest.mark.parametrize("culling", (True, False))
@pytest.mark.parametrize("K", (63, 64, 65))
def test_activation_of_a_long_stack_in_the_per_surfel_order(oracle, ctx, K, culling):
    """The same stacks on the fixture's surfels 13 times side by side.  With 67 granules, K >= 64 and culling on, the pass runs in the
    per-surfel order: it reads the sorted copy, writes the flag byte back through the permutation, and the granule boxes cull the
    look-away keyframes from the ballot of 64; K = 63, or culling off, is the granule order on the same surfels.  Every copy must
    come out as the fixture's own surfel does."""
    fixture = L.lifecycle_fixture("same_camera")
    associated, ambiguous = (np.tile(a, (COPIES, 1)) for a in L.stack_terms(fixture, K))
    set_culling(ctx, culling)
    try:
        with timed(f"activation stack K = {K} culling {culling}, {COPIES} copies"):
            failures, want, _ = L.check_activation(HipBackend(L.stack_scene(fixture, K, COPIES), ctx), associated, ambiguous, [L.KF_ACTIVE] * K)
    finally:
        set_culling(ctx, True)
    assert not failures, failures
    assert (want & 1).sum() > 300 * COPIES


@pytest.mark.parametrize("culling", (True, False))
@pytest.mark.parametrize("case", sorted(ST.CASES))
def test_activation_with_mixed_activity_in_the_per_surfel_order(oracle, ctx, case, culling):
    """The fixture's six keyframes eleven times in a row (66 keyframes), every round with the alternating activity mask, on the surfels
    13 times side by side: active, co-visible and inactive keyframes in both batches of 64, in the per-surfel order when culling is on."""
    fixture = L.lifecycle_fixture(case)
    mask, repeat = L.ACTIVITY_MASKS["alternating"], 11
    associated, ambiguous = (np.tile(a, (COPIES, repeat)) for a in L.ba_terms(fixture.inputs))
    set_culling(ctx, culling)
    try:
        with timed(f"activation {case} alternating x {repeat} culling {culling}, {COPIES} copies"):
            failures, want, undecided = L.check_activation(HipBackend(L.activity_scene(fixture, mask, COPIES, repeat), ctx), associated, ambiguous, mask * repeat)
    finally:
        set_culling(ctx, True)
    assert not failures, failures
    assert undecided.mean() <= L.MAX_AMBIGUOUS_SHARE and 0 < (want & 1).sum() < len(want)
