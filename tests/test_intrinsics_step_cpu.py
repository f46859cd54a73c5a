"""The oracle's float64 shadow of the alternating intrinsics step (bso_intrinsics_last_shadow) on the cases of
tests/intrinsics_parity.py, without a GPU: the shadow agrees with the oracle's own fp32 sums, every case holds the population
that tests/test_gpu_intrinsics_step.py relies on (so that no case there passes vacuously), and the cell arrays are indexed by
the cell grid's own width whatever the size of the cfactor buffer."""
import numpy as np
import pytest

from tests import bso, intrinsics_parity as ip

PAIRS = [(name, inst) for name in ip.CASES for inst in ip.INSTANTIATIONS]


@pytest.mark.parametrize("name,inst", PAIRS)
def test_shadow_is_consistent_with_the_fp32_sums(oracle, name, inst):
    """A serial fp32 sum of n terms is within n * 2^-24 * sum |term| of their exact sum: every global sum and every cell entry of
    the oracle against its own shadow; an entry without terms is exactly 0; obs sums to the number of depth terms."""
    depth, colour = ip.INSTANTIATIONS[inst]
    s = ip.oracle_step(name, inst)["shadow"]
    pairs = [("sums", s["sums32"], s["sum64"], s["abs64"], s["terms"])]
    if depth:
        pairs.append(("cells", s["cells32"], s["cell_sum64"], s["cell_abs64"], s["cell_terms"]))
    for what, f32, s64, a64, n in pairs:
        assert np.isfinite(f32).all() and np.isfinite(s64).all()
        err = np.abs(f32.astype(np.float64) - s64)
        assert np.all(err <= n * ip.U * a64), (name, inst, what, float((err / np.maximum(n * ip.U * a64, 1e-300)).max()))
        assert not f32[n == 0].any() and not a64[n == 0].any()
        assert np.all(np.abs(s64) <= a64)
    depth_terms = s["terms"][:20]
    assert np.all(depth_terms == depth_terms[0]), "every depth pair adds one term to each of A's and b1's entries"
    if depth:
        assert int(s["obs"].sum()) == int(depth_terms[0]) > 0
        assert np.array_equal(s["cell_terms"], np.broadcast_to(s["obs"], (7, s["obs"].size))), "one term per observation in each cell entry"
    else:
        assert depth_terms[0] == 0 and not s["obs"].any() and not s["cell_terms"].any()
    assert (s["terms"][20:34] > 0).all() == colour and (colour or not s["terms"][20:34].any())
    assert not s["terms"][34:].any()


@pytest.mark.parametrize("name", list(ip.CASES))
def test_case_population(oracle, name):
    """What the GPU cases are there for, on the oracle alone."""
    scene = ip.case_scene(name)
    width, height, cell, K, surfels, color_scale = ip.CASES[name]
    assert len(scene.keyframes) == K and scene.cfactor.shape == ((height - 1) // cell + 1, (width - 1) // cell + 1)
    s = ip.oracle_step(name, "both")["shadow"]
    obs = s["obs"].reshape(scene.cfactor.shape)
    print(f"{name}: {scene.surfels_size} surfels, {obs.size} cells, {int((obs == 0).sum())} without observation, "
          f"{int(s['terms'][0])} depth terms, {int(s['terms'][20])} colour terms")
    assert (obs > 0).any()
    assert (obs == 0).any() == (name not in ("k17", "odd-border")), "cells without an observation in every case but k17 and odd-border"
    assert (s["terms"][20:34] > 0).all(), "every colour entry has terms"
    slot = 512   # surfels per work slot of intrinsics_accumulate_kernel (256 threads, 2 surfels each)
    if name == "even":
        assert scene.surfels_size > 12 * slot and width % cell == 0 and height % cell == 0
    if name in ("odd", "odd-border"):
        assert scene.surfels_size > 2 * slot and scene.surfels_size % slot != 0, "several slots, the last one ragged"
        assert width % cell != 0 and height % cell != 0 and obs.shape == (29, 38)
    if name == "odd":
        # the last grid column holds pixel columns 148 and 149, the last grid row pixel row 112: all inside the border of two
        # pixels that depth preprocessing invalidates, so these cells are the unobserved ones; the last cells that can be are
        assert not obs[:, -1].any() and not obs[-1, :].any() and (obs[:, -2] > 0).any() and (obs[-2, :] > 0).any()
    if name == "odd-border":
        assert (obs[:, -1] > 0).any() and (obs[-1, :] > 0).any(), "observed cells in the last (partial) grid column and row"
    if name == "odd-513":
        assert scene.surfels_size == slot + 1
    if name == "odd-100":
        assert (obs == 0).sum() > 0.85 * obs.size
    if name == "odd-1":
        assert 1 <= int(s["terms"][0]) <= K
    if name == "tiny":
        assert scene.surfels_size < slot and cell == 3
    if name == "k17":
        assert K > 16
    if name == "colour-2x":
        assert scene.color_camera.width == 2 * scene.depth_camera.width


def test_comparator_rejects_the_faults_it_is_there_for(oracle):
    """accumulated_close at the committed tolerances accepts the float64 sums rounded to fp32 and rejects: a cell array indexed
    with a width one larger (a partial border cell lands in the next row), two swapped rows of the cell block B, one dropped
    term of a sum over ~3 500, and an off-diagonal entry of A that is off by 1e-5 of its abs64 (its terms cancel to a twentieth)."""
    s = ip.oracle_step("odd-border", "both")["shadow"]
    h, w = ip.case_scene("odd-border").cfactor.shape
    sums, cells = s["sum64"].astype(np.float32), s["cell_sum64"].astype(np.float32)
    ip.accumulated_close(sums, cells, s, "exact")

    wide = np.zeros((7, h, w + 1), np.float32)
    wide[:, :, :w] = cells.reshape(7, h, w)
    with pytest.raises(AssertionError, match="cell"):
        ip.accumulated_close(sums, wide.reshape(7, -1)[:, :h * w], s, "wide index")
    swapped = cells.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    with pytest.raises(AssertionError, match="cell B"):
        ip.accumulated_close(sums, swapped, s, "swapped rows")
    dropped = sums.copy()
    dropped[0] = np.float32(s["sum64"][0] - s["abs64"][0] / s["terms"][0])   # A[0, 0]: all terms >= 0, one average term missing
    with pytest.raises(AssertionError, match="fx fy cx cy"):
        ip.accumulated_close(dropped, cells, s, "dropped term")
    off = sums.copy()
    off[4] = np.float32(s["sum64"][4] + 1e-5 * s["abs64"][4])
    with pytest.raises(AssertionError, match="A mixed"):
        ip.accumulated_close(off, cells, s, "off-diagonal")


def test_enlarged_cfactor_buffer_changes_nothing(oracle):
    """The odd scene with its cfactor image as the top-left of a buffer 7 columns and 3 rows larger: the same shadow, the same
    cfactor image, and the rest of the buffer untouched."""
    exact = ip.oracle_step("odd", "both")
    large = ip.oracle_step("odd", "both", pad=(7, 3))
    for key, value in exact["shadow"].items():
        assert np.array_equal(value.view(np.uint8), large["shadow"][key].view(np.uint8)), key
    h, w = exact["scene"].cfactor.shape
    assert (h, w) == (29, 38) and large["buffer"].shape == (32, 45)
    assert np.array_equal(large["buffer"][:h, :w].view(np.uint32), exact["scene"].cfactor.view(np.uint32))
    assert not np.array_equal(exact["scene"].cfactor, ip.case_scene("odd").cfactor), "the step moved the cfactor image"
    outside = np.ones(large["buffer"].shape, bool)
    outside[:h, :w] = False
    assert np.all(large["buffer"][outside] == np.float32(-7.25)), "the step wrote outside the image"
    for cam in ("color_camera", "depth_camera"):
        a, b = getattr(exact["scene"], cam), getattr(large["scene"], cam)
        assert (a.fx, a.fy, a.cx, a.cy) == (b.fx, b.fy, b.cx, b.cy)
    assert exact["scene"].a == large["scene"].a
