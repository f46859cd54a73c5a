"""The oracle's float64 shadow sums of the shared PCG entries (bso_pcg_last_shared_sums) and the per-entry comparator that the
GPU parity tests judge those entries with (tests/pcg_parity.py).  CPU only."""
import functools

import numpy as np
import pytest

from tests import bso, pcg_parity as pp

U = 2.0 ** -24   # fp32 unit roundoff


@functools.lru_cache(maxsize=None)
def scene_of(use_depth, use_desc):
    return pp.variant_scene(3, 2, use_depth, use_desc, seed=41)


def run_to_step1(use_depth, use_desc, **layout_kw):
    """Oracle init, init2, step 1 (clear_g = 0 on a zero g), step 2, step 3, step 1 (clear_g = 1).
    Returns (scene, layout, pcg, {"r" | "M" | "g0" | "g1": (fp32 vector, sum64, abs64, terms)})."""
    scene = scene_of(use_depth, use_desc)
    layout = bso.pcg_layout(scene, gauge_keyframe_id=1, **layout_kw)
    pcg = bso.HostPCG(scene, layout)
    out = {}
    pcg.init()
    out["r"] = (pcg.r.copy(),) + pcg.shared_sums("r")
    out["M"] = (pcg.M.copy(),) + pcg.shared_sums("M")
    pcg.init2()
    pcg.step1(False)
    out["g0"] = (pcg.g.copy(),) + pcg.shared_sums("g")
    pcg.step2()
    pcg.step3()
    pcg.swap_alpha_beta()
    pcg.step1(True)
    out["g1"] = (pcg.g.copy(),) + pcg.shared_sums("g")
    return scene, layout, pcg, out


CONFIGS = {
    "depth+desc, all intrinsics": (True, True, dict(optimize_depth_intrinsics=True, optimize_color_intrinsics=True)),
    "depth, depth intrinsics, no geometry": (True, False, dict(optimize_depth_intrinsics=True, optimize_geometry=False)),
    "descriptors, colour intrinsics": (False, True, dict(optimize_color_intrinsics=True)),
    "depth+desc, poses only": (True, True, dict(optimize_geometry=False)),
}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_shadow_sums_bracket_the_fp32_serial_sums(oracle, config):
    use_depth, use_desc, kw = CONFIGS[config]
    scene, layout, _, out = run_to_step1(use_depth, use_desc, **kw)
    groups = pp.shared_groups(scene, layout)
    assert groups
    for which, (v32, sum64, abs64, terms) in out.items():
        for name, idx in groups.items():
            s, a, n = sum64[idx], abs64[idx], terms[idx].astype(np.float64)
            assert np.all(a >= np.abs(s)), f"{which} [{name}]: abs64 < |sum64|"
            assert np.all(a[n == 0] == 0), f"{which} [{name}]: an entry without terms has a sum"
            # a serial (or any other) fp32 sum of n terms is within gamma_(n-1) * sum |term| of their exact sum (Higham, Accuracy
            # and Stability of Numerical Algorithms, eq. 4.4); the pairs of descriptor products are added to each other first,
            # which is one more summation order of the same terms
            gamma = n * U / (1 - n * U)
            err = np.abs(v32[idx].astype(np.float64) - s)
            assert np.all(err <= gamma * a), f"{which} [{name}]: fp32 sum off its float64 shadow by {np.max(err / np.maximum(a, 1e-300)):.3e} of abs64"
            assert np.all(v32[idx][n == 0] == 0)
        if "depth a" in groups and use_depth:
            assert terms[groups["depth a"]][0] > 1000 and abs64[groups["depth a"]][0] > 0, "the a column is live (a != 0, cfactor != 0)"
    # the pose entries of the gauge-free keyframes all have terms
    if "poses" in groups:
        assert np.all(out["M"][3][groups["poses"]] > 0)


def test_shadow_starts_from_g_when_it_is_not_cleared(oracle):
    scene = scene_of(True, False)
    layout = bso.pcg_layout(scene, gauge_keyframe_id=1, optimize_depth_intrinsics=True)
    pcg = bso.HostPCG(scene, layout)
    pcg.init(); pcg.init2()
    a_index = layout.a_unknown_index
    pcg.g[a_index] = 3.0
    pcg.step1(False)
    sum64, abs64, terms = pcg.shared_sums("g")
    pcg2 = bso.HostPCG(scene, layout)
    pcg2.init(); pcg2.init2(); pcg2.step1(True)
    sum64_c, abs64_c, terms_c = pcg2.shared_sums("g")
    assert terms[a_index] == terms_c[a_index] + 1
    assert sum64[a_index] == pytest.approx(sum64_c[a_index] + 3.0, rel=1e-12)
    assert abs64[a_index] == pytest.approx(abs64_c[a_index] + 3.0, rel=1e-12)


def test_shadow_does_not_change_the_fp32_vectors(oracle):
    """The same call gives the same bits whether or not another layout's shadow was live before it."""
    scene = scene_of(True, True)
    la = bso.pcg_layout(scene, gauge_keyframe_id=1, optimize_depth_intrinsics=True, optimize_color_intrinsics=True)
    lb = bso.pcg_layout(scene, gauge_keyframe_id=0)
    a1 = bso.HostPCG(scene, la); a1.init()
    b = bso.HostPCG(scene, lb); b.init()
    a2 = bso.HostPCG(scene, la); a2.init()
    assert np.array_equal(a1.r.view(np.uint32), a2.r.view(np.uint32)) and np.array_equal(a1.M.view(np.uint32), a2.M.view(np.uint32))
    # pose entries do not depend on which other unknowns exist: keyframe 2's entries sit at 6.. in both layouts
    assert np.array_equal(a1.r[6:12].view(np.uint32), b.r[6:12].view(np.uint32))


class TestComparator:
    """With the oracle on both sides (its float64 sums, rounded to fp32, as the device vector)."""

    @pytest.fixture(scope="class")
    def state(self, oracle):
        scene, layout, _, out = run_to_step1(True, True, optimize_depth_intrinsics=True, optimize_color_intrinsics=True)
        return scene, layout, pp.shared_groups(scene, layout), out

    @pytest.mark.parametrize("which", ["r", "M", "g0", "g1"])
    def test_accepts_the_rounded_float64_sums(self, state, which):
        _, _, groups, out = state
        _, sum64, abs64, _ = out[which]
        worst = pp.shared_close(sum64.astype(np.float32), (sum64, abs64), groups, which)
        assert max(worst.values()) <= U

    def test_rejects_a_scaled_a_entry_of_M(self, state):
        _, layout, groups, out = state
        _, sum64, abs64, _ = out["M"]
        got = sum64.astype(np.float32)
        # a max-relative 1e-4 over the five depth-intrinsics entries accepts this: the fx entry is 3e7 times larger
        got[layout.a_unknown_index] *= np.float32(1.001)
        d = np.concatenate([groups["depth fx fy cx cy"], groups["depth a"]])
        assert np.abs(got[d] - sum64[d]).max() <= 1e-4 * np.abs(sum64[d]).max()
        with pytest.raises(AssertionError, match=r"\[depth a\]"):
            pp.shared_close(got, (sum64, abs64), groups, "M")

    @pytest.mark.parametrize("which", ["g0", "g1"])
    def test_rejects_a_zeroed_cfactor_cell_of_g(self, state, which):
        _, _, groups, out = state
        _, sum64, abs64, _ = out[which]
        got = sum64.astype(np.float32)
        cells = groups["cfactor cells"]
        live = cells[abs64[cells] > 0]
        cell = live[np.argmin(np.abs(sum64[live]))]   # the hardest to notice: the live cell with the smallest sum
        assert sum64[cell] != 0
        got[cell] = 0
        with pytest.raises(AssertionError, match=r"\[cfactor cells\]: 1 of"):
            pp.shared_close(got, (sum64, abs64), groups, which)

    def test_rejects_swapped_colour_intrinsics_entries_of_r(self, state):
        _, _, groups, out = state
        _, sum64, abs64, _ = out["r"]
        c = groups["colour fx fy cx cy"]
        for i, j in ((0, 1), (2, 3), (0, 3)):
            got = sum64.astype(np.float32)
            got[c[i]], got[c[j]] = got[c[j]], got[c[i]]
            with pytest.raises(AssertionError, match=r"\[colour fx fy cx cy\]: 2 of 4"):
                pp.shared_close(got, (sum64, abs64), groups, "r")

    def test_an_entry_without_terms_must_be_exactly_zero(self, state):
        _, _, groups, out = state
        _, sum64, abs64, _ = out["r"]
        cells = groups["cfactor cells"]
        dead = cells[abs64[cells] == 0]
        assert dead.size, "the scene has cfactor cells that no pair falls into"
        got = sum64.astype(np.float32)
        pp.shared_close(got, (sum64, abs64), groups, "r")
        got[dead[0]] = np.float32(1e-30)
        with pytest.raises(AssertionError, match=r"\[cfactor cells\]"):
            pp.shared_close(got, (sum64, abs64), groups, "r")

    def test_committed_tolerances_respect_the_ceiling(self):
        assert pp.TOL_CEILING == 1e-4
        assert all(0 < t <= pp.TOL_CEILING for t in pp.SHARED_TOL.values())
