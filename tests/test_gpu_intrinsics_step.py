"""-m gpu parity of the alternating intrinsics step (bslam_optimize_intrinsics through its tapped twin
bslam_debug_optimize_intrinsics) against the oracle, entry by entry, for the three instantiations of
intrinsics_accumulate_kernel -- <depth, ->, <-, colour>, <depth, colour> -- on every case of tests/intrinsics_parity.py.

Per case and instantiation: the observation counts are the oracle's exactly; every accumulated entry (the 40 sums, each cell's
B[5], D, b2) is within tol * abs64 of the oracle's float64 shadow sum, per entry; the Schur pass and the cfactor update are
judged on their own tapped inputs against NumPy float64; the solved cameras and `a` are compared with the oracle in the
full-rank cases at the bars of tests/test_gpu_direct_ba.py; two runs on the same inputs agree.

Not reached by any case: the `fabsf(corrected_inv_depth) > 1e-4` rejection (a corrected depth beyond 10 km) and a D that is
positive yet so small that 1 / D >= 1e12 -- neither can be produced from representable u16 depths, and no input is contrived
for them.  The only flagged cells are those with D = 0, which are the cells without an observation."""
import numpy as np
import pytest

from tests import intrinsics_parity as ip
from tests.test_gpu_pcg_variants import ulp_distance

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
PAIRS = [(name, inst) for name in ip.CASES for inst in ip.INSTANTIATIONS]
worst_seen = {}   # group -> (worst ratio, case it came from)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def raw(x):
    """The bytes of an array of any type (NaN flags compare equal)."""
    return np.ascontiguousarray(x).view(np.uint8)


def run_step(hip, scene, depth, colour, pad=(0, 0)):
    """One tapped step on a fresh copy of the scene's cfactor image, the top-left of a device buffer pad = (columns, rows)
    larger that is filled with SENTINEL.  Returns (color_camera, depth_camera, a, tap, the buffer afterwards)."""
    torch = hip.torch
    h, w = scene.cfactor.shape
    buf = torch.full((h + pad[1], w + pad[0]), SENTINEL, dtype=torch.float32, device=hip.d.device)
    buf[:h, :w] = torch.from_numpy(scene.cfactor).to(hip.d.device)
    out_c, out_d, a, tap = hip.debug_optimize_intrinsics(depth, colour, cfactor_buf=hip.d.tbuf(buf))
    return out_c, out_d, a, tap, buf.cpu().numpy()


def camera4(cam):
    return np.array([cam.fx, cam.fy, cam.cx, cam.cy], np.float64)


def note(ratios, case):
    for group, ratio in ratios.items():
        if np.isfinite(ratio) and ratio > worst_seen.get(group, (-1.0, ""))[0]:
            worst_seen[group] = (ratio, case)


@pytest.fixture(scope="module", autouse=True)
def report_measured_ratios():
    yield
    print("\nintrinsics step, worst |device - sum64| / abs64 per group:")
    for group, (ratio, case) in sorted(worst_seen.items()):
        print(f"  {group:<20} {ratio:.3e}   {case}")


@pytest.mark.parametrize("name,inst", PAIRS)
def test_intrinsics_step_matches_oracle(oracle, name, inst):
    from tests import gpu_util
    depth, colour = ip.INSTANTIATIONS[inst]
    what = f"{name} <{inst}>"
    shadow = ip.oracle_step(name, inst)["shadow"]
    scene = ip.case_scene(name)
    hip = gpu_util.Hip(scene.to_device())
    out_c, out_d, a, tap, buf = run_step(hip, scene, depth, colour)

    # --- accumulation
    if depth:
        bad = np.flatnonzero(tap["obs"] != shadow["obs"])
        assert bad.size == 0, f"{what}: obs differs in {bad.size} cells, first cell {bad[0]}: {tap['obs'][bad[0]]} != {shadow['obs'][bad[0]]}"
    ratios = ip.accumulated_close(tap["sums"], tap["cells"] if depth else None, shadow, what)
    print(f"{what}: " + ", ".join(f"{g} {r:.3e}" for g, r in ratios.items()))
    note(ratios, what)

    # --- Schur pass and cfactor update, on their own inputs
    if depth:
        schur = ip.schur_close(tap["cells"], tap["sums"], tap["schur_cells"], tap["schur_sums"], shadow, what)
        print(f"{what}: " + ", ".join(f"{g} {r:.3e}" for g, r in schur.items()))
        note(schur, what)
        assert np.array_equal(np.isnan(tap["schur_cells"][5]), tap["obs"] == 0), f"{what}: the flagged cells are not the unobserved ones"
        ip.pixel_update_close(scene.cfactor, buf, tap["schur_cells"], tap["x1"], tap["obs"], what)
        assert np.float32(a) == np.float32(scene.a) - tap["x1"][4]
    else:
        assert np.array_equal(tap["schur_sums"], tap["sums"].astype(np.float64)) and a == np.float32(scene.a)
        assert np.array_equal(bits(buf), bits(scene.cfactor)), f"{what}: the colour step wrote the cfactor image"
        assert not tap["cells"].any() and not tap["obs"].any() and not tap["schur_cells"].any() and not tap["x1"].any()
    if colour:
        assert np.array_equal(camera4(out_c), (camera4(scene.color_camera).astype(np.float32) - tap["x"]).astype(np.float64))
    else:
        assert not tap["x"].any()

    # --- the two host solves, on their own inputs (the ragged cases are rank-deficient: no solution to compare)
    if name in ip.FULL_RANK:
        if depth:
            A, b1 = tap["schur_sums"][:15].copy(), tap["schur_sums"][15:20].copy()
            A[14] += 100.0                                            # the prior on a, weight 10 (BS/kernel_opt_intrinsics.cc:143-155)
            b1[4] += np.float64(np.float32(100) * np.float32(scene.a))
            ip.solve_close(A, b1, tap["x1"], f"{what}: x1")
        if colour:
            ip.solve_close(tap["schur_sums"][20:30], tap["schur_sums"][30:34], tap["x"], f"{what}: x")

    # --- a second run on the same inputs, in the same context
    out_c2, out_d2, a2, tap2, buf2 = run_step(hip, scene, depth, colour)
    assert np.array_equal(bits(tap2["sums"]), bits(tap["sums"])), f"{what}: the 40 sums differ between two runs"
    assert np.array_equal(tap2["obs"], tap["obs"])
    assert ulp_distance(tap2["cells"], tap["cells"]).max() <= 1, f"{what}: cell entries differ by more than 1 ulp between two runs"
    if np.array_equal(bits(tap2["cells"]), bits(tap["cells"])):   # the same rounded cells: everything after them is a fixed-order computation
        for key in ("schur_sums", "schur_cells", "x1", "x"):
            assert np.array_equal(raw(tap2[key]), raw(tap[key])), f"{what}: {key} differs between two runs"
        assert np.array_equal(bits(buf2), bits(buf)) and a2 == a
        assert np.array_equal(camera4(out_c2), camera4(out_c)) and np.array_equal(camera4(out_d2), camera4(out_d))


@pytest.mark.parametrize("name,inst", [(name, inst) for name in ip.FULL_RANK for inst in ip.INSTANTIATIONS])
def test_solved_outputs_match_oracle(oracle, name, inst):
    """The cameras, a and the cfactor image after the step against the oracle with its global blocks summed in float64, at the
    bars of test_gpu_direct_ba.py's two step tests: depth camera 1e-4 relative, a 1e-3 of max(|a|, 1e-2), cfactor 1e-3 of the
    largest (at least 1e-3), colour camera 2e-4 px (held on the step x itself: these scenes start from the true colour camera,
    so the step is below the rounding of the camera's own values).  Full-rank cases only: the ragged ones are rank-deficient by
    construction.

    `a` is the weakly determined unknown of the 5 x 5 system (cond 1.6e8 in even, 7.1e8 in k17): 1e-7 of abs64 in b1's `a` entry
    moves it by 3e-5, three times the bar, and the oracle's own serial-fp32 mode lands 2.5e-04 (even) and 6.1e-04 (k17) from its
    float64-summed mode.  The device therefore sums the threads' fp32 sums in float64 and keeps the Schur correction and the
    solve's inputs in float64.  Measured on an MI355X, |a - oracle's a| (bar 1e-05; k17 1.107e-05):
        even 1.401e-06   odd 1.222e-06   odd-border 1.865e-06   tiny 3.763e-07   k17 8.823e-06   colour-2x 5.960e-07
    (depth camera <= 2.1e-07 relative, cfactor <= 4.2e-08, colour step <= 2.8e-09 px everywhere)."""
    from tests import gpu_util
    depth, colour = ip.INSTANTIATIONS[inst]
    what = f"{name} <{inst}>"
    ref = ip.oracle_step(name, inst)
    after = ref["scene"]
    scene = ip.case_scene(name)
    hip = gpu_util.Hip(scene.to_device())
    out_c, out_d, a, tap, buf = run_step(hip, scene, depth, colour)
    failures = []

    def judge(label, err, bar):
        print(f"{what}: {label} {err:.3e} (bar {bar:.3e})")
        if not err <= bar:
            failures.append(f"{label} {err:.3e} > {bar:.3e}")

    if depth:
        got, exp = camera4(out_d), camera4(after.depth_camera)
        judge("depth camera, worst relative", float((np.abs(got - exp) / np.abs(exp)).max()), 1e-4)
        judge("a", abs(a - after.a), 1e-3 * max(abs(after.a), 1e-2))
        judge("cfactor", float(np.abs(buf - after.cfactor).max()), 1e-3 * max(float(np.abs(after.cfactor).max()), 1e-3))
        assert (out_d.width, out_d.height) == (scene.depth_camera.width, scene.depth_camera.height)
    if colour:
        judge("colour camera, worst px", float(np.abs(camera4(out_c) - camera4(after.color_camera)).max()), 2e-4)
        judge("colour step x, worst px", float(np.abs(tap["x"].astype(np.float64) - ref["shadow"]["x"]).max()), 2e-4)
        print(f"{what}: colour step x {tap['x']!r}")
        assert (out_c.width, out_c.height) == (scene.color_camera.width, scene.color_camera.height)
    assert not failures, f"{what}: " + "; ".join(failures)


def test_larger_cfactor_buffer(oracle):
    """The odd scene with its cfactor image as the top-left of a buffer 7 columns and 3 rows larger: the cell arrays are indexed
    by the grid's own width, so every tapped entry and the cfactor image equal the exact-size run's (fixed-order sums bit for
    bit, cells within 1 ulp) and the rest of the buffer keeps its sentinel."""
    from tests import gpu_util
    scene = ip.case_scene("odd")
    h, w = scene.cfactor.shape
    hip = gpu_util.Hip(scene.to_device())
    out_c, out_d, a, tap, buf = run_step(hip, scene, True, True)
    big_c, big_d, big_a, big_tap, big = run_step(hip, scene, True, True, pad=(7, 3))
    assert big.shape == (h + 3, w + 7) == (32, 45)
    outside = np.ones(big.shape, bool)
    outside[:h, :w] = False
    assert np.all(big[outside] == np.float32(SENTINEL)), "the step wrote outside the cfactor image"
    assert np.array_equal(bits(big_tap["sums"]), bits(tap["sums"])) and np.array_equal(big_tap["obs"], tap["obs"])
    assert tap["obs"].any() and tap["obs"].reshape(h, w)[1:].any(), "cells beyond the first grid row are observed"
    assert ulp_distance(big_tap["cells"], tap["cells"]).max() <= 1
    if np.array_equal(bits(big_tap["cells"]), bits(tap["cells"])):
        for key in ("schur_sums", "schur_cells", "x1", "x"):
            assert np.array_equal(raw(big_tap[key]), raw(tap[key])), key
        assert np.array_equal(bits(big[:h, :w]), bits(buf)) and big_a == a
        assert np.array_equal(camera4(big_c), camera4(out_c)) and np.array_equal(camera4(big_d), camera4(out_d))
    else:
        ip.pixel_update_close(scene.cfactor, big[:h, :w], big_tap["schur_cells"], big_tap["x1"], big_tap["obs"], "odd, larger buffer")
    assert not np.array_equal(big[:h, :w], scene.cfactor), "the step moved the cfactor image"


@pytest.mark.parametrize("inst", list(ip.INSTANTIATIONS))
def test_intrinsics_step_without_surfels(oracle, inst):
    """surfels_size = 0 (BS/kernel_opt_intrinsics.cc:55-57): OK, and the out cameras, a, the cfactor image and the (zeroed) tap
    arrays are untouched."""
    import copy
    from tests import gpu_util
    depth, colour = ip.INSTANTIATIONS[inst]
    scene = copy.copy(ip.case_scene("tiny"))
    scene.surfels_size = 0
    hip = gpu_util.Hip(scene.to_device())
    out_c, out_d, a, tap, buf = run_step(hip, scene, depth, colour)   # debug_optimize_intrinsics checks the return code
    assert not camera4(out_c).any() and not camera4(out_d).any() and out_c.width == 0 and out_d.width == 0
    assert a == np.float32(scene.a)
    assert np.array_equal(bits(buf), bits(scene.cfactor))
    assert all(not arr.any() for arr in tap.values())


def test_partial_and_null_tap(oracle):
    """A null tap is the product call; a tap with only some members fills those and nothing else -- the same values as the full
    tap's, and the same results."""
    import ctypes as C
    import badslam_amd
    from badslam_amd import abi
    from tests import gpu_util
    scene = ip.case_scene("tiny")
    cells = scene.cfactor.size
    hip = gpu_util.Hip(scene.to_device())
    out_c, out_d, a, tap, buf = run_step(hip, scene, True, True)
    torch = hip.torch

    def call(tap_arg):
        cf = torch.from_numpy(scene.cfactor).to(hip.d.device)
        dp, sb = hip._common()
        dp.cfactor_buffer = hip.d.tbuf(cf)
        oc, od, av = abi.Camera4f(), abi.Camera4f(), C.c_float(scene.a)
        badslam_amd.check(hip.L.bslam_debug_optimize_intrinsics(
            hip.ctx.handle, gpu_util.stream_ptr(), 1, 1, len(scene.keyframes), hip.d.keyframe_views(), C.byref(scene.color_camera),
            C.byref(scene.depth_camera), C.byref(dp), scene.surfels_size, C.byref(sb), C.byref(oc), C.byref(od), C.byref(av), tap_arg))
        torch.cuda.synchronize()
        return oc, od, av.value, cf.cpu().numpy()

    part = {"obs": np.zeros(cells, np.uint32), "x1": np.zeros(5, np.float32), "schur_sums": np.zeros(40, np.float64)}
    results = [call(None), call(C.byref(abi.IntrinsicsTap())), call(C.byref(abi.IntrinsicsTap(**{k: v.ctypes.data for k, v in part.items()})))]
    for oc, od, av, cf in results:
        assert np.array_equal(camera4(oc), camera4(out_c)) and np.array_equal(camera4(od), camera4(out_d)) and av == a
        assert ulp_distance(cf, buf).max() <= 1
    assert np.array_equal(part["obs"], tap["obs"]) and tap["obs"].any()
    assert np.array_equal(bits(part["x1"]), bits(tap["x1"])) and np.array_equal(part["schur_sums"], tap["schur_sums"])
