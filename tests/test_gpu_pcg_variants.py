"""-m gpu parity of every pcg_{init,step1}_kernel<kDepth, kDesc, kIntr> instantiation, of the vector kernels with the a-prior
term and of bslam_update_cfactors_from_pcg_delta against the oracle, entry by entry.

Which case launches which instantiation (init and step 1 alike):
  <depth, -, ->        k17-depth, k65-depth, first100-depth     <depth, -, intr>     a, f-no-geometry, f-no-poses
  <depth, desc, ->     both-no-intr                             <depth, desc, intr>  b, c, d, b-gauge-first, b-gauge-last, k17-b, k65-b,
  <-, desc, ->         e-no-intr                                                     first100-b
  <-, desc, intr>      e-colour
K <= 16: every K = 3 case; 16 < K <= 64 (a full RowStash group and a flush of one more): k17-*; K > 64 (a second batch of the
keyframe walk): k65-*.

Shared entries (poses, intrinsics, cfactor cells) are sums over every (keyframe, surfel) pair and are judged per entry against
the oracle's float64 shadow sums (tests/pcg_parity.py); per-surfel entries are formed in the reference's order and keep the
relative bounds of tests/test_gpu_pcg.py.  The device vectors are reloaded from the oracle before every kernel."""
import copy
import functools

import numpy as np
import pytest

from tests import bso, pcg_parity as pp

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
K_DIAG_EPSILON, K_A_PRIOR = 1e-8, 100.0   # BS/kernel_pcg.cu:44, :48 (weight 10, squared)

#            K  cell depth  desc   poses  geom   dintr  cintr  gauge surfels
CASES = {
    "a":              (3, 2, True,  False, True,  True,  True,  False, 1, None),
    "b":              (3, 2, True,  True,  True,  True,  True,  True,  1, None),
    "c":              (3, 2, True,  True,  True,  True,  False, True,  1, None),
    "d":              (3, 2, True,  True,  True,  True,  True,  False, 1, None),
    "e-no-intr":      (3, 2, False, True,  True,  True,  False, False, 1, None),
    "e-colour":       (3, 2, False, True,  True,  True,  False, True,  1, None),
    "f-no-geometry":  (3, 2, True,  False, True,  False, True,  False, 1, None),
    "f-no-poses":     (3, 2, True,  False, False, True,  True,  False, 1, None),
    "both-no-intr":   (3, 2, True,  True,  True,  True,  False, False, 1, None),
    "b-gauge-first":  (3, 2, True,  True,  True,  True,  True,  True,  0, None),
    "b-gauge-last":   (3, 2, True,  True,  True,  True,  True,  True,  2, None),
    "k17-depth":      (17, 4, True, False, True,  True,  False, False, 1, None),
    "k17-b":          (17, 4, True, True,  True,  True,  True,  True,  1, None),
    "k65-depth":      (65, 4, True, False, True,  True,  False, False, 1, None),
    "k65-b":          (65, 4, True, True,  True,  True,  True,  True,  1, None),
    "first100-depth": (3, 2, True,  False, True,  True,  False, False, 1, 100),
    "first100-b":     (3, 2, True,  True,  True,  True,  True,  True,  1, 100),
}


@functools.lru_cache(maxsize=None)
def base_scene(K, cell, use_depth, use_desc):
    """One scene per (K, cell, residuals), shared by the cases and never modified."""
    return pp.variant_scene(K, cell, use_depth, use_desc, seed=100 + K)


def case_scene(name):
    K, cell, use_depth, use_desc, poses, geom, dintr, cintr, gauge, surfels = CASES[name]
    scene = base_scene(K, cell, use_depth, use_desc)
    if surfels is not None:
        assert scene.surfels_size > surfels
        scene = copy.copy(scene)   # the buffers stay shared; only the count differs
        scene.surfels_size = surfels
    layout = bso.pcg_layout(scene, optimize_poses=poses, optimize_geometry=geom, optimize_depth_intrinsics=dintr,
                            optimize_color_intrinsics=cintr, gauge_keyframe_id=gauge)
    return scene, layout


ulp_distance = pp.ulp_distance   # (test_gpu_intrinsics_step imports it from here)


def assert_same_run(first, second, groups, what):
    """Two runs on the same inputs: bit-identical but for the cfactor cells, whose float64 atomic sums may round differently
    once in a great while (1 fp32 ulp)."""
    d = ulp_distance(first, second)
    for name, idx in groups.items():
        worst = int(d[idx].max()) if len(idx) else 0
        allowed = 1 if name == "cfactor cells" else 0
        assert worst <= allowed, f"{what} [{name}]: two runs differ by {worst} ulp at unknown {idx[np.argmax(d[idx])]}"


def entrywise_close(got, ref, scale, what, groups):
    """Elementwise kernels on identical inputs: each entry takes at most six fp32 roundings (2^-24 of the largest intermediate,
    `scale`) on either side, and the two sides may fuse different products: 12 * 2^-24 < 1e-6 of scale, per entry."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    bound = 1e-6 * np.asarray(scale, np.float64)
    for name, idx in groups.items():
        bad = idx[~(err[idx] <= bound[idx])]
        assert bad.size == 0, (f"{what} [{name}]: {bad.size} of {len(idx)} entries off, first at unknown {bad[0]}: got {got[bad[0]]!r}, "
                               f"oracle {ref[bad[0]]!r}, |diff| {err[bad[0]]:.3e} > {bound[bad[0]]:.3e}")


def dot_close(got, terms64, what):
    """A dot product over the unknowns: the device's tree (4 serial, 6 wave, 3 block, then up to 10 levels over the block sums)
    is at most 23 roundings deep, 23 * 2^-24 = 1.4e-6 of sum |term|, on terms that are each within 1e-6 (entrywise_close):
    2.4e-6, granted 1e-5.  The reference value is the float64 sum of the oracle's terms."""
    ref, scale = float(np.sum(terms64)), float(np.sum(np.abs(terms64)))
    assert abs(got - ref) <= 1e-5 * scale, f"{what}: got {got!r}, float64 {ref!r}, |diff| / sum|term| {abs(got - ref) / max(scale, 1e-300):.3e} > 1e-5"


def diag_extra(layout, n):
    e = np.full(n, K_DIAG_EPSILON)
    if layout.a_unknown_index != pp.INVALID:
        e[layout.a_unknown_index] += K_A_PRIOR
    return e


@pytest.fixture(scope="module", autouse=True)
def report_measured_ratios():
    yield
    print("\nPCG shared entries, worst |device - sum64| / abs64 per group:", {k: float(f"{v:.3e}") for k, v in sorted(pp.measured.items())})


@pytest.mark.parametrize("name", list(CASES))
def test_pcg_variant_matches_oracle(oracle, name):
    from tests import gpu_util
    scene, layout = case_scene(name)
    hip = gpu_util.Hip(scene.to_device())
    ref = bso.HostPCG(scene, layout)
    got = gpu_util.HipPCG(hip, layout)
    n = layout.unknown_count
    groups = pp.entry_groups(scene, layout)
    shared = pp.shared_groups(scene, layout)
    surf = groups.get("surfels", np.zeros(0, np.int64))
    extra = diag_extra(layout, n)
    f64 = lambda x: np.asarray(x[:n], np.float64)
    if layout.optimize_depth_intrinsics:
        assert scene.a != 0 and scene.cfactor.any(), "the depth deformation has real values"

    # --- init: r0 and M
    ref.init(); got.init()
    r0, M0 = got.get("r")[:n], got.get("M")[:n]
    pp.rel_close(r0[surf], ref.r[surf], 1e-6, f"{name}: r0 [surfels]")
    pp.rel_close(M0[surf], ref.M[surf], 1e-6, f"{name}: M [surfels]")
    pp.shared_close(r0, ref.shared_sums("r"), shared, f"{name}: r0")
    pp.shared_close(M0, ref.shared_sums("M"), shared, f"{name}: M")
    got.init()
    assert_same_run(r0, got.get("r")[:n], groups, f"{name}: r0")
    assert_same_run(M0, got.get("M")[:n], groups, f"{name}: M")

    # --- init2 with the scene's a in the prior term
    got.load_from(ref)
    r_in, M_in = f64(ref.r), f64(ref.M)
    ref.init2(); got.init2()
    assert hip.h.a == scene.a
    prior = np.zeros(n)
    if layout.a_unknown_index != pp.INVALID:
        prior[layout.a_unknown_index] = K_A_PRIOR * abs(scene.a)
    r_scale = np.abs(r_in) + prior
    entrywise_close(got.get("p")[:n], ref.p[:n], r_scale / (M_in + extra), f"{name}: p0", groups)
    r_value = r_in - np.sign(scene.a) * prior
    dot_close(got.scalar("alpha_n"), r_value * f64(ref.p), f"{name}: alpha_n")
    assert not got.get("delta")[:n].any() and not got.get("g")[:n].any()

    for step in range(2):
        clear_g = step > 0
        what = f"{name}: step {step}"
        if step > 0:
            ref.swap_alpha_beta()
        # --- step 1: g = A p and alpha_d = p A p (once on a zero g that is not cleared, once cleared)
        got.load_from(ref)
        assert clear_g or not ref.g[:n].any()
        ref.step1(clear_g); got.step1(clear_g)
        g1 = got.get("g")[:n]
        ad64 = bso.lib().bso_pcg_last_alpha_d64()
        pp.shared_close([got.scalar("alpha_d")], (np.array([ad64]), np.array([abs(ad64)])), {"alpha_d": np.array([0])}, f"{what}: alpha_d")
        pp.rel_close(g1[surf], ref.g[surf], 1e-5, f"{what}: g [surfels]")
        pp.shared_close(g1, ref.shared_sums("g"), shared, f"{what}: g")
        alpha_d = got.scalar("alpha_d")
        if not clear_g:
            got.g.zero_()
        got.step1(clear_g)
        assert_same_run(g1, got.get("g")[:n], groups, f"{what}: g")
        assert got.scalar("alpha_d") == alpha_d, f"{what}: alpha_d differs between two runs"

        # --- step 2: delta, r, z and beta_n
        got.load_from(ref)
        alpha = float(ref.scalars[ref.an]) / float(ref.scalars[1]) if ref.scalars[1] >= 1e-35 else 0.0
        delta_in, r_in, g_in, p_in, M_in = f64(ref.delta), f64(ref.r), f64(ref.g), f64(ref.p), f64(ref.M)
        b_ref = ref.step2(); b_got = got.step2()
        r_scale = np.abs(r_in) + abs(alpha) * (np.abs(g_in) + extra * np.abs(p_in))
        z_scale = r_scale / (M_in + extra)
        entrywise_close(got.get("delta")[:n], ref.delta[:n], np.abs(delta_in) + abs(alpha) * np.abs(p_in), f"{what}: delta", groups)
        entrywise_close(got.get("r")[:n], ref.r[:n], r_scale, f"{what}: r", groups)
        entrywise_close(got.get("g")[:n], ref.g[:n], z_scale, f"{what}: z", groups)
        dot_close(b_got, f64(ref.g) * f64(ref.r), f"{what}: beta_n")
        assert b_got == got.scalar("beta_n") and np.isfinite(b_ref)

        # --- step 3: p
        got.load_from(ref)
        beta = float(ref.scalars[ref.bn]) / float(ref.scalars[ref.an]) if ref.scalars[ref.an] >= 1e-35 else 0.0
        z_in, p_in = f64(ref.g), f64(ref.p)
        ref.step3(); got.step3()
        entrywise_close(got.get("p")[:n], ref.p[:n], np.abs(z_in) + abs(beta) * np.abs(p_in), f"{what}: p", groups)


@pytest.mark.parametrize("name", ["a", "b", "k17-depth"])
def test_pcg_without_surfels(oracle, name):
    """surfels_size = 0: init leaves r and M all zero, step 1 leaves g and alpha_d zero (BS/kernel_pcg.cu:536-538), both OK."""
    from tests import gpu_util
    K, cell, use_depth, use_desc, poses, geom, dintr, cintr, gauge, _ = CASES[name]
    scene = copy.copy(base_scene(K, cell, use_depth, use_desc))
    scene.surfels_size = 0
    layout = bso.pcg_layout(scene, optimize_poses=poses, optimize_geometry=geom, optimize_depth_intrinsics=dintr,
                            optimize_color_intrinsics=cintr, gauge_keyframe_id=gauge)
    n = layout.unknown_count
    assert n > 0
    hip = gpu_util.Hip(scene.to_device())
    ref = bso.HostPCG(scene, layout)
    got = gpu_util.HipPCG(hip, layout)   # garbage-filled vectors
    ref.init(); got.init()               # HipPCG checks the return code
    assert not ref.r[:n].any() and not ref.M[:n].any()
    assert not got.get("r")[:n].any() and not got.get("M")[:n].any()
    got.load_from(ref)
    ref.init2(); got.init2()
    assert np.all(np.abs(got.get("p")[:n].astype(np.float64) - ref.p[:n]) <= 1e-6 * np.abs(ref.p[:n])), "p0 = prior term only"
    got.p.fill_(0.5); ref.p[:] = 0.5
    got.g.fill_(123.0)
    ref.step1(True); got.step1(True)
    assert not got.get("g")[:n].any() and got.scalar("alpha_d") == 0.0 == float(ref.scalars[1])


def test_apply_delta_to_cfactors_matches_oracle(oracle):
    """bslam_update_cfactors_from_pcg_delta on the 80x60 cfactor buffer of a 160x120 scene at cell 2, in a device buffer whose
    pitch is wider than its rows, with a random delta and a start index that is no multiple of 4: bit-exact with
    bso_update_cfactors_from_pcg_delta, and not one byte of the row padding touched."""
    import torch
    from tests import gpu_util
    base, _ = case_scene("f-no-geometry")       # poses + depth intrinsics: the cfactor unknowns start at 6 * 2 + 5 = 17
    scene = copy.copy(base)
    scene.cfactor = base.cfactor.copy()
    layout = bso.pcg_layout(scene, optimize_geometry=False, optimize_depth_intrinsics=True, gauge_keyframe_id=1)
    start = layout.depth_intrinsics_unknown_start_index + 5
    h, w = scene.cfactor.shape
    assert (h, w) == (60, 80) and start % 4 != 0 and start + h * w == layout.unknown_count
    hip = gpu_util.Hip(base.to_device())
    ref = bso.HostPCG(scene, layout)
    got = gpu_util.HipPCG(hip, layout)
    rng = np.random.default_rng(7)
    ref.delta[:] = rng.uniform(-0.005, 0.005, ref.delta.size).astype(np.float32)
    got.load_from(ref)

    padded_w = w + 13                            # pitch 372 bytes: rows start at odd multiples of 4 bytes
    sentinel = np.float32(-7.25)
    buf = torch.full((h, padded_w), float(sentinel), dtype=torch.float32, device=hip.d.device)
    buf[:, :w] = torch.from_numpy(base.cfactor).to(hip.d.device)
    cb = hip.d.tbuf(buf, h, w)
    assert cb.pitch == 4 * padded_w and cb.width == w and cb.height == h

    ref.apply_delta_to_cfactors(); got.apply_delta_to_cfactors(cfactor_buf=cb)
    out = buf.cpu().numpy()
    assert not np.array_equal(scene.cfactor, base.cfactor)
    assert np.array_equal(out[:, :w].view(np.uint32), scene.cfactor.view(np.uint32)), "cfactor cells differ from the oracle's"
    assert np.array_equal(out[:, w:].view(np.uint32), np.full((h, padded_w - w), sentinel, np.float32).view(np.uint32)), "row padding was written"
    assert np.array_equal(got.get("delta"), ref.delta), "delta is read only"

    # the scene's own contiguous buffer (pitch == row width), through the default arguments
    got.apply_delta_to_cfactors()
    assert np.array_equal(hip.d.cfactor.cpu().numpy().view(np.uint32), scene.cfactor.view(np.uint32))
