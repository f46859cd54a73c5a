"""-m gpu: the BA objective per keyframe and residual type (bslam_compute_ba_cost, DirectBA.ComputeCost / cost tracking).

Counts are held to the oracle's association flags exactly, costs to the float64 objective formed from the oracle's per-surfel
residuals (tests/ba_cost_util.py) at 1e-4; the value-only descriptor path gives the pose kernels' r1, r2 bit for bit; results are
deterministic and do not depend on culling; two surfel shards over gloo sum to the single-process rows."""
import ctypes as C
import os
import socket

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi, synthetic
from tests import ba_cost_util, bso, scenes
from tests.gpu_util import stream_ptr

pytestmark = pytest.mark.gpu
P = C.POINTER


def ba_cost(ctx, dev, use_depth, use_desc, surfels_size=None, active=None, views=None, K=None, allreduce=None, surfels=None):
    """bslam_compute_ba_cost on a tests.bso.DeviceScene: (rc, cost [K, 2], counts [K, 2])."""
    h = dev.host
    views = dev.keyframe_views() if views is None else views
    K = len(h.keyframes) if K is None else K
    n = dev.surfels_size if surfels_size is None else surfels_size
    cost, counts = np.zeros((max(1, K), 2), np.float32), np.zeros((max(1, K), 2), np.uint32)
    sb = dev.surfel_buf() if surfels is None else surfels
    ab = None if active is None else C.byref(dev.tbuf(active))
    rc = badslam_amd.lib().bslam_compute_ba_cost(
        ctx.handle, stream_ptr(), int(use_depth), int(use_desc), C.byref(h.color_camera), C.byref(h.depth_camera), C.byref(dev.depth_params()),
        K, views, n, C.byref(sb), ab, cost.ctypes.data_as(P(C.c_float)), counts.ctypes.data_as(P(C.c_uint32)),
        allreduce if allreduce is not None else C.cast(None, abi.ALLREDUCE_FN), None)
    return rc, cost[:K], counts[:K]


def check_against_oracle(got_cost, got_counts, want_cost, want_counts):
    assert np.array_equal(got_counts.astype(np.int64), want_counts), (got_counts, want_counts)
    for k, j, err, tol in ba_cost_util.oracle_terms(got_cost, want_cost, want_counts):
        assert err <= tol, (k, j, got_cost[k, j], want_cost[k, j])


def perturb(scene, rng, t=0.006, r=0.003):
    for kf in scene.keyframes:
        x = np.concatenate([rng.uniform(-t, t, 3), rng.uniform(-r, r, 3)]).astype(np.float32)
        kf.global_T_frame = bso.se3_mul(kf.global_T_frame, bso.se3_exp(x))


SCENES = {
    "geometric": lambda: scenes.pose_geometric_scene(seed=1)[0],
    "photometric": lambda: scenes.pose_photometric_scene(seed=2)[0],
    "synthetic": lambda: scenes.synthetic_scene(6, seed=5, use_depth_residuals=True, use_descriptor_residuals=True),
}


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("perturbed", [False, True])
def test_oracle_parity(oracle, name, perturbed):
    scene = SCENES[name]()
    if perturbed:
        perturb(scene, np.random.default_rng(7))
    ctx = badslam_amd.Context(0)
    ctx.set_texture_mode(scene.tex_mode)
    ud, uc = scene.use_depth_residuals, scene.use_descriptor_residuals
    S = scene.surfels_size
    rng = np.random.default_rng(13)
    dev = scene.to_device("cuda:0")
    # deleted surfels: NaN position (the lifecycle's mark) on the device; the oracle reads the intact host copy and the objective
    # leaves them out
    deleted = rng.choice(S, size=max(1, S // 50), replace=False)
    dev.surfels[0, deleted] = float("nan")
    keep = np.ones(S, bool)
    keep[deleted] = False
    want_c, want_n = ba_cost_util.scene_objective(scene, mask=keep)
    rc, c, n = ba_cost(ctx, dev, ud, uc)
    assert rc == 0, badslam_amd.lib().bslam_last_error()
    assert n.sum() > 1000
    check_against_oracle(c, n, want_c, want_n)
    # active mask: only bit 0 counts
    flags = rng.integers(0, 4, size=scene.max_surfels).astype(np.uint8)
    import torch
    act = torch.from_numpy(flags.reshape(1, -1)).to("cuda:0")
    mask = ((flags[:S] & 1) != 0) & keep
    want_c, want_n = ba_cost_util.scene_objective(scene, mask=mask)
    rc, c, n = ba_cost(ctx, dev, ud, uc, active=act)
    assert rc == 0
    check_against_oracle(c, n, want_c, want_n)
    # ragged surfel count (not a multiple of the 256-surfel granule)
    ragged = S - 37
    want_c, want_n = ba_cost_util.scene_objective(scene, mask=keep, surfels_size=ragged)
    rc, c, n = ba_cost(ctx, dev, ud, uc, surfels_size=ragged)
    assert rc == 0
    check_against_oracle(c, n, want_c, want_n)


def test_depth_cost_matches_the_per_keyframe_debug_entry_point(oracle):
    from tests import gpu_util
    scene = SCENES["synthetic"]()
    perturb(scene, np.random.default_rng(3))
    dev = scene.to_device("cuda:0")
    hip = gpu_util.Hip(dev)
    rc, c, n = ba_cost(hip.ctx, dev, True, False)
    assert rc == 0
    for k in range(len(scene.keyframes)):
        ref = hip.accumulate_pose(k, use_depth=True, use_desc=False)
        assert n[k, 0] == ref["count"] and n[k, 1] == 0
        # the debug entry point sums the reference's fp32 form of the Tukey term, (k^2 / 6)(1 - t^3), whose small terms keep few
        # digits, in another order: 1.7e-5 apart on this scene; the objective itself is held to the oracle at 1e-4 above
        assert abs(float(c[k, 0]) - ref["cost"]) <= 5e-5 * abs(ref["cost"]), (k, c[k, 0], ref["cost"])


def test_value_only_descriptor_residuals_are_bit_identical():
    import torch
    scene = SCENES["synthetic"]()
    perturb(scene, np.random.default_rng(4))
    dev = scene.to_device("cuda:0")
    ctx = badslam_amd.Context(0)
    ctx.set_texture_mode(scene.tex_mode)
    L = badslam_amd.lib()
    for mode in (abi.TEX_FIXED_POINT_1_8, abi.TEX_EXACT_FLOAT):
        ctx.set_texture_mode(mode)
        for k in range(len(scene.keyframes)):
            out = torch.zeros((dev.surfels_size, 4), dtype=torch.float32, device="cuda:0")
            badslam_amd.check(L.bslam_debug_ba_cost_descriptor_residuals(
                ctx.handle, stream_ptr(), C.byref(scene.color_camera), C.byref(scene.depth_camera), C.byref(dev.depth_params()),
                C.byref(dev.keyframe_view(k)), dev.surfels_size, C.byref(dev.surfel_buf()), C.c_void_p(out.data_ptr())))
            torch.cuda.synchronize()
            o = np.ascontiguousarray(out.cpu().numpy())
            assert np.count_nonzero(o[:, 0]) > 1000
            assert np.array_equal(o[:, :2].view(np.uint32), o[:, 2:].view(np.uint32))


def test_determinism_culling_and_empty_inputs():
    import torch
    L = badslam_amd.lib()
    K = 72
    dev = synthetic.TorchStack(K, "cuda:0", kind="trajectory", border_valid=True)
    assert dev.surfels_size >= 64 * 256
    ctx = badslam_amd.Context(0)
    cam = dev.stack.camera
    stream = stream_ptr()
    rng = np.random.default_rng(9)
    views = dev.keyframe_views()
    for k in range(K):
        _, M, Rg = dev.stack.pose(k, np.concatenate([rng.uniform(-0.004, 0.004, 3), rng.uniform(-0.002, 0.002, 3)]))
        views[k].frame_T_global, views[k].global_R_frame = M, Rg
    act = torch.from_numpy((rng.integers(0, 2, size=(1, dev.surfels_size))).astype(np.uint8)).to("cuda:0")

    def run(use_desc, active=None, n=None, kcount=K):
        cost, counts = np.zeros((K, 2), np.float32), np.zeros((K, 2), np.uint32)
        ab = None if active is None else C.byref(dev.buf(active))
        rc = L.bslam_compute_ba_cost(ctx.handle, stream, 1, int(use_desc), C.byref(cam), C.byref(cam), C.byref(dev.depth_params()), kcount, views,
                                     dev.surfels_size if n is None else n, C.byref(dev.buf(dev.surfels)), ab, cost.ctypes.data_as(P(C.c_float)),
                                     counts.ctypes.data_as(P(C.c_uint32)), C.cast(None, abi.ALLREDUCE_FN), None)
        assert rc == 0, L.bslam_last_error()
        return cost, counts

    for use_desc in (False, True):
        for active in (None, act):
            out = {}
            for on in (1, 0, 1):
                badslam_amd.check(L.bslam_set_culling(ctx.handle, on))
                out.setdefault(on, []).append(run(use_desc, active))
            a, b, c = out[1][0], out[1][1], out[0][0]
            for x, y in ((a, b), (a, c)):
                assert np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32)) and np.array_equal(x[1], y[1])
            assert a[1][:, 0].min() > 0 and a[1][:, 0].sum() > 100000
            if use_desc:
                assert a[1][:, 1].sum() > 100000 and a[0][:, 1].sum() > 0
    badslam_amd.check(L.bslam_set_culling(ctx.handle, 1))
    cost, counts = run(True, n=0)
    assert not cost.any() and not counts.any()
    cost, counts = run(True, kcount=0)
    assert not cost.any() and not counts.any()


def test_dense_300_keyframe_stack_counts_and_oracle_sample(oracle):
    import torch
    L = badslam_amd.lib()
    K = 300
    dev = synthetic.TorchStack(K, "cuda:0", kind="dense")
    S = dev.surfels_size
    ctx = badslam_amd.Context(0)
    cam = dev.stack.camera
    views = dev.keyframe_views()
    dp = dev.depth_params()
    sb = dev.buf(dev.surfels)

    def run(active=None):
        cost, counts = np.zeros((K, 2), np.float32), np.zeros((K, 2), np.uint32)
        badslam_amd.check(L.bslam_compute_ba_cost(ctx.handle, stream_ptr(), 1, 1, C.byref(cam), C.byref(cam), C.byref(dp), K, views, S, C.byref(sb),
                                                  None if active is None else C.byref(dev.buf(active)), cost.ctypes.data_as(P(C.c_float)),
                                                  counts.ctypes.data_as(P(C.c_uint32)), C.cast(None, abi.ALLREDUCE_FN), None))
        return cost, counts

    cost, counts = run()
    inb, assoc = C.c_uint64(), C.c_uint64()
    badslam_amd.check(L.bslam_debug_count_pairs(ctx.handle, stream_ptr(), C.byref(cam), C.byref(dp), K, views, S, C.byref(sb), C.byref(inb), C.byref(assoc)))
    assert int(counts[:, 0].sum(dtype=np.int64)) == assoc.value
    assert counts[:, 1].sum(dtype=np.int64) > 0 and cost[:, 0].sum() > 0 and cost[:, 1].sum() > 0
    # keyframes 0, 150, 299 against the oracle on a fixed sample of 2^14 surfel columns (the active mask selects them on the device)
    rng = np.random.default_rng(21)
    cols = np.sort(rng.choice(S, size=1 << 14, replace=False))
    flags = np.zeros((1, S), np.uint8)
    flags[0, cols] = 1
    sample_cost, sample_counts = run(torch.from_numpy(flags).to("cuda:0"))
    surf = np.ascontiguousarray(dev.surfels[:, cols].cpu().numpy())
    dp_host = abi.DepthParams(bso.np_buffer2d(dev.stack.cfactor), 0.0, float(dev.stack.raw_to_float_depth), dev.stack.baseline_fx, dev.stack.cell)
    for k in (0, 150, 299):
        depth, normals, radius, color = dev.host_keyframe(k)
        _, M, _ = dev.stack.pose(k)
        ps, _, _ = ba_cost_util.oracle_per_surfel(cam, cam, dp_host, depth, normals, color, M, surf, len(cols), abi.TEX_FIXED_POINT_1_8, True, True)
        want_c, want_n = ba_cost_util.objective_from_probe(ps, True, True)
        check_against_oracle(sample_cost[k:k + 1], sample_counts[k:k + 1], want_c[None], want_n[None])
        assert want_n[0] > 100


def _direct_ba(scene):
    from badslam_amd.direct_ba import DirectBA
    ba = DirectBA(scene.max_surfels, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, 0.8, 1, 1, 1, scene.color_camera, scene.depth_camera, 0,
                  scene.use_depth_residuals, scene.use_descriptor_residuals)
    ba.set_options(texture_mode=scene.tex_mode, scheme_end_tasks=False)
    for kf in scene.keyframes:
        ba.AddKeyframe(kf.id, max(kf.min_depth, 1e-3), max(kf.max_depth, 1e-2), kf.depth, kf.normals, kf.radius, kf.color, kf.global_T_frame)
    ba.SetSurfels(scene.surfels[:8], scene.surfels_size)
    return ba


def test_host_loop_cost_tracking():
    scene = scenes.synthetic_scene(6, seed=5)
    perturb(scene, np.random.default_rng(17), t=0.01, r=0.004)
    iterations = 5
    runs = {}
    for tracking in (False, True):
        ba = _direct_ba(scene)
        ba.SetCostTracking(tracking)
        if tracking:
            before = ba.ComputeCost()
            assert len(before["keyframe_ids"]) == 6 and before["counts"][:, 0].min() > 0 and before["counts"][:, 1].sum() == 0
            assert before["total"] == pytest.approx(float(before["cost"].astype(np.float64).sum()))
        it, _ = ba.BundleAdjustment(False, False, False, True, True, iterations, iterations, False, 0, len(scene.keyframes) - 1, False)
        assert it == iterations
        poses = np.array([bso.se3_to_np(ba.keyframe_pose(k)) for k in range(6)], np.float32)
        runs[tracking] = (poses, ba.GetSurfels(8), ba.cost_history)
        if tracking:
            after = ba.ComputeCost()
            active_only = ba.ComputeCost(active_surfels_only=True)
            assert active_only["counts"][:, 0].sum() <= after["counts"][:, 0].sum()
        ba.close()
    (p0, s0, h0), (p1, s1, h1) = runs[False], runs[True]
    assert np.array_equal(p0.view(np.uint32), p1.view(np.uint32))
    assert np.array_equal(np.ascontiguousarray(s0).view(np.uint32), np.ascontiguousarray(s1).view(np.uint32))
    assert len(h0) == 0 and h1.shape == (iterations + 1, 2)
    totals = h1.sum(axis=1)
    assert totals[-1] < totals[0], totals
    assert h1[0].sum() == pytest.approx(before["total"], rel=1e-12)
    assert h1[-1].sum() == pytest.approx(after["total"], rel=1e-12)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard_scene():
    scene = scenes.synthetic_scene(4, seed=11, use_depth_residuals=True, use_descriptor_residuals=True)
    perturb(scene, np.random.default_rng(5))
    return scene


def _worker(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from badslam_amd.distributed import AllReduceHook, shard_range
    bso.build_oracle()
    scene = _shard_scene()
    lo, hi = shard_range(scene.surfels_size, rank, world)
    shard = bso.HostScene(scene.color_camera, scene.depth_camera, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, max(1, hi - lo),
                          use_depth_residuals=True, use_descriptor_residuals=True, tex_mode=scene.tex_mode)
    shard.surfels = np.ascontiguousarray(scene.surfels[:, lo:hi])
    shard.active = np.ascontiguousarray(scene.active[:, lo:hi])
    shard.surfels_size = hi - lo
    shard.keyframes = scene.keyframes
    dev = shard.to_device("cuda:0")
    ctx = badslam_amd.Context(0)
    ctx.set_texture_mode(scene.tex_mode)
    hook = AllReduceHook(device=True)
    rc, cost, counts = ba_cost(ctx, dev, True, True, allreduce=hook.callback)
    assert rc == 0 and hook.calls == 1
    np.save(os.path.join(out_dir, f"cost_{rank}.npy"), cost)
    np.save(os.path.join(out_dir, f"counts_{rank}.npy"), counts)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_over_gloo_sum_to_the_single_process_rows(tmp_path, oracle):
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    c0, c1 = np.load(tmp_path / "cost_0.npy"), np.load(tmp_path / "cost_1.npy")
    n0, n1 = np.load(tmp_path / "counts_0.npy"), np.load(tmp_path / "counts_1.npy")
    assert np.array_equal(c0.view(np.uint32), c1.view(np.uint32)) and np.array_equal(n0, n1)
    scene = _shard_scene()
    dev = scene.to_device("cuda:0")
    ctx = badslam_amd.Context(0)
    ctx.set_texture_mode(scene.tex_mode)
    rc, cost, counts = ba_cost(ctx, dev, True, True)
    assert rc == 0
    assert np.array_equal(n0, counts) and counts[:, 0].min() > 0 and counts[:, 1].min() > 0
    assert np.allclose(c0, cost, rtol=1e-5, atol=1e-6 * float(np.abs(cost).max()))
