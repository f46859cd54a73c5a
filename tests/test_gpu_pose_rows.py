"""-m gpu: a partial pose row depends only on its (work slot, keyframe).

The photometric pose kernel (csrc/pose_kernels.hpp: pose_accumulate_desc) stages a work slot's surfels once per workgroup and
deals the visited keyframes of a chunk round-robin to its four waves; one wave forms the whole (slot, keyframe) row.  Which wave
that is depends on the keyframe's place in its chunk and on which other keyframes of the chunk were visited.  The rows, and so
the per-keyframe H / b sums, must not: each lane adds its surfels in a fixed order and the reduction order is fixed.  Checked
by putting the same keyframes at other places of the keyframe table -- reversed, rotated, and one keyframe repeated over the
whole table (every copy visited by another wave) -- and comparing bits."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi, synthetic

pytestmark = pytest.mark.gpu
P = C.POINTER


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Runner:
    def __init__(self, dev, use_depth=1):
        import torch
        self.dev, self.use_depth = dev, use_depth
        self.L = badslam_amd.lib()
        self.ctx = badslam_amd.Context(0)
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.K = dev.stack.K
        self.cam = dev.stack.camera

    def views(self, xis):
        kfs = self.dev.keyframe_views()
        for k in range(self.K):
            _, M, Rg = self.dev.stack.pose(k, xis[k])
            kfs[k].frame_T_global, kfs[k].global_R_frame = M, Rg
        return kfs

    def coeffs(self, kfs):
        dp, sb = self.dev.depth_params(), self.dev.buf(self.dev.surfels)
        Hb = np.zeros((self.K, 27), np.float32)
        counts = np.zeros(self.K, np.uint32)
        badslam_amd.check(self.L.bslam_accumulate_pose_coeffs_batched(
            self.ctx.handle, self.stream, self.use_depth, 1, C.byref(self.cam), C.byref(self.cam), C.byref(dp), self.K, kfs,
            self.dev.surfels_size, C.byref(sb), Hb.ctypes.data_as(P(C.c_float)), counts.ctypes.data_as(P(C.c_uint32))))
        return Hb, counts

    def poses(self, kfs, inits, iterations):
        dp, sb = self.dev.depth_params(), self.dev.buf(self.dev.surfels)
        poses = (abi.SE3f * self.K)()
        C.memmove(poses, inits, C.sizeof(poses))
        iters, conv = (C.c_int32 * self.K)(), (C.c_int32 * self.K)()
        badslam_amd.check(self.L.bslam_estimate_frame_poses_batched(
            self.ctx.handle, self.stream, self.use_depth, 1, C.byref(self.cam), C.byref(self.cam), C.byref(dp), self.K, kfs,
            self.dev.surfels_size, C.byref(sb), iterations, poses, iters, conv, C.cast(None, abi.ALLREDUCE_FN), None))
        return np.array([[*p.q, *p.t] for p in poses], np.float32), np.array(list(iters))


def permuted(kfs, order):
    out = (abi.KeyframeView * len(order))()
    for place, k in enumerate(order):
        C.memmove(C.byref(out[place]), C.byref(kfs[k]), C.sizeof(abi.KeyframeView))
    return out


# K = 8: one chunk, no culling; K >= 64: several chunks, block-level culling and (batched loop) the list of unconverged keyframes
@pytest.mark.parametrize("kind,K,use_depth", [("dense", 8, 1), ("dense", 8, 0), ("survey", 66, 1), ("trajectory", 72, 1)])
def test_pose_rows_do_not_depend_on_the_keyframes_place(kind, K, use_depth):
    dev = synthetic.TorchStack(K, "cuda:0", kind=kind, border_valid=True)
    assert dev.surfels_size >= 64 * 256 and K >= 4          # the per-surfel work order is in use
    run = Runner(dev, use_depth)
    rng = np.random.default_rng(5)
    pix = 1.0 / 525.0
    xis = [np.concatenate([rng.uniform(-1, 1, 3) * 0.002, rng.uniform(-1, 1, 3) * pix]) for _ in range(K)]
    kfs = run.views(xis)
    Hb, counts = run.coeffs(kfs)
    assert counts.min() > 1000, counts.min()                  # the sums are not trivially empty
    assert np.isfinite(Hb).all()
    order_sets = [list(range(K - 1, -1, -1)), [(k + 5) % K for k in range(K)], [(3 * k + 1) % K for k in range(K)] if K % 3 else None]
    for order in [o for o in order_sets if o is not None]:
        Hb2, counts2 = run.coeffs(permuted(kfs, order))
        assert np.array_equal(bits(Hb2), bits(Hb[order])), order[:4]
        assert np.array_equal(counts2, counts[order])
    # one keyframe at every place of the table: each copy's rows are formed by another wave and next to other visited copies
    for j in sorted({0, K // 2, K - 1}):
        Hb3, counts3 = run.coeffs(permuted(kfs, [j] * K))
        assert np.array_equal(bits(Hb3), np.broadcast_to(bits(Hb[j]), Hb3.shape)), j
        assert (counts3 == counts[j]).all()


@pytest.mark.parametrize("kind,K", [("dense", 8), ("trajectory", 72)])
def test_batched_poses_do_not_depend_on_the_keyframes_place(kind, K):
    """The batched Gauss-Newton loop: keyframes converge after different iteration counts, so from 64 keyframes on the list of
    unconverged keyframes moves every straggler to other places, chunks and waves; the poses must still be the same bits."""
    dev = synthetic.TorchStack(K, "cuda:0", kind=kind, border_valid=True)
    run = Runner(dev)
    rng = np.random.default_rng(9)
    inits = (abi.SE3f * K)()
    for k in range(K):
        inits[k] = dev.stack.pose(k, np.concatenate([rng.choice([-1, 1], 3) * 0.005, rng.choice([-1, 1], 3) * 0.001]))[0]
    kfs = dev.keyframe_views()
    poses, iters = run.poses(kfs, inits, 6)
    order = list(range(K - 1, -1, -1))
    inits2 = (abi.SE3f * K)(*[inits[k] for k in order])
    poses2, iters2 = run.poses(permuted(kfs, order), inits2, 6)
    assert np.array_equal(bits(poses2), bits(poses[order]))
    assert np.array_equal(iters2, iters[order])
