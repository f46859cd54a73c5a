#!/usr/bin/env python3
"""Times bslam_compute_ba_cost (the BA objective pass + its row sums, profile tag BSLAM_PROF_BA_COST) against one batched pose
accumulation launch (bslam_accumulate_pose_coeffs_batched, tag BSLAM_PROF_POSE_ACCUMULATE) on the synthetic stacks: the bench's
dense K = 300 stack with depth + descriptor residuals, the K = 50 geometry-only stack and the K = 1000 trajectory stack.  Tuning
tool: prints ms per launch; run it under `rocprofv3 --kernel-trace --stats` for the per-kernel split."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STACKS = {   # name -> (kind, keyframes, descriptor residuals)
    "dense300": ("dense", 300, True),
    "dense50-geo": ("dense", 50, False),
    "trajectory1000": ("trajectory", 1000, False),
}
PROF_POSE_ACCUMULATE, PROF_BA_COST = 0, 7


def run(name, reps):
    import torch
    import badslam_amd
    from badslam_amd import abi, synthetic
    P = C.POINTER
    kind, K, use_desc = STACKS[name]
    dev = synthetic.TorchStack(K, "cuda:0", kind=kind)
    L = badslam_amd.lib()
    ctx = badslam_amd.Context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cam = dev.stack.camera
    views, dp, sb = dev.keyframe_views(), dev.depth_params(), dev.buf(dev.surfels)
    cost, counts = np.zeros((K, 2), np.float32), np.zeros((K, 2), np.uint32)
    Hb, pose_counts = np.zeros((K, 27), np.float32), np.zeros(K, np.uint32)

    def cost_call():
        badslam_amd.check(L.bslam_compute_ba_cost(ctx.handle, stream, 1, int(use_desc), C.byref(cam), C.byref(cam), C.byref(dp), K, views, dev.surfels_size,
                                                  C.byref(sb), None, cost.ctypes.data_as(P(C.c_float)), counts.ctypes.data_as(P(C.c_uint32)),
                                                  C.cast(None, abi.ALLREDUCE_FN), None))

    def pose_call():
        badslam_amd.check(L.bslam_accumulate_pose_coeffs_batched(ctx.handle, stream, 1, int(use_desc), C.byref(cam), C.byref(cam), C.byref(dp), K, views,
                                                                 dev.surfels_size, C.byref(sb), Hb.ctypes.data_as(P(C.c_float)),
                                                                 pose_counts.ctypes.data_as(P(C.c_uint32))))

    def timed(fn, tag):
        fn()   # warm-up: schedule, sorted copy, records
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
        for _ in range(reps):
            fn()
        n, ms = C.c_int32(), C.c_float()
        badslam_amd.check(L.bslam_profile_read(ctx.handle, tag, C.byref(n), C.byref(ms)))
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 0))
        return ms.value / max(1, n.value)

    t_cost = timed(cost_call, PROF_BA_COST)
    t_pose = timed(pose_call, PROF_POSE_ACCUMULATE)
    pairs = int(counts[:, 0].sum(dtype=np.int64))
    print(f"{name}: K={K} S={dev.surfels_size} desc={int(use_desc)}  cost pass + row sums {t_cost:.3f} ms  pose accumulate {t_pose:.3f} ms  "
          f"ratio {t_cost / t_pose:.3f}  depth pairs {pairs}  desc pairs {int(counts[:, 1].sum(dtype=np.int64))}  "
          f"pairs/s {pairs / (t_cost * 1e-3):.3e}  objective {float(cost.astype(np.float64).sum()):.6e}", flush=True)
    del dev
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stacks", default=",".join(STACKS))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch  # noqa: F401  (HIP runtime first)
    for name in args.stacks.split(","):
        run(name, args.reps)


if __name__ == "__main__":
    main()
