#!/usr/bin/env python3
"""Times the surface views of a fused volume (bslam_prepare_volume_views, bslam_raycast_volume) on the synthetic stacks of
badslam_amd.synthetic at 640x480 -- K = 50 and K = 300 keyframes, fused as tools/bench_fusion.py fuses them: the box of the surfel
model padded by the truncation, 1 cm voxels, truncation 4 voxels, colour on -- from the pose of keyframe 0, with depth, colour
and normal views and a step of one voxel.  Device events around every call; every figure is the median of --reps calls after a
warm-up, with the block test on and off alternating inside the same run (on, off, on, off, ...), so that both see the same
clocks.  Beside the times: the in-range samples that reached the block test, those it skipped and those evaluated
(bslam_debug_cull_stats, from one extra call each that is not timed), samples per second, and the pixels hit.  Not part of
bench.py.  Prints one JSON line.
usage: tools/bench_raycast.py [--reps N] [--keyframes 50 300] [--voxel-size M] [--min-count N] [--max-depth M] [--kind dense]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 640, 480


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--keyframes", type=int, nargs="+", default=[50, 300])
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--min-depth", type=float, default=0.05)
    ap.add_argument("--max-depth", type=float, default=10.0)
    ap.add_argument("--kind", default="dense")
    args = ap.parse_args()
    from badslam_amd import build
    build.build()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_raycast.py needs a GPU: there is no CPU path to time")
    import badslam_amd
    from badslam_amd import abi, synthetic
    from tools import run_tum
    L = badslam_amd.lib()
    ctx = badslam_amd.Context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    truncation = 4 * args.voxel_size

    def timed(call):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e3

    res = {"size": [W, H], "reps": args.reps, "voxel_size_m": args.voxel_size, "step_m": args.voxel_size, "truncation_m": truncation, "min_count": args.min_count,
           "depth_range_m": [args.min_depth, args.max_depth], "kind": args.kind, "block": [8, 8, 8], "views": ["depth", "color", "normal"], "stacks": []}
    for K in args.keyframes:
        dev = synthetic.TorchStack(K, "cuda:0", width=W, height=H, kind=args.kind)
        cam = dev.stack.camera
        xyz = dev.surfels[:3, :dev.surfels_size]
        valid = ~torch.isnan(xyz[0])
        lo, hi = xyz[:, valid].min(dim=1).values.cpu().numpy(), xyz[:, valid].max(dim=1).values.cpu().numpy()
        origin, (nx, ny, nz) = run_tum.mesh_volume(lo, hi, args.voxel_size, truncation)
        vol = abi.Volume((C.c_float * 3)(*origin), args.voxel_size, nx, ny, nz)
        volumes = [torch.zeros((nz * ny, nx), dtype=torch.int32, device="cuda") for _ in range(3)]
        bufs = [abi.Buffer2D(t.data_ptr(), nz * ny, nx, nx * 4) for t in volumes]
        dp, kfs = dev.depth_params(), dev.keyframe_views()
        badslam_amd.check(L.bslam_fuse_keyframes(ctx.handle, stream, C.byref(cam), C.byref(cam), C.byref(dp), K, kfs, C.byref(vol), truncation,
                                                 C.byref(bufs[0]), C.byref(bufs[1]), C.byref(bufs[2])))
        M = np.array(list(kfs[0].frame_T_global.m), np.float64).reshape(3, 4)
        pose = np.concatenate([M[:, :3].T, (-M[:, :3].T @ M[:, 3])[:, None]], 1).astype(np.float32)
        G = abi.Mat3x4((C.c_float * 12)(*pose.reshape(12)))
        need = C.c_size_t()
        badslam_amd.check(L.bslam_volume_views_aux_bytes(C.byref(vol), C.byref(need)))
        aux = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
        depth = torch.zeros((H, W), dtype=torch.int16, device="cuda")
        color = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        normal = torch.zeros((H, 3 * W), dtype=torch.float32, device="cuda")
        views = [abi.Buffer2D(depth.data_ptr(), H, W, 2 * W), abi.Buffer2D(color.data_ptr(), H, W, 4 * W), abi.Buffer2D(normal.data_ptr(), H, W, 12 * W)]

        def prepare():
            badslam_amd.check(L.bslam_prepare_volume_views(ctx.handle, stream, C.byref(vol), C.byref(bufs[0]), C.byref(bufs[1]), args.min_count,
                                                           C.c_void_p(aux.data_ptr()), need.value))

        def march():
            badslam_amd.check(L.bslam_raycast_volume(ctx.handle, stream, C.byref(vol), C.byref(bufs[0]), C.byref(bufs[2]), C.c_void_p(aux.data_ptr()), C.byref(G), C.byref(cam),
                                                     args.min_depth, args.max_depth, args.voxel_size, 1.0 / dp.raw_to_float_depth, C.byref(views[0]), C.byref(views[1]),
                                                     C.byref(views[2])))

        prepare()
        march()                                                          # warm-up
        torch.cuda.synchronize()
        prepare_us = float(np.median([timed(prepare) for _ in range(args.reps)]))
        times = {1: [], 0: []}
        stats = {}
        for rep in range(args.reps):
            for on in (1, 0):
                badslam_amd.check(L.bslam_set_culling(ctx.handle, on))
                if rep == 0:                                             # the counters cost two atomics per wave: kept out of the timed calls
                    tested, culled = C.c_uint64(), C.c_uint64()
                    badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
                    badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))
                    march()
                    badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))
                    badslam_amd.check(L.bslam_profile_enable(ctx.handle, 0))
                    stats[on] = (tested.value, culled.value)
                times[on].append(timed(march))
        badslam_amd.check(L.bslam_set_culling(ctx.handle, 1))
        on_us, off_us = float(np.median(times[1])), float(np.median(times[0]))
        flags = aux[:((nx - 1 + 63) // 64) * ((ny - 1 + 7) // 8) * ((nz - 1 + 7) // 8)].cpu().numpy()
        blocks = ((nx - 1 + 7) // 8) * ((ny - 1 + 7) // 8) * ((nz - 1 + 7) // 8)
        res["stacks"].append({
            "keyframes": K, "volume": [nx, ny, nz], "voxels": nx * ny * nz, "aux_bytes": need.value, "blocks": blocks,
            "blocks_flagged": int(np.unpackbits(flags).sum()), "prepare_us": prepare_us,
            "march_us": on_us, "march_block_test_off_us": off_us, "march_us_all": [times[1], times[0]],
            "samples_in_range": stats[1][0], "samples_skipped": stats[1][1], "samples_evaluated": stats[1][0] - stats[1][1],
            "samples_in_range_block_test_off": stats[0][0], "skipped_with_block_test_off": stats[0][1],
            "samples_per_s": stats[1][0] / (on_us * 1e-6), "samples_per_s_block_test_off": stats[0][0] / (off_us * 1e-6),
            "pixels_hit": int((depth != 0).sum().item()), "pixels": W * H})
        del dev, volumes, aux
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
