#!/usr/bin/env python3
"""Times volumetric fusion and mesh extraction (bslam_fuse_keyframes, bslam_extract_mesh) on the synthetic stacks of
badslam_amd.synthetic at 640x480 -- K = 50 and K = 300 keyframes -- over the box of the surfel model padded by the truncation,
at 1 cm voxels and a truncation of 4 voxels.  Device events around every call; every figure is the median of --reps calls after a
warm-up, with culling on and off alternating inside the same run (on, off, on, off, ...), so that both see the same clocks.
Beside the times: the (voxel, keyframe) pairs a call stands for, the (brick, keyframe) pairs tested and culled
(bslam_debug_cull_stats), pairs per second, and the size of the mesh.  Not part of bench.py.  Prints one JSON line.
usage: tools/bench_fusion.py [--reps N] [--keyframes 50 300] [--voxel-size M] [--kind dense]"""
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
    ap.add_argument("--kind", default="dense")
    args = ap.parse_args()
    from badslam_amd import build
    build.build()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_fusion.py needs a GPU: there is no CPU path to time")
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

    res = {"size": [W, H], "reps": args.reps, "voxel_size_m": args.voxel_size, "truncation_m": truncation, "min_count": args.min_count, "kind": args.kind,
           "brick": [8, 8, 4], "stacks": []}
    for K in args.keyframes:
        dev = synthetic.TorchStack(K, "cuda:0", width=W, height=H, kind=args.kind)
        cam = dev.stack.camera
        xyz = dev.surfels[:3, :dev.surfels_size]
        valid = ~torch.isnan(xyz[0])
        lo, hi = xyz[:, valid].min(dim=1).values.cpu().numpy(), xyz[:, valid].max(dim=1).values.cpu().numpy()
        origin, (nx, ny, nz) = run_tum.mesh_volume(lo, hi, args.voxel_size, truncation)     # refuses more than 2^30 samples, naming the voxel size
        vol = abi.Volume((C.c_float * 3)(*origin), args.voxel_size, nx, ny, nz)
        volumes = [torch.zeros((nz * ny, nx), dtype=torch.int32, device="cuda") for _ in range(3)]
        bufs = [abi.Buffer2D(t.data_ptr(), nz * ny, nx, nx * 4) for t in volumes]
        dp, kfs = dev.depth_params(), dev.keyframe_views()
        badslam_amd.check(L.bslam_set_keyframe_cache(ctx.handle, 1))    # the images do not change between the calls

        def fuse():
            badslam_amd.check(L.bslam_fuse_keyframes(ctx.handle, stream, C.byref(cam), C.byref(cam), C.byref(dp), K, kfs, C.byref(vol), truncation,
                                                     C.byref(bufs[0]), C.byref(bufs[1]), C.byref(bufs[2])))

        counts = (C.c_uint32(), C.c_uint32())

        def extract(vcap=0, tcap=0, out=(None, None, None, None)):
            badslam_amd.check(L.bslam_extract_mesh(ctx.handle, stream, C.byref(vol), C.byref(bufs[0]), C.byref(bufs[1]), C.byref(bufs[2]), args.min_count, vcap, tcap,
                                                   *out, C.byref(counts[0]), C.byref(counts[1])))

        fuse()                                                           # warm-up: records, quads, first launch
        torch.cuda.synchronize()
        times = {1: [], 0: []}
        stats = {}
        for rep in range(args.reps):
            for on in (1, 0):
                badslam_amd.check(L.bslam_set_culling(ctx.handle, on))
                if rep == 0:                                             # the counters cost two atomics per brick: kept out of the timed calls
                    tested, culled = C.c_uint64(), C.c_uint64()
                    badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
                    badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))
                    fuse()
                    badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))
                    badslam_amd.check(L.bslam_profile_enable(ctx.handle, 0))
                    stats[on] = (tested.value, culled.value)
                times[on].append(timed(fuse))
        badslam_amd.check(L.bslam_set_culling(ctx.handle, 1))
        extract()
        V, T = counts[0].value, counts[1].value
        mesh = [torch.zeros(max(1, n), dtype=torch.int32, device="cuda") for n in (3 * V, 3 * V, V, 3 * T)]
        out = tuple(C.c_void_p(t.data_ptr()) for t in mesh)
        extract(V, T, out)
        torch.cuda.synchronize()
        count_only = float(np.median([timed(extract) for _ in range(args.reps)]))
        full = float(np.median([timed(lambda: extract(V, T, out)) for _ in range(args.reps)]))
        pairs = nx * ny * nz * K
        on_us, off_us = float(np.median(times[1])), float(np.median(times[0]))
        res["stacks"].append({
            "keyframes": K, "surfels": dev.surfels_size, "volume": [nx, ny, nz], "voxels": nx * ny * nz, "voxel_keyframe_pairs": pairs,
            "fuse_us": on_us, "fuse_culling_off_us": off_us, "fuse_us_all": [times[1], times[0]],
            "pairs_per_s": pairs / (on_us * 1e-6), "pairs_per_s_culling_off": pairs / (off_us * 1e-6),
            "brick_keyframe_pairs_tested": stats[1][0], "brick_keyframe_pairs_culled": stats[1][1], "culled_with_culling_off": stats[0][1],
            "extract_counts_us": count_only, "extract_us": full, "vertices": V, "triangles": T,
            "observed_share": float((volumes[1] > 0).float().mean().item())})
        badslam_amd.check(L.bslam_set_keyframe_cache(ctx.handle, 0))
        del dev, volumes, mesh
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
