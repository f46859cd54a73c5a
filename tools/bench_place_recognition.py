#!/usr/bin/env python3
"""Times the two place-recognition kernels with device events around --launches back-to-back calls; every figure is the
median of --reps runs after a warm-up.
  extraction  bslam_extract_keyframe_features on a 640x480 image of random 4 x 4 blocks (1200 cells, one block per cell)
  matching    bslam_match_features of one keyframe against K = 50 / 300 / 1000 database keyframes of random descriptors with
              1200 cells each (every slot filled: the worst case), with the comparison rate K * cells^2 / time
Prints one JSON line.
usage: tools/bench_place_recognition.py [--reps N] [--launches M] [--keyframes 50 300 1000]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 640, 480
CELLS = (W // 16) * (H // 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--keyframes", type=int, nargs="+", default=[50, 300, 1000])
    ap.add_argument("--max-distance", type=int, default=64)
    args = ap.parse_args()
    from badslam_amd import build
    build.build()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_place_recognition.py needs a GPU: there is no CPU path to time")
    import badslam_amd
    from badslam_amd import abi
    L = badslam_amd.lib()
    ctx = badslam_amd.Context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def kernel_us(launch):
        launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.launches):
                launch()
            end.record()
            end.synchronize()
            times.append(start.elapsed_time(end) * 1e3 / args.launches)
        return float(np.median(times))

    rng = np.random.default_rng(0)
    lum = np.kron(rng.integers(0, 256, (H // 4, W // 4)), np.ones((4, 4), np.int64)).astype(np.uint8)
    rgba = np.zeros((H, W, 4), np.uint8)
    rgba[:, :, 3] = lum
    color = torch.from_numpy(rgba.reshape(H, W * 4)).cuda()
    depth = torch.from_numpy(rng.integers(500, 30000, (H, W)).astype(np.int16)).cuda()
    color_buf = abi.Buffer2D(color.data_ptr(), H, W, W * 4)
    depth_buf = abi.Buffer2D(depth.data_ptr(), H, W, W * 2)
    xy = torch.zeros(CELLS, dtype=torch.int32, device="cuda")
    desc = torch.zeros((CELLS, 8), dtype=torch.int32, device="cuda")
    res = {"size": [W, H], "cells": CELLS, "reps": args.reps, "launches_per_rep": args.launches, "max_distance": args.max_distance}
    res["extraction_us"] = kernel_us(lambda: badslam_amd.check(
        L.bslam_extract_keyframe_features(ctx.handle, stream, C.byref(color_buf), C.byref(depth_buf), 10 ** 11, ptr(xy), ptr(desc))))
    res["features"] = int((xy != -1).sum().item())
    res["extraction_launch_shape"] = [CELLS, 256]

    res["matching"] = []
    for K in args.keyframes:
        database = torch.randint(-2 ** 31, 2 ** 31 - 1, (K, 9 * CELLS), dtype=torch.int32, device="cuda")
        database[:, :CELLS] &= 0x7FFFFFFF      # the xy words: no slot is empty
        match = torch.zeros((K, CELLS), dtype=torch.int32, device="cuda")
        count = torch.zeros(K, dtype=torch.int32, device="cuda")
        q_desc = torch.randint(-2 ** 31, 2 ** 31 - 1, (CELLS, 8), dtype=torch.int32, device="cuda")
        q_xy = torch.zeros(CELLS, dtype=torch.int32, device="cuda")
        us = kernel_us(lambda: badslam_amd.check(
            L.bslam_match_features(ctx.handle, stream, ptr(q_xy), ptr(q_desc), CELLS, ptr(database), K, args.max_distance, ptr(match), ptr(count))))
        res["matching"].append({"keyframes": K, "us": us, "comparisons": K * CELLS * CELLS, "comparisons_per_s": K * CELLS * CELLS / (us * 1e-6),
                                "launch_shape": [[(CELLS + 255) // 256, K], 256], "database_MB": K * 9 * CELLS * 4 / 1e6})
        del database, match, count
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
