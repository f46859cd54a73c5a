#!/usr/bin/env python3
"""Times the input-conditioning kernels at 640x480 (one depth median iteration, the depth downscale and the rgb downscale
at levels 1 and 2) with device events around --launches back-to-back launches, and a whole BadSlam::PreprocessFrame
(upload + conditioning + preprocessing kernels, host clock around a call that ends in a stream synchronise) with the
switches off, with one median iteration and at pyramid level 1.  Every figure is the median of --reps runs after a
warm-up.  The NumPy restatements of the test suite are timed once, for scale.  Prints one JSON line.
usage: tools/bench_preprocess.py [--reps N] [--launches M]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 640, 480


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    from badslam_amd import build
    build.build()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_preprocess.py needs a GPU: there is no CPU path to time")
    import badslam_amd
    from badslam_amd import abi, bad_slam
    from tests import bso
    from tests import test_gpu_input_conditioning as restated
    from tests.test_gpu_preprocess import raw_depth_image
    bso.build_oracle()
    _, raw = raw_depth_image()
    rgb = np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)
    L = badslam_amd.lib()
    ctx = badslam_amd.Context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def depth_image(h, w, host=None):
        t = torch.zeros((h, w), dtype=torch.int16, device="cuda") if host is None else torch.from_numpy(host.view(np.int16)).cuda()
        return t, abi.Buffer2D(t.data_ptr(), h, w, w * 2)

    def rgb_image(h, w, host=None):
        t = torch.zeros((h, w * 3), dtype=torch.uint8, device="cuda") if host is None else torch.from_numpy(host.reshape(h, w * 3)).cuda()
        return t, abi.Buffer2D(t.data_ptr(), h, w, w * 3)

    def kernel_us(fn, src, dst):
        def launch():
            badslam_amd.check(fn(ctx.handle, stream, C.byref(src[1]), C.byref(dst[1])))
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

    res = {"size": [W, H], "reps": args.reps, "launches_per_rep": args.launches}
    raw_d, rgb_d = depth_image(H, W, raw), rgb_image(H, W, rgb)
    res["median_iteration_us"] = kernel_us(L.bslam_median_filter_and_densify_depth, raw_d, depth_image(H, W))
    for level in (1, 2):
        res[f"depth_downscale_l{level}_us"] = kernel_us(L.bslam_downscale_depth_median, raw_d, depth_image(H >> level, W >> level))
        res[f"rgb_downscale_l{level}_us"] = kernel_us(L.bslam_downscale_rgb, rgb_d, rgb_image(H >> level, W >> level))

    def preprocess_ms(level, median_iterations):
        cam = bso.make_camera(525.0 / (1 << level), 525.0 / (1 << level), 320.0 / (1 << level), 240.0 / (1 << level), W >> level, H >> level)
        slam = bad_slam.BadSlam(cam, cam, max_surfel_count=100000, pyramid_level_for_depth=level, pyramid_level_for_color=level,
                                median_filter_and_densify_iterations=median_iterations)
        slam.PreprocessFrame(raw, rgb)
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            slam.PreprocessFrame(raw, rgb)
            times.append((time.perf_counter() - t0) * 1e3)
        slam.close()
        return float(np.median(times))

    res["preprocess_frame_plain_ms"] = preprocess_ms(0, 0)
    res["preprocess_frame_median1_ms"] = preprocess_ms(0, 1)
    res["preprocess_frame_level1_ms"] = preprocess_ms(1, 0)

    def once_ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    res["numpy_median_iteration_ms"] = once_ms(lambda: restated.np_median_filter_and_densify(raw))
    res["numpy_depth_downscale_l1_ms"] = once_ms(lambda: restated.np_downscale_depth_median(raw, 1))
    res["numpy_rgb_downscale_l1_ms"] = once_ms(lambda: restated.np_downscale_rgb(rgb, 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
