#!/usr/bin/env python3
"""Times the sensor-rectification kernels on 640x480 raw frames (a distorted colour camera and a distorted depth camera 25 mm
beside it, rectified into DecideUndistortedCamera of the colour camera) with device events around --launches back-to-back
launches, and a whole BadSlam::PreprocessFrame (upload + rectification + preprocessing kernels, host clock around a call that
ends in a stream synchronise) with the rectification on against the same call with it off, on the same instance, and
against a plain instance of the raw frames' size.  Every
figure is the median of --reps runs after a warm-up.  The NumPy restatements of the test suite are timed once, for scale.
Prints one JSON line.
usage: tools/bench_rectify.py [--reps N] [--launches M]"""
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
        sys.exit("bench_rectify.py needs a GPU: there is no CPU path to time")
    import badslam_amd
    from badslam_amd import abi, bad_slam
    from badslam_amd import rectification as rect
    from tests import rectify_util as ru
    from tests.test_gpu_preprocess import raw_depth_image
    color = rect.radtan_camera(W, H, 525.0, 525.0, 318.6, 241.3, -0.12, 0.03, 0.0, 4e-4, -3e-4)
    depth_cam = rect.radtan_camera(W, H, 570.0, 571.0, 321.4, 238.9, -0.08, 0.015, 0.0, -3e-4, 5e-4)
    color_T_depth = np.eye(4, dtype=np.float32)[:3].copy()
    color_T_depth[0, 3] = 0.025
    target = rect.decide_undistorted_camera(color, True)
    tw, th = target.width, target.height
    _, raw = raw_depth_image()
    rgb = np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)
    unprojection = rect.make_unprojection_map(depth_cam)
    L = badslam_amd.lib()
    ctx = badslam_amd.Context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def image(host=None, shape=None, dtype=None, elems=1):
        t = torch.zeros(shape, dtype=dtype, device="cuda") if host is None else torch.from_numpy(np.ascontiguousarray(host)).cuda()
        return t, abi.Buffer2D(t.data_ptr(), t.shape[0], t.shape[1] // elems, t.shape[1] * t.element_size())

    raw_d = image(raw.view(np.int16))
    rgb_d = image(rgb.reshape(H, W * 3), elems=3)
    unprojection_d = image(unprojection.reshape(H, W * 2), elems=2)
    map_d = image(shape=(th, tw * 2), dtype=torch.float32, elems=2)
    out_depth = image(shape=(th, tw), dtype=torch.int16)
    out_rgb = image(shape=(th, tw * 3), dtype=torch.uint8, elems=3)
    T = abi.Mat3x4()
    T.m[:] = [float(v) for v in color_T_depth.reshape(12)]

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

    res = {"raw_size": [W, H], "target_size": [tw, th], "reps": args.reps, "launches_per_rep": args.launches}
    res["build_undistortion_map_us"] = kernel_us(lambda: badslam_amd.check(L.bslam_build_undistortion_map(
        ctx.handle, stream, C.byref(color), C.byref(target), C.byref(map_d[1]))))
    res["undistort_rgb_us"] = kernel_us(lambda: badslam_amd.check(L.bslam_undistort_rgb(
        ctx.handle, stream, C.byref(rgb_d[1]), C.byref(map_d[1]), C.byref(out_rgb[1]))))
    res["reproject_depth_us"] = kernel_us(lambda: badslam_amd.check(L.bslam_reproject_depth(
        ctx.handle, stream, C.byref(raw_d[1]), 1.0 / 5000, C.byref(unprojection_d[1]), C.byref(T), C.byref(target), 0.05, 5000.0,
        C.byref(out_depth[1]))))
    res["reprojected_pixels_filled"] = float((out_depth[0] != 0).float().mean().item())

    slam = bad_slam.BadSlam(target, target, max_surfel_count=100000)
    ideal_depth = np.ascontiguousarray(out_depth[0].cpu().numpy().view(np.uint16))
    ideal_rgb = np.ascontiguousarray(out_rgb[0].cpu().numpy().reshape(th, tw, 3))

    def preprocess_ms(depth, colour):
        slam.PreprocessFrame(depth, colour)
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            slam.PreprocessFrame(depth, colour)
            times.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(times))

    res["preprocess_frame_off_ms"] = preprocess_ms(ideal_depth, ideal_rgb)
    slam.set_sensor_rectification(color, depth_cam, color_T_depth, raw_depth_to_metres=1.0 / 5000)
    res["preprocess_frame_on_ms"] = preprocess_ms(raw, rgb)
    slam.set_sensor_rectification(None)
    res["preprocess_frame_off_again_ms"] = preprocess_ms(ideal_depth, ideal_rgb)
    slam.close()

    # the same call on a plain instance of the raw frames' own size: the target's rows (669 pixels here) are not a multiple of
    # 16 bytes on the host, which the 2-D upload of the off path pays for and the on path, uploading 640-pixel rows, does not
    cam = abi.Camera4f(525.0, 525.0, 320.0, 240.0, W, H)
    slam = bad_slam.BadSlam(cam, cam, max_surfel_count=100000)
    res["preprocess_frame_plain_raw_size_ms"] = preprocess_ms(raw, rgb)
    slam.close()

    def once_ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    mapping = map_d[0].cpu().numpy().reshape(th, tw, 2)
    res["numpy_undistort_rgb_ms"] = once_ms(lambda: ru.undistort_rgb32(rgb, mapping))
    res["numpy_undistortion_map_ms"] = once_ms(lambda: ru.undistortion_map32(color, target))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
