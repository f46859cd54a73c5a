#!/usr/bin/env python3
"""Times loop closure: batched vs sequential verification tracking, a full CloseLoop at 640x480 and the host pose-graph
solve at K = 300 and K = 1000.  Prints one JSON line (milliseconds, median of --reps runs).
usage: tools/bench_loop_closure.py [--reps N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps):
    fn()   # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def pose_graph_case(k, loops, reps):
    from badslam_amd import direct_ba as dba
    from tests.test_pose_graph_cpu import noisy_graph, to_p7
    _, init, edges, meas = noisy_graph(np.random.default_rng(k), n=k, loops=loops, t_noise=0.002, r_noise=0.001)
    poses, meas = np.array([to_p7(T) for T in init]), np.array([to_p7(m) for m in meas])
    out = {"ms": median_ms(lambda: dba.optimize_pose_graph(poses, edges, meas, 0, 20), reps)}
    out["factor_blocks"] = dba.optimize_pose_graph(poses, edges, meas, 0, 1)[2]["factor_blocks"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from badslam_amd import build
    build.build()
    res = {}
    res["pose_graph_k300"] = pose_graph_case(300, [(299, 0), (200, 50), (150, 20)], args.reps)
    res["pose_graph_k1000"] = pose_graph_case(1000, [(999, 0), (700, 100), (500, 250)], args.reps)
    import torch
    if torch.cuda.is_available():
        from tests import bso
        from tests.test_gpu_loop_closure import circle_path, drifted
        from tests import test_gpu_loop_closure as tl
        from tests import scenes
        from badslam_amd import direct_ba as dba
        W, H = 640, 480
        cam = bso.make_camera(525.0, 525.0, 320.0, 240.0, W, H)
        gt = circle_path(12)
        rng = np.random.default_rng(5)
        planes = scenes.random_planes(rng, 20)
        frames = []
        for T in gt:
            M = np.array(list(bso.se3_matrix3x4(T).m), np.float64).reshape(3, 4)
            tt, pidx, dg, o = scenes.render_planes(cam, W, H, M[:, :3], M[:, 3], planes)
            valid = np.isfinite(tt) & (tt < 6.0)
            depth = np.where(valid, tt / tl.RAW_TO_FLOAT + 0.5, 0).astype(np.uint32)
            depth = np.where(depth >= 32768, 0, depth).astype(np.uint16)
            pts = o[None, None, :] + dg * np.where(valid, tt, 0.0)[..., None]
            lum = scenes.texture_at(pts, pidx, 0.37)
            frames.append((depth, np.ascontiguousarray(np.repeat(lum[:, :, None], 3, axis=2))))

        def new_ba(poses):
            ba = dba.DirectBA(400000, tl.RAW_TO_FLOAT, 40.0, 4, 0.8, 1, 1, 1, cam, cam, 0, True, True)
            for k, ((d, rgb), T) in enumerate(zip(frames, poses)):
                ba.AddKeyframeFromImages(k, d, rgb, T)
            return ba
        ba = new_ba(gt)
        last = len(gt) - 1
        inits = [bso.se3_mul(bso.se3_inverse(gt[last]), gt[k]) for k in (0, 1, 2)]

        def sequential():
            for k, init in zip((0, 1, 2), inits):
                ba.TrackKeyframePair(k, last, init, num_scales=5)
        res["verify_sequential_ms"] = median_ms(sequential, args.reps)
        res["verify_batched_ms"] = median_ms(lambda: ba.TrackKeyframesBatched(last, [0, 1, 2], inits, num_scales=5), args.reps)
        res["verify_speedup"] = res["verify_sequential_ms"] / res["verify_batched_ms"]
        ba.close()
        init = tl.perturbed_old_T_cur(gt, last, 0)
        times = []
        for _ in range(args.reps):
            b = new_ba(drifted(gt))
            t0 = time.perf_counter()
            r = b.CloseLoop(last, 0, init, num_scales=5)
            times.append((time.perf_counter() - t0) * 1e3)
            b.close()
        res["close_loop_640x480_ms"] = float(np.median(times))
        res["close_loop_status"] = r["status"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
