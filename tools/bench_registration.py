#!/usr/bin/env python3
"""Times surface registration on the stacks of tools/bench_fusion.py (badslam_amd.synthetic at 640x480, K = 50 and K = 300 keyframes,
fused at 1 cm samples, min_count 2): the centres of the valid surfels, moved by 2 cm and 1 degree about their centroid, are
registered to the extracted mesh at max_distance 0.1 with cell_size = max_distance.  Device events around single calls; every time
is the median of --reps calls after a warm-up:
  prepare_us   one bslam_registration_prepare (the triangle side: two count passes with their read-backs, records, lists)
  step_us      one bslam_registration_step at R = R0 from the start transform (sort and query of the moved points, rows, sums,
               one read-back)
  distance_us  one whole bslam_point_mesh_distance call on the same points and mesh, from the same process: what a step would
               cost if it rebuilt the triangle side
and steps_to_convergence, the steps the stage schedule of DirectBA::RegisterPoints takes from the identity (PLANE mode, Huber width
half the stage's radius), with the error that is left.  Not part of bench.py.  Prints one JSON line.
usage: tools/bench_registration.py [--reps N] [--keyframes 50 300] [--voxel-size M]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 640, 480
R0 = 0.1
UPPER = [(i, j) for i in range(6) for j in range(i, 6)]


def hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def se3_exp(delta):
    u, w = np.asarray(delta[:3], np.float64), np.asarray(delta[3:], np.float64)
    theta = np.linalg.norm(w)
    Wm = hat(w)
    if theta < 1e-8:
        a, b, c = 1.0, 0.5, 1.0 / 6
    else:
        a, b, c = np.sin(theta) / theta, (1 - np.cos(theta)) / theta ** 2, (theta - np.sin(theta)) / theta ** 3
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * Wm + b * Wm @ Wm
    T[:3, 3] = (np.eye(3) + b * Wm + c * Wm @ Wm) @ u
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--keyframes", type=int, nargs="+", default=[50, 300])
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--max-grid-entries", type=int, default=1 << 28)
    args = ap.parse_args()
    from badslam_amd import build
    build.build()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_registration.py needs a GPU: there is no CPU path to time")
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

    res = {"size": [W, H], "reps": args.reps, "voxel_size_m": args.voxel_size, "min_count": args.min_count, "max_distance": R0, "stacks": []}
    for K in args.keyframes:
        dev = synthetic.TorchStack(K, "cuda:0", width=W, height=H, kind="dense")
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
        counts = (C.c_uint32(), C.c_uint32())
        extract = lambda vcap, tcap, out: badslam_amd.check(L.bslam_extract_mesh(ctx.handle, stream, C.byref(vol), C.byref(bufs[0]), C.byref(bufs[1]), C.byref(bufs[2]),
                                                                                 args.min_count, vcap, tcap, *out, C.byref(counts[0]), C.byref(counts[1])))
        extract(0, 0, (None, None, None, None))
        V, T = counts[0].value, counts[1].value
        positions, normals = torch.zeros(max(1, 3 * V), dtype=torch.float32, device="cuda"), torch.zeros(max(1, 3 * V), dtype=torch.float32, device="cuda")
        colors, indices = torch.zeros(max(1, V), dtype=torch.int32, device="cuda"), torch.zeros(max(1, 3 * T), dtype=torch.int32, device="cuda")
        extract(V, T, tuple(C.c_void_p(t.data_ptr()) for t in (positions, normals, colors, indices)))
        del volumes, normals, colors
        # the source: the surfel centres in a frame of their own
        centres = xyz[:, valid].t().contiguous().cpu().numpy().astype(np.float64)
        centroid = centres.mean(axis=0)
        rng = np.random.default_rng(5)
        t, w = rng.standard_normal(3), rng.standard_normal(3)
        truth = se3_exp(np.concatenate([np.zeros(3), np.deg2rad(1.0) * w / np.linalg.norm(w)]))
        truth[:3, 3] = centroid - truth[:3, :3] @ centroid + 0.02 * t / np.linalg.norm(t)
        inverse = np.linalg.inv(truth)
        points = torch.from_numpy(np.ascontiguousarray(centres @ inverse[:3, :3].T + inverse[:3, 3], np.float32)).cuda()
        N = int(points.shape[0])
        cells, entries = C.c_uint64(), C.c_uint64()
        prepare = lambda: L.bslam_registration_prepare(ctx.handle, stream, V, C.c_void_p(positions.data_ptr()), T, C.c_void_p(indices.data_ptr()), R0, R0,
                                                       args.max_grid_entries, C.byref(cells), C.byref(entries))
        sums, step_counts = np.zeros(32, np.float32), np.zeros(4, np.uint64)

        def step(M, R, huber):
            m = np.ascontiguousarray(M, np.float32).reshape(12)
            return L.bslam_registration_step(ctx.handle, stream, N, C.c_void_p(points.data_ptr()), m.ctypes.data_as(C.POINTER(C.c_float)), R, 0, huber, None, None,
                                             sums.ctypes.data_as(C.POINTER(C.c_float)), step_counts.ctypes.data_as(C.POINTER(C.c_uint64)))

        out_d = torch.zeros(max(1, N), dtype=torch.float32, device="cuda")
        distance = lambda: L.bslam_point_mesh_distance(ctx.handle, stream, N, C.c_void_p(points.data_ptr()), V, C.c_void_p(positions.data_ptr()), T,
                                                       C.c_void_p(indices.data_ptr()), R0, R0, args.max_grid_entries, C.c_void_p(out_d.data_ptr()), None, None, None)
        stack = {"keyframes": K, "vertices": V, "triangles": T, "points": N}
        if prepare() != 0:                                                # also the warm-up: the slab grows here
            stack.update(refused=L.bslam_last_error().decode(), grid_cells=cells.value, grid_entries=entries.value)
            res["stacks"].append(stack)
            continue
        identity = np.eye(4)[:3]
        badslam_amd.check(step(identity, R0, R0 / 2))
        badslam_amd.check(distance())
        prepare_us = [timed(lambda: badslam_amd.check(prepare())) for _ in range(args.reps)]
        step_us = [timed(lambda: badslam_amd.check(step(identity, R0, R0 / 2))) for _ in range(args.reps)]
        distance_us = [timed(lambda: badslam_amd.check(distance())) for _ in range(args.reps)]
        first_hits = int(step_counts[1])
        # the schedule of DirectBA::RegisterPoints
        M, steps, R = np.eye(4), 0, R0
        while R >= R0 / 8:
            for _ in range(20):
                badslam_amd.check(step(M[:3], R, R / 2))
                steps += 1
                Hm = np.zeros((6, 6))
                for k, (i, j) in enumerate(UPPER):
                    Hm[i, j] = Hm[j, i] = sums[k]
                x = np.linalg.solve(Hm, -sums[21:27].astype(np.float64))
                M = se3_exp(x) @ M
                if np.dot(x[:3], x[:3]) + 100.0 * np.dot(x[3:], x[3:]) < 1e-10:
                    break
            R *= 0.5
        left = M @ inverse
        angle = float(np.arccos(np.clip((np.trace(left[:3, :3]) - 1) / 2, -1, 1)))
        stack.update(grid_cells=cells.value, grid_entries=entries.value, prepare_us=float(np.median(prepare_us)), step_us=float(np.median(step_us)),
                     distance_us=float(np.median(distance_us)), prepare_us_all=prepare_us, step_us_all=step_us, distance_us_all=distance_us,
                     hits_of_the_first_step=first_hits, steps_to_convergence=steps,
                     error_left_m=float(np.linalg.norm(left[:3, :3] @ centroid + left[:3, 3] - centroid)), error_left_rad=angle)
        res["stacks"].append(stack)
        del dev, positions, indices, points, out_d
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
