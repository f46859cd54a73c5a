#!/usr/bin/env python3
"""Times bslam_point_mesh_distance on the stacks of tools/bench_fusion.py (badslam_amd.synthetic at 640x480, K = 50 and K = 300
keyframes, fused at 1 cm samples, min_count 2): the mesh's own vertices and the centres of the valid surfels against the extracted
mesh, at max_distance 0.02 and 0.1 and cell_size R / 2, R and 2 R.  Device events around single calls; every figure is the median
of --reps calls after a warm-up.  A call builds the grid and queries it; the build is timed as a call with one point (triangle
passes, records, cell lists; one point's sort and query) and the query is the difference to the whole call.  Beside the times:
cells, (triangle, cell) entries, the pairs the grid offered and those that passed the box test (bslam_debug_cull_stats, from a
call of their own), and pairs per second of the query.  A case the budget refuses is reported as refused.  Not part of bench.py.
Prints one JSON line.
usage: tools/bench_point_mesh_distance.py [--reps N] [--keyframes 50 300] [--voxel-size M]"""
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
    ap.add_argument("--max-grid-entries", type=int, default=1 << 28)
    args = ap.parse_args()
    from badslam_amd import build
    build.build()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_point_mesh_distance.py needs a GPU: there is no CPU path to time")
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

    res = {"size": [W, H], "reps": args.reps, "voxel_size_m": args.voxel_size, "min_count": args.min_count, "stacks": []}
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
        centres = xyz[:, valid].t().contiguous()
        stack = {"keyframes": K, "vertices": V, "triangles": T, "surfel_centres": int(centres.shape[0]), "cases": []}
        for name, points in (("mesh vertices", positions), ("surfel centres", centres.reshape(-1))):
            N = points.numel() // 3
            out_d, out_t = torch.zeros(max(1, N), dtype=torch.float32, device="cuda"), torch.zeros(max(1, N), dtype=torch.int32, device="cuda")
            for R in (0.02, 0.1):
                for factor in (0.5, 1.0, 2.0):
                    cells, entries = C.c_uint64(), C.c_uint64()
                    call = lambda n: L.bslam_point_mesh_distance(ctx.handle, stream, n, C.c_void_p(points.data_ptr()), V, C.c_void_p(positions.data_ptr()), T,
                                                                 C.c_void_p(indices.data_ptr()), R, R * factor, args.max_grid_entries, C.c_void_p(out_d.data_ptr()),
                                                                 C.c_void_p(out_t.data_ptr()), C.byref(cells), C.byref(entries))
                    case = {"points": name, "count": N, "max_distance": R, "cell_size": R * factor}
                    if call(N) != 0:                                      # also the warm-up: the slab grows here
                        case.update(refused=L.bslam_last_error().decode(), grid_cells=cells.value, grid_entries=entries.value)
                        stack["cases"].append(case)
                        continue
                    tested, culled = C.c_uint64(), C.c_uint64()
                    badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
                    badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))
                    badslam_amd.check(call(N))
                    badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))
                    badslam_amd.check(L.bslam_profile_enable(ctx.handle, 0))
                    whole = [timed(lambda: badslam_amd.check(call(N))) for _ in range(args.reps)]
                    build_only = [timed(lambda: badslam_amd.check(call(1))) for _ in range(args.reps)]
                    badslam_amd.check(call(N))
                    hits = int(torch.isfinite(out_d[:N]).sum().item())
                    call_us, build_us = float(np.median(whole)), float(np.median(build_only))
                    query_us = max(call_us - build_us, 1e-3)
                    case.update(grid_cells=cells.value, grid_entries=entries.value, call_us=call_us, build_us=build_us, query_us=query_us, call_us_all=whole,
                                build_us_all=build_only, pairs_offered=tested.value, pairs_evaluated=tested.value - culled.value,
                                offered_pairs_per_s=tested.value / (query_us * 1e-6), brute_force_pairs=N * T, hits=hits)
                    stack["cases"].append(case)
        res["stacks"].append(stack)
        del dev, positions, indices, centres
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
