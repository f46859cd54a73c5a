#!/usr/bin/env python3
"""Times bslam_nearest_triangle on the stacks of tools/bench_point_mesh_distance.py (badslam_amd.synthetic at 640x480, K = 50 and
K = 300 keyframes, fused at 1 cm samples, min_count 2): the mesh's own vertices and the centres of the valid surfels against the
extracted mesh, at max_distance 0.02, 0.1 and none.  Device events around single calls; every figure is the median of --reps calls
after a warm-up.  A call builds the tree and queries it; the build is timed as a call with one point (census, keys, sort, radix tree,
boxes, packed nodes; one point's query) and the query is the difference to the whole call.  Beside the times: leaves and height, the
nodes the query fetched and the triangles it evaluated per point (bslam_debug_cull_stats, from a call of their own), and -- at each
finite radius, in the same run -- the grid call bslam_point_mesh_distance with cell_size = max_distance, timed the same way, and
whether the two agree bit for bit.  Not part of bench.py.  Prints one JSON line.
usage: tools/bench_mesh_bvh.py [--reps N] [--keyframes 50 300] [--voxel-size M]"""
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
        sys.exit("bench_mesh_bvh.py needs a GPU: there is no CPU path to time")
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

    def medians(call, N):
        """(call_us, build_us, query_us) of call(n): whole calls, calls with one point, the difference."""
        whole = [timed(lambda: badslam_amd.check(call(N))) for _ in range(args.reps)]
        build_only = [timed(lambda: badslam_amd.check(call(1))) for _ in range(args.reps)]
        call_us, build_us = float(np.median(whole)), float(np.median(build_only))
        return call_us, build_us, max(call_us - build_us, 1e-3)

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
            grid_d, grid_t = torch.zeros_like(out_d), torch.zeros_like(out_t)
            for R in (0.02, 0.1, float("inf")):
                leaves, height = C.c_uint32(), C.c_uint32()
                call = lambda n: L.bslam_nearest_triangle(ctx.handle, stream, n, C.c_void_p(points.data_ptr()), V, C.c_void_p(positions.data_ptr()), T,
                                                          C.c_void_p(indices.data_ptr()), R, C.c_void_p(out_d.data_ptr()), C.c_void_p(out_t.data_ptr()),
                                                          C.byref(leaves), C.byref(height))
                case = {"points": name, "count": N, "max_distance": None if R == float("inf") else R}
                badslam_amd.check(call(N))                                    # also the warm-up: the slab grows here
                tested, culled = C.c_uint64(), C.c_uint64()
                badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
                badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))
                badslam_amd.check(call(N))
                badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))
                badslam_amd.check(L.bslam_profile_enable(ctx.handle, 0))
                nodes, evaluated = tested.value, (tested.value - culled.value) % (1 << 64)
                call_us, build_us, query_us = medians(call, N)
                badslam_amd.check(call(N))
                hits = int(torch.isfinite(out_d[:N]).sum().item())
                case.update(leaves=leaves.value, height=height.value, call_us=call_us, build_us=build_us, query_us=query_us, query_ns_per_point=1e3 * query_us / max(N, 1),
                            nodes_per_point=nodes / max(N, 1), triangles_per_point=evaluated / max(N, 1), hits=hits)
                if R != float("inf"):
                    cells, entries = C.c_uint64(), C.c_uint64()
                    grid = lambda n: L.bslam_point_mesh_distance(ctx.handle, stream, n, C.c_void_p(points.data_ptr()), V, C.c_void_p(positions.data_ptr()), T,
                                                                 C.c_void_p(indices.data_ptr()), R, R, args.max_grid_entries, C.c_void_p(grid_d.data_ptr()),
                                                                 C.c_void_p(grid_t.data_ptr()), C.byref(cells), C.byref(entries))
                    if grid(N) != 0:
                        case["grid"] = dict(refused=L.bslam_last_error().decode(), grid_cells=cells.value, grid_entries=entries.value)
                    else:
                        g_call, g_build, g_query = medians(grid, N)
                        badslam_amd.check(grid(N))
                        same = bool(torch.equal(grid_d[:N].view(torch.int32), out_d[:N].view(torch.int32)) and torch.equal(grid_t[:N], out_t[:N]))
                        case["grid"] = dict(cell_size=R, grid_cells=cells.value, grid_entries=entries.value, call_us=g_call, build_us=g_build, query_us=g_query,
                                            query_ns_per_point=1e3 * g_query / max(N, 1), same_bits=same)
                stack["cases"].append(case)
        res["stacks"].append(stack)
        del dev, positions, indices, centres
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
