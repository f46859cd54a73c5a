#!/usr/bin/env python3
"""Times bslam_mesh_rays and bslam_mesh_visibility on the stacks of tools/bench_mesh_bvh.py (badslam_amd.synthetic at 640x480, K = 50 and
K = 300 keyframes, fused at 1 cm samples, min_count 2), against the extracted mesh: the tree build (a call with one ray), the
640x480 pixel-centre rays of keyframe 0, closest hit and any hit, and the visibility of the valid surfels' centres from all K
keyframes.  Device events around single calls; every figure is the median of --reps calls after a warm-up, and a kernel's time is
the call's minus the build's.  Beside the times: the nodes fetched and the triangles evaluated per ray (bslam_debug_cull_stats, from
calls of their own), bslam_nearest_triangle of the surfel centres without a radius timed in the same run, and -- for information --
the share of pixels whose closest-hit triangle is the one bslam_render_mesh draws there.  Not part of bench.py.  Prints one JSON line.
usage: tools/bench_mesh_rays.py [--reps N] [--keyframes 50 300] [--voxel-size M] [--margin M]"""
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
    ap.add_argument("--margin", type=float, default=0.02)
    args = ap.parse_args()
    from badslam_amd import build
    build.build()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_rays.py needs a GPU: there is no CPU path to time")
    import badslam_amd
    from badslam_amd import abi, synthetic
    from tools import run_tum
    L = badslam_amd.lib()
    ctx = badslam_amd.Context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    truncation = 4 * args.voxel_size
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def timed(call):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        badslam_amd.check(call())
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e3

    def median_us(call):
        badslam_amd.check(call())                                            # the warm-up: slabs grow here
        return float(np.median([timed(call) for _ in range(args.reps)]))

    def counted(call):
        """(nodes fetched, triangles evaluated) of one call."""
        tested, culled = C.c_uint64(), C.c_uint64()
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
        badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))
        badslam_amd.check(call())
        badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 0))
        return tested.value, (tested.value - culled.value) % (1 << 64)

    res = {"size": [W, H], "reps": args.reps, "voxel_size_m": args.voxel_size, "min_count": args.min_count, "margin_m": args.margin, "stacks": []}
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
        extract(V, T, tuple(ptr(t) for t in (positions, normals, colors, indices)))
        del volumes, normals, colors
        centres = xyz[:, valid].t().contiguous()
        P = int(centres.shape[0])
        # the pixel-centre rays of keyframe 0: o = its centre, d = R ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1)
        R0, t0 = np.asarray(dev.stack.R[0], np.float64), np.asarray(dev.stack.t[0], np.float64)
        px, py = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
        local = np.stack([(px - cam.cx) / cam.fx, (py - cam.cy) / cam.fy, np.ones_like(px)], -1).reshape(-1, 3)
        N = W * H
        directions = torch.from_numpy(np.ascontiguousarray(local @ R0.T, np.float32)).cuda()
        origins = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(t0, (N, 3)), np.float32)).cuda()
        out_t, out_tri = torch.zeros(N, dtype=torch.float32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
        out_hit = torch.zeros(N, dtype=torch.uint8, device="cuda")
        leaves, height = C.c_uint32(), C.c_uint32()
        mesh = (V, ptr(positions), T, ptr(indices))
        closest = lambda n=N: L.bslam_mesh_rays(ctx.handle, stream, n, ptr(origins), ptr(directions), None, *mesh, 0, ptr(out_t), ptr(out_tri), None, None, None,
                                                C.byref(leaves), C.byref(height))
        any_hit = lambda n=N: L.bslam_mesh_rays(ctx.handle, stream, n, ptr(origins), ptr(directions), None, *mesh, 1, None, None, None, None, ptr(out_hit),
                                                C.byref(leaves), C.byref(height))
        views = (abi.Mat3x4 * K)(*[dev.stack.pose(k)[1] for k in range(K)])
        view_centres = np.ascontiguousarray(np.asarray(dev.stack.t[:K], np.float32).reshape(-1, 3))
        out_count, out_first = torch.zeros(max(1, P), dtype=torch.int32, device="cuda"), torch.zeros(max(1, P), dtype=torch.int32, device="cuda")
        visibility = lambda n=P: L.bslam_mesh_visibility(ctx.handle, stream, n, ptr(centres), None, *mesh, K, views, view_centres.ctypes.data, C.byref(cam), 0.05, 50.0,
                                                         args.margin, ptr(out_count), ptr(out_first), C.byref(leaves), C.byref(height))
        out_d = torch.zeros(max(1, P), dtype=torch.float32, device="cuda")
        nearest = lambda n=P: L.bslam_nearest_triangle(ctx.handle, stream, n, ptr(centres), *mesh, float("inf"), ptr(out_d), None, C.byref(leaves), C.byref(height))
        build_us = median_us(lambda: closest(1))
        stack = {"keyframes": K, "vertices": V, "triangles": T, "surfel_centres": P, "build_us": build_us, "cases": []}
        for name, call, count, pairs in (("closest hit", closest, N, N), ("any hit", any_hit, N, N), ("visibility", visibility, P, None),
                                         ("nearest triangle, no radius", nearest, P, P)):
            nodes, evaluated = counted(call)
            call_us = median_us(call)
            kernel_us = max(call_us - build_us, 1e-3)
            case = {"case": name, "count": count, "call_us": call_us, "kernel_us": kernel_us, "leaves": leaves.value, "height": height.value}
            if name == "visibility":
                seen = out_count[:P]
                case.update(views=K, seen_pairs=int(seen.sum().item()), points_seen=int((seen > 0).sum().item()), nodes=nodes, triangles=evaluated,
                            kernel_ns_per_pair=1e3 * kernel_us / max(P * K, 1))
            else:
                case.update(kernel_ns_per_ray=1e3 * kernel_us / max(pairs, 1), nodes_per_ray=nodes / max(pairs, 1), triangles_per_ray=evaluated / max(pairs, 1))
            if name == "closest hit":
                case["hits"] = int(torch.isfinite(out_t).sum().item())
            if name == "any hit":
                case["hits"] = int(out_hit.sum().item())
                case["equals_closest"] = bool(torch.equal(out_hit.bool(), torch.isfinite(out_t)))
            stack["cases"].append(case)
        # for information: the triangle bslam_render_mesh draws at each pixel of the same view
        index = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        index_buf = abi.Buffer2D(index.data_ptr(), H, W, W * 4)
        badslam_amd.check(closest())
        badslam_amd.check(L.bslam_render_mesh(ctx.handle, stream, C.byref(dev.stack.pose(0)[1]), C.byref(cam), V, ptr(positions), None, None, T, ptr(indices), 0.05, 50.0, 0,
                                              1.0 / float(dev.stack.raw_to_float_depth), None, C.byref(index_buf), None, None))
        stack["closest_equals_render_index"] = float((index.reshape(-1) == out_tri).float().mean().item())
        res["stacks"].append(stack)
        del dev, positions, indices, centres
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
