#!/usr/bin/env python3
"""Times surface sampling (bslam_sample_mesh) on the meshes of tools/bench_fusion.py -- the synthetic stacks of
badslam_amd.synthetic at 640x480, K = 50 and K = 300 keyframes, fused at 1 cm voxels with a truncation of 4 voxels and extracted --
at sample spacings of 5 mm and 2 mm, and on a wall of two triangles, 4 m a side, at 2 mm: a dense mesh, where every wave's samples
span a handful of triangles, and a coarse one, where whole waves share a triangle.  Device events around every call; every figure
is the median of --reps calls after a warm-up.  Per case: the count-only call (count pass and read-back) and the full call (count
pass, scan, emit) in microseconds and samples per second.  There is nothing to compare with: neither an earlier version nor the
reference samples a surface.  Not part of bench.py.  Prints one JSON line.
usage: tools/bench_sample_mesh.py [--reps N] [--keyframes 50 300] [--spacings 0.005 0.002] [--voxel-size M]"""
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
    ap.add_argument("--keyframes", type=int, nargs="*", default=[50, 300])
    ap.add_argument("--spacings", type=float, nargs="+", default=[0.005, 0.002])
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--wall-size", type=float, default=4.0)
    ap.add_argument("--wall-spacing", type=float, default=0.002)
    args = ap.parse_args()
    from badslam_amd import build
    build.build()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_sample_mesh.py needs a GPU: there is no CPU path to time")
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

    def bench(name, V, positions, T, indices, spacing):
        """positions, indices: device tensors."""
        density, count = 1.0 / (spacing * spacing), C.c_uint64()
        ptr = lambda t: C.c_void_p(t.data_ptr())

        def sample(capacity=0, out=(None, None, None)):
            badslam_amd.check(L.bslam_sample_mesh(ctx.handle, stream, V, ptr(positions), T, ptr(indices), density, 0, capacity, *out, C.byref(count)))

        sample()                                                         # warm-up of the count pass; the slab grows here
        N = count.value
        buffers = [torch.zeros(max(1, n), dtype=torch.int32, device="cuda") for n in (3 * N, 3 * N, N)]
        out = tuple(ptr(t) for t in buffers)
        sample(N, out)                                                   # warm-up of the scan and the emit pass
        torch.cuda.synchronize()
        count_us = float(np.median([timed(sample) for _ in range(args.reps)]))
        full_us = float(np.median([timed(lambda: sample(N, out)) for _ in range(args.reps)]))
        return {"mesh": name, "vertices": V, "triangles": T, "spacing_m": spacing, "density_per_m2": density, "samples": N, "samples_per_triangle": N / max(T, 1),
                "count_us": count_us, "full_us": full_us, "count_samples_per_s": N / (count_us * 1e-6), "full_samples_per_s": N / (full_us * 1e-6)}

    res = {"size": [W, H], "reps": args.reps, "voxel_size_m": args.voxel_size, "truncation_m": truncation, "min_count": args.min_count, "cases": []}
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

        def extract(vcap=0, tcap=0, out=(None, None, None, None)):
            badslam_amd.check(L.bslam_extract_mesh(ctx.handle, stream, C.byref(vol), C.byref(bufs[0]), C.byref(bufs[1]), C.byref(bufs[2]), args.min_count, vcap, tcap,
                                                   *out, C.byref(counts[0]), C.byref(counts[1])))

        extract()
        V, T = counts[0].value, counts[1].value
        mesh = [torch.zeros(max(1, n), dtype=torch.int32, device="cuda") for n in (3 * V, 3 * V, V, 3 * T)]
        extract(V, T, tuple(C.c_void_p(t.data_ptr()) for t in mesh))
        torch.cuda.synchronize()
        for spacing in args.spacings:
            res["cases"].append(bench(f"K = {K}", V, mesh[0], T, mesh[3], spacing))
        del dev, volumes, mesh
        torch.cuda.empty_cache()
    s = args.wall_size
    wall_positions = torch.tensor([[0, 0, 0], [s, 0, 0], [s, s, 0], [0, s, 0]], dtype=torch.float32, device="cuda")
    wall_indices = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device="cuda")
    res["cases"].append(bench(f"wall {s:g} m", 4, wall_positions, 2, wall_indices, args.wall_spacing))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
