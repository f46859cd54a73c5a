#!/usr/bin/env python3
"""Times mesh smoothing (bslam_smooth_mesh) on the meshes of tools/bench_fusion.py -- the synthetic stacks of badslam_amd.synthetic
at 640x480, K = 50 and K = 300 keyframes, fused at 1 cm voxels with a truncation of 4 voxels and extracted -- for --iterations of the
Taubin filter.  Device events around every call, and, in calls of their own with profiling on, around the five stages (keys, the two
sorts, adjacency, steps, normals); every figure is the median of --reps calls after a warm-up.  Per mesh: the call and its stages in
microseconds, the time per step launch, the share of the call that builds the adjacency (keys, sorts and lists), and the accuracy and
completeness against the extracted mesh (surface_eval.evaluate at samples drawn by area, --sample-spacing apart: the figures of
tools/bench_decimate_mesh.py) of the mesh decimated to --ratio of its vertices, and of the mesh smoothed and then decimated.  There
is nothing to compare with: neither an earlier version nor the reference smooths a mesh.  Not part of bench.py.  Prints one JSON
line.
usage: tools/bench_smooth_mesh.py [--reps N] [--keyframes 50 300] [--iterations N] [--lambda L] [--mu M] [--boundary fixed|rim|free] [--ratio R]"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 640, 480
STAGES = ("keys_us", "sorts_us", "adjacency_us", "steps_us", "normals_us")
MODES = {"fixed": 0, "rim": 1, "free": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--keyframes", type=int, nargs="*", default=[50, 300])
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--lambda", dest="lambda_", type=float, default=0.5)
    ap.add_argument("--mu", type=float, default=-0.53)
    ap.add_argument("--boundary", choices=tuple(MODES), default="fixed")
    ap.add_argument("--ratio", type=float, default=0.25)
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--sample-spacing", type=float, default=0.01)
    args = ap.parse_args()
    from badslam_amd import build
    build.build()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_smooth_mesh.py needs a GPU: there is no CPU path to time")
    import badslam_amd
    from badslam_amd import abi, surface_eval, synthetic
    from badslam_amd.direct_ba import DirectBA
    from tools import run_tum
    L = badslam_amd.lib()
    ctx = badslam_amd.Context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    truncation = 4 * args.voxel_size
    ptr = lambda t: C.c_void_p(t.data_ptr())
    launches = args.iterations * (2 if args.mu != 0.0 else 1)

    def timed(call):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e3

    def decimated(positions, normals, colors, indices, V, T):
        """bslam_decimate_mesh of device tensors to --ratio -> host dict of positions and triangles."""
        out = [torch.zeros(max(1, n), dtype=torch.int32, device="cuda") for n in (3 * V, 3 * V, V, 3 * T, V)]
        counts = (C.c_uint32(), C.c_uint32(), C.c_uint32())
        badslam_amd.check(L.bslam_decimate_mesh(ctx.handle, stream, V, T, ptr(positions), ptr(normals), ptr(colors), ptr(indices), math.ceil(args.ratio * V), 1.0,
                                                float("inf"), 0, *[ptr(t) for t in out], C.byref(counts[0]), C.byref(counts[1]), C.byref(counts[2])))
        V2, T2 = counts[0].value, counts[1].value
        return dict(positions=out[0][:3 * V2].cpu().numpy().view(np.float32).reshape(V2, 3), triangles=out[3][:3 * T2].cpu().numpy().view(np.uint32).reshape(T2, 3))

    def bench(name, ba, V, T, mesh):
        """mesh: device tensors (positions, normals, colours, indices)."""
        out = [torch.zeros(max(1, 3 * V), dtype=torch.int32, device="cuda") for _ in range(2)]

        def smooth():
            badslam_amd.check(L.bslam_smooth_mesh(ctx.handle, stream, V, T, ptr(mesh[0]), ptr(mesh[1]), ptr(mesh[3]), args.iterations, args.lambda_, args.mu,
                                                  MODES[args.boundary], ptr(out[0]), ptr(out[1])))

        smooth()                                                         # warm-up; the slab grows here
        torch.cuda.synchronize()
        call_us = float(np.median([timed(smooth) for _ in range(args.reps)]))
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
        stages = []
        for _ in range(args.reps):
            smooth()
            ms = (C.c_float * 5)()
            badslam_amd.check(L.bslam_smooth_stage_times(ctx.handle, ms))
            stages.append([1e3 * v for v in ms])
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 0))
        stage_us = np.median(np.array(stages), axis=0)
        row = {"mesh": name, "vertices": V, "triangles": T, "step_launches": launches, "call_us": call_us}
        row.update({k: float(v) for k, v in zip(STAGES, stage_us)})
        row["us_per_step_launch"] = float(stage_us[3]) / max(1, launches)
        row["adjacency_share_of_stages"] = float(stage_us[:3].sum() / max(stage_us.sum(), 1e-9))
        moved = (out[0][:3 * V].view(torch.float32) - mesh[0][:3 * V].view(torch.float32)).view(V, 3).norm(dim=1)
        row["displacement_mean_m"], row["displacement_max_m"] = float(moved.mean()), float(moved.max())
        # either mesh as the reconstruction, the extracted one as the ground truth, both sampled by area
        before = dict(positions=mesh[0][:3 * V].cpu().numpy().view(np.float32).reshape(V, 3), triangles=mesh[3][:3 * T].cpu().numpy().view(np.uint32).reshape(T, 3))
        for key, positions, normals in (("decimated", mesh[0], mesh[1]), ("smoothed_decimated", out[0], out[1])):
            after = decimated(positions, normals, mesh[2], mesh[3], V, T)
            e = surface_eval.evaluate(ba, after, before, max_distance=0.1, thresholds=(0.5 * args.voxel_size, args.voxel_size), sample_density=1.0 / args.sample_spacing ** 2)
            row[key] = dict(vertices=len(after["positions"]), triangles=len(after["triangles"]), accuracy_mean_m=e["accuracy"]["mean"], accuracy_p99_m=e["accuracy"]["p99"],
                            completeness_mean_m=e["completeness"]["mean"], completeness_p99_m=e["completeness"]["p99"], f_score_at_half_voxel=e["f_scores"][0]["f_score"],
                            f_score_at_voxel=e["f_scores"][1]["f_score"])
        return row

    res = {"size": [W, H], "reps": args.reps, "voxel_size_m": args.voxel_size, "truncation_m": truncation, "min_count": args.min_count, "iterations": args.iterations,
           "lambda": args.lambda_, "mu": args.mu, "boundary": args.boundary, "ratio": args.ratio, "sample_spacing_m": args.sample_spacing, "cases": []}
    for K in args.keyframes:
        dev = synthetic.TorchStack(K, "cuda:0", width=W, height=H, kind="dense")
        cam = dev.stack.camera
        ba = DirectBA(1024, 1.0 / 5000, 40.0, 4, 0.8, 1, 1, 1, cam, cam, 0, True, False)   # for evaluate: SampleMesh and PointMeshDistance
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
        extract(V, T, tuple(ptr(t) for t in mesh))
        torch.cuda.synchronize()
        res["cases"].append(bench(f"K = {K}", ba, V, T, mesh))
        ba.close()
        del dev, volumes, mesh
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
