#!/usr/bin/env python3
"""Times mesh decimation (bslam_decimate_mesh) on the meshes of tools/bench_fusion.py -- the synthetic stacks of
badslam_amd.synthetic at 640x480, K = 50 and K = 300 keyframes, fused at 1 cm voxels with a truncation of 4 voxels and extracted --
at the given ratios of the vertex count.  Device events around every call, and, with profiling on, around the seven stages of every
round (keys, the two sorts, head flags with their scan, evaluation, selection, collapses, triangle compaction), summed over the
rounds; every figure is the median of --reps calls after a warm-up.  Per case: the output counts, the rounds and the collapses of
each, the call and its stages in microseconds, and the accuracy and completeness of the decimated mesh against the undecimated one
(surface_eval.evaluate at samples drawn by area, --sample-spacing apart), the figures of tools/bench_simplify_mesh.py.  There is
nothing to compare with: neither an earlier version nor the reference decimates a mesh.  Not part of bench.py.  Prints one JSON line.
usage: tools/bench_decimate_mesh.py [--reps N] [--keyframes 50 300] [--ratios 0.25 0.06] [--voxel-size M] [--sample-spacing M]"""
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
STAGES = ("keys_us", "sorts_us", "heads_scan_us", "evaluation_us", "selection_us", "collapses_us", "triangles_us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--keyframes", type=int, nargs="*", default=[50, 300])
    ap.add_argument("--ratios", type=float, nargs="+", default=[0.25, 0.06])
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--sample-spacing", type=float, default=0.01)
    ap.add_argument("--boundary-weight", type=float, default=1.0)
    args = ap.parse_args()
    from badslam_amd import build
    build.build()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_decimate_mesh.py needs a GPU: there is no CPU path to time")
    import badslam_amd
    from badslam_amd import abi, surface_eval, synthetic
    from badslam_amd.direct_ba import DirectBA
    from tools import run_tum
    L = badslam_amd.lib()
    ctx = badslam_amd.Context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    truncation = 4 * args.voxel_size
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def timed(call):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e3

    def bench(name, ba, V, T, mesh, ratio):
        """mesh: device tensors (positions, normals, colours, indices)."""
        target = math.ceil(ratio * V)
        out = [torch.zeros(max(1, n), dtype=torch.int32, device="cuda") for n in (3 * V, 3 * V, V, 3 * T, V)]
        counts = (C.c_uint32(), C.c_uint32(), C.c_uint32())

        def decimate():
            badslam_amd.check(L.bslam_decimate_mesh(ctx.handle, stream, V, T, ptr(mesh[0]), ptr(mesh[1]), ptr(mesh[2]), ptr(mesh[3]), target, args.boundary_weight,
                                                    float("inf"), 0, *[ptr(t) for t in out], C.byref(counts[0]), C.byref(counts[1]), C.byref(counts[2])))

        decimate()                                                       # warm-up; the slab grows here
        torch.cuda.synchronize()
        call_us = float(np.median([timed(decimate) for _ in range(args.reps)]))
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
        stages = []
        for _ in range(args.reps):
            decimate()
            ms = (C.c_float * 7)()
            badslam_amd.check(L.bslam_decimate_stage_times(ctx.handle, ms))
            stages.append([1e3 * v for v in ms])
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 0))
        stage_us = np.median(np.array(stages), axis=0)
        V2, T2, rounds = counts[0].value, counts[1].value, counts[2].value
        collapses = (C.c_uint32 * max(1, rounds))()
        n = C.c_uint32()
        badslam_amd.check(L.bslam_decimate_round_collapses(ctx.handle, collapses, rounds, C.byref(n)))
        host = lambda t, n, dtype, shape: t[:n].cpu().numpy().view(dtype).reshape(shape)
        before = dict(positions=host(mesh[0], 3 * V, np.float32, (V, 3)), triangles=host(mesh[3], 3 * T, np.uint32, (T, 3)))
        after = dict(positions=host(out[0], 3 * V2, np.float32, (V2, 3)), triangles=host(out[3], 3 * T2, np.uint32, (T2, 3)))
        row = {"mesh": name, "vertices": V, "triangles": T, "ratio": ratio, "target_vertices": target, "out_vertices": V2, "out_triangles": T2, "rounds": rounds,
               "collapses_per_round": [int(c) for c in collapses[:n.value]], "call_us": call_us, "us_per_round": call_us / max(1, rounds)}
        row.update({k: float(v) for k, v in zip(STAGES, stage_us)})
        # the decimated mesh as the reconstruction, the undecimated one as the ground truth, both sampled by area
        e = surface_eval.evaluate(ba, after, before, max_distance=0.1, thresholds=(0.5 * args.voxel_size, args.voxel_size), sample_density=1.0 / args.sample_spacing ** 2)
        row.update(accuracy_mean_m=e["accuracy"]["mean"], accuracy_p99_m=e["accuracy"]["p99"], completeness_mean_m=e["completeness"]["mean"],
                   completeness_p99_m=e["completeness"]["p99"], f_score_at_half_voxel=e["f_scores"][0]["f_score"], f_score_at_voxel=e["f_scores"][1]["f_score"],
                   samples=[e["sampling"]["reconstruction_samples"], e["sampling"]["ground_truth_samples"]])
        return row

    res = {"size": [W, H], "reps": args.reps, "voxel_size_m": args.voxel_size, "truncation_m": truncation, "min_count": args.min_count,
           "sample_spacing_m": args.sample_spacing, "boundary_weight": args.boundary_weight, "cases": []}
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
        for ratio in args.ratios:
            res["cases"].append(bench(f"K = {K}", ba, V, T, mesh, ratio))
        ba.close()
        del dev, volumes, mesh
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
