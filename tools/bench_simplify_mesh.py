#!/usr/bin/env python3
"""Times mesh simplification (bslam_simplify_mesh) on the meshes of tools/bench_fusion.py -- the synthetic stacks of
badslam_amd.synthetic at 640x480, K = 50 and K = 300 keyframes, fused at 1 cm voxels with a truncation of 4 voxels and extracted --
at cells of 2 and 4 voxels.  Device events around every call, and, with profiling on, around each of its five stages (key pass,
sort, head flags and scan, cluster pass, triangle pass); every figure is the median of --reps calls after a warm-up.  Per case: the
output counts, the call and its stages in microseconds, the time of the NumPy restatement of tests/simplify_mesh_util.py on the same
input for scale, and the accuracy and completeness of the simplified mesh against the unsimplified one
(surface_eval.evaluate at samples drawn by area, --sample-spacing apart).  There is nothing to compare with: neither an earlier
version nor the reference simplifies a mesh.  Not part of bench.py.  Prints one JSON line.
usage: tools/bench_simplify_mesh.py [--reps N] [--keyframes 50 300] [--cell-voxels 2 4] [--voxel-size M] [--sample-spacing M]"""
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
STAGES = ("key_us", "sort_us", "heads_scan_us", "cluster_us", "triangles_us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--keyframes", type=int, nargs="*", default=[50, 300])
    ap.add_argument("--cell-voxels", type=float, nargs="+", default=[2.0, 4.0])
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--sample-spacing", type=float, default=0.01)
    ap.add_argument("--no-restatement", action="store_true")
    args = ap.parse_args()
    from badslam_amd import build
    build.build()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_simplify_mesh.py needs a GPU: there is no CPU path to time")
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

    def bench(name, ba, V, T, mesh, cell):
        """mesh: device tensors (positions, normals, colours, indices)."""
        origin = mesh[0].view(torch.float32).reshape(-1, 3)[:V].min(dim=0).values.cpu().numpy()     # exact and order-free, as DirectBA.SimplifyMesh takes it
        o = (C.c_float * 3)(*[float(v) for v in origin])
        out = [torch.zeros(max(1, n), dtype=torch.int32, device="cuda") for n in (3 * V, 3 * V, V, 3 * T, V)]
        counts = (C.c_uint32(), C.c_uint32())

        def simplify():
            badslam_amd.check(L.bslam_simplify_mesh(ctx.handle, stream, V, T, ptr(mesh[0]), ptr(mesh[1]), ptr(mesh[2]), ptr(mesh[3]), o, cell, *[ptr(t) for t in out],
                                                    C.byref(counts[0]), C.byref(counts[1])))

        simplify()                                                       # warm-up; the slab grows here
        torch.cuda.synchronize()
        call_us = float(np.median([timed(simplify) for _ in range(args.reps)]))
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
        stages = []
        for _ in range(args.reps):
            simplify()
            ms = (C.c_float * 5)()
            badslam_amd.check(L.bslam_simplify_stage_times(ctx.handle, ms))
            stages.append([1e3 * v for v in ms])
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 0))
        stage_us = np.median(np.array(stages), axis=0)
        V2, T2 = counts[0].value, counts[1].value
        host = lambda t, n, dtype, shape: t[:n].cpu().numpy().view(dtype).reshape(shape)
        before = dict(positions=host(mesh[0], 3 * V, np.float32, (V, 3)), normals=host(mesh[1], 3 * V, np.float32, (V, 3)), colors=host(mesh[2], V, np.uint8, (V, 4)),
                      triangles=host(mesh[3], 3 * T, np.uint32, (T, 3)))
        after = dict(positions=host(out[0], 3 * V2, np.float32, (V2, 3)), triangles=host(out[3], 3 * T2, np.uint32, (T2, 3)))
        row = {"mesh": name, "vertices": V, "triangles": T, "cell_m": cell, "out_vertices": V2, "out_triangles": T2, "call_us": call_us,
               "vertices_per_s": V / (call_us * 1e-6)}
        row.update({k: float(v) for k, v in zip(STAGES, stage_us)})
        if not args.no_restatement:
            from tests import simplify_mesh_util as su
            t0 = time.perf_counter()
            want = su.simplify(before["positions"], before["normals"], before["colors"], before["triangles"], origin, cell)
            row["numpy_restatement_us"] = (time.perf_counter() - t0) * 1e6
            row["equals_restatement"] = bool(np.array_equal(want["positions"].view(np.uint32), after["positions"].view(np.uint32)) and
                                             np.array_equal(want["triangles"], after["triangles"]))
        # the simplified mesh as the reconstruction, the unsimplified one as the ground truth, both sampled by area
        e = surface_eval.evaluate(ba, after, before, max_distance=0.1, thresholds=(0.5 * cell, cell), sample_density=1.0 / args.sample_spacing ** 2)
        row.update(accuracy_mean_m=e["accuracy"]["mean"], accuracy_p99_m=e["accuracy"]["p99"], completeness_mean_m=e["completeness"]["mean"],
                   completeness_p99_m=e["completeness"]["p99"], f_score_at_half_cell=e["f_scores"][0]["f_score"], f_score_at_cell=e["f_scores"][1]["f_score"],
                   samples=[e["sampling"]["reconstruction_samples"], e["sampling"]["ground_truth_samples"]])
        return row

    res = {"size": [W, H], "reps": args.reps, "voxel_size_m": args.voxel_size, "truncation_m": truncation, "min_count": args.min_count,
           "sample_spacing_m": args.sample_spacing, "cases": []}
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
        for voxels in args.cell_voxels:
            res["cases"].append(bench(f"K = {K}", ba, V, T, mesh, float(np.float32(voxels * args.voxel_size))))
        ba.close()
        del dev, volumes, mesh
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
