#!/usr/bin/env python3
"""Times the mesh clean-up calls (bslam_mesh_components, bslam_filter_mesh at min_vertices = 64) on the meshes of the stacks
tools/bench_fusion.py fuses: badslam_amd.synthetic at 640x480, K = 50 and K = 300 keyframes, the box of the surfel model padded by
the truncation, 1 cm voxels, a truncation of 4 voxels, min_count 2.  Device events around every call; every figure is the median of
--reps calls after a warm-up.  Beside the times: the full extraction of the same mesh for scale, the size of the mesh, its
components, what the filter removes, the hooks (compare-and-swaps) the union kernel attempted and had to retry -- counted in one
call of its own with profiling on, outside the timed ones -- and, once, the time the sequential host restatement of
tests/mesh_components_util.py takes for the same answer, which the device results are compared with.  Not part of bench.py.
Prints one JSON line.
usage: tools/bench_mesh_components.py [--reps N] [--keyframes 50 300] [--voxel-size M] [--min-vertices N] [--kind dense]"""
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
LAUNCHES = {"label": "init, seed, compress, union, flatten + count, sizes: 6 launches, 1 read-back of 2 words",
            "filter": "memset, keep flags, 2 scans of 3, scatter: 8 launches and a memset, 1 read-back of 4 words"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--keyframes", type=int, nargs="+", default=[50, 300])
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--min-vertices", type=int, default=64)
    ap.add_argument("--kind", default="dense")
    args = ap.parse_args()
    from badslam_amd import build
    build.build()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_components.py needs a GPU: there is no CPU path to time")
    import badslam_amd
    from badslam_amd import abi, synthetic
    from tests import mesh_components_util as mu
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

    res = {"size": [W, H], "reps": args.reps, "voxel_size_m": args.voxel_size, "truncation_m": truncation, "min_count": args.min_count,
           "min_vertices": args.min_vertices, "kind": args.kind, "launches": LAUNCHES, "stacks": []}
    for K in args.keyframes:
        dev = synthetic.TorchStack(K, "cuda:0", width=W, height=H, kind=args.kind)
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
        new = lambda words: torch.zeros(max(1, words), dtype=torch.int32, device="cuda")
        mesh = [new(n) for n in (3 * V, 3 * V, V, 3 * T)]
        filtered = [new(n) for n in (3 * V, 3 * V, V, 3 * T)]
        labels, sizes = new(V), new(V)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        out = tuple(ptr(t) for t in mesh)
        extract(V, T, out)
        components, kept_v, kept_t = C.c_uint32(), C.c_uint32(), C.c_uint32()

        def label():
            badslam_amd.check(L.bslam_mesh_components(ctx.handle, stream, V, T, out[3], ptr(labels), ptr(sizes), C.byref(components)))

        def keep():
            badslam_amd.check(L.bslam_filter_mesh(ctx.handle, stream, V, T, out[0], out[1], out[2], out[3], ptr(sizes), args.min_vertices,
                                                  *[ptr(t) for t in filtered], C.byref(kept_v), C.byref(kept_t)))

        label()                                                          # warm-up: scratch, first launches
        keep()
        torch.cuda.synchronize()
        extract_us = float(np.median([timed(lambda: extract(V, T, out)) for _ in range(args.reps)]))
        label_all = [timed(label) for _ in range(args.reps)]
        filter_all = [timed(keep) for _ in range(args.reps)]
        tested, culled = C.c_uint64(), C.c_uint64()                      # the counters cost two atomics per triangle: kept out of the timed calls
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
        badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))
        label()
        badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 0))
        triangles = mesh[3][:3 * T].cpu().numpy().view(np.uint32).reshape(T, 3)
        t0 = time.perf_counter()
        want = mu.components(V, triangles)
        want_t, _ = mu.filter_mesh(want[1], args.min_vertices, triangles)
        host_s = time.perf_counter() - t0
        got_labels, got_sizes = labels[:V].cpu().numpy().view(np.uint32), sizes[:V].cpu().numpy().view(np.uint32)
        same = bool(np.array_equal(got_labels, want[0]) and np.array_equal(got_sizes, want[1]) and components.value == want[2] and
                    np.array_equal(filtered[3][:3 * kept_t.value].cpu().numpy().view(np.uint32).reshape(-1, 3), want_t))
        per_component = np.sort(want[1][want[0] == np.arange(V)])[::-1]
        res["stacks"].append({
            "keyframes": K, "volume": [nx, ny, nz], "vertices": V, "triangles": T, "components": components.value,
            "largest_components": per_component[:8].tolist(), "kept_vertices": kept_v.value, "kept_triangles": kept_t.value,
            "extract_us": extract_us, "label_us": float(np.median(label_all)), "filter_us": float(np.median(filter_all)),
            "label_us_all": label_all, "filter_us_all": filter_all, "hooks_attempted": tested.value, "hooks_retried": culled.value,
            "host_restatement_s": host_s, "equals_host_restatement": same})
        del dev, volumes, mesh, filtered
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
