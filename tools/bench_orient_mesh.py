#!/usr/bin/env python3
"""Times mesh orientation (bslam_orient_mesh) on the mesh of tools/bench_mesh_repair.py -- the synthetic stack of badslam_amd.synthetic
at 640x480 with K = 50 keyframes, fused at 1 cm voxels with a truncation of 4 voxels, extracted and cleaned -- with a seeded half of its
triangles flipped, in the three modes.  Device events around every call and, with profiling on, around each of its stages
(bslam_repair_stage_times); every figure is the median of --reps calls after a warm-up.  Next to them, from the same run,
bslam_mesh_topology on the same mesh: the two calls share the key pass, the sort and the runs, so the difference is what the parity
union-find, the conflict pass and the votes cost.  Nothing to compare with: neither an earlier version nor the reference orients a
mesh.  Not part of bench.py.  Prints one JSON line.
usage: tools/bench_orient_mesh.py [--reps N] [--keyframes K] [--voxel-size M] [--seed S]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 640, 480
ORIENT_STAGES = ("keys_us", "sort_us", "runs_us", "union_us", "conflict_us", "votes_us", "write_us")
TOPOLOGY_STAGES = ("keys_us", "sort_us", "census_us", "loops_us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--keyframes", type=int, default=50)
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    from badslam_amd import build
    build.build()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_orient_mesh.py needs a GPU: there is no CPU path to time")
    import badslam_amd
    from badslam_amd import abi, synthetic
    from tools import run_tum
    L = badslam_amd.lib()
    ctx = badslam_amd.Context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    truncation = 4 * args.voxel_size
    ptr = lambda t: C.c_void_p(t.data_ptr())
    room = lambda *words: [torch.zeros(max(1, n), dtype=torch.int32, device="cuda") for n in words]

    def timed(call):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e3

    def measure(call, stage_names):
        """-> {"call_us": median, stage: median ...} of `call` after a warm-up (the slab grows there)."""
        call()
        torch.cuda.synchronize()
        row = {"call_us": float(np.median([timed(call) for _ in range(args.reps)]))}
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
        stages = []
        for _ in range(args.reps):
            call()
            ms = (C.c_float * 8)()
            badslam_amd.check(L.bslam_repair_stage_times(ctx.handle, ms))
            stages.append([1e3 * v for v in ms][:len(stage_names)])
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 0))
        row.update({k: float(v) for k, v in zip(stage_names, np.median(np.array(stages), axis=0))})
        return row

    K = args.keyframes
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
    V0, T0 = counts[0].value, counts[1].value
    mesh = room(3 * V0, 3 * V0, V0, 3 * T0)
    extract(V0, T0, tuple(ptr(t) for t in mesh))
    # the census and the orientation refuse what cleaning removes
    cleaned = room(3 * V0, 3 * V0, V0, 3 * T0)
    counts4 = (C.c_uint32 * 4)()
    badslam_amd.check(L.bslam_clean_mesh(ctx.handle, stream, V0, T0, *[ptr(t) for t in mesh], 1, 1, 1, *[ptr(t) for t in cleaned], None, None, C.byref(counts[0]),
                                         C.byref(counts[1]), counts4))
    V, T = counts[0].value, counts[1].value
    positions, normals = cleaned[0], cleaned[1]
    triangles = cleaned[3][:3 * T].reshape(T, 3).clone()
    mask = torch.from_numpy(np.random.default_rng(args.seed).random(T) < 0.5).cuda()
    triangles[mask] = triangles[mask][:, [0, 2, 1]]
    indices = triangles.reshape(-1).contiguous()
    torch.cuda.synchronize()
    res = {"size": [W, H], "keyframes": K, "reps": args.reps, "voxel_size_m": args.voxel_size, "min_count": args.min_count, "vertices": V, "triangles": T,
           "flipped_on_input": int(mask.sum().item()), "modes": {}}

    report = abi.MeshReport()
    census = lambda: badslam_amd.check(L.bslam_mesh_topology(ctx.handle, stream, V, T, ptr(indices), C.byref(report), None, None))
    res["mesh_topology"] = measure(census, TOPOLOGY_STAGES)
    res["mesh_topology"].update(report.as_dict())
    out, flipped, patches = room(3 * T, (T + 3) // 4, T)
    for mode, number in abi.ORIENT_MODES.items():
        counts10 = abi.OrientReport()
        call = lambda: badslam_amd.check(L.bslam_orient_mesh(ctx.handle, stream, V, T, ptr(positions), ptr(normals), ptr(indices), number, ptr(out), ptr(flipped),
                                                             ptr(patches), C.byref(counts10)))
        row = measure(call, ORIENT_STAGES)
        row["beyond_the_census_stages_us"] = row["union_us"] + row["conflict_us"] + row["votes_us"] + row["write_us"]
        row.update(counts10.as_dict())
        census_after = abi.MeshReport()
        badslam_amd.check(L.bslam_mesh_topology(ctx.handle, stream, V, T, ptr(out), C.byref(census_after), None, None))
        row["inconsistent_edges_after"] = int(census_after.inconsistent_edges)
        res["modes"][mode] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
