#!/usr/bin/env python3
"""Times mesh repair (bslam_clean_mesh, bslam_mesh_topology, bslam_fill_mesh_holes) on the mesh of tools/bench_simplify_mesh.py -- the
synthetic stack of badslam_amd.synthetic at 640x480 with K = 50 keyframes, fused at 1 cm voxels with a truncation of 4 voxels and
extracted: 150 710 vertices -- in three forms: as it is, as a triangle soup (every corner a vertex of its own: 3 T vertices) and
simplified at 4 cm, then cleaned.  Device events around every call and, with profiling on, around each of its stages
(bslam_repair_stage_times); every figure is the median of --reps calls after a warm-up.  Next to them, from the same run, the times of
bslam_simplify_mesh at 4 cm and of bslam_decimate_mesh to a quarter of the vertices on the mesh as it is: what cleaning adds to the
pipeline.  Nothing to compare with: neither an earlier version nor the reference repairs a mesh.  Not part of bench.py.  Prints one JSON
line.
usage: tools/bench_mesh_repair.py [--reps N] [--keyframes K] [--voxel-size M] [--max-hole-edges N]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 640, 480
CLEAN_STAGES = ("vertex_keys_us", "weld_sorts_us", "representatives_us", "triangle_keys_us", "triangle_sorts_us", "duplicates_us", "flags_scans_us", "scatter_us")
TOPOLOGY_STAGES = ("keys_us", "sort_us", "census_us", "loops_us")
FILL_STAGES = TOPOLOGY_STAGES + ("hole_scans_us", "copy_fans_us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=50)
    ap.add_argument("--voxel-size", type=float, default=0.01)
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--simplify-cell", type=float, default=0.04)
    ap.add_argument("--max-hole-edges", type=int, default=64)
    args = ap.parse_args()
    from badslam_amd import build
    build.build()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_repair.py needs a GPU: there is no CPU path to time")
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

    def measure(call, stage_names=None, stage_times=None):
        """-> {"call_us": median, stage: median ...} of `call` after a warm-up (the slab grows there)."""
        call()
        torch.cuda.synchronize()
        row = {"call_us": float(np.median([timed(call) for _ in range(args.reps)]))}
        if stage_names:
            badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
            stages = []
            for _ in range(args.reps):
                call()
                ms = (C.c_float * 8)()
                badslam_amd.check(stage_times(ctx.handle, ms))
                stages.append([1e3 * v for v in ms][:len(stage_names)])
            badslam_amd.check(L.bslam_profile_enable(ctx.handle, 0))
            row.update({k: float(v) for k, v in zip(stage_names, np.median(np.array(stages), axis=0))})
        return row

    def clean(V, T, mesh):
        out = room(3 * V, 3 * V, V, 3 * T, V, T)
        counts, counts4 = (C.c_uint32(), C.c_uint32()), (C.c_uint32 * 4)()
        call = lambda: badslam_amd.check(L.bslam_clean_mesh(ctx.handle, stream, V, T, *[ptr(t) for t in mesh], 1, 1, 1, *[ptr(t) for t in out], C.byref(counts[0]),
                                                            C.byref(counts[1]), counts4))
        row = measure(call, CLEAN_STAGES, L.bslam_repair_stage_times)
        row.update(out_vertices=counts[0].value, out_triangles=counts[1].value, welded_vertices=counts4[0], unreferenced_vertices=counts4[1],
                   degenerate_triangles=counts4[2], duplicate_triangles=counts4[3])
        return row, out, counts[0].value, counts[1].value

    def topology(V, T, indices):
        report = abi.MeshReport()
        uses, loops = room(3 * T, 3 * T)
        call = lambda: badslam_amd.check(L.bslam_mesh_topology(ctx.handle, stream, V, T, ptr(indices), C.byref(report), ptr(uses), ptr(loops)))
        row = measure(call, TOPOLOGY_STAGES, L.bslam_repair_stage_times)
        row.update(report.as_dict())
        return row

    def fill(V, T, mesh):
        counts = (C.c_uint32(), C.c_uint32(), C.c_uint32())
        tail = [C.byref(c) for c in counts]
        badslam_amd.check(L.bslam_fill_mesh_holes(ctx.handle, stream, V, T, *[ptr(t) for t in mesh], args.max_hole_edges, 0, 0, None, None, None, None, None, *tail))
        V2, T2 = counts[0].value, counts[1].value
        out = room(3 * V2, 3 * V2, V2, 3 * T2, T2 - T)
        call = lambda: badslam_amd.check(L.bslam_fill_mesh_holes(ctx.handle, stream, V, T, *[ptr(t) for t in mesh], args.max_hole_edges, V2, T2, *[ptr(t) for t in out], *tail))
        row = measure(call, FILL_STAGES, L.bslam_repair_stage_times)
        row.update(max_hole_edges=args.max_hole_edges, out_vertices=V2, out_triangles=T2, filled_holes=counts[2].value)
        return row

    def repair(name, V, T, mesh):
        """Clean the mesh, then census and hole filling of the cleaned mesh (the census refuses what cleaning removes)."""
        row = {"mesh": name, "vertices": V, "triangles": T}
        row["clean"], cleaned, V2, T2 = clean(V, T, mesh)
        row["topology"] = topology(V2, T2, cleaned[3])
        row["fill_holes"] = fill(V2, T2, cleaned[:4])
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
    V, T = counts[0].value, counts[1].value
    mesh = room(3 * V, 3 * V, V, 3 * T)
    extract(V, T, tuple(ptr(t) for t in mesh))
    torch.cuda.synchronize()
    res = {"size": [W, H], "keyframes": K, "reps": args.reps, "voxel_size_m": args.voxel_size, "min_count": args.min_count, "cases": []}

    # the pipeline's own operators on the same mesh, in the same run
    cell = float(np.float32(args.simplify_cell))
    corner = mesh[0].view(torch.float32).reshape(-1, 3)[:V].min(dim=0).values.cpu().numpy()
    o = (C.c_float * 3)(*[float(v) for v in corner])
    simplified = room(3 * V, 3 * V, V, 3 * T, V)
    sc = (C.c_uint32(), C.c_uint32())
    simplify = lambda: badslam_amd.check(L.bslam_simplify_mesh(ctx.handle, stream, V, T, *[ptr(t) for t in mesh], o, cell, *[ptr(t) for t in simplified], C.byref(sc[0]),
                                                               C.byref(sc[1])))
    res["simplify_mesh"] = dict(measure(simplify), cell_m=cell)
    res["simplify_mesh"].update(out_vertices=sc[0].value, out_triangles=sc[1].value)
    decimated = room(3 * V, 3 * V, V, 3 * T, V)
    dc = (C.c_uint32(), C.c_uint32(), C.c_uint32())
    decimate = lambda: badslam_amd.check(L.bslam_decimate_mesh(ctx.handle, stream, V, T, *[ptr(t) for t in mesh], V // 4, 1.0, float("inf"), 0, *[ptr(t) for t in decimated],
                                                               C.byref(dc[0]), C.byref(dc[1]), C.byref(dc[2])))
    res["decimate_mesh"] = dict(measure(decimate), target_vertices=V // 4, out_vertices=dc[0].value, out_triangles=dc[1].value, rounds=dc[2].value)
    del decimated

    res["cases"].append(repair("as extracted", V, T, mesh))
    # the soup: every corner a vertex of its own
    flat = mesh[3][:3 * T].long()
    gather = lambda t, per: t[:per * V].reshape(V, per)[flat].reshape(-1).contiguous()
    soup = [gather(mesh[0], 3), gather(mesh[1], 3), gather(mesh[2], 1), torch.arange(3 * T, dtype=torch.int32, device="cuda")]
    res["cases"].append(repair("soup", 3 * T, T, soup))
    del soup
    res["cases"].append(repair(f"simplified at {cell:g} m", sc[0].value, sc[1].value, simplified[:4]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
