#!/usr/bin/env python3
"""Times the mesh views (bslam_render_mesh: clear, vertex, draw and resolve launches and the read-back of the error word) at 640x480
on two scenes seen from inside: a room-sized, slightly bumpy sphere tessellated like a surface-nets mesh (--rings x --segments
vertices, 274 x 550 = 150 700 by default, triangles of a few pixels), and the same mesh decimated by bslam_decimate_mesh to --ratio of
its vertices, until single triangles span thousands of pixels.  Device events around --launches back-to-back calls; every figure is
the median of --reps runs after a warm-up.  Each scene is timed with the library's defaults and with every alternative of
bslam_set_render_mesh_tuning: the box sizes up to which a lane and a wave draw alone, vertices projected once or per triangle, and a
resolve pass that reads the projected vertices or projects again.  Beside the times it counts the triangles that pass the per-triangle
tests, the pixel tests of their boxes and the boxes above the default threshold.  Prints one JSON line.
usage: tools/bench_render_mesh.py [--reps N] [--launches M] [--rings R] [--segments S] [--ratio F]"""
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
MIN_DEPTH, MAX_DEPTH = 0.05, 50.0
INT_MAX = (1 << 31) - 1
SMALL_BOXES = (0, 16, 64, 256, 1024)
WAVE_BOXES = (64, 256, 1024, 4096, 16384, INT_MAX)
DEFAULT = (64, 256, 0, 0)      # small_box, wave_box, project_once, resolve_reads_projected


def room(rings, segments):
    """A sphere of radius about 2 m around the origin, wound counter-clockwise seen from inside: (positions, normals, colours, triangles)."""
    theta = (np.arange(rings) + 0.5) / rings * np.pi
    phi = np.arange(segments) / segments * 2 * np.pi
    t, p = np.meshgrid(theta, phi, indexing="ij")
    radius = 2.0 + 0.02 * np.sin(7 * t) * np.cos(5 * p)
    unit = np.stack([np.sin(t) * np.cos(p), np.cos(t), np.sin(t) * np.sin(p)], -1).reshape(-1, 3)
    positions = (unit * radius.reshape(-1, 1)).astype(np.float32)
    normals = (-unit).astype(np.float32)
    colors = np.concatenate([(127.5 * (unit + 1)).astype(np.uint8), np.full((len(unit), 1), 255, np.uint8)], 1)
    r, s = np.meshgrid(np.arange(rings - 1), np.arange(segments), indexing="ij")
    v00, v01 = (r * segments + s).reshape(-1), (r * segments + (s + 1) % segments).reshape(-1)
    v10, v11 = v00 + segments, v01 + segments
    triangles = np.concatenate([np.stack([v00, v10, v01], -1), np.stack([v01, v10, v11], -1)]).astype(np.uint32)
    return positions, normals, colors, triangles


def census(positions, triangles, T, cam, cull=True):
    """Triangles that pass the per-triangle tests and the pixel tests of their boxes (the rule in float64: counts, not bits)."""
    m = np.array(list(T.m), np.float64).reshape(3, 4)
    L = positions.astype(np.float64) @ m[:, :3].T + m[:, 3]
    with np.errstate(all="ignore"):
        px, py = cam.fx * L[:, 0] / L[:, 2] + cam.cx, cam.fy * L[:, 1] / L[:, 2] + cam.cy
    a, b, c = triangles[:, 0], triangles[:, 1], triangles[:, 2]
    z_ok = np.all((L[triangles, 2] >= MIN_DEPTH) & (L[triangles, 2] <= MAX_DEPTH), axis=1)
    area = (px[b] - px[a]) * (py[c] - py[a]) - (py[b] - py[a]) * (px[c] - px[a])
    live = z_ok & (area < 0 if cull else area != 0)
    tx, ty = px[triangles[live]], py[triangles[live]]
    bw = np.clip(np.floor(tx.max(1) - 0.5), -1, cam.width - 1) - np.clip(np.ceil(tx.min(1) - 0.5), 0, cam.width) + 1
    bh = np.clip(np.floor(ty.max(1) - 0.5), -1, cam.height - 1) - np.clip(np.ceil(ty.min(1) - 0.5), 0, cam.height) + 1
    box = (np.maximum(bw, 0) * np.maximum(bh, 0)).astype(np.int64)
    return dict(triangles_passed=int(live.sum()), triangles_with_a_box=int((box > 0).sum()), pixel_tests=int(box.sum()),
                cooperative_triangles=int((box > DEFAULT[0]).sum()), cooperative_pixel_tests=int(box[box > DEFAULT[0]].sum()), queued_triangles=int((box > DEFAULT[1]).sum()),
                largest_box=int(box.max(initial=0)), median_box=float(np.median(box[box > 0])) if (box > 0).any() else 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rings", type=int, default=274)
    ap.add_argument("--segments", type=int, default=550)
    ap.add_argument("--ratio", type=float, default=0.002)
    args = ap.parse_args()
    from badslam_amd import build
    build.build()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_render_mesh.py needs a GPU: there is no CPU path to time")
    import badslam_amd
    from badslam_amd import abi
    L = badslam_amd.lib()
    ctx = badslam_amd.Context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def image(shape, dtype, elems=1):
        t = torch.zeros(shape, dtype=dtype, device="cuda")
        return t, abi.Buffer2D(t.data_ptr(), shape[0], shape[1] // elems, shape[1] * t.element_size())

    depth, index = image((H, W), torch.int16), image((H, W), torch.int32)
    color, normal = image((H, W), torch.int32), image((H, 3 * W), torch.float32, elems=3)
    cam = abi.Camera4f(525.0, 525.0, 320.0, 240.0, W, H)
    T = abi.Mat3x4()      # the camera 0.3 m off the centre, looking along +z of a slightly turned frame
    angle = 0.2
    T.m[:] = [math.cos(angle), 0.0, math.sin(angle), 0.1, 0.0, 1.0, 0.0, -0.05, -math.sin(angle), 0.0, math.cos(angle), 0.3]

    def kernel_us(launch):
        launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.launches):
                launch()
            end.record()
            end.synchronize()
            times.append(start.elapsed_time(end) * 1e3 / args.launches)
        return float(np.median(times))

    host = room(args.rings, args.segments)
    fine = [torch.from_numpy(a.view(np.int32) if a.dtype != np.uint8 else a).cuda() for a in host]
    V, Tn = len(host[0]), len(host[3])
    out = [torch.zeros(max(1, n), dtype=torch.int32, device="cuda") for n in (3 * V, 3 * V, V, 3 * Tn, V)]
    counts = (C.c_uint32(), C.c_uint32(), C.c_uint32())
    badslam_amd.check(L.bslam_decimate_mesh(ctx.handle, stream, V, Tn, *[ptr(t) for t in fine], math.ceil(args.ratio * V), 1.0, float("inf"), 0, *[ptr(t) for t in out],
                                            C.byref(counts[0]), C.byref(counts[1]), C.byref(counts[2])))
    V2, T2 = counts[0].value, counts[1].value
    coarse_host = (out[0][:3 * V2].cpu().numpy().view(np.float32).reshape(V2, 3), None, None, out[3][:3 * T2].cpu().numpy().view(np.uint32).reshape(T2, 3))
    res = {"size": [W, H], "reps": args.reps, "launches_per_rep": args.launches, "depth_range_m": [MIN_DEPTH, MAX_DEPTH], "defaults": list(DEFAULT), "scenes": []}
    for name, mesh, nv, nt, arrays in (("fine", fine, V, Tn, host), ("decimated", out[:4], V2, T2, coarse_host)):

        def call(d, i, c, n):
            badslam_amd.check(L.bslam_render_mesh(ctx.handle, stream, C.byref(T), C.byref(cam), nv, ptr(mesh[0]), ptr(mesh[1]), ptr(mesh[2]), nt, ptr(mesh[3]), MIN_DEPTH,
                                                  MAX_DEPTH, 1, 5000.0, d, i, c, n))

        everything = lambda: call(C.byref(depth[1]), C.byref(index[1]), C.byref(color[1]), C.byref(normal[1]))
        entry = {"scene": name, "vertices": nv, "triangles": nt}
        entry.update(census(arrays[0], arrays[3], T, cam))
        badslam_amd.check(L.bslam_set_render_mesh_tuning(ctx.handle, *DEFAULT))
        entry["all_views_us"] = kernel_us(everything)
        entry["depth_only_us"] = kernel_us(lambda: call(C.byref(depth[1]), None, None, None))
        entry["pixels_covered"] = float((depth[0] != 0).float().mean().item())
        reference = [t[0].clone() for t in (depth, index, color, normal)]
        variants = ([(n, DEFAULT[1], 0, 0) for n in SMALL_BOXES] + [(DEFAULT[0], n, 0, 0) for n in WAVE_BOXES] + [(INT_MAX, INT_MAX, 0, 0)] +
                    [(DEFAULT[0], DEFAULT[1], 1, 1), (DEFAULT[0], DEFAULT[1], 1, 0), (DEFAULT[0], DEFAULT[1], 0, 0)])
        entry["all_views_us_by_tuning"] = []
        for tuning in variants:
            badslam_amd.check(L.bslam_set_render_mesh_tuning(ctx.handle, *tuning))
            us = kernel_us(everything)
            same = all(bool((a == b[0]).all()) for a, b in zip(reference, (depth, index, color, normal)))
            entry["all_views_us_by_tuning"].append({"small_box": tuning[0], "wave_box": tuning[1], "project_once": tuning[2], "resolve_reads_projected": tuning[3], "us": us, "same_bits": same})
        badslam_amd.check(L.bslam_set_render_mesh_tuning(ctx.handle, *DEFAULT))
        res["scenes"].append(entry)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
