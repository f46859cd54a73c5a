#!/usr/bin/env python3
"""Times the model views (bslam_render_surfels: clear, splat and resolve launches) on the synthetic stacks of
badslam_amd.synthetic at 640x480 -- the K = 50 geometry-only stack (0.96 M surfels) and the K = 300 stack (5.76 M surfels) --
from the pose of keyframe 0, with device events around --launches back-to-back calls; every figure is the median of --reps runs
after a warm-up.  Beside the times it counts, from the boxes (the kernel's rule restated with torch in fp32), how many pixel
tests a call makes, how many of them hit a disc (each of those issues a 64-bit atomic minimum unless the plain load before it
shows a key that already wins, so this is an upper bound of the atomics), and how many surfels go the cooperative way.
Prints one JSON line.
usage: tools/bench_render.py [--reps N] [--launches M] [--keyframes 50 300]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 640, 480
MIN_DEPTH, MAX_DEPTH = 0.05, 50.0
SMALL_BOX = 64


def census(torch, surfels, T, cam, radius_scale, chunk=1 << 20):
    """Pixel tests, disc hits and box statistics of one call, from the surfel rows on the device."""
    f = torch.float32
    m = [torch.tensor(float(v), dtype=f, device=surfels.device) for v in T.m]
    fx, fy, cx, cy = [torch.tensor(float(v), dtype=f, device=surfels.device) for v in (cam.fx, cam.fy, cam.cx, cam.cy)]
    out = dict(surfels_drawn=0, pixel_tests=0, disc_hits=0, cooperative_surfels=0, cooperative_pixel_tests=0, largest_box=0)
    for start in range(0, surfels.shape[1], chunk):
        s = surfels[:, start:start + chunk]
        x, y, z = s[0], s[1], s[2]
        Lx = ((m[0] * x + m[1] * y) + m[2] * z) + m[3]
        Ly = ((m[4] * x + m[5] * y) + m[6] * z) + m[7]
        Lz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11]
        packed = s[3].view(torch.int32)
        sx, sy, sz = [((packed << shift) >> 22).to(f) for shift in (22, 12, 2)]
        nx = (m[0] * sx + m[1] * sy) + m[2] * sz
        ny = (m[4] * sx + m[5] * sy) + m[6] * sz
        nz = (m[8] * sx + m[9] * sy) + m[10] * sz
        r2 = s[4] * (radius_scale * radius_scale)
        r = torch.sqrt(torch.clamp(r2, min=0))
        k = (nx * Lx + ny * Ly) + nz * Lz
        live = (x == x) & (r2 > 0) & (Lz - r >= MIN_DEPTH) & (Lz <= MAX_DEPTH) & (k < 0)
        near, far = Lz - r, Lz + r
        qx = torch.stack([(Lx - r) / near, (Lx - r) / far, (Lx + r) / near, (Lx + r) / far])
        qy = torch.stack([(Ly - r) / near, (Ly - r) / far, (Ly + r) / near, (Ly + r) / far])
        i0 = torch.clamp(torch.ceil(fx * qx.min(0).values + cx - 0.5) - 1, 0, cam.width)
        i1 = torch.clamp(torch.floor(fx * qx.max(0).values + cx - 0.5) + 1, -1, cam.width - 1)
        j0 = torch.clamp(torch.ceil(fy * qy.min(0).values + cy - 0.5) - 1, 0, cam.height)
        j1 = torch.clamp(torch.floor(fy * qy.max(0).values + cy - 0.5) + 1, -1, cam.height - 1)
        bw, bh = torch.clamp(i1 - i0 + 1, min=0), torch.clamp(j1 - j0 + 1, min=0)
        live &= (bw > 0) & (bh > 0)
        area = torch.where(live, bw * bh, torch.zeros_like(bw)).to(torch.int64)
        out["surfels_drawn"] += int(live.sum())
        out["pixel_tests"] += int(area.sum())
        out["cooperative_surfels"] += int((area > SMALL_BOX).sum())
        out["cooperative_pixel_tests"] += int(area[area > SMALL_BOX].sum())
        out["largest_box"] = max(out["largest_box"], int(area.max()))
        # every test of the chunk, expanded: test t of surfel a is the centre (i0 + t % bw, j0 + t // bw)
        keep = torch.nonzero(area > 0)[:, 0]
        for part in torch.split(keep, 1 << 17):
            a = area[part]
            owner = torch.repeat_interleave(part, a)
            first = torch.cumsum(a, 0) - a
            t = torch.arange(int(a.sum()), device=surfels.device) - torch.repeat_interleave(first, a)
            w = bw[owner].to(torch.int64)
            dx = ((i0[owner] + (t % w).to(f) + 0.5) - cx) / fx
            dy = ((j0[owner] + (t // w).to(f) + 0.5) - cy) / fy
            den = (nx[owner] * dx + ny[owner] * dy) + nz[owner]
            depth = k[owner] / den
            hx, hy, hz = depth * dx - Lx[owner], depth * dy - Ly[owner], depth - Lz[owner]
            out["disc_hits"] += int(((den < 0) & ((hx * hx + hy * hy) + hz * hz <= r2[owner])).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--keyframes", type=int, nargs="+", default=[50, 300])
    ap.add_argument("--radius-scale", type=float, default=1.0)
    args = ap.parse_args()
    from badslam_amd import build
    build.build()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_render.py needs a GPU: there is no CPU path to time")
    import badslam_amd
    from badslam_amd import abi, synthetic
    L = badslam_amd.lib()
    ctx = badslam_amd.Context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def image(shape, dtype, elems=1):
        t = torch.zeros(shape, dtype=dtype, device="cuda")
        return t, abi.Buffer2D(t.data_ptr(), shape[0], shape[1] // elems, shape[1] * t.element_size())

    depth, index = image((H, W), torch.int16), image((H, W), torch.int32)
    color, normal = image((H, W), torch.int32), image((H, 3 * W), torch.float32, elems=3)

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

    res = {"size": [W, H], "reps": args.reps, "launches_per_rep": args.launches, "radius_scale": args.radius_scale,
           "depth_range_m": [MIN_DEPTH, MAX_DEPTH], "stacks": []}
    for K in args.keyframes:
        dev = synthetic.TorchStack(K, "cuda:0", width=W, height=H)
        cam = dev.stack.camera
        _, T, _ = dev.stack.pose(0)
        rows = dev.buf(dev.surfels)
        S = dev.surfels_size
        m2d = float(1.0 / np.float32(dev.stack.raw_to_float_depth))

        def call(d, i, c, n):
            badslam_amd.check(L.bslam_render_surfels(ctx.handle, stream, C.byref(T), C.byref(cam), S, C.byref(rows), MIN_DEPTH, MAX_DEPTH,
                                                     args.radius_scale, m2d, d, i, c, n))

        entry = {"keyframes": K, "surfels": S,
                 "launch_shapes": {"clear": [(W * H + 255) // 256, 256], "splat": [(S + 255) // 256, 256], "resolve": [[(W + 255) // 256, H], 256]}}
        entry["all_views_us"] = kernel_us(lambda: call(C.byref(depth[1]), C.byref(index[1]), C.byref(color[1]), C.byref(normal[1])))
        entry["depth_only_us"] = kernel_us(lambda: call(C.byref(depth[1]), None, None, None))
        entry["pixels_covered"] = float((depth[0] != 0).float().mean().item())
        entry.update(census(torch, dev.surfels, T, cam, args.radius_scale))
        res["stacks"].append(entry)
        del dev
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
