"""-m gpu: the image-pair Gauss-Newton rows, bit for bit against rows recorded before the pairwise tracking stack was folded
into one pair kernel and one driver (tests/golden/pair_rows.npz).  The oracle comparisons of these kernels carry tolerances;
this module pins the bits: every variant of the four single-pair entry points and the batched entry point with 1, 3 and 8
pairs, at three shapes and in both texture modes, and batched row p against the single-pair row of the same pair.

The file holds the inputs next to the rows, so the test computes nothing on the host but `u16 depth * f32(1 / 5000)`.
`python -m tests.test_gpu_pair_rows_recorded --record OUT.npz` writes such a file with the library of the checkout it runs in;
it uses public entry points only.

A row is 32 uint32 words, the layout of the kernels' partial rows as far as the entry points return it: columns 0 ... 20 the
bits of H, 21 ... 26 the bits of b, 27 the bits of the cost, 28 the count (visible pixels of a coefficient row, residuals of a
cost row); what an entry point does not return stays 0.

Shapes: 20x12 (240 pixels: one partly filled block, 4 partial rows, fewer than the reduction's 8 parts), 84x60 (5040 pixels:
80 partial rows, the last block partly filled) and 84x60 with a 42x30 colour camera (the depth-to-colour mapping is not the
identity).  Pairs: two tracked frames in turn, each pair with an estimate of its own near the rendered motion; the last pair of
a batch of 3 or 8 looks away from the scene and sees nothing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi

pytestmark = pytest.mark.gpu
P = C.POINTER
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_rows.npz")
RAW_TO_FLOAT = np.float32(1.0 / 5000)
BASELINE_FX = 40.0
ROW = 32
COL_COST, COL_COUNT = 27, 28
BLIND = 8                                   # index of the transform that sees nothing
# name -> (depth size, colour size, depth camera fx fy cx cy, threshold factor); the colour camera is the depth camera scaled
SHAPES = {
    "20x12": ((20, 12), (20, 12), (40.0, 40.0, 10.0, 6.0), 4.0),
    "84x60": ((84, 60), (84, 60), (100.0, 100.0, 42.3, 29.6), 1.0),
    "84x60_color42x30": ((84, 60), (42, 30), (100.0, 100.0, 42.3, 29.6), 1.0),
}
MODES = {"fixed": abi.TEX_FIXED_POINT_1_8, "exact": abi.TEX_EXACT_FLOAT}
RESIDUAL_SETS = {"depth": (1, 0), "desc": (0, 1), "both": (1, 1)}
PAIR_COUNTS = (1, 3, 8)
INPUT_KEYS = ("depth", "normals", "color_depth", "color", "M")
STORED_WITH = {"84x60_color42x30": "84x60"}   # a shape whose inputs, but for the tracked colour, are another shape's and stored there


def cameras(shape):
    (dw, dh), (cw, ch), (fx, fy, cx, cy), _ = SHAPES[shape]
    f = cw / dw
    return abi.Camera4f(fx * f, fy * f, cx * f, cy * f, cw, ch), abi.Camera4f(fx, fy, cx, cy, dw, dh)


def batch_pairs(n):
    """The pairs of a batch of n as (tracked frame 1 or 2, transform index): pair p tracks frame 1 + p % 2 with transform p; the
    last pair of a batch of more than one looks away (transform BLIND)."""
    return [(1 + p % 2, BLIND if (n > 1 and p == n - 1) else p) for p in range(n)]


def single_pairs():
    seen = []
    for n in PAIR_COUNTS:
        for pair in batch_pairs(n):
            if pair not in seen:
                seen.append(pair)
    return seen


# ---- the fixture's inputs (recording only) ---------------------------------------------------------------------------
def rodrigues(w):
    w = np.asarray(w, np.float64)
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) if a == 0 else np.eye(3) + np.sin(a) / a * K + (1 - np.cos(a)) / (a * a) * K @ K


FRAME_MOTION = [((0, 0, 0), (0, 0, 0)), ((0.010, -0.008, 0.005), (0.020, -0.010, 0.015)), ((-0.006, 0.012, -0.004), (-0.015, 0.020, -0.010))]
PLANES = [(np.array([0.15, -0.10, -1.0]), np.array([0.0, 0.0, 1.6])), (np.array([-0.45, 0.05, -1.0]), np.array([0.25, 0.0, 1.6]))]   # normal, point


def cast(fx, fy, cx, cy, w, h, R, t, wavelength):
    """Rays through the pixel centres of a camera with frame_T_base = [R | t] against the roof of PLANES (the nearer of the two
    planes): depth z, normal in the frame, luma of the texture at the hit point (a function of its base coordinates)."""
    x, y = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    g = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x)], -1)
    z, normal = np.full(x.shape, np.inf), np.zeros(x.shape + (3,))
    for n, p in PLANES:
        n = n / np.linalg.norm(n)
        nf = R @ n                                         # the plane n . X = d in the frame: nf . Y = d + nf . t
        zi = (n @ p + nf @ t) / (g @ nf)
        nearer = (zi > 0) & (zi < z)
        z = np.where(nearer, zi, z)
        normal[nearer] = nf
    X = (g * z[..., None] - t) @ R                         # R^T (Y - t)
    k = 2 * np.pi / wavelength
    luma = 128 + 60 * np.sin(k * X[..., 0] + 0.3) * np.cos(0.8 * k * X[..., 1]) + 40 * np.sin(0.6 * k * (X[..., 0] + X[..., 1]))
    return z, normal, np.clip(luma + 0.5, 0, 255).astype(np.uint8)


def make_inputs(shape):
    """Inputs of one shape: depth u16 [3, h, w], normals u16 [3, h, w], colour u8 in the depth geometry [3, h, w] and in the colour
    camera's [3, ch, cw] (frame 0 is the base, 1 and 2 are tracked), transforms f32 [9, 12] (frame_T_base estimates; 8 = BLIND)."""
    (dw, dh), (cw, ch), (fx, fy, cx, cy), _ = SHAPES[shape]
    wavelength = 8 * 1.6 / fx                              # eight depth pixels at the scene's distance
    depth, normals, color_d, color_c = [], [], [], []
    for i, (w, t) in enumerate(FRAME_MOTION):
        R, t = rodrigues(w), np.array(t, np.float64)
        z, n, luma = cast(fx, fy, cx, cy, dw, dh, R, t, wavelength)
        raw = np.clip(z / float(RAW_TO_FLOAT) + 0.5, 0, 32767).astype(np.uint16)
        yy, xx = np.mgrid[0:dh, 0:dw]
        raw[(xx * 7 + yy * 13 + i) % 31 == 0] = 0                                           # scattered holes
        raw[dh // 6 + i:dh // 6 + i + max(2, dh // 6), dw // 3:dw // 3 + max(3, dw // 6)] = 0   # and a block of them
        n8 = np.rint(n[..., :2] * 127).astype(np.int8).view(np.uint8).astype(np.uint16)
        depth.append(raw)
        normals.append(n8[..., 0] | (n8[..., 1] << 8))
        color_d.append(luma)
        f = cw / dw
        color_c.append(cast(fx * f, fy * f, cx * f, cy * f, cw, ch, R, t, wavelength)[2])
    M = np.zeros((9, 12), np.float32)
    for p in range(8):
        w, t = FRAME_MOTION[1 + p % 2]
        dw_, dt_ = 0.0005 * (p + 1) * np.array([1, -1, 0.5]), 0.0012 * (p + 1) * np.array([-1, 0.5, 1])
        M[p] = np.concatenate([rodrigues(np.array(w) + dw_), (np.array(t) + dt_)[:, None]], 1).reshape(12)
    M[BLIND] = np.concatenate([np.eye(3), np.array([[0], [0], [-50.0]])], 1).reshape(12)    # the scene lies behind this camera
    return {"depth": np.stack(depth), "normals": np.stack(normals), "color_depth": np.stack(color_d), "color": np.stack(color_c), "M": M}


# ---- running the entry points ----------------------------------------------------------------------------------------
def _buf(t):
    return abi.Buffer2D(t.data_ptr(), t.shape[0], t.shape[1], t.stride(0) * t.element_size())


def _fp(a):
    return a.ctypes.data_as(P(C.c_float))


def run_all(torch, L, ctx, shape, inputs):
    """Every call of the module on one shape, in a fixed order -> (labels, rows uint32 [n, 32])."""
    color_cam, depth_cam = cameras(shape)
    threshold = SHAPES[shape][3]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    depth = [dev(d.astype(np.float32) * RAW_TO_FLOAT) for d in inputs["depth"]]
    normals = [dev(n.view(np.int16)) for n in inputs["normals"]]
    base_color = dev(inputs["color_depth"][0])
    color = [dev(c) for c in inputs["color"]]
    torch.cuda.synchronize()
    stream = C.c_void_p(None)
    bd, bn, bc = _buf(depth[0]), _buf(normals[0]), _buf(base_color)
    Ms = [abi.Mat3x4((C.c_float * 12)(*[float(v) for v in m])) for m in inputs["M"]]
    labels, rows = [], []

    def single(frame, m, use, coeffs, gradmag):
        row = np.zeros(ROW, np.uint32)
        td, tn, tc = _buf(depth[frame]), _buf(normals[frame]), _buf(color[frame])
        head = (ctx.handle, stream, use[0], use[1], C.byref(color_cam), C.byref(depth_cam), BASELINE_FX, threshold, C.byref(td), C.byref(tn), C.byref(tc),
                C.byref(Ms[m]), C.byref(bd), C.byref(bn), C.byref(bc))
        count = C.c_uint32()
        if coeffs:
            H, b = np.zeros(21, np.float32), np.zeros(6, np.float32)
            fn = L.bslam_accumulate_pose_coeffs_from_images_gradmag if gradmag else L.bslam_accumulate_pose_coeffs_from_images
            badslam_amd.check(fn(*head, C.byref(count), _fp(H), _fp(b)))
            row[0:21], row[21:27] = H.view(np.uint32), b.view(np.uint32)
        else:
            cost = C.c_float()
            fn = L.bslam_compute_cost_and_residual_count_from_images_gradmag if gradmag else L.bslam_compute_cost_and_residual_count_from_images
            badslam_amd.check(fn(*head, C.byref(count), C.byref(cost)))
            row[COL_COST] = np.array([cost.value], np.float32).view(np.uint32)[0]
        row[COL_COUNT] = count.value
        return row

    # the ten variants of the single-pair entry points, on pair 0
    for name, use in RESIDUAL_SETS.items():
        for gradmag in ((False, True) if use[1] else (False,)):
            for coeffs in (True, False):
                labels.append(f"variant/{name}/{'coeffs' if coeffs else 'cost'}{'/gradmag' if gradmag else ''}")
                rows.append(single(1, 0, use, coeffs, gradmag))
    # the coefficient row of every pair a batch holds, through the single-pair entry point
    for name, use in RESIDUAL_SETS.items():
        for frame, m in single_pairs():
            labels.append(f"single/{name}/frame{frame}/m{m}")
            rows.append(single(frame, m, use, True, False))
    # the batched entry point
    for name, use in RESIDUAL_SETS.items():
        for n in PAIR_COUNTS:
            pairs = batch_pairs(n)
            Buffers = abi.Buffer2D * n
            td, tn, tc = (Buffers(*[_buf(images[f]) for f, _ in pairs]) for images in (depth, normals, color))
            Marr = (abi.Mat3x4 * n)(*[Ms[m] for _, m in pairs])
            H, b, counts = np.zeros(21 * n, np.float32), np.zeros(6 * n, np.float32), np.zeros(n, np.uint32)
            badslam_amd.check(L.bslam_accumulate_pose_coeffs_from_images_batched(
                ctx.handle, stream, use[0], use[1], C.byref(color_cam), C.byref(depth_cam), BASELINE_FX, threshold, n, td, tn, tc, Marr, C.byref(bd),
                C.byref(bn), C.byref(bc), counts.ctypes.data_as(P(C.c_uint32)), _fp(H), _fp(b)))
            for p, (frame, m) in enumerate(pairs):
                row = np.zeros(ROW, np.uint32)
                row[0:21], row[21:27], row[COL_COUNT] = H[21 * p:21 * p + 21].view(np.uint32), b[6 * p:6 * p + 6].view(np.uint32), counts[p]
                labels.append(f"batched/{name}/n{n}/p{p}/frame{frame}/m{m}")
                rows.append(row)
    return labels, np.stack(rows)


def check_rows(shape, inputs, labels, rows):
    """What holds of any set of rows, recorded or fresh: a batched row equals the single-pair row of its pair, a pair that looks
    away sees nothing, and every other coefficient row sees at least 100 pixels (20x12) or a third of the valid base pixels."""
    at = {label: row for label, row in zip(labels, rows)}
    valid_base = int((inputs["depth"][0] != 0).sum())
    least = 100 if shape == "20x12" else (valid_base + 2) // 3
    for label, row in at.items():
        part = label.split("/")
        if part[0] == "batched":
            assert np.array_equal(row, at[f"single/{part[1]}/{part[4]}/{part[5]}"]), (shape, label)
        if part[0] == "variant" and part[2] == "cost":
            continue                                                     # counts residuals, not pixels
        if label.endswith(f"/m{BLIND}"):
            assert row[COL_COUNT] == 0, (shape, label)
        else:
            assert row[COL_COUNT] >= least, (shape, label, int(row[COL_COUNT]), least)


def record(path):
    import torch
    L, ctx = badslam_amd.lib(), badslam_amd.Context(0)
    out = {}
    for shape in SHAPES:
        inputs = make_inputs(shape)
        for key, value in inputs.items():
            if shape in STORED_WITH and key != "color":
                assert np.array_equal(value, out[f"{STORED_WITH[shape]}/{key}"])
            else:
                out[f"{shape}/{key}"] = value
        for mode_name, mode in MODES.items():
            ctx.set_texture_mode(mode)
            labels, rows = run_all(torch, L, ctx, shape, inputs)
            check_rows(shape, inputs, labels, rows)
            out[f"{shape}/{mode_name}/labels"], out[f"{shape}/{mode_name}/rows"] = np.array(labels), rows
            print(shape, mode_name, len(labels), "rows; visible pixels", int(rows[:, COL_COUNT].min()), "...", int(rows[:, COL_COUNT].max()),
                  "of", int((inputs["depth"][0] != 0).sum()), "valid base pixels")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


# ---- the test ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN) as f:
        return {key: f[key] for key in f.files}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pair_rows_equal_the_recorded_rows_bit_for_bit(recorded, shape, mode):
    import torch
    L, ctx = badslam_amd.lib(), badslam_amd.Context(0)
    ctx.set_texture_mode(MODES[mode])
    inputs = {key: recorded[f"{shape if key == 'color' else STORED_WITH.get(shape, shape)}/{key}"] for key in INPUT_KEYS}
    labels, rows = run_all(torch, L, ctx, shape, inputs)
    want_labels, want = [str(s) for s in recorded[f"{shape}/{mode}/labels"]], recorded[f"{shape}/{mode}/rows"]
    assert labels == want_labels
    assert rows.dtype == np.uint32 and want.dtype == np.uint32 and rows.shape == want.shape == (len(labels), ROW)
    check_rows(shape, inputs, want_labels, want)            # the fixture's conditions, from the stored counts
    check_rows(shape, inputs, labels, rows)
    differing = [(label, np.nonzero(a != b)[0].tolist()) for label, a, b in zip(labels, rows, want) if not np.array_equal(a, b)]
    assert not differing, (shape, mode, len(differing), differing[:5])
    ctx.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":
        record(sys.argv[2])
    else:
        sys.exit("usage: python -m tests.test_gpu_pair_rows_recorded --record OUT.npz")
