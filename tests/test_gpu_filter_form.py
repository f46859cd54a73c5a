"""-m gpu: the kernels that end in descriptor_samples_finish, bit for bit against arrays recorded before the bilinear value got one
form for both texture modes (tests/golden/filter_form.npz; device_math.hpp: bilinear_top / bilinear_inner_* / bilinear_value).

The stack: 6 keyframes of 64 x 48 pixels and 700 surfels -- three granules of 256, the last one partly filled -- one of them with a
NaN position (the mark of a deleted surfel).  The keyframe poses are shifted off the poses the images were rendered at, and the
surfels of the image's outermost cells carry tangent sample points two pixels away, so some samples fall in the half-pixel border
strip (the gradient reads another quad than the value) and some tangent samples fall outside the image (clamp addressing); the file
holds the census (`census`: samples in the strip, tangent samples outside) and the test asks for both to be there.

For both texture modes, compared as uint32 words with what the parent build gave:
  * one photometric geometry iteration (the eight data rows of the surfel buffer);
  * the rows of bslam_accumulate_pose_coeffs_batched with depth + descriptor and with descriptor residuals only;
  * H, b, cost and residual count of every keyframe through the per-keyframe entry point with `debug` set (the kernels' `cost`
    variant), for the same two residual sets;
  * the vectors r, M, g, p and the three scalars after PCGInit, PCGInit2 and PCGStep1.
The pose and PCG calls read the RECORDED surfel rows of the geometry iteration (descriptors fitted), so that one kernel's
difference shows in its own comparison only.

The file holds the inputs next to the results, so nothing is rendered here.  Recording, with the library of the checkout it runs
in (BSLAM_HIP_LIB as usual): `BSLAM_RECORD_FILTER_FORM=OUT.npz python -m tests.test_gpu_filter_form`; public entry points only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi, synthetic

pytestmark = pytest.mark.gpu
P = C.POINTER
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filter_form.npz")
RECORD_ENV = "BSLAM_RECORD_FILTER_FORM"
K, W, H, CELL, S = 6, 64, 48, 4, 700
NAN_SURFEL = 389
FX, FY, CX, CY = 60.0, 60.0, 32.0, 24.0
RAW_TO_FLOAT, BASELINE_FX = 1.0 / 5000, 40.0
MODES = {"fixed": abi.TEX_FIXED_POINT_1_8, "exact": abi.TEX_EXACT_FLOAT}
RESIDUAL_SETS = {"both": (1, 1), "desc": (0, 1)}
DATA_ROWS = abi.SURFEL_DATA_ATTRIBUTE_COUNT
INPUT_KEYS = ("depth", "normals", "radius", "luma", "surfels", "frame_T_global", "global_R_frame")
GAUGE = 3
N_POSE, N_UNKNOWNS = 6 * (K - 1), 6 * (K - 1) + 3 * S


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the fixture's inputs (recording only) ---------------------------------------------------------------------------
def make_inputs():
    """depth, normals, radius u16 [K, H, W], luma u8 [K, H, W], surfels f32 [8, S] (descriptors 0), the shifted poses as
    frame_T_global f32 [K, 12] and global_R_frame f32 [K, 9], and the census of the border cases."""
    stack = synthetic.SyntheticStack(K, width=W, height=H, cell=CELL, seed=20261020, fx=FX, fy=FY, cx=CX, cy=CY, raw_to_float_depth=RAW_TO_FLOAT,
                                     baseline_fx=BASELINE_FX, translation_range=0.12, rotation_range=0.06, kind="dense")
    assert stack.surfels_size >= S + 64, stack.surfels_size
    # surfels of every keyframe: every other column of the stack's list (it is ordered by keyframe)
    pick = np.linspace(0, stack.surfels_size - 1, S).astype(np.int64)
    surfels = np.ascontiguousarray(stack.surfels[:DATA_ROWS, pick])
    surfels[0, NAN_SURFEL] = np.nan
    rng = np.random.default_rng(41)
    Ms, Rgs = [], []
    for k in range(K):
        xi = np.concatenate([rng.uniform(-1, 1, 3) * 0.02, rng.uniform(-1, 1, 3) * 0.008])       # up to about half a pixel each
        _, M, Rg = stack.pose(k, xi)
        Ms.append(np.array(list(M.m), np.float32))
        Rgs.append(np.array(list(Rg.m), np.float32))
    inputs = {"depth": stack.depth, "normals": stack.normals, "radius": stack.radius, "luma": np.ascontiguousarray(stack.color[..., 3]),
              "surfels": surfels, "frame_T_global": np.stack(Ms), "global_R_frame": np.stack(Rgs)}
    assert (stack.color == stack.color[..., 3:4]).all()
    return inputs, census(inputs)


def census(inputs):
    """(samples whose 2x2 footprint touches the image border while the sample lies inside the image, tangent samples outside the
    image), over the (surfel, keyframe) pairs whose centre projects onto a pixel with a depth measurement near the surfel's: a
    float64 estimate of what the kernels meet, good enough to say that both cases occur."""
    s = inputs["surfels"].astype(np.float64)
    keep = np.isfinite(s[0])
    p = s[0:3, keep].T
    packed = inputs["surfels"][3, keep].view(np.uint32).astype(np.int64)
    n = np.stack([(((packed >> sh) & 0x3FF) ^ 0x200) - 0x200 for sh in (0, 10, 20)], 1) / 511.0
    axis = np.where((np.abs(n[:, 0]) > 0.9)[:, None], [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    length = 2 * np.sqrt(s[4, keep])[:, None]
    t1 = np.cross(n, axis)
    t1 *= length / np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(n, t1)
    t2 *= length / np.linalg.norm(t2, axis=1, keepdims=True)
    strip = outside = 0
    for k in range(K):
        T = inputs["frame_T_global"][k].astype(np.float64).reshape(3, 4)

        def project(q):
            l = q @ T[:, :3].T + T[:, 3]
            z = np.where(l[:, 2] > 0, l[:, 2], np.nan)
            return FX * l[:, 0] / z + CX, FY * l[:, 1] / z + CY, z

        x, y, z = project(p)
        with np.errstate(invalid="ignore"):
            inside = (x >= 0) & (y >= 0) & (x < W) & (y < H)
        px, py = np.where(inside, x, 0).astype(np.int64), np.where(inside, y, 0).astype(np.int64)
        raw = inputs["depth"][k][py, px]
        seen = inside & (raw < 32768) & (np.abs(raw * RAW_TO_FLOAT - z) < 0.05)
        for centre, (sx, sy, _) in ((True, (x, y, z)), (False, project(p + t1)), (False, project(p + t2))):
            with np.errstate(invalid="ignore"):
                out = seen & ~((sx >= 0) & (sy >= 0) & (sx < W) & (sy < H))
                bx, by = np.floor(sx - 0.5), np.floor(sy - 0.5)
                edge = seen & ~out & ~((bx >= 0) & (bx <= W - 2) & (by >= 0) & (by <= H - 2))
            strip += int(edge.sum())
            outside += 0 if centre else int(out.sum())
    return np.array([strip, outside], np.int64)


# ---- running the entry points ----------------------------------------------------------------------------------------
class _Host:
    """What synthetic.DeviceStack reads of a stack, from the recorded arrays."""

    def __init__(self, inputs, surfels):
        self.K, self.cell = K, CELL
        self.camera = abi.Camera4f(FX, FY, CX, CY, W, H)
        self.raw_to_float_depth, self.baseline_fx = np.float32(RAW_TO_FLOAT), BASELINE_FX
        self.depth, self.normals, self.radius = inputs["depth"], inputs["normals"], inputs["radius"]
        self.color = np.ascontiguousarray(np.repeat(inputs["luma"][..., None], 4, axis=3))
        self.surfels = np.zeros((abi.SURFEL_ATTRIBUTE_COUNT, S), np.float32)
        self.surfels[:DATA_ROWS] = surfels
        self.surfels_size = S
        self.cfactor = np.zeros(((H - 1) // CELL + 1, (W - 1) // CELL + 1), np.float32)
        self._M, self._Rg = inputs["frame_T_global"], inputs["global_R_frame"]

    def pose(self, k, xi=None):
        M, Rg = abi.Mat3x4(), abi.Mat3x3()
        M.m[:] = [float(v) for v in self._M[k]]
        Rg.m[:] = [float(v) for v in self._Rg[k]]
        return None, M, Rg


def _fp(a):
    return a.ctypes.data_as(P(C.c_float))


def run_geometry(torch, L, ctx, inputs):
    """The data rows of the surfel buffer after one photometric geometry iteration on the input surfels."""
    dev = synthetic.DeviceStack(_Host(inputs, inputs["surfels"]), "cuda:0")
    kfs, cam, dp = dev.keyframe_views(), dev.stack.camera, dev.depth_params()
    sb, ab = dev.buf(dev.surfels), dev.buf(dev.active)
    badslam_amd.check(L.bslam_optimize_geometry_iteration(ctx.handle, C.c_void_p(None), 1, 1, C.byref(cam), C.byref(cam), C.byref(dp), K, kfs, S, C.byref(sb), C.byref(ab)))
    torch.cuda.synchronize()
    return bits(dev.surfels[:DATA_ROWS].cpu().numpy())


def run_pose_and_pcg(torch, L, ctx, inputs, surfel_rows):
    """The pose rows (batched and per keyframe with cost) and the PCG vectors on the given surfel rows -> {name: uint32 array}."""
    dev = synthetic.DeviceStack(_Host(inputs, surfel_rows.view(np.float32)), "cuda:0")
    kfs, cam, dp, sb = dev.keyframe_views(), dev.stack.camera, dev.depth_params(), dev.buf(dev.surfels)
    stream = C.c_void_p(None)
    out = {}
    for name, use in RESIDUAL_SETS.items():
        Hb, counts = np.zeros((K, 27), np.float32), np.zeros(K, np.uint32)
        badslam_amd.check(L.bslam_accumulate_pose_coeffs_batched(ctx.handle, stream, use[0], use[1], C.byref(cam), C.byref(cam), C.byref(dp), K, kfs, S, C.byref(sb),
                                                                 _fp(Hb), counts.ctypes.data_as(P(C.c_uint32))))
        out[f"batched/{name}/Hb"], out[f"batched/{name}/counts"] = bits(Hb), counts
        rows = np.zeros((K, 29), np.uint32)                 # 21 H, 6 b, cost, residual count
        for k in range(K):
            Hk, bk, count, cost = np.zeros(21, np.float32), np.zeros(6, np.float32), C.c_uint32(), C.c_float()
            v = kfs[k]
            badslam_amd.check(L.bslam_accumulate_pose_estimation_coeffs(ctx.handle, stream, use[0], use[1], C.byref(cam), C.byref(cam), C.byref(dp), C.byref(v.depth),
                                                                        C.byref(v.normals), C.byref(v.color), C.byref(v.frame_T_global), S, C.byref(sb), 1,
                                                                        C.byref(count), C.byref(cost), _fp(Hk), _fp(bk)))
            rows[k, 0:21], rows[k, 21:27] = bits(Hk), bits(bk)
            rows[k, 27], rows[k, 28] = bits(np.array([cost.value], np.float32))[0], count.value
        out[f"keyframe/{name}/rows"] = rows
    layout = abi.PCGLayout(N_UNKNOWNS, N_POSE, abi.INVALID_INDEX, abi.INVALID_INDEX, abi.INVALID_INDEX, GAUGE, 1, 1, 0, 0, 1, 1)
    vec = {nm: torch.full((N_UNKNOWNS,), 123.0, dtype=torch.float32, device="cuda:0") for nm in ("r", "M", "delta", "g", "p")}
    scal = torch.full((3,), 7.0, dtype=torch.float32, device="cuda:0")
    v = abi.PCGVectors()
    for nm, t in vec.items():
        setattr(v, nm, t.data_ptr())
    v.alpha_n, v.alpha_d, v.beta_n = scal.data_ptr(), scal.data_ptr() + 4, scal.data_ptr() + 8
    badslam_amd.check(L.bslam_pcg_init(ctx.handle, stream, C.byref(layout), C.byref(cam), C.byref(cam), C.byref(dp), K, kfs, S, C.byref(sb), C.byref(v)))
    badslam_amd.check(L.bslam_pcg_init2(ctx.handle, stream, C.byref(layout), 0.0, C.byref(v)))
    badslam_amd.check(L.bslam_pcg_step1(ctx.handle, stream, C.byref(layout), C.byref(cam), C.byref(cam), C.byref(dp), K, kfs, S, C.byref(sb), C.byref(v), 1))
    torch.cuda.synchronize()
    for nm in ("r", "M", "g", "p"):
        out[f"pcg/{nm}"] = bits(vec[nm].cpu().numpy())
    out["pcg/scalars"] = bits(scal.cpu().numpy())
    return out


def check_fixture(inputs, census_counts, results):
    """What holds of any recording: the shapes the module's text promises, both border cases present, every keyframe with residuals
    of both kinds, and results that are numbers."""
    assert inputs["surfels"].shape == (DATA_ROWS, S) and S > 2 * 256 and S % 256 != 0
    assert np.isnan(inputs["surfels"][0, NAN_SURFEL]) and np.isfinite(np.delete(inputs["surfels"][0], NAN_SURFEL)).all()
    assert inputs["depth"].shape == (K, H, W)
    assert census_counts[0] >= 20 and census_counts[1] >= 20, census_counts
    for mode in MODES:
        r = results[mode]
        assert r["batched/both/counts"].min() >= 200 and r["batched/desc/counts"].min() >= 100, (r["batched/both/counts"], r["batched/desc/counts"])
        for key, value in r.items():
            if value.dtype == np.uint32 and not key.endswith("counts"):
                floats = value.view(np.float32) if "rows" not in key else value[:, :28].view(np.float32)
                if key == "geometry":                     # position, radius, descriptors (the other rows are packed words)
                    floats = np.delete(floats[[0, 1, 2, 4, 6, 7]], NAN_SURFEL, axis=1)
                assert np.isfinite(floats).all(), (mode, key)
    assert not np.array_equal(results["fixed"]["geometry"], results["exact"]["geometry"])          # the two filters ran
    assert not np.array_equal(results["fixed"]["batched/both/Hb"], results["exact"]["batched/both/Hb"])


def record(path):
    import torch
    L = badslam_amd.lib()
    inputs, counts = make_inputs()
    out = dict(inputs, census=counts)
    results = {}
    for mode_name, mode in MODES.items():
        ctx = badslam_amd.Context(0)
        ctx.set_texture_mode(mode)
        r = {"geometry": run_geometry(torch, L, ctx, inputs)}
        r.update(run_pose_and_pcg(torch, L, ctx, inputs, r["geometry"]))
        ctx.close()
        results[mode_name] = r
        for key, value in r.items():
            out[f"{mode_name}/{key}"] = value
        print(mode_name, "residuals per keyframe", r["batched/both/counts"].tolist(), "descriptor only", r["batched/desc/counts"].tolist())
    check_fixture(inputs, counts, results)
    np.savez_compressed(path, **out)
    print("census (border strip, tangent samples outside)", counts.tolist(), "; wrote", path, os.path.getsize(path), "bytes")


# ---- the test ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN) as f:
        return {key: f[key] for key in f.files}


def results_of(recorded, mode):
    return {key[len(mode) + 1:]: value for key, value in recorded.items() if key.startswith(mode + "/")}


def test_the_recording_holds_the_cases_it_promises(recorded):
    inputs = {key: recorded[key] for key in INPUT_KEYS}
    assert np.array_equal(census(inputs), recorded["census"])
    check_fixture(inputs, recorded["census"], {mode: results_of(recorded, mode) for mode in MODES})


@pytest.mark.parametrize("mode", list(MODES))
def test_geometry_iteration_equals_the_recorded_rows_bit_for_bit(recorded, mode):
    import torch
    L, ctx = badslam_amd.lib(), badslam_amd.Context(0)
    ctx.set_texture_mode(MODES[mode])
    got = run_geometry(torch, L, ctx, {key: recorded[key] for key in INPUT_KEYS})
    ctx.close()
    want = recorded[f"{mode}/geometry"]
    assert got.dtype == want.dtype == np.uint32 and got.shape == want.shape
    assert np.array_equal(got, want), (mode, np.argwhere(got != want)[:5].tolist())


@pytest.mark.parametrize("mode", list(MODES))
def test_pose_rows_and_pcg_vectors_equal_the_recorded_ones_bit_for_bit(recorded, mode):
    import torch
    L, ctx = badslam_amd.lib(), badslam_amd.Context(0)
    ctx.set_texture_mode(MODES[mode])
    got = run_pose_and_pcg(torch, L, ctx, {key: recorded[key] for key in INPUT_KEYS}, recorded[f"{mode}/geometry"])
    ctx.close()
    want = results_of(recorded, mode)
    assert sorted(got) == sorted(k for k in want if k != "geometry")
    differing = {}
    for key, value in got.items():
        assert value.dtype == want[key].dtype == np.uint32 and value.shape == want[key].shape, key
        if not np.array_equal(value, want[key]):
            differing[key] = np.argwhere(value != want[key])[:5].tolist()
    assert not differing, (mode, differing)


if __name__ == "__main__":
    if not os.environ.get(RECORD_ENV):
        sys.exit(f"usage: {RECORD_ENV}=OUT.npz python -m tests.test_gpu_filter_form")
    record(os.environ[RECORD_ENV])
