"""-m gpu: the model views (bslam_render_surfels, badslam_amd/csrc/render_kernels.hpp; DirectBA.RenderModel; tools/run_tum.py
--render-dir) against the NumPy float32 restatement of tests/render_util.py: depth, index and colour bit for bit, the normal
view at 1e-6.  Never against the kernel's own output, except where a test is about two calls agreeing.  Surfel counts are no
multiple of 64, surfel rows and images are pitched wider than their content."""
import ctypes as C
import itertools

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi
from tests import render_util as ru

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT = -1   # BSLAM_ERR_INVALID_ARGUMENT
VIEWS = ("depth", "index", "color", "normal")
# per view: NumPy type of the storage, elements per pixel, sentinel
STORAGE = {"depth": (np.int16, 1, 0x5A5A), "index": (np.int32, 1, 0x5A5A5A5A), "color": (np.int32, 1, 0x5A5A5A5A), "normal": (np.float32, 3, -7.0)}
MIN_DEPTH, MAX_DEPTH, SCALE = 0.5, 4.0, 5000.0


@pytest.fixture(scope="module")
def gpu():
    import torch
    from badslam_amd import build
    build.build()
    return torch, badslam_amd.lib(), badslam_amd.Context(0)


# ------------------------------------------------------------------------------------------------
# device plumbing
# ------------------------------------------------------------------------------------------------
def stream_ptr(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def device_rows(torch, rows, pad=5):
    """Surfel rows on the device with `pad` columns of padding per row: (tensor, abi.Buffer2D)."""
    host = np.zeros((rows.shape[0], rows.shape[1] + pad), np.float32)
    host[:, :rows.shape[1]] = rows
    t = torch.from_numpy(host).cuda()
    return t, abi.Buffer2D(t.data_ptr(), t.shape[0], rows.shape[1], t.stride(0) * 4)


def device_view(torch, name, cam, pad=3):
    """A sentinel-filled output image with `pad` elements of padding per row: (tensor, abi.Buffer2D)."""
    dtype, elems, sentinel = STORAGE[name]
    host = np.full((cam.height, elems * cam.width + pad), sentinel, dtype)
    t = torch.from_numpy(host).cuda()
    return t, abi.Buffer2D(t.data_ptr(), cam.height, cam.width, t.stride(0) * t.element_size())


def fetch_view(name, tensor, cam):
    """(image, padding) of an output tensor; the image in the type of the restatement's view."""
    dtype, elems, _ = STORAGE[name]
    host = tensor.cpu().numpy()
    image, padding = np.ascontiguousarray(host[:, :elems * cam.width]), host[:, elems * cam.width:]
    if name == "depth":
        image = image.view(np.uint16)
    elif name == "index":
        image = image.view(np.uint32)
    elif name == "color":
        image = image.view(np.uint8).reshape(cam.height, cam.width, 4)
    else:
        image = image.reshape(cam.height, cam.width, 3)
    return image, padding


def untouched(name, array):
    return bool((array == np.array(STORAGE[name][2], STORAGE[name][0])).all())


def gpu_render(gpu, rows, surfels_size, T, cam, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, radius_scale=1.0, metres_to_depth=SCALE, wanted=VIEWS):
    """bslam_render_surfels into sentinel-filled pitched images; all four are allocated, the wanted ones are passed.  Returns
    {view: image} for the wanted views; asserts that padding and unwanted images keep their sentinel."""
    torch, L, ctx = gpu
    rows_t, rows_b = device_rows(torch, rows)
    images = {name: device_view(torch, name, cam) for name in VIEWS}
    M = ru.mat3x4(T)
    args = [C.byref(images[name][1]) if name in wanted else None for name in VIEWS]
    badslam_amd.check(L.bslam_render_surfels(ctx.handle, stream_ptr(torch), C.byref(M), C.byref(cam), surfels_size, C.byref(rows_b), min_depth, max_depth,
                                             radius_scale, metres_to_depth, *args))
    torch.cuda.synchronize()
    out = {}
    for name in VIEWS:
        image, padding = fetch_view(name, images[name][0], cam)
        assert untouched(name, padding), f"{name}: padding written"
        if name in wanted:
            out[name] = image
        else:
            assert untouched(name, images[name][0].cpu().numpy()), f"{name}: written although not asked for"
    return out


def assert_equal_to_restatement(got, want, label=""):
    for name in ("depth", "index", "color"):
        if name in got:
            differ = got[name] != want[name]
            assert not differ.any(), f"{label}{name}: {int(differ.sum())} values differ, first at {np.argwhere(differ)[0]}"
    if "normal" in got:
        assert np.abs(got["normal"].astype(np.float64) - want["normal"]).max() <= 1e-6


# ------------------------------------------------------------------------------------------------
# scenes (built in the camera's frame, then moved into the global frame by the inverse of the view's pose)
# ------------------------------------------------------------------------------------------------
def view_pose(rng):
    """camera_T_global, (3, 4) float32, and its float64 inverse."""
    T = np.hstack([ru.rotation(rng.normal(size=3), 0.3), rng.uniform(-0.5, 0.5, (3, 1))]).astype(np.float32)
    return T, ru.invert(T)


def to_global(G, points, normals):
    return points @ G[:, :3].T + G[:, 3], normals @ G[:, :3].T


def plane_patch(rng, cam, count, depth, spacing):
    """`count` surfels on a random plane through (0, 0, depth) facing the camera, on a jittered grid around a random image position."""
    n = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), -1.0])
    n /= np.linalg.norm(n)
    side = int(np.ceil(np.sqrt(count)))
    gx, gy = np.meshgrid(np.arange(side), np.arange(side))
    px = rng.uniform(0.2, 0.6) * cam.width + spacing * gx.reshape(-1)[:count] + rng.uniform(-0.3, 0.3, count)
    py = rng.uniform(0.1, 0.5) * cam.height + spacing * gy.reshape(-1)[:count] + rng.uniform(-0.3, 0.3, count)
    rays = np.stack([(px - cam.cx) / cam.fx, (py - cam.cy) / cam.fy, np.ones(count)], -1)
    t = (n[2] * depth) / (rays @ n)
    radius = spacing * t / cam.fx * rng.uniform(0.6, 1.3, count)
    return rays * t[:, None], np.tile(n, (count, 1)), radius


def at_pixel(cam, px, py, depth, radius, normal=(0.0, 0.0, -1.0)):
    """One surfel whose centre projects to the pixel-corner position (px, py)."""
    return np.array([[(px - cam.cx) / cam.fx * depth, (py - cam.cy) / cam.fy * depth, depth]]), np.array([normal], np.float64), np.array([radius])


def mixed_scene(seed=21):
    """2 003 surfels for a 97 x 61 view: three plane patches and every kind of surfel that must not be drawn, or only in part.
    Returns (rows (8, 2003), camera_T_global, camera, the two columns of the coincident pair)."""
    rng = np.random.default_rng(seed)
    cam = abi.Camera4f(70.0, 68.0, 48.3, 30.6, 97, 61)
    T, G = view_pose(rng)
    w, h = cam.width, cam.height
    special = []
    for px, py in ((-40.0, 30.0), (w + 40.0, 30.0), (50.0, -40.0), (50.0, h + 40.0)):       # wholly off each side
        for _ in range(6):
            special.append(at_pixel(cam, px + rng.uniform(-5, 5), py + rng.uniform(-5, 5), rng.uniform(1.0, 3.0), 0.05))
    for px, py in ((-1.0, 20.0), (w + 1.0, 40.0), (30.0, -1.5), (70.0, h + 1.2), (0.2, 0.3), (w - 0.4, h - 0.1)):   # cut by each side, two corners
        for _ in range(5):
            special.append(at_pixel(cam, px + rng.uniform(-0.5, 0.5), py + rng.uniform(-0.5, 0.5), rng.uniform(1.0, 2.0), rng.uniform(0.06, 0.12),
                                    (rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), -1.0)))
    for _ in range(40):                                                                                       # behind the camera
        special.append(at_pixel(cam, rng.uniform(0, w), rng.uniform(0, h), -rng.uniform(0.2, 3.0), 0.05))
    for _ in range(40):                                                # around min_depth, in the left half: some balls cross it, some clear it
        special.append(at_pixel(cam, rng.uniform(8, 40), rng.uniform(10, h - 10), MIN_DEPTH + rng.uniform(0.0, 0.2), rng.uniform(0.01, 0.09)))
    for _ in range(40):                                                                                       # around and beyond max_depth
        special.append(at_pixel(cam, rng.uniform(0, w), rng.uniform(0, h), MAX_DEPTH + rng.uniform(-0.02, 0.5), 0.2))
    for _ in range(60):                                                                                       # back faces, edge-on discs
        special.append(at_pixel(cam, rng.uniform(0, w), rng.uniform(0, h), rng.uniform(0.8, 2.0), 0.08,
                                (rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.choice([1.0, 0.02]))))
    special.append(at_pixel(cam, 72.0, 40.0, 0.62, 0.024))             # nearest of all: it and its copy in the last column coincide
    points = np.concatenate([s[0] for s in special])
    normals = np.concatenate([s[1] for s in special])
    radii = np.concatenate([s[2] for s in special])
    n_patch = 2003 - len(points) - 80 - 1        # 80 copies with NaN x / bad radius below, 1 coincident copy
    sizes = [n_patch // 3, n_patch // 3, n_patch - 2 * (n_patch // 3)]
    for size, depth, spacing in zip(sizes, (1.2, 1.9, 2.8), (1.1, 1.6, 2.3)):
        p, n, r = plane_patch(rng, cam, size, depth, spacing)
        points, normals, radii = np.concatenate([points, p]), np.concatenate([normals, n]), np.concatenate([radii, r])
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    order = rng.permutation(len(points))
    points, normals, radii = points[order], normals[order], radii[order]
    # copies of drawable surfels that must not be drawn: NaN x, r2 = 0, r2 < 0, r2 = NaN
    first_patch = np.nonzero(order >= len(special))[0]
    copies = rng.choice(first_patch, 80, replace=False)
    points, normals, radii = np.concatenate([points, points[copies]]), np.concatenate([normals, normals[copies]]), np.concatenate([radii, radii[copies]])
    # the coincident pair: the last column repeats the nearest surfel
    gp, gn = to_global(G, points, normals)
    twin = int(np.nonzero(order == len(special) - 1)[0][0])
    gp, gn, radii = np.concatenate([gp, gp[twin:twin + 1]]), np.concatenate([gn, gn[twin:twin + 1]]), np.concatenate([radii, radii[twin:twin + 1]])
    count = len(gp)
    assert count == 2003
    colors = rng.integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)
    rows = ru.surfel_rows(gp, ru.pack_normals(gn), radii ** 2, colors)
    bad = np.arange(count - 81, count - 1)
    rows[abi.SURFEL_X, bad[:40]] = np.nan
    rows[abi.SURFEL_RADIUS_SQUARED, bad[40:60]] = 0.0
    rows[abi.SURFEL_RADIUS_SQUARED, bad[60:70]] = -0.01
    rows[abi.SURFEL_RADIUS_SQUARED, bad[70:]] = np.nan
    return rows, T, cam, (twin, count - 1)


def large_splat_scene(seed=33):
    """301 small surfels and 3 whose boxes hold more than 100 x 100 pixel centres of the 160 x 120 view: two in one wave (columns
    5 and 37), one in the second block (column 300).  The large discs are tilted against each other so that each wins somewhere,
    and small surfels lie before, between and behind them."""
    rng = np.random.default_rng(seed)
    cam = abi.Camera4f(120.0, 120.0, 80.4, 59.7, 160, 120)
    T, G = view_pose(rng)
    count = 304
    px, py = rng.uniform(5, 155, count), rng.uniform(5, 115, count)
    depth = rng.uniform(0.3, 1.6, count)
    points = np.stack([(px - cam.cx) / cam.fx * depth, (py - cam.cy) / cam.fy * depth, depth], -1)
    normals = np.stack([rng.uniform(-0.4, 0.4, count), rng.uniform(-0.4, 0.4, count), -np.ones(count)], -1)
    radii = rng.uniform(1.0, 2.5, count) * depth / cam.fx
    for column, centre, normal, radius in ((5, (0.05, 0.0, 0.9), (0.35, 0.1, -1.0), 0.55), (37, (-0.1, 0.05, 0.95), (-0.3, -0.2, -1.0), 0.6),
                                           (300, (0.0, -0.05, 0.9), (0.0, 0.5, -1.0), 0.5)):
        points[column], normals[column], radii[column] = centre, normal, radius
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    gp, gn = to_global(G, points, normals)
    rows = ru.surfel_rows(gp, ru.pack_normals(gn), radii ** 2, rng.integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32))
    return rows, T, cam, (5, 37, 300)


_REFERENCE = {}


def reference(key, make):
    """A restatement result computed once and shared between the tests that need it."""
    if key not in _REFERENCE:
        _REFERENCE[key] = make()
    return _REFERENCE[key]


def mixed_reference(radius_scale):
    rows, T, cam, _ = mixed_scene()
    return reference(("mixed", radius_scale), lambda: ru.render32(rows, rows.shape[1], T, cam, MIN_DEPTH, MAX_DEPTH, radius_scale, SCALE))


# ------------------------------------------------------------------------------------------------
# 1. mixed surfels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius_scale", (1.0, 2.5))
def test_mixed_surfels(gpu, radius_scale):
    rows, T, cam, (twin, copy) = mixed_scene()
    want = mixed_reference(radius_scale)
    covered = want["keys"] != ru.EMPTY
    drawn = np.unique(want["index"][covered])
    print(f"scale {radius_scale}: {covered.mean():.3f} of the pixels covered by {len(drawn)} of {rows.shape[1]} surfels")
    assert 0.2 < covered.mean() < 0.95 and len(drawn) > 300
    for border in (covered[0], covered[-1], covered[:, 0], covered[:, -1]):
        assert border.any(), "the scene must reach every image side"
    # the coincident pair: the lower column wins, the copy is second at the same depth
    assert (want["index"] == twin).any() and not (want["index"] == copy).any()
    at = want["index"] == twin
    assert ((want["second"][at] & np.uint64(0xFFFFFFFF)) == copy).all() and (ru.depth_bits(want["second"][at]) == ru.depth_bits(want["keys"][at])).all()
    got = gpu_render(gpu, rows, rows.shape[1], T, cam, radius_scale=radius_scale)
    assert_equal_to_restatement(got, want, f"scale {radius_scale} ")


# ------------------------------------------------------------------------------------------------
# 2. large splats: the cooperative path
# ------------------------------------------------------------------------------------------------
def test_large_splats(gpu):
    rows, T, cam, large = large_splat_scene()
    want = reference("large", lambda: ru.render32(rows, rows.shape[1], T, cam, 0.1, MAX_DEPTH, 1.0, SCALE))
    for column in large:
        # the ball's projection, (L.x -/+ r) / (L.z -/+ r) and the same in y, spans more than 100 x 100 pixel centres of the image
        L = T.astype(np.float64)[:, :3] @ rows[:3, column].astype(np.float64) + T.astype(np.float64)[:, 3]
        r = np.sqrt(float(rows[abi.SURFEL_RADIUS_SQUARED, column]))
        for axis, f, c, size in ((0, cam.fx, cam.cx, cam.width), (1, cam.fy, cam.cy, cam.height)):
            q = [f * (L[axis] + sr) / (L[2] + sz) + c for sr in (-r, r) for sz in (-r, r)]
            assert min(max(q), size) - max(min(q), 0) > 101
        assert ((want["keys"] != ru.EMPTY) & (want["index"] == column)).sum() > 1000, f"surfel {column} must win many pixels"
    small = np.setdiff1d(np.unique(want["index"]), list(large) + [ru.NO_INDEX])
    assert len(small) > 100
    got = gpu_render(gpu, rows, rows.shape[1], T, cam, min_depth=0.1)
    assert_equal_to_restatement(got, want)


# ------------------------------------------------------------------------------------------------
# 3. order
# ------------------------------------------------------------------------------------------------
def test_order_of_arrival_does_not_matter(gpu):
    rows, T, cam, _ = mixed_scene()
    count = rows.shape[1]
    want = mixed_reference(1.0)
    first = gpu_render(gpu, rows, count, T, cam)
    again = gpu_render(gpu, rows, count, T, cam)
    for name in VIEWS:
        assert np.array_equal(first[name].view(np.uint8), again[name].view(np.uint8)), name
    perm = np.random.default_rng(4).permutation(count)        # new column j holds old column perm[j]
    shuffled = gpu_render(gpu, np.ascontiguousarray(rows[:, perm]), count, T, cam)
    assert np.array_equal(shuffled["depth"], first["depth"])
    covered = want["keys"] != ru.EMPTY
    tie = covered & (ru.depth_bits(want["keys"]) == ru.depth_bits(want["second"]))
    print(f"{int(tie.sum())} of {int(covered.sum())} covered pixels have two best keys of equal depth")
    assert 0 < tie.sum() <= 0.01 * covered.sum()
    assert np.array_equal(shuffled["index"] == ru.NO_INDEX, ~covered)
    mapped = np.where(covered, perm[np.where(covered, shuffled["index"], 0)], ru.NO_INDEX)
    assert np.array_equal(mapped[~tie], want["index"][~tie])


# ------------------------------------------------------------------------------------------------
# 4. outputs and arguments
# ------------------------------------------------------------------------------------------------
def small_scene():
    rows, _ = ru.plane_scene(4)
    return rows, 191, ru.invert(ru.plane_global_T_camera()).astype(np.float32), ru.plane_camera()     # 191 of the 192 surfels


SUBSETS = [s for k in range(1, 5) for s in itertools.combinations(VIEWS, k)]


@pytest.mark.parametrize("wanted", SUBSETS, ids=["+".join(s) for s in SUBSETS])
def test_every_subset_of_the_outputs(gpu, wanted):
    rows, count, T, cam = small_scene()
    want = reference("small", lambda: ru.render32(rows, count, T, cam, 0.05, 50.0, 1.0, SCALE))
    assert 0.9 < (want["keys"] != ru.EMPTY).mean() < 1.0          # the missing surfel leaves a hole
    got = gpu_render(gpu, rows, count, T, cam, min_depth=0.05, max_depth=50.0, wanted=wanted)     # checks the views not asked for
    assert set(got) == set(wanted)
    assert_equal_to_restatement(got, want)


def test_no_surfels_give_empty_views(gpu):
    rows, _, T, cam = small_scene()
    got = gpu_render(gpu, rows, 0, T, cam, min_depth=0.05, max_depth=50.0)
    assert (got["depth"] == 0).all() and (got["index"] == ru.NO_INDEX).all() and (got["color"] == 0).all() and (got["normal"] == 0).all()


ARGUMENT_CASES = ("null_context", "null_camera", "null_pose", "null_surfels", "null_surfel_address", "surfels_size_beyond_the_rows", "too_few_surfel_rows",
                  "depth_of_wrong_size", "normal_of_wrong_size", "normal_with_4_byte_pixels", "depth_pitch_too_small", "index_rows_misaligned",
                  "depth_rows_misaligned", "surfel_rows_misaligned", "outputs_overlap", "output_overlaps_surfels", "fx_zero", "fy_negative", "fx_nan", "fy_infinite",
                  "radius_scale_zero", "radius_scale_nan", "metres_to_depth_zero", "metres_to_depth_infinite", "min_depth_zero", "min_depth_nan",
                  "max_depth_below_min_depth", "max_depth_nan", "too_many_pixels", "all_outputs_null")


@pytest.mark.parametrize("case", ARGUMENT_CASES)
def test_argument_errors(gpu, case):
    torch, L, ctx = gpu
    rows, count, T, cam = small_scene()
    cam = abi.Camera4f(cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height)
    rows_t, rows_b = device_rows(torch, rows)
    images = {name: device_view(torch, name, cam) for name in VIEWS}
    M = ru.mat3x4(T)
    a = dict(ctx=ctx.handle, pose=C.byref(M), cam=C.byref(cam), size=count, rows=C.byref(rows_b), min_depth=0.05, max_depth=50.0, radius_scale=1.0,
             metres_to_depth=SCALE)
    out = {name: C.byref(images[name][1]) for name in VIEWS}
    nan, inf = float("nan"), float("inf")
    if case == "null_context":
        a["ctx"] = None
    elif case == "null_camera":
        a["cam"] = None
    elif case == "null_pose":
        a["pose"] = None
    elif case == "null_surfels":
        a["rows"] = None
    elif case == "null_surfel_address":
        rows_b.address = None
    elif case == "surfels_size_beyond_the_rows":
        a["size"] = rows_b.width + 1
    elif case == "too_few_surfel_rows":
        rows_b.height = abi.SURFEL_COLOR
    elif case == "depth_of_wrong_size":
        images["depth"][1].width -= 1
    elif case == "normal_of_wrong_size":
        images["normal"][1].height += 1
    elif case == "normal_with_4_byte_pixels":
        images["normal"][1].pitch = 4 * cam.width
    elif case == "depth_pitch_too_small":
        images["depth"][1].pitch = 2 * cam.width - 2
    elif case == "index_rows_misaligned":
        images["index"][1].address += 2
    elif case == "depth_rows_misaligned":
        images["depth"][1].pitch += 1
    elif case == "surfel_rows_misaligned":
        rows_b.address += 2
    elif case == "outputs_overlap":
        images["color"][1].address = images["index"][1].address + images["index"][1].pitch * 3
    elif case == "output_overlaps_surfels":
        images["depth"][1].address = rows_b.address + rows_b.pitch * 2
    elif case == "fx_zero":
        cam.fx = 0.0
    elif case == "fy_negative":
        cam.fy = -60.0
    elif case == "fx_nan":
        cam.fx = nan
    elif case == "fy_infinite":
        cam.fy = inf
    elif case == "radius_scale_zero":
        a["radius_scale"] = 0.0
    elif case == "radius_scale_nan":
        a["radius_scale"] = nan
    elif case == "metres_to_depth_zero":
        a["metres_to_depth"] = 0.0
    elif case == "metres_to_depth_infinite":
        a["metres_to_depth"] = inf
    elif case == "min_depth_zero":
        a["min_depth"] = 0.0
    elif case == "min_depth_nan":
        a["min_depth"] = nan
    elif case == "max_depth_below_min_depth":
        a["min_depth"], a["max_depth"] = 1.0, 0.99
    elif case == "max_depth_nan":
        a["max_depth"] = nan
    elif case == "too_many_pixels":            # 2^31 pixels; the images claim that size too, nothing may be touched
        cam.width, cam.height = 65536, 32768
        for name in VIEWS:
            buf = images[name][1]
            buf.width, buf.height, buf.pitch = 65536, 32768, 65536 * 12
    elif case == "all_outputs_null":
        out = {name: None for name in VIEWS}
    rc = L.bslam_render_surfels(a["ctx"], stream_ptr(torch), a["pose"], a["cam"], a["size"], a["rows"], a["min_depth"], a["max_depth"], a["radius_scale"],
                                a["metres_to_depth"], *[out[name] for name in VIEWS])
    torch.cuda.synchronize()
    assert rc == INVALID_ARGUMENT, (case, rc, L.bslam_last_error())
    for name in VIEWS:
        assert untouched(name, images[name][0].cpu().numpy()), f"{case}: {name} written"
    assert np.array_equal(rows_t.cpu().numpy()[:, :rows.shape[1]].view(np.uint32), rows.view(np.uint32))


# ------------------------------------------------------------------------------------------------
# 5. through DirectBA
# ------------------------------------------------------------------------------------------------
def direct_ba_scene():
    """Three keyframes at 160 x 120 (tests/scenes.py: 20 random planes, poses T0 * exp(xi)), one surfel per 2 x 2 pixel cell."""
    from tests import bso, scenes
    cam = bso.make_camera(131.25, 131.25, 80.0, 60.0, 160, 120)
    return scenes.synthetic_scene(3, width=160, height=120, cell=2, camera=cam)


def test_render_model_through_direct_ba(oracle):
    """DirectBA.RenderModel at keyframe 0's pose on surfels the library created (CreateSurfelsForKeyframe) equals the
    restatement applied to the surfel rows it holds; and the view is a plausible image of keyframe 0.  radius_scale 2 because
    the cell size is 2: a surfel's radius is that of one pixel.

    Plausibility bounds: the restatement on the CPU, on the surfels the oracle's creation path (tests/bso.py) makes of the same
    scene -- 6 207 surfels -- covered 1.0000 of the pixels where keyframe 0 has depth (0.943 of the image), with a median
    |rendered - keyframe depth| of 0 raw units (mean 0.31, 99th percentile 1).  Asserted: the share at 0.9 x that = 0.9, the
    median at 2 x that = 0."""
    from badslam_amd.direct_ba import DirectBA
    scene = direct_ba_scene()
    ba = DirectBA(scene.max_surfels, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, 0.8, 1, 1, 1, scene.color_camera, scene.depth_camera, 0,
                  True, False)
    for kf in scene.keyframes:
        ba.AddKeyframe(kf.id, max(kf.min_depth, 1e-3), max(kf.max_depth, 1e-2), kf.depth, kf.normals, kf.radius, kf.color, kf.global_T_frame)
    for kf in scene.keyframes:
        ba.CreateSurfelsForKeyframe(False, kf.id)
    count = ba.surfels_size()
    assert count > 4000 and count % 64 != 0
    rows = ba.GetSurfels(8)
    got = ba.RenderModel(ba.keyframe_pose(0), radius_scale=2.0, views=VIEWS)
    assert got["depth"].shape == (120, 160) and got["color"].shape == (120, 160, 4) and got["normal"].shape == (120, 160, 3)
    want = ru.render32(rows, count, got["camera_T_global"], scene.depth_camera, 0.05, 50.0, 2.0, 1.0 / np.float32(scene.raw_to_float_depth))
    assert_equal_to_restatement(got, want)
    # the default camera is the depth camera; an explicit one gives the same, and a view alone comes alone
    only_depth = ba.RenderModel(ba.keyframe_pose(0), camera=scene.depth_camera, radius_scale=2.0, views=("depth",))
    assert set(only_depth) == {"depth", "camera_T_global"} and np.array_equal(only_depth["depth"], got["depth"])
    keyframe_depth = scene.keyframes[0].depth
    has_depth = (keyframe_depth != 0) & (keyframe_depth < 32768)
    covered = got["depth"] != 0
    share = (covered & has_depth).sum() / has_depth.sum()
    error = np.abs(got["depth"].astype(np.int64) - keyframe_depth.astype(np.int64))[covered & has_depth]
    print(f"{count} surfels: covered share of keyframe 0's depth pixels {share:.4f}, median |rendered - keyframe| {np.median(error)} raw units, mean {error.mean():.2f}")
    assert share >= 0.9 * 1.0
    assert np.median(error) <= 2 * 0
    with pytest.raises(ValueError):
        ba.RenderModel(ba.keyframe_pose(0), views=("depth", "albedo"))
    ba.close()


# ------------------------------------------------------------------------------------------------
# 6. the tool
# ------------------------------------------------------------------------------------------------
def test_run_tum_render_dir(oracle, tmp_path):
    """tools/run_tum.py --render-dir on five frames of the rendered sequence of tests/test_gpu_bad_slam.py (keyframes at
    frames 0 and 4: the shortest run with a second keyframe): the directory loads back through the project's dataset reader,
    and its first depth image is RenderModel at keyframe 0's pose."""
    from badslam_amd import direct_ba as dba
    from badslam_amd import png
    from tests import bso
    from tests.test_gpu_bad_slam import render_sequence
    from tools import run_tum
    n = 5
    cam, raw_to_float, frames, gt = render_sequence(n, seed=5)
    source = tmp_path / "source"
    (source / "rgb").mkdir(parents=True)
    (source / "depth").mkdir()
    assoc = []
    for k, (depth, rgb) in enumerate(frames):
        ts = f"{200.0 + 0.1 * k:.6f}"
        png.write_png(source / "rgb" / f"{ts}.png", rgb)
        png.write_png(source / "depth" / f"{ts}.png", depth)
        assoc.append(f"{ts} rgb/{ts}.png {ts} depth/{ts}.png")
    (source / "associated.txt").write_text("\n".join(assoc) + "\n")
    (source / "calibration.txt").write_text(f"{cam.fx} {cam.fy} {cam.cx - 0.5} {cam.cy - 0.5}\n")
    rendered = tmp_path / "rendered"
    seen = {}

    def inspect(slam, result):
        seen["views"] = slam.ba().RenderModel(slam.ba().keyframe_pose(0), radius_scale=4.0)      # the tool's default: the cell size
        seen["every"] = run_tum.render_keyframes(slam.ba(), result["rendered"], tmp_path / "every", every=2, radius_scale=4.0)

    r = run_tum.run(source, keyframe_interval=4, ba_iterations=2, max_depth=6.0, num_scales=4, max_surfel_count=400000, render_dir=rendered,
                    inspect=inspect)
    assert r["keyframes"] == 2 and [kf for kf, _ in r["rendered"]] == [0, 1]
    ds = dba.read_tum_dataset(rendered, "groundtruth.txt")
    assert (ds["width"], ds["height"]) == (cam.width, cam.height) and len(ds["frames"]) == 2
    assert [f["depth_timestamp"] for f in ds["frames"]] == ["200.000000", "200.400000"]
    depth = dba.read_png(ds["frames"][0]["depth_path"])
    rgb = dba.read_png(ds["frames"][0]["rgb_path"])
    assert depth.dtype == np.uint16 and np.array_equal(depth, seen["views"]["depth"])
    assert np.array_equal(rgb, seen["views"]["color"][:, :, :3])
    assert (depth != 0).mean() > 0.5
    # every second keyframe only
    assert [kf for kf, _ in seen["every"]] == [0] and len(dba.read_tum_dataset(tmp_path / "every")["frames"]) == 1
