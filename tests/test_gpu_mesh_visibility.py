"""-m gpu: bslam_mesh_visibility (badslam_amd/csrc/ray_kernels.hpp) against the restatement of tests/mesh_rays_util.py, counts and first
view bit for bit, on a room of two walls with an occluding panel between them; the panel's shadow by similar triangles; and
surface_eval.evaluate(visible_from=...) against the same evaluation on the restatement."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi
from tests import mesh_rays_util as mr
from tests.test_gpu_fusion import SENTINEL, stream_ptr
from tests.test_gpu_mesh_components import Guarded

pytestmark = pytest.mark.gpu
F = np.float32
INVALID_ARGUMENT = -1   # BSLAM_ERR_INVALID_ARGUMENT
SPARE = 5
CAMERA = abi.Camera4f(*mr.ROOM_CAMERA)
SHADOW_CLEARANCE = 0.01   # metres kept from the shadow's outline: six orders of magnitude above the rounding of a segment 4 m long


@pytest.fixture(scope="module")
def gpu():
    import torch
    from badslam_amd import build
    build.build()
    return torch, badslam_amd.lib(), badslam_amd.Context(0)


@pytest.fixture(scope="module")
def scene():
    """The room, its four views and 560 points with normals: on the far wall, on the panel, in front of the near wall (behind three of
    the cameras), floating in the room, and far outside every image."""
    positions, triangles, parts = mr.room()
    rng = np.random.default_rng(5)
    wall = np.stack([rng.uniform(-3, 3, 300), rng.uniform(-2, 2, 300), np.full(300, 4.0)], -1)
    panel = np.stack([rng.uniform(-0.5, 0.5, 60), rng.uniform(-0.5, 0.5, 60), np.full(60, 2.0)], -1)
    behind = np.stack([rng.uniform(-0.3, 0.7, 60), rng.uniform(-0.3, 0.5, 60), np.full(60, -0.6)], -1)
    floating = np.stack([rng.uniform(-3, 3, 100), rng.uniform(-2, 2, 100), rng.uniform(0.02, 3.9, 100)], -1)
    outside = np.stack([rng.uniform(6, 9, 40) * rng.choice([-1, 1], 40), rng.uniform(-2, 2, 40), rng.uniform(0.5, 3.5, 40)], -1)
    points = np.ascontiguousarray(np.concatenate([wall, panel, behind, floating, outside]), F)
    normals = np.concatenate([np.tile([0, 0, -1.0], (360, 1)), np.tile([0, 0, 1.0], (60, 1)), rng.standard_normal((140, 3))])
    views, centres = mr.view_arrays(mr.room_views())
    return dict(positions=positions, triangles=triangles, parts=parts, points=points, normals=np.ascontiguousarray(normals, F), views=views, centres=centres)


def call(gpu, points, normals, positions, triangles, views, centres, min_depth=0.05, max_depth=50.0, margin=0.02, camera=CAMERA, with_first=True):
    """-> (rc, count, first or None, leaves, height); asserts that the inputs, the guard words and the outputs beyond N are untouched."""
    torch, L, ctx = gpu
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    positions, triangles = np.ascontiguousarray(positions, F).reshape(-1, 3), np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    views, centres = np.ascontiguousarray(views, F).reshape(-1, 3, 4), np.ascontiguousarray(centres, F).reshape(-1, 3)
    N, V, T, K = len(points), len(positions), len(triangles), len(views)
    ins = [Guarded(torch, 3 * N, points), Guarded(torch, 3 * V, positions), Guarded(torch, 3 * T, triangles)]
    if normals is not None:
        ins.append(Guarded(torch, 3 * N, np.ascontiguousarray(normals, F)))
    before = [b.read() for b in ins]
    out_count, out_first = Guarded(torch, N + SPARE), Guarded(torch, N + SPARE) if with_first else None
    leaves, height = C.c_uint32(SENTINEL), C.c_uint32(SENTINEL)
    rc = L.bslam_mesh_visibility(ctx.handle, stream_ptr(torch), N, ins[0].ptr, ins[3].ptr if normals is not None else None, V, ins[1].ptr, T, ins[2].ptr, K,
                                 views.ctypes.data if K else None, centres.ctypes.data if K else None, C.byref(camera), float(min_depth), float(max_depth), float(margin),
                                 out_count.ptr, out_first.ptr if with_first else None, C.byref(leaves), C.byref(height))
    for b, was in zip(ins, before):
        assert np.array_equal(b.read(), was), "an input was written to"
    count, first = out_count.read(), out_first.read() if with_first else None
    assert (count[N:] == SENTINEL).all() and (first is None or (first[N:] == SENTINEL).all()), "written beyond N"
    return rc, count[:N], None if first is None else first[:N], leaves.value, height.value


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("limits", [(0.05, 50.0, 0.02), (0.05, 3.0, 0.02), (1.0, 50.0, 8.0), (0.05, 50.0, 0.0)], ids=["typical", "max_depth 3", "margin 8", "margin 0"])
def test_counts_and_first_view_equal_the_restatement(gpu, scene, with_normals, limits):
    s = scene
    normals = s["normals"] if with_normals else None
    want_count, want_first = mr.visibility(s["points"], normals, s["positions"], s["triangles"], s["views"], s["centres"], mr.ROOM_CAMERA, *limits)
    rc, count, first, leaves, height = call(gpu, s["points"], normals, s["positions"], s["triangles"], s["views"], s["centres"], *limits)
    badslam_amd.check(rc)
    assert leaves == len(s["triangles"]) and 0 < height <= 62
    assert np.array_equal(count, want_count), f"{int((count != want_count).sum())} counts differ, first at {np.flatnonzero(count != want_count)[:1]}"
    assert np.array_equal(first, want_first)
    # what the scene is meant to show
    wall, panel, behind, outside = count[:300], count[300:360], count[360:420], count[520:]
    assert (outside == 0).all(), "a point outside every image is seen"
    if limits == (0.05, 50.0, 0.02):
        assert (wall >= 1).all() and (wall == 3).sum() > 20 and (wall < 3).sum() > 100, "every wall point is seen by some camera that looks through, few by all three"
        assert (panel == 3).all() and (behind == 1).all() and (first[360:420] == 3).all(), "the panel faces all three; only the camera that faces away sees behind"
    if limits[1] == 3.0:
        assert (wall == 0).all() and (panel == 3).all(), "the wall is beyond max_depth, the panel is not"
    if limits[2] == 8.0:
        assert (wall == 3).sum() > 300 * 0.6, "a margin beyond the point's distance empties the interval: nothing occludes"


def test_the_panels_shadow(gpu, scene):
    """From the view behind the panel (view 2, at the origin, looking along z): the panel [-0.5, 0.5]^2 at z = 2 shadows [-1, 1]^2 of the
    wall at z = 4, by similar triangles.  Points of the wall closer than SHADOW_CLEARANCE to the outline are left out."""
    s = scene
    centre = s["centres"][2].astype(np.float64)
    x0, x1, y0, y1 = s["parts"]["panel"]["rect"]
    scale = (s["parts"]["far"]["z"] - centre[2]) / (s["parts"]["panel"]["z"] - centre[2])
    shadow = [centre[0] + scale * (x0 - centre[0]), centre[0] + scale * (x1 - centre[0]), centre[1] + scale * (y0 - centre[1]), centre[1] + scale * (y1 - centre[1])]
    assert shadow == [-1.0, 1.0, -1.0, 1.0]
    xs, ys = np.meshgrid(np.linspace(-2.95, 2.95, 60), np.linspace(-1.95, 1.95, 40), indexing="ij")
    wall = np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, 4.0)], -1)
    to_outline = np.maximum(np.abs(wall[:, 0]) - 1.0, np.abs(wall[:, 1]) - 1.0)             # < 0 inside the shadow
    keep = np.abs(to_outline) > SHADOW_CLEARANCE
    wall, to_outline = np.ascontiguousarray(wall[keep], F), to_outline[keep]
    rc, count, first, _, _ = call(gpu, wall, None, s["positions"], s["triangles"], s["views"][2:3], s["centres"][2:3])
    badslam_amd.check(rc)
    assert (to_outline < 0).sum() > 200 and (to_outline > 0).sum() > 1000
    assert (count[to_outline < 0] == 0).all(), "a point in the panel's shadow is seen from behind the panel"
    assert (count[to_outline > 0] == 1).all() and (first[to_outline > 0] == 0).all(), "a point of the wall outside the shadow is not seen"


def test_empty_inputs_and_arguments(gpu, scene):
    s = scene
    L = gpu[1]
    args = (s["positions"], s["triangles"], s["views"], s["centres"])
    rc, count, first, _, _ = call(gpu, s["points"][:50], None, s["positions"], s["triangles"], s["views"][:0], s["centres"][:0])
    assert rc == 0 and (count == 0).all() and (first == mr.NO_VIEW).all()
    rc, count, first, leaves, _ = call(gpu, s["points"][:0], None, *args)
    assert rc == 0 and leaves == len(s["triangles"])
    rc, count, first, leaves, height = call(gpu, s["points"][:50], None, s["positions"], s["triangles"][:0], s["views"], s["centres"])
    want = mr.visibility(s["points"][:50], None, s["positions"], s["triangles"][:0], s["views"], s["centres"], mr.ROOM_CAMERA, 0.05, 50.0, 0.02)
    assert rc == 0 and (leaves, height) == (0, 0) and np.array_equal(count, want[0]) and np.array_equal(first, want[1]) and count.max() == 3
    rc, count, first, _, _ = call(gpu, s["points"][:50], None, *args, with_first=False)
    assert rc == 0 and first is None

    def refused(message, **kw):
        rc, count, first, _, _ = call(gpu, s["points"][:9], None, *args, **kw)
        assert rc == INVALID_ARGUMENT and message in L.bslam_last_error(), (rc, L.bslam_last_error())
        assert (count == SENTINEL).all() and (first == SENTINEL).all(), "outputs touched by a refused call"

    for bad in (dict(min_depth=float("nan")), dict(max_depth=float("inf")), dict(margin=float("inf")), dict(min_depth=-float("inf"))):
        refused(b"must be finite", **bad)
    refused(b"min_depth <= max_depth", min_depth=2.0, max_depth=1.0)
    refused(b"margin must be >= 0", margin=-0.01)
    refused(b"focal lengths must be positive", camera=abi.Camera4f(0.0, 60.0, 64.0, 48.0, 128, 96))
    refused(b"between 1 and 2^31 - 1 pixels", camera=abi.Camera4f(60.0, 60.0, 64.0, 48.0, 0, 96))
    torch, _, ctx = gpu
    out = Guarded(torch, 9)
    rc = L.bslam_mesh_visibility(ctx.handle, stream_ptr(torch), 0, None, None, 0, None, 0, None, 65537, None, None, C.byref(CAMERA), 0.05, 50.0, 0.02, out.ptr, None, None, None)
    assert rc == INVALID_ARGUMENT and b"more than 65536 views" in L.bslam_last_error()


def test_surface_eval_over_the_visible_part(scene):
    from badslam_amd import surface_eval
    from badslam_amd.direct_ba import DirectBA
    s = scene
    ground_truth = dict(positions=s["positions"], triangles=s["triangles"])
    far = s["parts"]["far"]
    v0, v1 = far["vertices"]
    t0, t1 = far["triangles"]
    reconstruction = dict(positions=s["positions"][v0:v1], triangles=s["triangles"][t0:t1] - np.uint32(v0))     # the far wall alone was built
    poses = mr.room_views()[:3]                                                                       # the three cameras that look into the room
    visible_from = dict(poses=poses, camera=CAMERA, margin=0.02)
    ba = DirectBA(1000, 1.0 / 5000.0, 40.0, 4, 0.8, 1, 1, 1, CAMERA, CAMERA, 0, True, False)          # no keyframe: the mesh calls need none
    thresholds = (0.01, 0.05)
    plain = surface_eval.evaluate(ba, reconstruction, ground_truth, max_distance=None, thresholds=thresholds)
    assert set(plain) == {"max_distance", "accuracy", "completeness", "f_scores", "accuracy_tree", "completeness_tree"}, "the result without visible_from changed"
    got = surface_eval.evaluate(ba, reconstruction, ground_truth, max_distance=None, thresholds=thresholds, visible_from=visible_from)
    want = surface_eval.evaluate(mr.RestatementBA(), reconstruction, ground_truth, max_distance=None, thresholds=thresholds, visible_from=visible_from)
    assert set(got) == set(plain) | {"completeness_all", "visibility"}
    assert got["completeness_all"] == plain["completeness"] and got["accuracy"] == plain["accuracy"]
    assert got["visibility"] == want["visibility"] and got["completeness"] == want["completeness"] and got["f_scores"] == want["f_scores"]
    wall, panel, near = v1 - v0, np.subtract(*s["parts"]["panel"]["vertices"][::-1]), np.subtract(*s["parts"]["near"]["vertices"][::-1])
    assert got["visibility"] == dict(views=3, points=wall + panel + near, visible_points=wall + panel, visible_fraction=(wall + panel) / (wall + panel + near),
                                     margin=0.02, min_views=1)
    assert plain["f_scores"][0]["recall"] == wall / (wall + panel + near) < 0.7, "over all vertices the unseen near wall and the panel count against the reconstruction"
    assert got["f_scores"][0]["recall"] == wall / (wall + panel) and got["completeness"]["count"] == wall + panel
    # samples, with their normals: the near wall faces the cameras' backs and stays out, the rest is seen
    sampled = surface_eval.evaluate(ba, reconstruction, ground_truth, max_distance=None, thresholds=thresholds, sample_density=20.0, sample_seed=1, visible_from=visible_from)
    share = sampled["visibility"]["visible_fraction"]
    area = lambda r: (r[1] - r[0]) * (r[3] - r[2])
    expected = (area(far["rect"]) + area(s["parts"]["panel"]["rect"])) / (area(far["rect"]) + area(s["parts"]["panel"]["rect"]) + area(s["parts"]["near"]["rect"]))
    assert abs(share - expected) < 0.05 and sampled["completeness_all"]["count"] == sampled["visibility"]["points"] > 800
    assert sampled["f_scores"][0]["recall"] > plain["f_scores"][0]["recall"] + 0.2
    with pytest.raises(ValueError):
        surface_eval.evaluate(ba, reconstruction, dict(positions=s["positions"]), max_distance=None, visible_from=visible_from)
    # through DirectBA the views are those of the restatement
    seen = ba.MeshVisibility(s["points"], ground_truth, mr.room_views(), camera=CAMERA, normals=s["normals"])
    want_count, want_first = mr.visibility(s["points"], s["normals"], s["positions"], s["triangles"], s["views"], s["centres"], mr.ROOM_CAMERA, 0.05, 50.0, 0.02)
    assert np.array_equal(seen["count"], want_count) and np.array_equal(seen["first"], want_first) and seen["leaves"] == len(s["triangles"])
    ba.close()
