"""The NumPy float32 restatement of the mesh-view rule (tests/render_mesh_util.py) against closed forms and against the properties
the rule promises: these tests pin the restatement that tests/test_gpu_render_mesh.py holds bslam_render_mesh to."""
import numpy as np
import pytest

from tests import render_mesh_util as mu
from tests import render_util as ru

SCALE = 5000.0   # metres_to_depth


@pytest.fixture(scope="module")
def plane_views():
    """The plane as two large triangles and as a 7 x 7 tessellation, seen from the generating pose."""
    cam = ru.plane_camera()
    T = ru.invert(ru.plane_global_T_camera()).astype(np.float32)
    return [mu.render32(mu.plane_mesh(n), T, cam, 0.5, 4.0, 1, SCALE) for n in (1, 7)]


def test_plane_against_the_closed_form(plane_views):
    """Every pixel centre lies inside the outline of both meshes.  The u16 depth is the rounding of a value that perspective-correct
    interpolation over a planar triangle reproduces up to fp32 rounding: within 1 unit of the analytic depth, and of each other."""
    exact = ru.plane_depth_at_centres(ru.plane_global_T_camera()) * SCALE
    coarse, fine = plane_views
    for views in plane_views:
        assert (views["index"] != mu.NO_INDEX).all() and (views["depth"] != 0).all(), "an interior pixel is empty"
        assert np.abs(views["depth"].astype(np.float64) - exact).max() <= 1.0
    assert np.abs(coarse["depth"].astype(np.int64) - fine["depth"].astype(np.int64)).max() <= 1
    assert len(np.unique(coarse["index"])) == 2 and len(np.unique(fine["index"])) > 60
    # the vertex normals are the plane's: so is every pixel's, in the camera frame
    n = ru.PLANE_NORMAL / np.linalg.norm(ru.PLANE_NORMAL)
    assert np.abs(fine["normal"].astype(np.float64) - n).max() <= 1e-6


def test_exact_centres_take_the_lower_id():
    mesh, cam = mu.exact_centre_mesh()
    views = mu.render32(mesh, mu.IDENTITY, cam, 0.5, 4.0, 1, SCALE)
    index = views["index"]
    want = np.full((cam.height, cam.width), mu.NO_INDEX, np.uint32)
    for j in range(2, 15):
        for i in range(2, 15):
            dx, dy = i - 8, j - 8
            owners = [t for t, inside in enumerate((dy <= -abs(dx), dx >= abs(dy), dy >= abs(dx), dx <= -abs(dy))) if inside]   # top, right, bottom, left
            want[j, i] = min(owners)
    assert np.array_equal(index, want)
    assert want[8, 8] == 0 and want[5, 5] == 0 and want[5, 11] == 0 and want[11, 11] == 1 and want[11, 5] == 2   # the shared vertex and the four shared edges
    assert (views["depth"][want != mu.NO_INDEX] == int(SCALE)).all()
    # the vertices themselves carry their own colours, up to the rounding of the weights
    for (i, j), colour in zip(((2, 2), (14, 2), (2, 14), (14, 14), (8, 8)), mesh["colors"]):
        assert np.abs(views["color"][j, i].astype(int) - colour.astype(int)).max() <= 1


def test_coincident_triangles_lower_id_wins():
    mesh, cam = mu.coincident_pair()
    views = mu.render32(mesh, mu.IDENTITY, cam, 0.5, 4.0, 1, SCALE)
    drawn = views["index"] != mu.NO_INDEX
    assert drawn.sum() > 200 and (views["index"][drawn] == 0).all()
    swapped = mu.mesh_dict(mesh["positions"], mesh["triangles"][::-1], None, mesh["colors"])
    again = mu.render32(swapped, mu.IDENTITY, cam, 0.5, 4.0, 1, SCALE)
    assert np.array_equal(again["index"], views["index"]) and np.array_equal(again["depth"], views["depth"]) and np.array_equal(again["color"], views["color"])


def test_opposite_winding_and_the_cull_flag():
    mesh, cam = mu.coincident_pair(reverse_second=True)
    culled = mu.render32(mesh, mu.IDENTITY, cam, 0.5, 4.0, 1, SCALE)
    assert list(culled["passed"]) == [True, False]
    both = mu.render32(mesh, mu.IDENTITY, cam, 0.5, 4.0, 0, SCALE)
    assert list(both["passed"]) == [True, True]
    assert np.array_equal(both["index"], culled["index"]) and (culled["index"] != mu.NO_INDEX).sum() > 200
    # the back-facing one first: culled it is the only one left, id 1; unculled it has the lower id and wins
    flipped = mu.mesh_dict(mesh["positions"], mesh["triangles"][::-1], None, mesh["colors"])
    culled = mu.render32(flipped, mu.IDENTITY, cam, 0.5, 4.0, 1, SCALE)
    both = mu.render32(flipped, mu.IDENTITY, cam, 0.5, 4.0, 0, SCALE)
    drawn = culled["index"] != mu.NO_INDEX
    assert (culled["index"][drawn] == 1).all() and (both["index"][drawn] == 0).all() and np.array_equal(both["depth"], culled["depth"])


def test_colour_is_interpolated_perspective_correctly():
    """Vertices at 0.6 m, 1.5 m and 3 m: at the centroid the perspective-correct weights are 1/z-weighted, (5/8, 1/4, 1/8) against
    the screen-space (1/3, 1/3, 1/3) -- 159 / 64 / 32 against 85 per channel."""
    cam = ru.plane_camera()
    corners = [(8.0, 6.0, 0.6), (58.0, 12.0, 1.5), (24.0, 44.0, 3.0)]
    points = mu.front_facing(cam, corners)
    order = [int(np.argmin(np.abs(points[:, 2] - c[2]))) for c in corners]   # front_facing may have swapped two corners
    colours = np.zeros((3, 4), np.uint8)
    colours[:, 3] = 255
    for k, row in enumerate(order):
        colours[row, k] = 255
    views = mu.render32(mu.mesh_dict(points, [(0, 1, 2)], None, colours), mu.IDENTITY, cam, 0.5, 4.0, 1, SCALE)
    i, j = 29, 20     # the pixel whose centre (29.5, 20.5) is next to the centroid (30, 20.67)
    assert views["index"][j, i] == 0
    p = np.array([c[:2] for c in corners], np.float64)
    z = np.array([c[2] for c in corners], np.float64)
    lam = np.linalg.solve(np.vstack([p.T, np.ones(3)]), np.array([i + 0.5, j + 0.5, 1.0]))
    assert (lam > 0.2).all()
    perspective = 255.0 * (lam / z) / (lam / z).sum()
    linear = 255.0 * lam
    got = views["color"][j, i, :3].astype(np.float64)
    assert np.abs(got - perspective).max() <= 1.0
    assert np.abs(got - linear).min() > 1.0 and np.abs(perspective - linear).min() > 20.0
    assert abs(float(views["depth"][j, i]) - SCALE / (lam / z).sum()) <= 1.0


def test_edge_case_scene_drops_what_the_rule_drops():
    mesh, cam, case = mu.edge_case_scene(0.5, 4.0)
    views = mu.render32(mesh, mu.IDENTITY, cam, 0.5, 4.0, 1, SCALE)
    dropped = [name for name in mu.EDGE_CASES if name not in ("left of the image", "cut by the border")]
    assert not views["passed"][[case[name] for name in dropped]].any()
    assert views["passed"][[0, 1, case["left of the image"], case["cut by the border"], len(mesh["triangles"]) - 1]].all()
    seen = set(np.unique(views["index"]).tolist())
    assert seen == {0, 1, case["cut by the border"], len(mesh["triangles"]) - 1, mu.NO_INDEX}
    assert not views["bad_index"]
