"""The model-view rule on the CPU (tests/render_util.py, the restatement every GPU test of the views compares against) and the
PNG writer of the rendered TUM directory."""
import numpy as np
import pytest

from badslam_amd import direct_ba as dba
from badslam_amd import png
from tests import render_util as ru

MIN_DEPTH, MAX_DEPTH = 0.05, 50.0


def view_from(global_T_view, step):
    rows, r_max = ru.plane_scene(step)
    out = ru.render32(rows, rows.shape[1], ru.invert(global_T_view), ru.plane_camera(), MIN_DEPTH, MAX_DEPTH, 1.0, 5000.0)
    return out, r_max


def around_plane_point(angle_about_y):
    """The generating camera turned about the plane point (0, 0, 1.5) of its own frame by `angle_about_y`: (3, 4) global_T_view."""
    G = ru.plane_global_T_camera()
    R = ru.rotation([0.0, 1.0, 0.0], angle_about_y)
    centre = ru.PLANE_POINT - R @ ru.PLANE_POINT
    return np.hstack([G[:, :3] @ R, (G[:, :3] @ centre + G[:, 3])[:, None]])


@pytest.mark.parametrize("step", (1, 2, 4))
def test_plane_from_the_generating_pose(step):
    """Every pixel is covered, and the depth is the plane's up to the tilt of a 10-bit normal: a component is off by at most
    1 / 1022 of the quantisation step's unit, the normalised normal by less than 2e-3 rad, and a disc of radius r tilted by
    that much about its centre -- which lies on the plane -- leaves the plane by at most 2e-3 * r."""
    G = ru.plane_global_T_camera()
    out, r_max = view_from(G, step)
    covered = out["keys"] != ru.EMPTY
    t = ru.depth_bits(out["keys"]).view(np.float32).astype(np.float64)
    err = np.abs(t - ru.plane_depth_at_centres(G))[covered]
    print(f"step {step}: coverage {covered.mean():.4f}, max depth error {err.max():.3g} m, bound {2e-3 * r_max:.3g} m, r_max {r_max:.4f} m")
    assert covered.mean() == 1.0
    assert err.max() <= 2e-3 * r_max
    # the views follow the keys
    assert (out["depth"] == (5000.0 * t + 0.5).astype(np.uint16)).mean() > 0.99 and (out["depth"] != 0).all()
    assert (out["index"] < ru.plane_scene(step)[0].shape[1]).all()
    assert np.allclose(np.linalg.norm(out["normal"], axis=-1), 1.0, atol=1e-12)


@pytest.mark.parametrize("step", (1, 2, 4))
def test_plane_from_behind_and_obliquely(step):
    behind, _ = view_from(around_plane_point(np.pi), step)
    assert (behind["keys"] == ru.EMPTY).all()
    assert (behind["depth"] == 0).all() and (behind["index"] == ru.NO_INDEX).all() and (behind["color"] == 0).all() and (behind["normal"] == 0).all()
    V = around_plane_point(0.3)
    oblique, r_max = view_from(V, step)
    covered = oblique["keys"] != ru.EMPTY
    exact = ru.plane_depth_at_centres(V)
    err = np.abs(ru.depth_bits(oblique["keys"]).view(np.float32).astype(np.float64) - exact)[covered]
    print(f"step {step}: oblique coverage {covered.mean():.4f}, max depth error {err.max():.3g} m")
    assert covered.mean() > 0.5
    assert err.max() <= 2e-3 * r_max


def test_nearest_surface_and_index_tie():
    """Two parallel discs: the nearer one wins whatever its index; two coincident discs: the lower index wins, the other is second."""
    cam = ru.plane_camera()
    normal = ru.pack_normals(np.array([[0.0, 0.0, -1.0]] * 4))
    rows = ru.surfel_rows([[0, 0, 2.0], [0, 0, 1.0], [0, 0, 1.0], [0.2, 0, 3.0]], normal, [0.0025] * 4, [1, 2, 3, 4])
    out = ru.render32(rows, 4, np.eye(4)[:3], cam, MIN_DEPTH, MAX_DEPTH, 1.0, 1000.0)
    assert out["index"][24, 32] == 1 and out["depth"][24, 32] == 1000 and (out["second"][24, 32] & np.uint64(0xFFFFFFFF)) == 2
    assert ru.depth_bits(out["keys"])[24, 32] == ru.depth_bits(out["second"])[24, 32]
    assert out["index"][24, 36] == 3 and out["depth"][24, 36] == 3000
    assert set(np.unique(out["index"])) == {1, 3, ru.NO_INDEX}


@pytest.mark.parametrize("kind", ("gray16", "rgb8"))
def test_png_round_trip(tmp_path, kind):
    rng = np.random.default_rng(3)
    if kind == "gray16":
        image = rng.integers(0, 65536, (17, 33)).astype(np.uint16)
        image[0, :3] = [0, 255, 65535]
    else:
        image = rng.integers(0, 256, (17, 33, 3)).astype(np.uint8)
    path = tmp_path / f"{kind}.png"
    png.write_png(path, image)
    back = dba.read_png(path)
    assert back.dtype == image.dtype and np.array_equal(back, image)
    with pytest.raises(ValueError):
        png.encode_png(np.zeros((4, 4), np.float32))
