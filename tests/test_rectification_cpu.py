"""The once-per-sensor host side of the sensor rectification (badslam_amd/host/rectification.hpp) through the host library's C
API, which loads without a device: the radtan inverse, the choice of the undistorted camera and the unprojection map, against
the NumPy float64 model of tests/rectify_util.py.

The two distortion profiles are a strong barrel (k1 = -0.25, k2 = +0.07) and a pincushion (k1 = +0.25, k2 = -0.07) with small
tangential terms on a 67 x 45 camera of focal length 60: the image corners lie at a normalised radius of 0.67.  The distortion is
invertible there: the radial factor d(r (1 + k1 r^2 + k2 r^4)) / dr = 1 + 3 k1 r^2 + 5 k2 r^4 stays positive up to r = 0.75
(barrel: 1 - 0.42 + 0.11 = 0.69, pincushion: 1 + 0.42 - 0.11 = 1.31) -- checked on the grid by test_profiles_are_invertible."""
import numpy as np
import pytest

from badslam_amd import build
from badslam_amd import rectification as rect
from tests import rectify_util as ru

PROFILES = {"barrel": (-0.25, 0.07, 0.0, 1e-3, -7e-4), "pincushion": (0.25, -0.07, 0.0, -8e-4, 1.1e-3)}
W, H = 67, 45


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()


def camera(profile, width=W, height=H):
    return rect.radtan_camera(width, height, 60.0, 61.0, 33.2, 21.7, *PROFILES[profile])


def normalised_grid(cam, nx=14, ny=10):
    """Distorted normalised coordinates of a grid of raw pixel positions that includes the four corners."""
    xs, ys = np.meshgrid(np.linspace(0, cam.width - 1, nx), np.linspace(0, cam.height - 1, ny))
    return np.stack([(xs - cam.cx) / cam.fx, (ys - cam.cy) / cam.fy], -1)


@pytest.mark.parametrize("profile", sorted(PROFILES))
def test_profiles_are_invertible(profile):
    """The Jacobian determinant of the forward model is positive on every undistorted point the image needs."""
    cam = camera(profile)
    x, y = ru.undistort64(cam, *np.moveaxis(normalised_grid(cam, 40, 30), -1, 0))
    eps = 1e-6
    jac = np.array([[(np.array(ru.distort64(cam, x + eps * (a == 0), y + eps * (a == 1))[b]) - np.array(ru.distort64(cam, x, y)[b])) / eps
                     for a in range(2)] for b in range(2)])
    det = jac[0, 0] * jac[1, 1] - jac[0, 1] * jac[1, 0]
    assert det.min() > 0.3, det.min()


def test_zero_distortion_keeps_the_camera_up_to_the_half_pixel():
    cam = rect.radtan_camera(W, H, 60.0, 61.0, 33.2, 21.7)
    for avoid in (True, False):
        out = rect.decide_undistorted_camera(cam, avoid)
        assert (out.width, out.height) == (W, H)
        assert out.fx == cam.fx and out.fy == cam.fy
        assert out.cx == np.float32(cam.cx) + np.float32(0.5) and out.cy == np.float32(cam.cy) + np.float32(0.5)


@pytest.mark.parametrize("profile", sorted(PROFILES))
def test_distort_of_undistort_is_the_identity(profile):
    cam = camera(profile)
    d = normalised_grid(cam)
    u = rect.undistort(cam, d)
    assert np.abs(rect.distort(cam, u) - d).max() <= 1e-9
    # and the library's forward model is the NumPy one
    assert np.abs(np.stack(ru.distort64(cam, u[..., 0], u[..., 1]), -1) - rect.distort(cam, u)).max() <= 1e-14


@pytest.mark.parametrize("profile", sorted(PROFILES))
def test_avoiding_invalid_pixels_keeps_every_target_pixel_inside_the_source(profile):
    cam = camera(profile)
    target = rect.decide_undistorted_camera(cam, True)
    assert target.width >= 8 and target.height >= 8
    xs, ys = ru.pixel_grid(target.width, target.height)
    px, py = ru.source_position64(cam, target, xs, ys)
    # strictly inside the image area, whose pixel-centre coordinates span (-0.5, w - 0.5) ...
    assert px.min() > -0.5 and px.max() < cam.width - 0.5 and py.min() > -0.5 and py.max() < cam.height - 0.5
    # ... and inside the rectangle of the pixel centres, where the bilinear interpolation has its four texels, up to the fp32
    # rounding of the target's cx, cy (values below 64: half an ulp is 2e-6 pixels)
    slack = 1e-5
    assert px.min() >= -slack and px.max() <= cam.width - 1 + slack and py.min() >= -slack and py.max() <= cam.height - 1 + slack
    # the bounds are tight: the first column and row touch the source's, and one more column or row would leave the source
    assert px.min() < 0.05 and py.min() < 0.05
    more_x, more_y = ru.source_position64(cam, target, *ru.pixel_grid(target.width + 1, target.height + 1))
    assert more_x.max() > cam.width - 1 and more_y.max() > cam.height - 1


@pytest.mark.parametrize("profile", sorted(PROFILES))
def test_keeping_every_pixel_maps_the_source_border_inside_the_target(profile):
    cam = camera(profile)
    target = rect.decide_undistorted_camera(cam, False)
    xs, ys = ru.pixel_grid(cam.width, cam.height)
    border = (xs == 0) | (ys == 0) | (xs == cam.width - 1) | (ys == cam.height - 1)
    nx, ny = ru.undistort64(cam, (xs[border] - cam.cx) / cam.fx, (ys[border] - cam.cy) / cam.fy)
    tx, ty = target.fx * nx + target.cx, target.fy * ny + target.cy      # pixel-corner coordinates: the image is [0, w] x [0, h]
    assert tx.min() > 0 and tx.max() < target.width and ty.min() > 0 and ty.max() < target.height
    # even inside the rectangle of the target's pixel centres, up to the fp32 rounding of its cx, cy
    assert tx.max() <= target.width - 0.5 + 1e-5 and ty.max() <= target.height - 0.5 + 1e-5
    # the first pixel centre sits on the lowest border point
    assert abs(tx.min() - 0.5) < 1e-4 and abs(ty.min() - 0.5) < 1e-4


@pytest.mark.parametrize("profile", sorted(PROFILES))
def test_unprojection_map_equals_the_float64_restatement(profile):
    cam = camera(profile)
    got = rect.make_unprojection_map(cam)
    assert got.shape == (H, W, 2) and got.dtype == np.float32
    assert np.abs(got.astype(np.float64) - ru.unprojection_map64(cam)).max() <= 1e-6


def test_bad_cameras_are_rejected():
    from badslam_amd import direct_ba as dba
    with pytest.raises(dba.DirectBAError):
        rect.decide_undistorted_camera(rect.radtan_camera(1, 45, 60.0, 61.0, 0.0, 21.7))
    with pytest.raises(dba.DirectBAError):
        rect.make_unprojection_map(rect.radtan_camera(67, 45, 0.0, 61.0, 33.2, 21.7))
