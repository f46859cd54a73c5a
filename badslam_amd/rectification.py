"""ctypes binding of badslam_amd/host/rectification.hpp: the once-per-sensor host side of the sensor rectification.  The radtan
camera model (abi.RadtanCamera) is in the pixel-CENTRE convention of sensor SDKs, abi.Camera4f in the library's pixel-corner
convention; decide_undistorted_camera is where the half pixel is added.  The per-frame kernels are bslam_build_undistortion_map,
bslam_undistort_rgb and bslam_reproject_depth (include/badslam_hip.h); BadSlam.set_sensor_rectification runs them per frame."""
import ctypes as C

import numpy as np

from . import abi
from . import direct_ba as dba


def _lib():
    L = dba.host_lib()
    if not getattr(L, "_rectification_ready", False):
        cam, dp = C.POINTER(abi.RadtanCamera), C.POINTER(C.c_double)
        L.bsh_decide_undistorted_camera.argtypes = [cam, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int)]
        L.bsh_make_unprojection_map.argtypes = [cam, C.POINTER(C.c_float)]
        L.bsh_radtan_points.argtypes = [cam, C.c_int, C.c_int, dp, dp]
        L._rectification_ready = True
    return L


def _check(L, rc):
    if rc < 0:
        raise dba.DirectBAError(L.bsh_last_error().decode())


def radtan_camera(width, height, fx, fy, cx, cy, k1=0.0, k2=0.0, k3=0.0, p1=0.0, p2=0.0):
    return abi.RadtanCamera(width, height, fx, fy, cx, cy, k1, k2, k3, p1, p2)


def decide_undistorted_camera(camera, avoid_invalid_pixels=True):
    """DecideUndistortedCamera: the pinhole abi.Camera4f (pixel-corner) whose image is the undistorted view of `camera`; True keeps
    only pixels that see the raw image, False keeps every raw pixel."""
    L = _lib()
    params, size = (C.c_float * 4)(), (C.c_int * 2)()
    _check(L, L.bsh_decide_undistorted_camera(C.byref(camera), int(avoid_invalid_pixels), params, size))
    return abi.Camera4f(params[0], params[1], params[2], params[3], size[0], size[1])


def make_unprojection_map(camera):
    """MakeUnprojectionMap: (height, width, 2) float32, (x, y) of the unit-z ray through every raw pixel centre."""
    L = _lib()
    out = np.zeros((camera.height, camera.width, 2), np.float32)
    _check(L, L.bsh_make_unprojection_map(C.byref(camera), dba._f(out)))
    return out


def _points(camera, xy, inverse):
    L = _lib()
    pts = np.ascontiguousarray(xy, np.float64)
    out = np.zeros_like(pts)
    _check(L, L.bsh_radtan_points(C.byref(camera), inverse, pts.size // 2, dba._d(pts), dba._d(out)))
    return out


def distort(camera, xy):
    """(..., 2) normalised points through the radtan distortion, in double."""
    return _points(camera, xy, 0)


def undistort(camera, xy):
    """The inverse of distort (Gauss-Newton, at most 100 iterations)."""
    return _points(camera, xy, 1)
