"""ctypes binding of bslam_host::BadSlam (badslam_amd/host/bad_slam.hpp): the sequential front end of the reference's
vis::BadSlam (BS/bad_slam.cc) -- preprocessing, pairwise odometry with the constant-motion estimates, keyframe
scheduling and the planned bundle-adjustment iterations -- without threads, GUI and loop detection."""
import ctypes as C

import numpy as np

from . import direct_ba as dba


class BadSlam:
    def __init__(self, color_camera, depth_camera, keyframe_interval=10, max_num_ba_iterations_per_keyframe=10, num_scales=5,
                 max_surfel_count=25 * 1000 * 1000, sparse_surfel_cell_size=4, use_motion_model=True, use_geometric_residuals=True,
                 use_photometric_residuals=True, do_surfel_updates=True, use_pcg=False, optimize_intrinsics=False, disable_deactivation=False,
                 start_frame=0, raw_to_float_depth=1.0 / 5000, max_depth=3.0, baseline_fx=40.0, device=0, pyramid_level_for_depth=0,
                 pyramid_level_for_color=0, median_filter_and_densify_iterations=0):
        """Keyword defaults = BS/bad_slam_config.h.  The cameras are those of the pyramid levels in use (already scaled);
        ProcessFrame takes the full-resolution images, (width << level, height << level) per stream."""
        self.L = dba.host_lib()
        L = self.L
        f32p = C.POINTER(C.c_float)
        L.bsh_slam_create.restype = C.c_void_p
        L.bsh_slam_create.argtypes = [C.POINTER(C.c_int), f32p, C.c_int, C.c_int, f32p, C.c_int, C.c_int, f32p, C.c_int]
        L.bsh_slam_destroy.argtypes = [C.c_void_p]
        L.bsh_slam_direct_ba.restype = C.c_void_p
        L.bsh_slam_direct_ba.argtypes = [C.c_void_p]
        L.bsh_slam_process_frame.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint16), C.POINTER(C.c_uint8), C.c_int]
        L.bsh_slam_preprocess_frame.argtypes = [C.c_void_p, C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)]
        L.bsh_slam_run_bundle_adjustment.argtypes = [C.c_void_p] + [C.c_int] * 10 + [C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.bsh_slam_frame_count.argtypes = [C.c_void_p]
        L.bsh_slam_get_frame_poses.argtypes = [C.c_void_p, f32p, C.c_int]
        L.bsh_slam_state.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        cfg = (C.c_int * 16)(keyframe_interval, max_num_ba_iterations_per_keyframe, num_scales, max_surfel_count, sparse_surfel_cell_size,
                             int(use_motion_model), int(use_geometric_residuals), int(use_photometric_residuals), int(do_surfel_updates), int(use_pcg),
                             int(optimize_intrinsics), int(disable_deactivation), start_frame, pyramid_level_for_depth, pyramid_level_for_color,
                             median_filter_and_densify_iterations)
        fcfg = (C.c_float * 3)(raw_to_float_depth, max_depth, baseline_fx)
        cc = np.array([color_camera.fx, color_camera.fy, color_camera.cx, color_camera.cy], np.float32)
        dc = np.array([depth_camera.fx, depth_camera.fy, depth_camera.cx, depth_camera.cy], np.float32)
        self._slam = L.bsh_slam_create(cfg, fcfg, color_camera.width, color_camera.height, dba._f(cc), depth_camera.width, depth_camera.height,
                                       dba._f(dc), device)
        if not self._slam:
            raise dba.DirectBAError(L.bsh_last_error().decode())
        # non-owning view of the DirectBA inside
        self.direct_ba = dba.DirectBA.__new__(dba.DirectBA)
        self.direct_ba.L = L
        self.direct_ba._ba = None                       # close() / __del__ of the view must not destroy it
        self.direct_ba.stream = C.c_void_p(None)
        self.direct_ba.close = lambda: None             # instance attribute: shadows DirectBA.close for this view only
        self._ba_ptr = L.bsh_slam_direct_ba(self._slam)
        # what ProcessFrame reads from the host: the full-resolution frame of each stream
        self._depth_shape = (depth_camera.height << pyramid_level_for_depth, depth_camera.width << pyramid_level_for_depth)
        self._rgb_shape = (color_camera.height << pyramid_level_for_color, color_camera.width << pyramid_level_for_color, 3)
        self._plain_shapes = (self._depth_shape, self._rgb_shape)
        self._num_scales = num_scales

    def ba(self):
        """The DirectBA of this BadSlam (valid while the BadSlam object lives)."""
        view = self.direct_ba
        view._ba = self._ba_ptr
        return _BorrowedBA(view, self)

    def _check(self, rc):
        if rc < 0:
            raise dba.DirectBAError(self.L.bsh_last_error().decode())
        return rc

    def close(self):
        if self._slam:
            self.direct_ba._ba = None
            self.L.bsh_slam_destroy(self._slam)
            self._slam = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _frame(self, depth_u16, rgb_u8):
        """The two host images, contiguous and of the sizes the native side reads (camera size << pyramid level)."""
        d = np.ascontiguousarray(depth_u16, np.uint16)
        rgb = np.ascontiguousarray(rgb_u8, np.uint8)
        if d.shape != self._depth_shape or rgb.size != int(np.prod(self._rgb_shape)) or rgb.shape[0] != self._rgb_shape[0]:
            raise ValueError(f"frame of depth {d.shape} / rgb {rgb.shape}: expected the full-resolution images {self._depth_shape} / {self._rgb_shape}")
        return d, rgb

    def ProcessFrame(self, frame_index, depth_u16, rgb_u8, force_keyframe=False):
        d, rgb = self._frame(depth_u16, rgb_u8)
        self._check(self.L.bsh_slam_process_frame(self._slam, frame_index, d.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                  rgb.ctypes.data_as(C.POINTER(C.c_uint8)), int(force_keyframe)))

    def PreprocessFrame(self, depth_u16, rgb_u8):
        """The first stage of ProcessFrame alone (upload, input conditioning, preprocessing kernels), finished on return."""
        d, rgb = self._frame(depth_u16, rgb_u8)
        self._check(self.L.bsh_slam_preprocess_frame(self._slam, d.ctypes.data_as(C.POINTER(C.c_uint16)), rgb.ctypes.data_as(C.POINTER(C.c_uint8))))

    def set_sensor_rectification(self, color_camera=None, depth_camera=None, color_T_depth=None, depth_difference_threshold=0.05,
                                 raw_depth_to_metres=0.001):
        """BadSlam::SetSensorRectification: from now on ProcessFrame / PreprocessFrame take the RAW frames of a sensor with the two
        radtan cameras (abi.RadtanCamera, pixel-centre convention; rectification.radtan_camera builds one): u16 depth of the depth
        camera's size in units of raw_depth_to_metres, rgb of the colour camera's size.  color_T_depth: 3x4 (or 12 values, row-major)
        pose of the depth camera in the colour camera's frame, identity if None.  This object must have been constructed with
        rectification.decide_undistorted_camera(color_camera, True), scaled by the pyramid levels, for both streams.  Without
        cameras: off again."""
        from . import abi
        L = self.L
        L.bsh_slam_set_sensor_rectification.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.RadtanCamera), C.POINTER(C.c_float), C.c_float, C.c_float]
        if color_camera is None and depth_camera is None:
            self._check(L.bsh_slam_set_sensor_rectification(self._slam, 0, None, None, 0.0, 0.0))
            self._depth_shape, self._rgb_shape = self._plain_shapes
            return
        if color_camera is None or depth_camera is None:
            raise ValueError("set_sensor_rectification needs both raw cameras (or neither, to switch it off)")
        cameras = (abi.RadtanCamera * 2)(color_camera, depth_camera)
        T = np.ascontiguousarray(np.eye(4)[:3] if color_T_depth is None else color_T_depth, np.float32).reshape(12)
        self._check(L.bsh_slam_set_sensor_rectification(self._slam, 1, cameras, dba._f(T), depth_difference_threshold, raw_depth_to_metres))
        self._depth_shape = (depth_camera.height, depth_camera.width)
        self._rgb_shape = (color_camera.height, color_camera.width, 3)

    def RunBundleAdjustment(self, frame_index, optimize_depth_intrinsics, optimize_color_intrinsics, optimize_poses, optimize_geometry,
                            min_iterations, max_iterations, window_start=-1, window_end=-1, increase_ba_iteration_count=True):
        done, conv = C.c_int(), C.c_int()
        self._check(self.L.bsh_slam_run_bundle_adjustment(self._slam, frame_index, int(optimize_depth_intrinsics), int(optimize_color_intrinsics),
                                                          int(optimize_poses), int(optimize_geometry), min_iterations, max_iterations, window_start,
                                                          window_end, int(increase_ba_iteration_count), C.byref(done), C.byref(conv)))
        return done.value, bool(conv.value)

    def frame_poses(self):
        """(n, 7) rows qx qy qz qw tx ty tz: global_T_frame of every processed frame."""
        n = self.L.bsh_slam_frame_count(self._slam)
        out = np.zeros((max(1, n), 7), np.float32)
        self._check(self.L.bsh_slam_get_frame_poses(self._slam, dba._f(out), n))
        return out[:n]

    def CloseLoop(self, matched_id, old_T_cur_initial):
        """Loop closure of the newest keyframe against keyframe matched_id (DirectBA.CloseLoop's dict); when the loop is
        closed, the non-keyframe poses follow their keyframes."""
        L = dba._loop_lib()
        ints, floats, chi2 = dba._loop_buffers(self._num_scales)
        self._check(L.bsh_slam_close_loop(self._slam, matched_id, dba._f(dba.pose7(old_T_cur_initial)), dba._i(ints), dba._f(floats), dba._d(chi2)))
        return dba._loop_result(ints, floats, chi2, self._num_scales)

    def set_loop_candidate_search(self, enable, min_keyframe_gap=10):
        """Opt-in geometric loop candidates (off by default): on every new keyframe, the nearest older keyframe (id <= new id -
        min_keyframe_gap) whose frustum intersects the new one is tried with CloseLoop.  Not place recognition: it closes
        only drift the pairwise tracker can still converge over."""
        self._check(dba._loop_lib().bsh_slam_set_loop_candidate_search(self._slam, int(enable), int(min_keyframe_gap)))

    def loop_closure_log(self):
        """[{keyframe, candidate, status, mean_pixel_distance}] of the candidate search, oldest first."""
        L = dba._loop_lib()
        n = L.bsh_slam_loop_log_size(self._slam)
        e, d = np.zeros(3 * max(1, n), np.int32), np.zeros(max(1, n), np.float32)
        self._check(L.bsh_slam_loop_log(self._slam, dba._i(e), dba._f(d), n))
        return [{"keyframe": int(e[3 * i]), "candidate": int(e[3 * i + 1]), "status": dba.LOOP_STATUS_NAMES[int(e[3 * i + 2])],
                 "mean_pixel_distance": float(d[i])} for i in range(n)]

    def set_place_recognition(self, enable, **options):
        """Opt-in place recognition (off by default): every new keyframe's features enter a device database, and before its BA
        iterations the keyframe is matched against the keyframes at least min_keyframe_gap ids older; a recognised place gets
        a RANSAC start pose and CloseLoop.  options: see direct_ba.place_recognition_options.  Excludes
        set_loop_candidate_search."""
        L = dba._place_lib()
        o, thr = dba._place_options_arrays(dba.place_recognition_options(**options))
        self._check(L.bsh_slam_set_place_recognition(self._slam, int(enable), o.ctypes.data_as(C.POINTER(C.c_int64)), thr))

    def place_recognition_log(self):
        """[{keyframe, candidate (-1: none), match_count, inlier_count, pose_found, old_T_cur, loop_attempted, status,
        mean_pixel_distance}] of place recognition, one entry per keyframe added while it was on, oldest first."""
        L = dba._place_lib()
        n = L.bsh_slam_place_log_size(self._slam)
        e, d, p = np.zeros(7 * max(1, n), np.int32), np.zeros(max(1, n), np.float32), np.zeros(7 * max(1, n))
        self._check(L.bsh_slam_place_log(self._slam, dba._i(e), dba._f(d), dba._d(p), n))
        return [{"keyframe": int(e[7 * i]), "candidate": int(e[7 * i + 1]), "match_count": int(e[7 * i + 2]), "inlier_count": int(e[7 * i + 3]),
                 "pose_found": bool(e[7 * i + 4]), "old_T_cur": p[7 * i:7 * i + 7].copy(), "loop_attempted": bool(e[7 * i + 5]),
                 "status": dba.LOOP_STATUS_NAMES[int(e[7 * i + 6])] if e[7 * i + 5] else None, "mean_pixel_distance": float(d[i])} for i in range(n)]

    def state(self):
        s = (C.c_int * 5)()
        self._check(self.L.bsh_slam_state(self._slam, s))
        return dict(keyframe_created=bool(s[0]), pose_estimated=bool(s[1]), num_planned_ba_iterations=s[2], base_kf_id=s[3], motion_model_length=s[4])


class _BorrowedBA:
    """Forwards to the DirectBA wrapper; keeps the owning BadSlam alive and never destroys the native object."""

    def __init__(self, view, owner):
        object.__setattr__(self, "_view", view)
        object.__setattr__(self, "_owner", owner)

    def __getattr__(self, name):
        if name in ("close", "__del__"):
            raise AttributeError(name)
        return getattr(self._view, name)
