"""ctypes binding of the C++ host class bslam_host::DirectBA (badslam_amd/host/), the MI355X
counterpart of the reference's DirectBA (BS/direct_ba.h).  Method names follow the reference."""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "libbadslam_host.so")
_host = None


class DirectBAError(RuntimeError):
    pass


def host_lib():
    global _host
    if _host is not None:
        return _host
    from . import preload_torch_hip_runtime
    preload_torch_hip_runtime()
    if not os.path.exists(HOST_LIB_PATH):
        raise DirectBAError(f"{HOST_LIB_PATH} is missing: build it with `python -m badslam_amd.build`")
    L = C.CDLL(HOST_LIB_PATH)
    f32p, u16p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)
    L.bsh_last_error.restype = C.c_char_p
    L.bsh_create.restype = C.c_void_p
    L.bsh_create.argtypes = [C.c_int, C.c_float, C.c_float, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int,
                             f32p, C.c_int, C.c_int, f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.bsh_destroy.argtypes = [C.c_void_p]
    L.bsh_context.restype = C.c_void_p
    L.bsh_context.argtypes = [C.c_void_p]
    L.bsh_add_keyframe.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, u16p, u16p, u16p, u8p, f32p]
    L.bsh_add_keyframe_from_images.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, u16p, u8p, f32p]
    L.bsh_get_keyframe_images.argtypes = [C.c_void_p, C.c_void_p, C.c_int, u16p, u16p, u16p, u8p, f32p]
    L.bsh_set_surfels.argtypes = [C.c_void_p, C.c_void_p, f32p, C.c_size_t, C.c_uint32]
    L.bsh_get_surfels.argtypes = [C.c_void_p, C.c_void_p, f32p, C.c_size_t, C.c_int]
    L.bsh_get_active_surfels.argtypes = [C.c_void_p, C.c_void_p, u8p]
    L.bsh_surfels_size.restype = C.c_uint32
    L.bsh_surfels_size.argtypes = [C.c_void_p]
    L.bsh_keyframe_count.argtypes = [C.c_void_p]
    L.bsh_get_keyframe_pose.argtypes = [C.c_void_p, C.c_int, f32p]
    L.bsh_set_keyframe_pose.argtypes = [C.c_void_p, C.c_int, f32p]
    L.bsh_get_keyframe_activation.argtypes = [C.c_void_p, C.c_int]
    L.bsh_set_keyframe_activation.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.bsh_keyframe_covisibility.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int]
    L.bsh_upload_keyframe_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_int, u16p]
    L.bsh_upload_keyframe_normals.argtypes = [C.c_void_p, C.c_void_p, C.c_int, u16p]
    L.bsh_set_options.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.bsh_set_scheme_end_tasks.argtypes = [C.c_void_p, C.c_int]
    L.bsh_set_timings_file.argtypes = [C.c_void_p, C.c_char_p]
    L.bsh_keyframe_is_deleted.argtypes = [C.c_void_p, C.c_int]
    L.bsh_delete_keyframe.argtypes = [C.c_void_p, C.c_int]
    L.bsh_merge_keyframes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    L.bsh_update_keyframe_covisibility.argtypes = [C.c_void_p, C.c_int]
    L.bsh_assign_colors.argtypes = [C.c_void_p, C.c_void_p]
    L.bsh_export_point_cloud.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, f32p, u8p, f32p, C.POINTER(C.c_uint64)]
    L.bsh_create_surfels_for_keyframe.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.bsh_depth_camera_size.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.bsh_render_model.argtypes = [C.c_void_p, C.c_void_p, f32p, f32p, C.c_int, C.c_int, f32p, u16p, C.POINTER(C.c_uint32), u8p, f32p, f32p]
    L.bsh_render_volume.argtypes = [C.c_void_p, C.c_void_p, f32p, f32p, C.c_int, C.c_int, f32p, C.c_uint32, u16p, u8p, f32p, f32p]
    L.bsh_set_allreduce.argtypes = [C.c_void_p, abi.ALLREDUCE_FN, C.c_void_p]
    L.bsh_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.bsh_comm_destroy.argtypes = [C.c_void_p]
    L.bsh_estimate_frame_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_int, f32p, f32p]
    L.bsh_bundle_adjustment.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 12 + [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.bsh_get_intrinsics.argtypes = [C.c_void_p, f32p, f32p, f32p]
    L.bsh_set_intrinsics.argtypes = [C.c_void_p, f32p, f32p, C.c_float]
    L.bsh_get_cfactor.argtypes = [C.c_void_p, C.c_void_p, f32p]
    L.bsh_compute_cost.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), f32p, C.POINTER(C.c_uint32), C.POINTER(C.c_int),
                                   C.POINTER(C.c_double)]
    L.bsh_set_cost_tracking.argtypes = [C.c_void_p, C.c_int]
    L.bsh_cost_history.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    u32p = C.POINTER(C.c_uint32)
    L.bsh_model_bounds.argtypes = [C.c_void_p, C.c_void_p, f32p]
    L.bsh_fuse_keyframes.argtypes = [C.c_void_p, C.c_void_p, f32p, C.c_float, C.POINTER(C.c_int), C.c_float]
    L.bsh_extract_mesh.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
    L.bsh_mesh_copy.argtypes = [f32p, f32p, u8p, u32p]
    L.bsh_extract_mesh_filtered.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), u32p]
    L.bsh_mesh_component_sizes.argtypes = [u32p, C.c_uint32]
    L.bsh_mesh_components.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, u32p, u32p, u32p, u32p]
    L.bsh_volume.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), f32p, f32p, u32p, u8p]
    u64p = C.POINTER(C.c_uint64)
    L.bsh_point_mesh_distance.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, f32p, C.c_uint64, f32p, C.c_uint64, u32p, C.c_float, C.c_float, C.c_uint64, f32p, u32p,
                                          f32p, u64p]
    L.bsh_nearest_triangle.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, f32p, C.c_uint64, f32p, C.c_uint64, u32p, C.c_float, f32p, u32p, u32p]
    L.bsh_mesh_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, f32p, f32p, f32p, C.c_uint64, f32p, C.c_uint64, u32p, C.c_int, f32p, u32p, f32p, u8p, u8p, u32p]
    L.bsh_mesh_visibility.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, f32p, f32p, C.c_uint64, f32p, C.c_uint64, u32p, C.c_uint64, f32p, f32p, f32p, C.c_int, C.c_int,
                                      f32p, u32p, u32p, u32p]
    L.bsh_surfel_mesh_distance.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_uint64, u64p, f32p, u64p]
    L.bsh_distance_copy.argtypes = [f32p, u32p]
    L.bsh_simplify_mesh.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, f32p, f32p, u8p, C.c_uint64, u32p, f32p, C.c_float, u64p]
    L.bsh_simplified_copy.argtypes = [f32p, f32p, u8p, u32p, u32p]
    L.bsh_decimate_mesh.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, f32p, f32p, u8p, C.c_uint64, u32p, C.c_uint32, C.c_float, C.c_float, C.c_uint32, u64p]
    L.bsh_decimated_copy.argtypes = [f32p, f32p, u8p, u32p, u32p]
    L.bsh_clean_mesh.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, f32p, f32p, u8p, C.c_uint64, u32p, C.POINTER(C.c_int), u64p]
    L.bsh_cleaned_copy.argtypes = [f32p, f32p, u8p, u32p, u32p, u32p]
    L.bsh_mesh_topology.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, u32p, C.POINTER(abi.MeshReport), u32p, u32p]
    L.bsh_orient_mesh.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, f32p, f32p, C.c_uint64, u32p, C.c_int, u32p, u8p, u32p, C.POINTER(abi.OrientReport)]
    L.bsh_fill_mesh_holes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, f32p, f32p, u8p, C.c_uint64, u32p, C.c_uint32, u64p]
    L.bsh_filled_copy.argtypes = [f32p, f32p, u8p, u32p]
    L.bsh_smooth_mesh.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, f32p, f32p, C.c_uint64, u32p, C.c_uint32, C.c_float, C.c_float, C.c_uint32]
    L.bsh_smooth_extracted_mesh.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_uint32, u64p]
    L.bsh_smoothed_copy.argtypes = [f32p, f32p]
    L.bsh_render_mesh.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, f32p, f32p, u8p, C.c_uint64, u32p, f32p, f32p, C.c_int, C.c_int, f32p, C.c_int, u16p, u32p, u8p,
                                  f32p, f32p]
    L.bsh_sample_mesh.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, f32p, C.c_uint64, u32p, C.c_float, C.c_uint32, u64p]
    L.bsh_samples_copy.argtypes = [f32p, f32p, u32p]
    f64p = C.POINTER(C.c_double)
    L.bsh_register_points.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, f32p, C.c_uint64, f32p, C.c_uint64, u32p, f64p, f64p, f64p, C.POINTER(C.c_int32), f64p]
    L.bsh_registration_history.argtypes = [f64p]
    L.bsh_registration_reason.argtypes = [C.c_int]
    L.bsh_registration_reason.restype = C.c_char_p
    _host = L
    return L


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _u16(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint16))


def _u32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


_VIEW_ARRAYS = {"depth": ((), np.uint16), "index": ((), np.uint32), "color": ((4,), np.uint8), "normal": ((3,), np.float32)}


def _alloc_views(views, allowed, h, w):
    """The zeroed (h, w) output arrays of the views named in `views`, which must be some of `allowed`."""
    if not views or set(views) - set(allowed):
        raise ValueError(f"views must name some of {', '.join(allowed)} (got {sorted(views)})")
    return {name: np.zeros((h, w) + _VIEW_ARRAYS[name][0], _VIEW_ARRAYS[name][1]) for name in allowed if name in views}


def pose7(se3f):
    return np.array(list(se3f.q) + list(se3f.t), np.float32)


def se3f_from7(p):
    T = abi.SE3f()
    for i in range(4):
        T.q[i] = float(p[i])
    for i in range(3):
        T.t[i] = float(p[4 + i])
    return T


def pose_matrix(pose):
    """global_T_camera as a 4 x 4 float64 matrix: of an abi.SE3f (unit quaternion x y z w and translation), or of anything that
    already is 4 x 4."""
    if isinstance(pose, abi.SE3f):
        x, y, z, w = (float(v) for v in pose.q)
        M = np.eye(4)
        M[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        M[:3, 3] = [float(v) for v in pose.t]
        return M
    return np.asarray(pose, np.float64).reshape(4, 4)


def view_rows(poses):
    """The views of MeshVisibility from global_T_camera poses (abi.SE3f or 4 x 4): (camera_T_global (K, 3, 4) f32 -- the inverse
    R^T | -R^T t formed in float64 and rounded -- and centres (K, 3) f32, the translations rounded)."""
    rows, centres = np.zeros((len(poses), 3, 4), np.float32), np.zeros((len(poses), 3), np.float32)
    for k, pose in enumerate(poses):
        M = pose_matrix(pose)
        rows[k, :, :3] = M[:3, :3].T
        rows[k, :, 3] = -(M[:3, :3].T @ M[:3, 3])
        centres[k] = M[:3, 3]
    return rows, centres


# ---- loop closure (badslam_amd/host/pose_graph.hpp, loop_closure.hpp) ------------------------------------------
LOOP_CLOSED, LOOP_IGNORED_SMALL, LOOP_REJECTED_NO_NEIGHBOURS, LOOP_REJECTED_INCONSISTENT = 0, 1, 2, 3
LOOP_STATUS_NAMES = {0: "closed", 1: "ignored_small", 2: "rejected_no_neighbours", 3: "rejected_inconsistent"}
LOOP_POSE_GRAPH_ITERATIONS = 20


def _loop_lib():
    L = host_lib()
    if getattr(L, "_loop_ready", False):
        return L
    dp, ip, fp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_float)
    L.bsh_optimize_pose_graph.argtypes = [C.c_int, dp, C.c_int, ip, dp, C.c_int, C.c_int, dp, dp, C.POINTER(C.c_longlong)]
    L.bsh_optimize_keyframe_pose_graph.argtypes = [C.c_int, ip, dp, C.c_int, ip, dp, C.c_int, dp, dp, C.POINTER(C.c_longlong)]
    L.bsh_average_pose.argtypes = [C.c_int, dp, dp]
    L.bsh_track_keyframes_batched.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, ip, fp, C.c_int, fp, ip]
    L.bsh_close_loop.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, fp, C.c_int, ip, fp, dp]
    L.bsh_slam_close_loop.argtypes = [C.c_void_p, C.c_int, fp, ip, fp, dp]
    L.bsh_slam_set_loop_candidate_search.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.bsh_slam_loop_log_size.argtypes = [C.c_void_p]
    L.bsh_slam_loop_log.argtypes = [C.c_void_p, ip, fp, C.c_int]
    L._loop_ready = True
    return L


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _i(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def optimize_pose_graph(poses7, edges, measurements7, fixed_id, iterations=LOOP_POSE_GRAPH_ITERATIONS):
    """Keyframe pose graph (BS/pose_graph_optimizer.cc semantics, g2o EdgeSE3 / VertexSE3, plain Gauss-Newton) on the host,
    in double.  poses7: (V, 7) [qx qy qz qw tx ty tz] global_T_frame; edges: (E, 2) vertex pairs (from, to);
    measurements7: (E, 7) from_T_to.  Vertex fixed_id is held.  Returns (poses7 (V, 7), chi2 after each iteration,
    info dict with initial_chi2 and factor_blocks)."""
    L = _loop_lib()
    poses = np.array(poses7, np.float64).reshape(-1, 7).copy()
    e = np.ascontiguousarray(np.asarray(edges, np.int32).reshape(-1, 2))
    m = np.ascontiguousarray(np.asarray(measurements7, np.float64).reshape(-1, 7))
    if len(e) != len(m):
        raise ValueError("one measurement per edge")
    chi2, init, blocks = np.zeros(max(1, iterations)), C.c_double(), C.c_longlong()
    if L.bsh_optimize_pose_graph(len(poses), _d(poses), len(e), _i(e), _d(m), int(fixed_id), int(iterations), _d(chi2), C.byref(init), C.byref(blocks)) < 0:
        raise DirectBAError(L.bsh_last_error().decode())
    return poses, chi2[:iterations].copy(), {"initial_chi2": init.value, "factor_blocks": blocks.value}


def optimize_keyframe_pose_graph(poses7, exists, loop_edges, loop_measurements7, iterations=LOOP_POSE_GRAPH_ITERATIONS):
    """The graph loop closure builds over a keyframe list: a vertex per existing keyframe, odometry edges between
    consecutive existing keyframes from the current poses, the given loop edges (keyframe ids); the lowest-id existing
    keyframe is the gauge.  Returns (poses7, chi2 per iteration, info dict with gauge, initial_chi2, factor_blocks)."""
    L = _loop_lib()
    poses = np.array(poses7, np.float64).reshape(-1, 7).copy()
    ex = np.ascontiguousarray(np.asarray(exists, np.int32).reshape(-1))
    e = np.ascontiguousarray(np.asarray(loop_edges, np.int32).reshape(-1, 2))
    m = np.ascontiguousarray(np.asarray(loop_measurements7, np.float64).reshape(-1, 7))
    chi2, init, blocks = np.zeros(max(1, iterations)), C.c_double(), C.c_longlong()
    gauge = L.bsh_optimize_keyframe_pose_graph(len(poses), _i(ex), _d(poses), len(e), _i(e), _d(m), int(iterations), _d(chi2), C.byref(init), C.byref(blocks))
    if gauge < 0:
        raise DirectBAError(L.bsh_last_error().decode())
    return poses, chi2[:iterations].copy(), {"gauge": gauge, "initial_chi2": init.value, "factor_blocks": blocks.value}


def average_pose(poses7):
    """AveragePose (BS/util.cc:110-129) in double: SVD projection of the summed rotations, mean translation."""
    L = _loop_lib()
    p = np.ascontiguousarray(np.asarray(poses7, np.float64).reshape(-1, 7))
    out = np.zeros(7)
    if L.bsh_average_pose(len(p), _d(p), _d(out)) < 0:
        raise DirectBAError(L.bsh_last_error().decode())
    return out


def _loop_result(ints, floats, chi2, num_scales):
    n_chi2 = int(ints[5])
    return {"status": LOOP_STATUS_NAMES[int(ints[0])], "status_code": int(ints[0]), "old_keyframe_ids": [int(v) for v in ints[1:4]],
            "cur_T_old_refined": [se3f_from7(floats[7 * i:7 * i + 7]) for i in range(3)], "cur_T_old_averaged": se3f_from7(floats[21:28]),
            "mean_pixel_distance": float(floats[28]), "pixel_count": int(ints[4]), "chi2": [float(v) for v in chi2[:n_chi2]],
            "tracking_iterations": [[int(v) for v in ints[6 + num_scales * i:6 + num_scales * (i + 1)]] for i in range(3)]}


def _loop_buffers(num_scales):
    return np.zeros(6 + 3 * num_scales, np.int32), np.zeros(29, np.float32), np.zeros(LOOP_POSE_GRAPH_ITERATIONS)


# ---- place recognition (badslam_amd/host/place_recognition.hpp) -----------------------------------------------
def _place_lib():
    L = _loop_lib()
    if getattr(L, "_place_ready", False):
        return L
    dp, ip, fp, i64p, u32p = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_uint32)
    L.bsh_place_default_options.argtypes = [i64p, dp]
    L.bsh_estimate_relative_pose.argtypes = [C.c_int, C.c_int, C.c_int, dp, dp, C.c_int, C.c_double, C.c_int, dp, ip, C.POINTER(C.c_uint8)]
    L.bsh_place_ransac_seed.restype = C.c_uint32
    L.bsh_place_ransac_seed.argtypes = [C.c_int, C.c_int]
    L.bsh_place_cells.argtypes = [C.c_void_p]
    L.bsh_extract_keyframe_features.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, u32p, u32p]
    L.bsh_match_keyframe_features.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, ip, C.c_int, C.POINTER(C.c_int32), u32p]
    L.bsh_recognize_place.argtypes = [C.c_void_p, C.c_void_p, C.c_int, i64p, C.c_double, C.c_int, ip, dp, ip, fp, dp]
    L.bsh_slam_set_place_recognition.argtypes = [C.c_void_p, C.c_int, i64p, C.c_double]
    L.bsh_slam_place_log_size.argtypes = [C.c_void_p]
    L.bsh_slam_place_log.argtypes = [C.c_void_p, ip, fp, dp, C.c_int]
    L._place_ready = True
    return L


def place_recognition_options(**overrides):
    """PlaceRecognitionOptions as a dict: min_keyframe_gap, score_threshold, max_distance, min_matches, ransac_iterations,
    ransac_min_inliers, ransac_inlier_threshold (metres) -- the native defaults with `overrides` applied."""
    L = _place_lib()
    o, thr = np.zeros(6, np.int64), C.c_double()
    L.bsh_place_default_options(o.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(thr))
    names = ("min_keyframe_gap", "score_threshold", "max_distance", "min_matches", "ransac_iterations", "ransac_min_inliers")
    opts = {n: int(v) for n, v in zip(names, o)}
    opts["ransac_inlier_threshold"] = thr.value
    unknown = set(overrides) - set(opts)
    if unknown:
        raise ValueError(f"unknown place recognition options {sorted(unknown)}")
    opts.update(overrides)
    return opts


def _place_options_arrays(opts):
    o = np.array([opts[n] for n in ("min_keyframe_gap", "score_threshold", "max_distance", "min_matches", "ransac_iterations", "ransac_min_inliers")], np.int64)
    return o, float(opts["ransac_inlier_threshold"])


def estimate_relative_pose(current_id, matched_id, p_cur, p_old, iterations=500, inlier_threshold=0.06, min_inliers=10):
    """3D-3D RANSAC of place recognition on the host, in double (no GPU): p_cur, p_old (n, 3) corresponding points in the
    frames of the current and the matched keyframe.  Returns a dict: found, old_T_cur (7,) float64 [qx qy qz qw tx ty tz],
    inlier_count, inliers (n,) bool."""
    L = _place_lib()
    a = np.ascontiguousarray(np.asarray(p_cur, np.float64).reshape(-1, 3))
    b = np.ascontiguousarray(np.asarray(p_old, np.float64).reshape(-1, 3))
    if len(a) != len(b):
        raise ValueError("one point of each frame per correspondence")
    pose, count, mask = np.zeros(7), C.c_int(), np.zeros(max(1, len(a)), np.uint8)
    rc = L.bsh_estimate_relative_pose(int(current_id), int(matched_id), len(a), _d(a), _d(b), int(iterations), float(inlier_threshold), int(min_inliers),
                                      _d(pose), C.byref(count), mask.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc < 0:
        raise DirectBAError(L.bsh_last_error().decode())
    return {"found": bool(rc), "old_T_cur": pose, "inlier_count": count.value, "inliers": mask[:len(a)].astype(bool)}


# ---- file formats (badslam_amd/host/io.hpp) -----------------------------------------------------------------
def _io_lib():
    L = host_lib()
    if getattr(L, "_io_ready", False):
        return L
    L.bsh_png_info.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    L.bsh_read_png_gray16.argtypes = [C.c_char_p, C.POINTER(C.c_uint16), C.c_size_t]
    L.bsh_read_png_rgb8.argtypes = [C.c_char_p, C.POINTER(C.c_uint8), C.c_size_t]
    L.bsh_tum_open.restype = C.c_void_p
    L.bsh_tum_open.argtypes = [C.c_char_p, C.c_char_p]
    L.bsh_tum_close.argtypes = [C.c_void_p]
    L.bsh_tum_frame_count.argtypes = [C.c_void_p]
    L.bsh_tum_camera.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.bsh_tum_frame.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.bsh_save_poses.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int, C.c_char_p]
    L.bsh_save_point_cloud_ply.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_float)]
    L.bsh_save_mesh_ply.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_uint64, C.POINTER(C.c_uint32)]
    L.bsh_load_ply.argtypes = [C.c_char_p, C.POINTER(C.c_uint64)]
    L.bsh_ply_copy.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)]
    L.bsh_save_calibration_arrays.argtypes = [C.c_char_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.bsh_load_calibration_arrays.argtypes = [C.c_char_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.bsh_save_calibration.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p]
    L.bsh_load_calibration.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p]
    L._io_ready = True
    return L


def _io_check(L, rc):
    if rc != 0:
        raise DirectBAError(L.bsh_last_error().decode())


def read_png(path):
    """16-bit gray -> (h, w) uint16; 8-bit colour / gray -> (h, w, 3) uint8."""
    L = _io_lib()
    info = (C.c_int * 4)()
    _io_check(L, L.bsh_png_info(str(path).encode(), info))
    w, h, depth, channels = info[0], info[1], info[2], info[3]
    if channels == 1 and depth == 16:
        out = np.zeros((h, w), np.uint16)
        _io_check(L, L.bsh_read_png_gray16(str(path).encode(), out.ctypes.data_as(C.POINTER(C.c_uint16)), out.size))
        return out
    out = np.zeros((h, w, 3), np.uint8)
    _io_check(L, L.bsh_read_png_rgb8(str(path).encode(), out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size))
    return out


def read_tum_dataset(folder, trajectory_filename=None):
    """ReadTUMRGBDDatasetAssociatedAndCalibrated: dict(width, height, camera (corner convention), frames=[dict])."""
    L = _io_lib()
    h = L.bsh_tum_open(str(folder).encode(), trajectory_filename.encode() if trajectory_filename else None)
    if not h:
        raise DirectBAError(L.bsh_last_error().decode())
    try:
        cam = (C.c_float * 4)()
        w, ht = C.c_int(), C.c_int()
        L.bsh_tum_camera(h, cam, C.byref(w), C.byref(ht))
        frames = []
        for i in range(L.bsh_tum_frame_count(h)):
            bufs = [C.create_string_buffer(512) for _ in range(4)]
            p_rgb, p_depth = np.zeros(7, np.float32), np.zeros(7, np.float32)
            _io_check(L, L.bsh_tum_frame(h, i, bufs[0], bufs[1], bufs[2], bufs[3], 512, _f(p_rgb), _f(p_depth)))
            frames.append(dict(rgb_path=bufs[0].value.decode(), depth_path=bufs[1].value.decode(), rgb_timestamp=bufs[2].value.decode(),
                               depth_timestamp=bufs[3].value.decode(), rgb_global_T_frame=p_rgb, depth_global_T_frame=p_depth))
        return dict(width=w.value, height=ht.value, camera=np.array(list(cam), np.float32), frames=frames)
    finally:
        L.bsh_tum_close(h)


def save_poses(timestamp_strings, poses7, start_frame, path):
    """SavePoses (BS/io.cc:537-568); poses7 = (n, 7) rows qx qy qz qw tx ty tz of global_T_frame."""
    L = _io_lib()
    n = len(timestamp_strings)
    arr = (C.c_char_p * n)(*[t.encode() for t in timestamp_strings])
    p = np.ascontiguousarray(poses7, np.float32)
    _io_check(L, L.bsh_save_poses(n, arr, _f(p), start_frame, str(path).encode()))


def SavePointCloudAsPLY(path, positions, colors=None, normals=None):
    """Binary little-endian PLY of a point cloud (BS/io.cc:694): positions (n, 3) f32, colors (n, 3) u8, normals (n, 3) f32 -- the
    arrays of DirectBA.ExportToPointCloud; colors / normals may be None."""
    L = _io_lib()
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    col = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if (col is not None and len(col) != len(pos)) or (nrm is not None and len(nrm) != len(pos)):
        raise ValueError("colors and normals need one row per point")
    _io_check(L, L.bsh_save_point_cloud_ply(str(path).encode(), len(pos), _f(pos), None if col is None else col.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            None if nrm is None else _f(nrm)))


def SaveMeshAsPLY(path, mesh):
    """Binary little-endian PLY of a triangle mesh: vertex x y z nx ny nz red green blue, face list uchar int vertex_indices.
    mesh: the dict of DirectBA.ExtractMesh -- positions (V, 3) f32, normals (V, 3) f32, colors (V, 4) u8, triangles (T, 3) u32."""
    L = _io_lib()
    pos = np.ascontiguousarray(mesh["positions"], np.float32).reshape(-1, 3)
    nrm = np.ascontiguousarray(mesh["normals"], np.float32).reshape(-1, 3)
    col = np.ascontiguousarray(mesh["colors"], np.uint8).reshape(-1, 4)
    tri = np.ascontiguousarray(mesh["triangles"], np.uint32).reshape(-1, 3)
    if len(nrm) != len(pos) or len(col) != len(pos):
        raise ValueError("normals and colors need one row per vertex")
    _io_check(L, L.bsh_save_mesh_ply(str(path).encode(), len(pos), _f(pos), _f(nrm), col.ctypes.data_as(C.POINTER(C.c_uint8)), len(tri),
                                     tri.ctypes.data_as(C.POINTER(C.c_uint32))))


def LoadPLY(path):
    """Reads a PLY point cloud or mesh (ascii or binary little-endian; float or double x y z; faces with any integer count and index
    types, polygons fan-triangulated; other properties and elements skipped) -> dict of positions (V, 3) f32, normals (V, 3) f32 or
    None, colors (V, 3) u8 or None, triangles (T, 3) u32 (T may be 0).  A malformed or truncated file raises DirectBAError."""
    L = _io_lib()
    counts = (C.c_uint64 * 4)()
    _io_check(L, L.bsh_load_ply(str(path).encode(), counts))
    V, T = int(counts[0]), int(counts[1])
    out = dict(positions=np.zeros((V, 3), np.float32), normals=np.zeros((V, 3), np.float32) if counts[2] else None,
               colors=np.zeros((V, 3), np.uint8) if counts[3] else None, triangles=np.zeros((T, 3), np.uint32))
    _io_check(L, L.bsh_ply_copy(_f(out["positions"]), None if out["normals"] is None else _f(out["normals"]),
                                None if out["colors"] is None else out["colors"].ctypes.data_as(C.POINTER(C.c_uint8)), out["triangles"].ctypes.data_as(C.POINTER(C.c_uint32))))
    return out


def save_calibration_arrays(base, depth4, color4, a, cfactor):
    L = _io_lib()
    cf = np.ascontiguousarray(cfactor, np.float32)
    _io_check(L, L.bsh_save_calibration_arrays(str(base).encode(), _f(np.ascontiguousarray(depth4, np.float32)), _f(np.ascontiguousarray(color4, np.float32)),
                                               a, cf.shape[1], cf.shape[0], _f(cf)))


def load_calibration_arrays(base, cfactor_shape):
    L = _io_lib()
    d, c, a = np.zeros(4, np.float32), np.zeros(4, np.float32), C.c_float()
    cf = np.zeros(cfactor_shape, np.float32)
    _io_check(L, L.bsh_load_calibration_arrays(str(base).encode(), _f(d), _f(c), C.byref(a), cf.shape[1], cf.shape[0], _f(cf)))
    return d, c, a.value, cf


def state_file_round_trip(src, dst):
    """LoadState + SaveState of a version-1 state file; returns the summary (ints[8], floats[11])."""
    L = _io_lib()
    L.bsh_state_load.restype = C.c_void_p
    L.bsh_state_load.argtypes = [C.c_char_p]
    L.bsh_state_free.argtypes = [C.c_void_p]
    L.bsh_state_save.argtypes = [C.c_void_p, C.c_char_p]
    L.bsh_state_summary.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    h = L.bsh_state_load(str(src).encode())
    if not h:
        raise DirectBAError(L.bsh_last_error().decode())
    try:
        ints, floats = np.zeros(8, np.int32), np.zeros(11, np.float32)
        L.bsh_state_summary(h, ints.ctypes.data_as(C.POINTER(C.c_int32)), _f(floats))
        _io_check(L, L.bsh_state_save(h, str(dst).encode()))
        return ints, floats
    finally:
        L.bsh_state_free(h)


class DirectBA:
    """Drives bslam_host::DirectBA.  Constructor arguments are those of BS/direct_ba.h:73-88."""

    def __init__(self, max_surfel_count, raw_to_float_depth, baseline_fx, sparse_surfel_cell_size, surfel_merge_dist_factor,
                 min_observation_count_while_bootstrapping_1, min_observation_count_while_bootstrapping_2, min_observation_count,
                 color_camera, depth_camera, pyramid_level_for_color, use_depth_residuals, use_descriptor_residuals, device=0, stream=None):
        self.L = host_lib()
        cc = np.array([color_camera.fx, color_camera.fy, color_camera.cx, color_camera.cy], np.float32)
        dc = np.array([depth_camera.fx, depth_camera.fy, depth_camera.cx, depth_camera.cy], np.float32)
        self._ba = self.L.bsh_create(max_surfel_count, raw_to_float_depth, baseline_fx, sparse_surfel_cell_size, surfel_merge_dist_factor,
                                     min_observation_count_while_bootstrapping_1, min_observation_count_while_bootstrapping_2,
                                     min_observation_count, _f(cc), color_camera.width, color_camera.height, _f(dc), depth_camera.width,
                                     depth_camera.height, pyramid_level_for_color, int(use_depth_residuals), int(use_descriptor_residuals), device)
        if not self._ba:
            raise DirectBAError(self.L.bsh_last_error().decode())
        self.stream = C.c_void_p(stream) if stream else C.c_void_p(None)

    def context_handle(self):
        """bslam_context* of the kernel library used by this DirectBA (for bslam_profile_*)."""
        return C.c_void_p(self.L.bsh_context(self._ba))

    def _check(self, rc):
        if rc < 0:
            raise DirectBAError(self.L.bsh_last_error().decode())
        return rc

    def close(self):
        if self._ba:
            self.L.bsh_destroy(self._ba)
            self._ba = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def AddKeyframe(self, frame_index, min_depth, max_depth, depth, normals, radius, color, global_T_frame):
        p = pose7(global_T_frame)
        u16 = lambda a: np.ascontiguousarray(a, np.uint16).ctypes.data_as(C.POINTER(C.c_uint16))
        col = np.ascontiguousarray(color, np.uint8)
        return self._check(self.L.bsh_add_keyframe(self._ba, self.stream, frame_index, min_depth, max_depth, u16(depth), u16(normals), u16(radius),
                                                   col.ctypes.data_as(C.POINTER(C.c_uint8)), _f(p)))

    def AddKeyframeFromImages(self, frame_index, depth_u16, rgb_u8, global_T_frame):
        """Keyframe(stream, frame_index, depth_params, depth_camera, depth_image, color_image, pose) + AddKeyframe: the raw
        images are preprocessed on the device (BS/keyframe.cc:82-161)."""
        d = np.ascontiguousarray(depth_u16, np.uint16)
        rgb = np.ascontiguousarray(rgb_u8, np.uint8)
        return self._check(self.L.bsh_add_keyframe_from_images(self._ba, self.stream, frame_index, d.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                               rgb.ctypes.data_as(C.POINTER(C.c_uint8)), _f(pose7(global_T_frame))))

    def keyframe_images(self, kf_id, height, width):
        u16 = lambda: np.zeros((height, width), np.uint16)
        depth, normals, radius, color, mm = u16(), u16(), u16(), np.zeros((height, width, 4), np.uint8), np.zeros(2, np.float32)
        p16 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16))
        self._check(self.L.bsh_get_keyframe_images(self._ba, self.stream, kf_id, p16(depth), p16(normals), p16(radius),
                                                   color.ctypes.data_as(C.POINTER(C.c_uint8)), _f(mm)))
        return depth, normals, radius, color, float(mm[0]), float(mm[1])

    def TrackKeyframePair(self, tracked_id, base_id, init1, init2=None, num_scales=5, test_different_initial_estimates=False,
                          use_pyramid_level_0=True, use_gradmag=False):
        """TrackFramePairwise (BS/pairwise_frame_tracking.cc:256-678) of keyframe `tracked_id` against keyframe `base_id`:
        returns (base_T_tracked, iterations per scale)."""
        self.L.bsh_track_keyframe_pair_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                      C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_int, C.c_int]
        out = np.zeros(7, np.float32)
        its = (C.c_int * num_scales)()
        p1 = pose7(init1)
        p2 = pose7(init2 if init2 is not None else init1)
        self._check(self.L.bsh_track_keyframe_pair_ex(self._ba, self.stream, tracked_id, base_id, num_scales, int(test_different_initial_estimates), _f(p1),
                                                      _f(p2), _f(out), its, int(use_pyramid_level_0), int(use_gradmag)))
        return se3f_from7(out), list(its)

    def TrackKeyframesBatched(self, base_id, tracked_ids, inits, num_scales=5):
        """TrackFramesPairwiseBatched: keyframes `tracked_ids` (up to 8) against keyframe `base_id` in lockstep, as loop
        verification runs it (use_pyramid_level_0, no gradmag, one initial estimate).  Returns ([base_T_tracked], [iterations
        per scale]); each entry is bit-identical to TrackKeyframePair(tracked_id, base_id, init, num_scales=num_scales)."""
        L = _loop_lib()
        n = len(tracked_ids)
        ids = np.asarray(tracked_ids, np.int32)
        p = np.concatenate([pose7(T) for T in inits]).astype(np.float32)
        out = np.zeros(7 * n, np.float32)
        its = np.zeros(num_scales * n, np.int32)
        self._check(L.bsh_track_keyframes_batched(self._ba, self.stream, base_id, n, _i(ids), _f(p), num_scales, _f(out), _i(its)))
        return [se3f_from7(out[7 * i:7 * i + 7]) for i in range(n)], [list(its[num_scales * i:num_scales * (i + 1)]) for i in range(n)]

    def CloseLoop(self, current_id, matched_id, old_T_cur_initial, num_scales=5):
        """Loop closure (BS/loop_detector.cc:440-712 after RANSAC) from keyframe current_id to matched_id: verification by
        three trackings, averaging, the BA-can-handle-it test and the pose graph.  Returns a dict: status ("closed",
        "ignored_small", "rejected_no_neighbours", "rejected_inconsistent"), old_keyframe_ids, cur_T_old_refined (3),
        cur_T_old_averaged, mean_pixel_distance, pixel_count, chi2, tracking_iterations."""
        L = _loop_lib()
        ints, floats, chi2 = _loop_buffers(num_scales)
        self._check(L.bsh_close_loop(self._ba, self.stream, current_id, matched_id, _f(pose7(old_T_cur_initial)), num_scales, _i(ints), _f(floats), _d(chi2)))
        return _loop_result(ints, floats, chi2, num_scales)

    def ExtractKeyframeFeatures(self, kf_id, score_threshold=None):
        """Extracts keyframe kf_id's place-recognition features into the device database (bslam_extract_keyframe_features) and
        returns them: xy (cells,) uint32 = x | y << 16 or 0xFFFFFFFF, desc (cells, 8) uint32; one slot per 16 x 16 cell."""
        L = _place_lib()
        if score_threshold is None:
            score_threshold = place_recognition_options()["score_threshold"]
        cells = self._check(L.bsh_place_cells(self._ba))
        xy, desc = np.zeros(cells, np.uint32), np.zeros((cells, 8), np.uint32)
        u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
        self._check(L.bsh_extract_keyframe_features(self._ba, self.stream, int(kf_id), int(score_threshold), u32(xy), u32(desc)))
        return xy, desc

    def MatchKeyframeFeatures(self, query_id, ids, max_distance=None):
        """One bslam_match_features launch of keyframe query_id against the keyframes `ids` (all extracted before): returns
        match (len(ids), cells) int32 (the matched slot or -1) and count (len(ids),) uint32."""
        L = _place_lib()
        if max_distance is None:
            max_distance = place_recognition_options()["max_distance"]
        cells = self._check(L.bsh_place_cells(self._ba))
        idv = np.ascontiguousarray(ids, np.int32)
        match, count = np.zeros((max(1, len(idv)), cells), np.int32), np.zeros(max(1, len(idv)), np.uint32)
        self._check(L.bsh_match_keyframe_features(self._ba, self.stream, int(query_id), len(idv), _i(idv), int(max_distance),
                                                  match.ctypes.data_as(C.POINTER(C.c_int32)), count.ctypes.data_as(C.POINTER(C.c_uint32))))
        return match[:len(idv)], count[:len(idv)]

    def RecognizePlace(self, current_id, num_scales=5, **options):
        """Place recognition for keyframe current_id: candidate by feature matching, start pose by 3D-3D RANSAC, then CloseLoop.
        options: see place_recognition_options.  Returns a dict: candidate (-1: none), match_count, inlier_count, pose_found,
        old_T_cur (7,) float64 [qx qy qz qw tx ty tz] of the RANSAC estimate, loop_attempted and loop (CloseLoop's dict, or None)."""
        L = _place_lib()
        o, thr = _place_options_arrays(place_recognition_options(**options))
        out5, pose = np.zeros(5, np.int32), np.zeros(7)
        ints, floats, chi2 = _loop_buffers(num_scales)
        self._check(L.bsh_recognize_place(self._ba, self.stream, int(current_id), o.ctypes.data_as(C.POINTER(C.c_int64)), thr, num_scales, _i(out5), _d(pose),
                                          _i(ints), _f(floats), _d(chi2)))
        return {"candidate": int(out5[0]), "match_count": int(out5[1]), "inlier_count": int(out5[2]), "pose_found": bool(out5[3]), "old_T_cur": pose,
                "loop_attempted": bool(out5[4]), "loop": _loop_result(ints, floats, chi2, num_scales) if out5[4] else None}

    def SaveState(self, path, frame_count):
        """The DirectBA part of SaveState (BS/io.cc:38-178) as a version-1 state file."""
        L = _io_lib()
        L.bsh_state_save_from_ba.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_char_p]
        self._check(L.bsh_state_save_from_ba(self._ba, self.stream, frame_count, str(path).encode()))

    def LoadState(self, path):
        L = _io_lib()
        L.bsh_state_load_into_ba.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p]
        self._check(L.bsh_state_load_into_ba(self._ba, self.stream, str(path).encode()))

    def SaveCalibration(self, base_path):
        L = _io_lib()
        self._check(L.bsh_save_calibration(self._ba, self.stream, str(base_path).encode()))

    def LoadCalibration(self, base_path):
        L = _io_lib()
        self._check(L.bsh_load_calibration(self._ba, self.stream, str(base_path).encode()))

    def SetSurfels(self, rows, count):
        rows = np.ascontiguousarray(rows, np.float32)
        self._check(self.L.bsh_set_surfels(self._ba, self.stream, _f(rows), rows.strides[0], count))

    def GetSurfels(self, nrows=8):
        n = self.surfels_size()
        out = np.zeros((nrows, max(1, n)), np.float32)
        self._check(self.L.bsh_get_surfels(self._ba, self.stream, _f(out), out.strides[0], nrows))
        return out[:, :n]

    def GetActiveSurfels(self):
        n = self.surfels_size()
        out = np.zeros(max(1, n), np.uint8)
        self._check(self.L.bsh_get_active_surfels(self._ba, self.stream, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out[:n]

    def surfels_size(self):
        return self.L.bsh_surfels_size(self._ba)

    def keyframe_pose(self, kf_id):
        out = np.zeros(7, np.float32)
        self._check(self.L.bsh_get_keyframe_pose(self._ba, kf_id, _f(out)))
        return se3f_from7(out)

    def set_keyframe_pose(self, kf_id, T):
        self._check(self.L.bsh_set_keyframe_pose(self._ba, kf_id, _f(pose7(T))))

    def keyframe_activation(self, kf_id):
        return self.L.bsh_get_keyframe_activation(self._ba, kf_id)

    def set_keyframe_activation(self, kf_id, act):
        self._check(self.L.bsh_set_keyframe_activation(self._ba, kf_id, act))

    def keyframe_count(self):
        """keyframes().size(): includes deleted (null) entries."""
        return self.L.bsh_keyframe_count(self._ba)

    def keyframe_covisibility(self, kf_id):
        buf = (C.c_int * 4096)()
        n = self.L.bsh_keyframe_covisibility(self._ba, kf_id, buf, 4096)
        return list(buf[:n])

    # --- keyframe management and export (BS/direct_ba.h:95-126)
    def keyframe_is_deleted(self, kf_id):
        return bool(self.L.bsh_keyframe_is_deleted(self._ba, kf_id))

    def DeleteKeyframe(self, kf_id):
        self._check(self.L.bsh_delete_keyframe(self._ba, kf_id))

    def MergeKeyframes(self, approx_merge_count):
        """Returns the ids of the deleted keyframes."""
        ids = (C.c_int * 4096)()
        n = C.c_int()
        self._check(self.L.bsh_merge_keyframes(self._ba, self.stream, approx_merge_count, ids, 4096, C.byref(n)))
        return list(ids[:n.value])

    def UpdateKeyframeCoVisibility(self, kf_id):
        self._check(self.L.bsh_update_keyframe_covisibility(self._ba, kf_id))

    def AssignColors(self):
        self._check(self.L.bsh_assign_colors(self._ba, self.stream))

    def ExportToPointCloud(self):
        """(positions (n, 3) f32, colors (n, 3) u8, normals (n, 3) f32) of the valid surfels."""
        cap = max(1, self.surfels_size())
        pos, col, nrm = np.zeros((cap, 3), np.float32), np.zeros((cap, 3), np.uint8), np.zeros((cap, 3), np.float32)
        n = C.c_uint64()
        self._check(self.L.bsh_export_point_cloud(self._ba, self.stream, cap, _f(pos), _u8(col), _f(nrm), C.byref(n)))
        return pos[:n.value], col[:n.value], nrm[:n.value]

    def RenderModel(self, global_T_camera, camera=None, min_depth=0.05, max_depth=50.0, radius_scale=1.0, views=("depth", "color")):
        """Views of the surfel model from the pose global_T_camera (abi.SE3f) with `camera` (abi.Camera4f, pixel-corner; default:
        the depth camera): every surfel an oriented disc of radius_scale times its radius, the nearest one per pixel.  Returns a
        dict of NumPy arrays of the camera's size with the entries named in `views` -- "depth" (h, w) uint16 in the units of a
        keyframe depth image (0: nothing drawn), "index" (h, w) uint32 surfel columns (0xFFFFFFFF: nothing drawn), "color"
        (h, w, 4) uint8, "normal" (h, w, 3) float32 in the camera frame -- and "camera_T_global" (3, 4) float32, the matrix
        the kernels took.  Surfels whose ball leaves [min_depth, max_depth] metres are dropped.  A sharded (multi-GPU) object
        renders its local shard only."""
        params, w, h = self._view_camera(camera)
        out = _alloc_views(views, ("depth", "index", "color", "normal"), h, w)
        ptr = lambda name, pointer: pointer(out[name]) if name in out else None
        out["camera_T_global"] = np.zeros((3, 4), np.float32)
        options = np.array([min_depth, max_depth, radius_scale], np.float32)
        self._check(self.L.bsh_render_model(self._ba, self.stream, _f(pose7(global_T_camera)), _f(params), w, h, _f(options), ptr("depth", _u16), ptr("index", _u32),
                                            ptr("color", _u8), ptr("normal", _f), _f(out["camera_T_global"])))
        return out

    def _view_camera(self, camera):
        """(fx fy cx cy as float32, width, height) of `camera` (abi.Camera4f), by default of the depth camera."""
        if camera is None:
            size = (C.c_int * 2)()
            self._check(self.L.bsh_depth_camera_size(self._ba, size))
            return np.ascontiguousarray(self.intrinsics()[1], np.float32), size[0], size[1]
        return np.array([camera.fx, camera.fy, camera.cx, camera.cy], np.float32), int(camera.width), int(camera.height)

    # --- volumetric fusion and meshing (bslam_fuse_keyframes, bslam_extract_mesh)
    def ModelBounds(self):
        """(min (3,), max (3,)) float32 of the valid surfels, or None when there is none."""
        b = np.zeros(6, np.float32)
        rc = self.L.bsh_model_bounds(self._ba, self.stream, _f(b))
        self._check(min(rc, 0))
        return (b[:3].copy(), b[3:].copy()) if rc == 1 else None

    def FuseKeyframes(self, origin, voxel_size, dims, truncation):
        """Fuses all keyframes that are not deleted, at their current poses and with the current depth calibration, into a
        truncated signed distance volume of dims = (nx, ny, nz) samples; sample (x, y, z) lies at origin + (i + 0.5) * voxel_size.
        A full rebuild: call it after bundle adjustment.  At most 2^30 samples."""
        o = np.ascontiguousarray(origin, np.float32).reshape(3)
        d = (C.c_int * 3)(*[int(v) for v in dims])
        self._check(self.L.bsh_fuse_keyframes(self._ba, self.stream, _f(o), float(voxel_size), d, float(truncation)))

    def ExtractMesh(self, min_count=1, min_component_vertices=0, report=False):
        """Surface nets of the fused volume over the samples seen by at least min_count keyframes: dict of positions (V, 3) f32,
        normals (V, 3) f32 (towards free space), colors (V, 4) u8, triangles (T, 3) u32 (counter-clockwise seen from free space).
        min_component_vertices >= 2: connected components (vertices joined by a triangle) of fewer vertices are dropped on the
        device before the download; the rest keeps its order.  report=True: returns (mesh, dict of components, removed_vertices,
        removed_triangles, sizes_descending -- the vertex count of every component of the mesh as extracted)."""
        counts = (C.c_uint64 * 2)()
        info = None
        if not report and int(min_component_vertices) < 2:
            self._check(self.L.bsh_extract_mesh(self._ba, self.stream, int(min_count), counts))
        else:
            report3 = (C.c_uint32 * 3)()
            self._check(self.L.bsh_extract_mesh_filtered(self._ba, self.stream, int(min_count), int(min_component_vertices), counts, report3 if report else None))
            if report:
                sizes = np.zeros(report3[0], np.uint32)
                self._check(self.L.bsh_mesh_component_sizes(_u32(sizes), len(sizes)))
                info = dict(components=int(report3[0]), removed_vertices=int(report3[1]), removed_triangles=int(report3[2]), sizes_descending=sizes)
        V, T = int(counts[0]), int(counts[1])
        out = dict(positions=np.zeros((V, 3), np.float32), normals=np.zeros((V, 3), np.float32), colors=np.zeros((V, 4), np.uint8),
                   triangles=np.zeros((T, 3), np.uint32))
        self._check(self.L.bsh_mesh_copy(_f(out["positions"]), _f(out["normals"]), _u8(out["colors"]), _u32(out["triangles"])))
        return (out, info) if report else out

    def MeshComponents(self, mesh):
        """Connected components of a mesh dict (positions (V, 3), triangles (T, 3)): vertices are joined iff a triangle holds both.
        -> (labels (V,) u32: the smallest vertex id of the vertex's component, sizes (V,) u32: its vertex count)."""
        V = len(mesh["positions"])
        tri = np.ascontiguousarray(mesh["triangles"], np.uint32).reshape(-1, 3)
        labels, sizes = np.zeros(V, np.uint32), np.zeros(V, np.uint32)
        n = C.c_uint32()
        self._check(self.L.bsh_mesh_components(self._ba, self.stream, V, len(tri), _u32(tri), _u32(labels), _u32(sizes),
                                               C.byref(n)))
        return labels, sizes

    @staticmethod
    def _mesh_arrays(mesh, who):
        """(positions (V, 3) f32, normals or None, colors (V, 4) u8 or None, triangles (T, 3) u32, the input's colour channels) of an
        ExtractMesh or LoadPLY dict; three colour channels get an alpha of 255."""
        pos = np.ascontiguousarray(mesh["positions"], np.float32).reshape(-1, 3)
        nrm, col, tri = mesh.get("normals"), mesh.get("colors"), mesh.get("triangles")
        if nrm is not None:
            nrm = np.ascontiguousarray(nrm, np.float32).reshape(-1, 3)
        channels = 4
        if col is not None:
            col = np.ascontiguousarray(col, np.uint8).reshape(len(pos), -1)
            channels = col.shape[1]
            if channels == 3:
                col = np.concatenate([col, np.full((len(col), 1), 255, np.uint8)], axis=1)
            if col.shape[1] != 4:
                raise ValueError(f"{who}: colors need 3 or 4 channels")
            col = np.ascontiguousarray(col)
        if nrm is not None and len(nrm) != len(pos):
            raise ValueError(f"{who}: normals need one row per vertex")
        tri = np.zeros((0, 3), np.uint32) if tri is None else np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
        return pos, nrm, col, tri, channels

    # --- mesh decimation (bslam_decimate_mesh)
    def DecimateMesh(self, mesh, target_vertices=None, ratio=None, boundary_weight=1.0, max_cost=None, max_rounds=0):
        """Quadric-error edge collapse of `mesh` (the dict of ExtractMesh or LoadPLY) down to target_vertices, or to
        ceil(ratio * V) of its V vertices; exactly one of the two is given.  Rounds of pairwise non-adjacent collapses, each to the
        cheaper end or the midpoint of its edge, run until the target is met, no edge may collapse any more or max_rounds (0: no limit)
        have run.  boundary_weight (>= 0) holds open boundaries in place, max_cost (None: no bound) refuses dearer collapses.  -> dict
        with the keys of ExtractMesh (normals / colors None where the input has none, colors with the input's channel count) plus
        vertex_map (V,) u32, the output vertex of every input vertex, and rounds.  Survivors keep their relative order, and so do the
        triangles."""
        if (target_vertices is None) == (ratio is None):
            raise ValueError("DecimateMesh: give exactly one of target_vertices and ratio")
        pos, nrm, col, tri, channels = self._mesh_arrays(mesh, "DecimateMesh")
        if ratio is not None:
            if not 0.0 <= float(ratio) <= 1.0:
                raise ValueError("DecimateMesh: ratio must lie in [0, 1]")
            target_vertices = int(np.ceil(float(ratio) * len(pos)))
        if not 0 <= int(target_vertices) <= 0xFFFFFFFF or not 0 <= int(max_rounds) <= 0xFFFFFFFF:
            raise ValueError("DecimateMesh: target_vertices and max_rounds must fit 32 bits")
        counts = (C.c_uint64 * 3)()
        self._check(self.L.bsh_decimate_mesh(self._ba, self.stream, len(pos), _f(pos), None if nrm is None else _f(nrm), None if col is None else _u8(col),
                                             len(tri), _u32(tri), int(target_vertices), float(boundary_weight), float("inf") if max_cost is None else float(max_cost),
                                             int(max_rounds), counts))
        V, T = int(counts[0]), int(counts[1])
        out = dict(positions=np.zeros((V, 3), np.float32), normals=None if nrm is None else np.zeros((V, 3), np.float32),
                   colors=None if col is None else np.zeros((V, 4), np.uint8), triangles=np.zeros((T, 3), np.uint32), vertex_map=np.zeros(len(pos), np.uint32),
                   rounds=int(counts[2]))
        self._check(self.L.bsh_decimated_copy(_f(out["positions"]), None if nrm is None else _f(out["normals"]), None if col is None else _u8(out["colors"]),
                                              _u32(out["triangles"]), _u32(out["vertex_map"])))
        if col is not None and channels == 3:
            out["colors"] = np.ascontiguousarray(out["colors"][:, :3])
        return out

    # --- mesh smoothing (bslam_smooth_mesh)
    SMOOTH_BOUNDARY = {"fixed": 0, "rim": 1, "free": 2}

    def SmoothMesh(self, mesh, iterations=10, lambda_=0.5, mu=-0.53, boundary="fixed"):
        """Taubin lambda|mu smoothing of `mesh` (the dict of ExtractMesh or LoadPLY): `iterations` times a one-ring step with lambda_
        in (0, 1] and then, unless mu is 0, one with mu in [-1, 0]; mu = 0 is plain Laplacian smoothing, which shrinks.  boundary:
        "fixed" holds the vertices of open boundaries, "rim" smooths them along the boundary, "free" treats them like any other.  The
        defaults are provisional: they have been tried on synthetic meshes only.  -> the dict of ExtractMesh: positions and normals
        new -- the normals are the area-weighted ones of the smoothed geometry, the input's (or zero) where a vertex has no triangle
        with an area --, colors (with the input's channel count) and triangles passed through."""
        if boundary not in self.SMOOTH_BOUNDARY:
            raise ValueError("SmoothMesh: boundary must be 'fixed', 'rim' or 'free'")
        if not 0 <= int(iterations) <= 0xFFFFFFFF:
            raise ValueError("SmoothMesh: iterations must fit 32 bits")
        pos, nrm, col, tri, channels = self._mesh_arrays(mesh, "SmoothMesh")
        self._check(self.L.bsh_smooth_mesh(self._ba, self.stream, len(pos), _f(pos), None if nrm is None else _f(nrm), len(tri), _u32(tri), int(iterations),
                                           float(lambda_), float(mu), self.SMOOTH_BOUNDARY[boundary]))
        out = dict(positions=np.zeros((len(pos), 3), np.float32), normals=np.zeros((len(pos), 3), np.float32),
                   colors=None if col is None else np.ascontiguousarray(col[:, :channels]), triangles=tri.copy())
        self._check(self.L.bsh_smoothed_copy(_f(out["positions"]), _f(out["normals"])))
        return out

    def SmoothExtractedMesh(self, iterations=10, lambda_=0.5, mu=-0.53, boundary="fixed"):
        """SmoothMesh of the mesh the last ExtractMesh left on the device, without an upload -> (positions (V, 3) f32, normals (V, 3)
        f32).  The device mesh stays as it is and holds no normals, so a vertex without a triangle that has an area gets (0, 0, 0)."""
        if boundary not in self.SMOOTH_BOUNDARY:
            raise ValueError("SmoothExtractedMesh: boundary must be 'fixed', 'rim' or 'free'")
        if not 0 <= int(iterations) <= 0xFFFFFFFF:
            raise ValueError("SmoothExtractedMesh: iterations must fit 32 bits")
        count = C.c_uint64()
        self._check(self.L.bsh_smooth_extracted_mesh(self._ba, self.stream, int(iterations), float(lambda_), float(mu), self.SMOOTH_BOUNDARY[boundary], C.byref(count)))
        positions, normals = np.zeros((count.value, 3), np.float32), np.zeros((count.value, 3), np.float32)
        self._check(self.L.bsh_smoothed_copy(_f(positions), _f(normals)))
        return positions, normals

    def MeshNormals(self, mesh):
        """`mesh` with vertex normals computed from its geometry: SmoothMesh with iterations=0, so the positions keep their bits."""
        return self.SmoothMesh(mesh, iterations=0)

    # --- mesh views (bslam_render_mesh)
    def RenderMesh(self, mesh, global_T_camera, camera=None, min_depth=0.05, max_depth=50.0, cull_backfaces=True, views=("depth", "color")):
        """Views of `mesh` (a dict with positions and triangles and optionally normals and colors: the result of ExtractMesh, SmoothMesh,
        SimplifyMesh, DecimateMesh or LoadPLY) from the pose global_T_camera (abi.SE3f) with `camera` (abi.Camera4f, pixel-corner;
        default: the depth camera): the nearest triangle per pixel.  Returns the dict of RenderModel, where "index" holds triangle ids,
        "color" the perspective-correct vertex colours and "normal" the interpolated vertex normals -- face normals for a mesh without
        normals.  A triangle with a vertex outside [min_depth, max_depth] metres is dropped, not clipped; cull_backfaces draws only
        triangles seen counter-clockwise, i.e. an extracted mesh from free space.  "color" of a mesh without colours is a ValueError."""
        params, w, h = self._view_camera(camera)
        out = _alloc_views(views, ("depth", "index", "color", "normal"), h, w)
        pos, nrm, col, tri, _ = self._mesh_arrays(mesh, "RenderMesh")
        if "color" in out and col is None:
            raise ValueError("RenderMesh: a colour view needs a mesh with colours")
        ptr = lambda name, pointer: pointer(out[name]) if name in out else None
        out["camera_T_global"] = np.zeros((3, 4), np.float32)
        options = np.array([min_depth, max_depth], np.float32)
        self._check(self.L.bsh_render_mesh(self._ba, self.stream, len(pos), _f(pos), None if nrm is None else _f(nrm), None if col is None else _u8(col), len(tri),
                                           _u32(tri), _f(pose7(global_T_camera)), _f(params), w, h, _f(options), 1 if cull_backfaces else 0, ptr("depth", _u16),
                                           ptr("index", _u32), ptr("color", _u8), ptr("normal", _f), _f(out["camera_T_global"])))
        return out

    # --- mesh simplification (bslam_simplify_mesh)
    def SimplifyMesh(self, mesh, cell_size, origin=None):
        """Vertex clustering of `mesh` (the dict of ExtractMesh or LoadPLY) on a uniform grid of cells of cell_size: all vertices of a
        cell become one vertex (the mean position, the normalised sum of the normals, the rounded mean colour), triangles are remapped
        and those whose corners no longer differ are dropped.  -> dict with the keys of ExtractMesh (normals / colors None where the
        input has none, colors with the input's channel count) plus vertex_cluster (V,) u32, the new vertex of every input vertex.
        New vertices are ordered by cell (z, then y, then x); kept triangles keep their order and orientation.  origin (3,): the
        grid's corner, default the per-axis minimum of the positions; every vertex has to lie at or above it and within 2^21 cells.
        A mesh without triangles is a point cloud: voxel-grid down-sampling."""
        pos, nrm, col, tri, channels = self._mesh_arrays(mesh, "SimplifyMesh")
        if origin is None:
            origin = pos.min(axis=0) if len(pos) else np.zeros(3, np.float32)
        o = np.ascontiguousarray(origin, np.float32).reshape(3)
        counts = (C.c_uint64 * 2)()
        self._check(self.L.bsh_simplify_mesh(self._ba, self.stream, len(pos), _f(pos), None if nrm is None else _f(nrm), None if col is None else _u8(col),
                                             len(tri), _u32(tri), _f(o), float(cell_size), counts))
        V, T = int(counts[0]), int(counts[1])
        out = dict(positions=np.zeros((V, 3), np.float32), normals=None if nrm is None else np.zeros((V, 3), np.float32),
                   colors=None if col is None else np.zeros((V, 4), np.uint8), triangles=np.zeros((T, 3), np.uint32), vertex_cluster=np.zeros(len(pos), np.uint32))
        self._check(self.L.bsh_simplified_copy(_f(out["positions"]), None if nrm is None else _f(out["normals"]), None if col is None else _u8(out["colors"]),
                                               _u32(out["triangles"]), _u32(out["vertex_cluster"])))
        if col is not None and channels == 3:
            out["colors"] = np.ascontiguousarray(out["colors"][:, :3])
        return out

    # --- mesh repair (bslam_clean_mesh, bslam_mesh_topology, bslam_fill_mesh_holes)
    def _mesh_result(self, V, T, nrm, col, **extra):
        """The zeroed dict of an operator's result: the keys of ExtractMesh, normals / colors None where the input has none."""
        return dict(positions=np.zeros((V, 3), np.float32), normals=None if nrm is None else np.zeros((V, 3), np.float32),
                    colors=None if col is None else np.zeros((V, 4), np.uint8), triangles=np.zeros((T, 3), np.uint32), **extra)

    def CleanMesh(self, mesh, weld=True, remove_duplicates=True, remove_unreferenced=True):
        """`mesh` (the dict of ExtractMesh or LoadPLY) without what it should not hold.  weld: vertices with equal coordinates (-0.0
        equals 0.0) become the one with the smallest id, whose normal and colour stay -- a triangle soup gets its shared vertices back.
        Triangles that then repeat a vertex are dropped.  remove_duplicates: of the triangles on the same three vertices, whatever their
        orientation, the first stays.  remove_unreferenced: vertices that no surviving triangle names are dropped (never those of a mesh
        without triangles).  What stays keeps its order and its bits, so a clean mesh comes back identical.  -> dict with the keys of
        ExtractMesh (normals / colors None where the input has none, colors with the input's channel count) plus vertex_map (V,) u32
        and triangle_map (T,) u32 -- the output id of every input vertex and triangle, 0xFFFFFFFF where dropped -- and report, a dict
        of welded_vertices, unreferenced_vertices, degenerate_triangles and duplicate_triangles."""
        pos, nrm, col, tri, channels = self._mesh_arrays(mesh, "CleanMesh")
        counts = (C.c_uint64 * 6)()
        flags = (C.c_int * 3)(int(bool(weld)), int(bool(remove_duplicates)), int(bool(remove_unreferenced)))
        self._check(self.L.bsh_clean_mesh(self._ba, self.stream, len(pos), _f(pos), None if nrm is None else _f(nrm), None if col is None else _u8(col), len(tri),
                                          _u32(tri), flags, counts))
        out = self._mesh_result(int(counts[0]), int(counts[1]), nrm, col, vertex_map=np.zeros(len(pos), np.uint32), triangle_map=np.zeros(len(tri), np.uint32),
                                report=dict(welded_vertices=int(counts[2]), unreferenced_vertices=int(counts[3]), degenerate_triangles=int(counts[4]),
                                            duplicate_triangles=int(counts[5])))
        self._check(self.L.bsh_cleaned_copy(_f(out["positions"]), None if nrm is None else _f(out["normals"]), None if col is None else _u8(out["colors"]),
                                            _u32(out["triangles"]), _u32(out["vertex_map"]), _u32(out["triangle_map"])))
        if col is not None and channels == 3:
            out["colors"] = np.ascontiguousarray(out["colors"][:, :3])
        return out

    def MeshTopology(self, mesh, per_slot=False):
        """The census of the edges and boundary loops of `mesh` (the dict of ExtractMesh or LoadPLY; triangles that repeat a vertex
        are refused: CleanMesh first) -> dict of referenced_vertices, unique_edges, boundary_edges (used by one triangle),
        interior_edges (by two), nonmanifold_edges (by more), inconsistent_edges (interior, and both triangles run along it the same
        way), blocked_vertices (boundary vertices that do not have exactly one boundary edge in and one out), loops, longest_loop,
        loop_edges, open_boundary_slots (boundary edges on no loop), euler = referenced_vertices - unique_edges + triangles, components
        (of MeshComponents, vertices without a triangle included), and closed (no boundary and no non-manifold edge), manifold_edges
        (no non-manifold edge), oriented (no inconsistent edge).  per_slot=True adds edge_uses (T, 3) u32 -- the uses of the edge from
        corner k to corner k + 1 -- and loop_of_slot (T, 3) u32: the smallest slot 3 t + k of the boundary loop that edge lies on,
        0xFFFFFFFF for every other."""
        pos, _, _, tri, _ = self._mesh_arrays(mesh, "MeshTopology")
        report = abi.MeshReport()
        uses = np.zeros((len(tri), 3), np.uint32) if per_slot else None
        loops = np.zeros((len(tri), 3), np.uint32) if per_slot else None
        self._check(self.L.bsh_mesh_topology(self._ba, self.stream, len(pos), len(tri), _u32(tri), C.byref(report), None if uses is None else _u32(uses),
                                             None if loops is None else _u32(loops)))
        out = report.as_dict()
        labels, _ = self.MeshComponents(dict(positions=pos, triangles=tri))
        out["components"] = int((labels == np.arange(len(pos), dtype=np.uint32)).sum())
        out["closed"] = out["boundary_edges"] == 0 and out["nonmanifold_edges"] == 0
        out["manifold_edges"] = out["nonmanifold_edges"] == 0
        out["oriented"] = out["inconsistent_edges"] == 0
        if per_slot:
            out["edge_uses"], out["loop_of_slot"] = uses, loops
        return out

    def FillHoles(self, mesh, max_hole_edges):
        """`mesh` (the dict of ExtractMesh or LoadPLY) with every boundary loop of at most max_hole_edges (3 .. 4096) edges closed by
        a new vertex at the centroid of the loop's vertices (mean colour, normalised sum of the normals) and a fan of triangles that
        continues the orientation across the boundary.  Larger loops -- the outer rim of an open scan -- stay, and so does every
        boundary through a vertex where more than two boundary edges meet.  The input comes first and unchanged; the new vertices and
        triangles follow.  -> dict with the keys of ExtractMesh plus filled_holes."""
        if not 0 <= int(max_hole_edges) <= 0xFFFFFFFF:
            raise ValueError("FillHoles: max_hole_edges must fit 32 bits")
        pos, nrm, col, tri, channels = self._mesh_arrays(mesh, "FillHoles")
        counts = (C.c_uint64 * 3)()
        self._check(self.L.bsh_fill_mesh_holes(self._ba, self.stream, len(pos), _f(pos), None if nrm is None else _f(nrm), None if col is None else _u8(col), len(tri),
                                               _u32(tri), int(max_hole_edges), counts))
        out = self._mesh_result(int(counts[0]), int(counts[1]), nrm, col, filled_holes=int(counts[2]))
        self._check(self.L.bsh_filled_copy(_f(out["positions"]), None if nrm is None else _f(out["normals"]), None if col is None else _u8(out["colors"]),
                                           _u32(out["triangles"])))
        if col is not None and channels == 3:
            out["colors"] = np.ascontiguousarray(out["colors"][:, :3])
        return out

    # --- mesh orientation (bslam_orient_mesh)
    def OrientMesh(self, mesh, mode="majority", recompute_normals=False, report=False):
        """`mesh` (the dict of ExtractMesh or LoadPLY; triangles that repeat a vertex are refused: CleanMesh first) with one winding
        per patch.  A patch is a set of triangles connected over edges that exactly two triangles use; where it can be oriented at all,
        its triangles are flipped -- (a, b, c) becomes (a, c, b) -- until no such edge is run the same way twice, and `mode` picks the
        side: "majority" keeps the winding most of its triangles have (the fewest flips; a tie keeps that of its first triangle),
        "normals" the one the mesh's vertex normals vote for, "volume" the one that encloses a positive volume (closed patches; an
        open one, and any vote that does not decide, falls back to "majority").  A patch that cannot be oriented (a Moebius band) stays
        as it is.  -> the dict of ExtractMesh with new triangles -- positions, normals and colors are the input's -- plus flipped (T,)
        bool, patch_of_triangle (T,) u32, the smallest triangle id of every triangle's patch, and, with report=True, report: a dict of
        patches, orientable_patches, nonorientable_patches, closed_patches, seams, disagreeing_seams_before, disagreeing_seams_after,
        flipped_triangles, inverted_patches and fallback_patches.  recompute_normals=True replaces the normals by MeshNormals of the
        result."""
        if mode not in abi.ORIENT_MODES:
            raise ValueError("OrientMesh: mode must be 'majority', 'normals' or 'volume'")
        pos, nrm, col, tri, channels = self._mesh_arrays(mesh, "OrientMesh")
        if mode == "normals" and nrm is None:
            raise ValueError("OrientMesh: the mode 'normals' needs a mesh with normals")
        counts = abi.OrientReport()
        out = dict(positions=pos.copy(), normals=None if nrm is None else nrm.copy(), colors=None if col is None else np.ascontiguousarray(col[:, :channels]),
                   triangles=np.zeros((len(tri), 3), np.uint32), flipped=np.zeros(len(tri), np.uint8), patch_of_triangle=np.zeros(len(tri), np.uint32))
        self._check(self.L.bsh_orient_mesh(self._ba, self.stream, len(pos), _f(pos), None if nrm is None else _f(nrm), len(tri), _u32(tri), abi.ORIENT_MODES[mode],
                                           _u32(out["triangles"]), _u8(out["flipped"]), _u32(out["patch_of_triangle"]), C.byref(counts)))
        out["flipped"] = out["flipped"].astype(bool)
        if recompute_normals:
            out["normals"] = self.MeshNormals(out)["normals"]
        if report:
            out["report"] = counts.as_dict()
        return out

    # --- surface evaluation (bslam_point_mesh_distance)
    @staticmethod
    def _distance_result(distance, triangle, cell, grid):
        return dict(distance=distance, triangle=triangle, cell_size=float(cell.value), grid_cells=int(grid[0]), grid_entries=int(grid[1]))

    def PointMeshDistance(self, points, mesh, max_distance, cell_size=None, max_grid_entries=1 << 28):
        """Distance of every point (n, 3) to the nearest triangle of `mesh` within max_distance: dict of distance (n,) f32 (+inf
        beyond max_distance), triangle (n,) u32 (0xFFFFFFFF there), cell_size (the grid cell used), grid_cells, grid_entries.
        mesh: the dict of ExtractMesh or LoadPLY, or {"positions": ...} alone for a point cloud (a mesh without triangles counts
        as one too): every vertex then is the triangle (i, i, i).  cell_size None: max_distance, doubled while the grid exceeds
        max_grid_entries."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        pos = np.ascontiguousarray(mesh["positions"], np.float32).reshape(-1, 3)
        tri = mesh.get("triangles")
        if tri is None or len(tri) == 0:
            tri = np.repeat(np.arange(len(pos), dtype=np.uint32)[:, None], 3, axis=1)
        tri = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
        distance, triangle = np.zeros(len(pts), np.float32), np.zeros(len(pts), np.uint32)
        cell, grid = C.c_float(), (C.c_uint64 * 2)()
        self._check(self.L.bsh_point_mesh_distance(self._ba, self.stream, len(pts), _f(pts), len(pos), _f(pos), len(tri), _u32(tri), float(max_distance),
                                                   0.0 if cell_size is None else float(cell_size), int(max_grid_entries), _f(distance), _u32(triangle),
                                                   C.byref(cell), grid))
        return self._distance_result(distance, triangle, cell, grid)

    def NearestTriangle(self, points, mesh, max_distance=None):
        """Distance of every point (n, 3) to the nearest triangle of `mesh` through a bounding-volume hierarchy
        (bslam_nearest_triangle): any max_distance > 0, None for no radius at all -- every point then hits a mesh that has a valid
        triangle.  dict of distance (n,) f32 (+inf beyond max_distance), triangle (n,) u32 (0xFFFFFFFF there), leaves (the
        triangles with finite coordinates) and height (of the tree).  mesh: as in PointMeshDistance; without triangles every
        vertex is the triangle (i, i, i)."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        pos = np.ascontiguousarray(mesh["positions"], np.float32).reshape(-1, 3)
        tri = mesh.get("triangles")
        if tri is None or len(tri) == 0:
            tri = np.repeat(np.arange(len(pos), dtype=np.uint32)[:, None], 3, axis=1)
        tri = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
        distance, triangle = np.zeros(len(pts), np.float32), np.zeros(len(pts), np.uint32)
        tree = (C.c_uint32 * 2)()
        self._check(self.L.bsh_nearest_triangle(self._ba, self.stream, len(pts), _f(pts), len(pos), _f(pos), len(tri), _u32(tri),
                                                float("inf") if max_distance is None else float(max_distance), _f(distance), _u32(triangle), tree))
        return dict(distance=distance, triangle=triangle, leaves=int(tree[0]), height=int(tree[1]))

    # --- mesh rays (bslam_mesh_rays, bslam_mesh_visibility)
    def RayCastMesh(self, origins, directions, mesh, t_min=0.0, t_max=None, any_hit=False):
        """What every ray origins[i] + t * directions[i] ((n, 3) each; directions need not be normalised, t is in their units) hits
        on `mesh` (the dict of ExtractMesh or LoadPLY) for t in [t_min, t_max] -- scalars or (n,) arrays; t_max None: +inf.  Both
        faces hit.  -> dict of t (n,) f32 (+inf: a miss), triangle (n,) u32 (0xFFFFFFFF), uv (n, 2) f32 (the hit is (1 - u - v) a +
        u b + v c), front (n,) bool (the ray meets the counter-clockwise side), leaves and height of the tree; with any_hit=True a
        dict of hit (n,) bool, leaves, height: whether anything is hit, which is cheaper and all an occlusion test needs.  The bits
        are those of the rule in include/badslam_hip.h "Mesh rays": among equal t the lowest triangle."""
        org = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        dirs = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        if len(org) != len(dirs):
            raise ValueError("RayCastMesh: one direction per origin")
        pos = np.ascontiguousarray(mesh["positions"], np.float32).reshape(-1, 3)
        tri = mesh.get("triangles")
        tri = np.zeros((0, 3), np.uint32) if tri is None else np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
        n = len(org)
        t_range = None
        if np.ndim(t_min) != 0 or np.ndim(t_max) != 0 or float(t_min) != 0.0 or t_max is not None:
            t_range = np.empty((n, 2), np.float32)
            t_range[:, 0] = t_min
            t_range[:, 1] = np.inf if t_max is None else t_max
        tree = (C.c_uint32 * 2)()
        if any_hit:
            hit = np.zeros(n, np.uint8)
            self._check(self.L.bsh_mesh_rays(self._ba, self.stream, n, _f(org), _f(dirs), None if t_range is None else _f(t_range), len(pos), _f(pos), len(tri),
                                             _u32(tri), 1, None, None, None, None, _u8(hit), tree))
            return dict(hit=hit.astype(bool), leaves=int(tree[0]), height=int(tree[1]))
        t, triangle, uv, front = np.zeros(n, np.float32), np.zeros(n, np.uint32), np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
        self._check(self.L.bsh_mesh_rays(self._ba, self.stream, n, _f(org), _f(dirs), None if t_range is None else _f(t_range), len(pos), _f(pos), len(tri),
                                         _u32(tri), 0, _f(t), _u32(triangle), _f(uv), _u8(front), None, tree))
        return dict(t=t, triangle=triangle, uv=uv, front=front.astype(bool), leaves=int(tree[0]), height=int(tree[1]))

    def MeshVisibility(self, points, mesh, poses, camera=None, min_depth=0.05, max_depth=50.0, margin=0.02, normals=None):
        """From how many of the views `poses` (global_T_camera each, as for RenderMesh: abi.SE3f, or 4 x 4 matrices) every point
        (n, 3) is seen past `mesh`: inside the view's image (`camera`, abi.Camera4f, default the depth camera) at a depth in
        [min_depth, max_depth], facing it if `normals` (n, 3) are given, and with nothing of the mesh on the segment from the
        camera centre to the point short of `margin` before it.  -> dict of count (n,) u32, first (n,) u32 (the lowest view that
        sees the point, 0xFFFFFFFF for none), leaves, height.  view_rows(poses) are the views the kernel is given."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if nrm is not None and len(nrm) != len(pts):
            raise ValueError("MeshVisibility: one normal per point")
        pos = np.ascontiguousarray(mesh["positions"], np.float32).reshape(-1, 3)
        tri = mesh.get("triangles")
        tri = np.zeros((0, 3), np.uint32) if tri is None else np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
        params, w, h = self._view_camera(camera)
        rows, centres = view_rows(list(poses))
        options = np.array([min_depth, max_depth, margin], np.float32)
        count, first, tree = np.zeros(len(pts), np.uint32), np.zeros(len(pts), np.uint32), (C.c_uint32 * 2)()
        self._check(self.L.bsh_mesh_visibility(self._ba, self.stream, len(pts), _f(pts), None if nrm is None else _f(nrm), len(pos), _f(pos), len(tri), _u32(tri),
                                               len(rows), _f(rows), _f(centres), _f(params), w, h, _f(options), _u32(count), _u32(first), tree))
        return dict(count=count, first=first, leaves=int(tree[0]), height=int(tree[1]))

    def SurfelMeshDistance(self, max_distance, cell_size=None, max_grid_entries=1 << 28):
        """PointMeshDistance of the centres of the valid surfels (the positions of ExportToPointCloud, in its order) against the mesh
        the last ExtractMesh returned, which is still on the device.  Raises if no mesh was extracted."""
        count, cell, grid = C.c_uint64(), C.c_float(), (C.c_uint64 * 2)()
        self._check(self.L.bsh_surfel_mesh_distance(self._ba, self.stream, float(max_distance), 0.0 if cell_size is None else float(cell_size), int(max_grid_entries),
                                                    C.byref(count), C.byref(cell), grid))
        distance, triangle = np.zeros(count.value, np.float32), np.zeros(count.value, np.uint32)
        self._check(self.L.bsh_distance_copy(_f(distance), _u32(triangle)))
        return self._distance_result(distance, triangle, cell, grid)

    # --- surface sampling (bslam_sample_mesh)
    def SampleMesh(self, mesh, density=None, spacing=None, seed=0):
        """Points drawn uniformly by area from `mesh` (the dict of ExtractMesh or LoadPLY): dict of positions (N, 3) f32, normals
        (N, 3) f32 (the triangle's) and triangle (N,) u32, ordered by triangle.  density: samples per square unit; each triangle gets
        area * density samples on average, however small it is.  spacing: shorthand for density = 1 / spacing^2.  Exactly one of
        the two has to be given.  The samples are a function of (seed, triangle, ordinal) alone: two calls give identical bits.
        Degenerate triangles and a mesh without triangles (a point cloud) yield nothing."""
        if (density is None) == (spacing is None):
            raise ValueError("SampleMesh: give exactly one of density and spacing")
        if density is None:
            density = 1.0 / (float(spacing) * float(spacing))
        pos = np.ascontiguousarray(mesh["positions"], np.float32).reshape(-1, 3)
        tri = mesh.get("triangles")
        tri = np.zeros((0, 3), np.uint32) if tri is None else np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
        count = C.c_uint64()
        self._check(self.L.bsh_sample_mesh(self._ba, self.stream, len(pos), _f(pos), len(tri), _u32(tri), float(density), int(seed) & 0xFFFFFFFF, C.byref(count)))
        out = dict(positions=np.zeros((count.value, 3), np.float32), normals=np.zeros((count.value, 3), np.float32), triangle=np.zeros(count.value, np.uint32))
        self._check(self.L.bsh_samples_copy(_f(out["positions"]), _f(out["normals"]), _u32(out["triangle"])))
        return out

    # --- surface registration (bslam_registration_prepare / bslam_registration_step)
    REGISTRATION_PLANE, REGISTRATION_POINT = 0, 1

    def RegisterPoints(self, points, mesh, max_distance, min_distance=None, initial=None, mode=None, huber=None, shrink=0.5, iterations_per_stage=20,
                       cell_size=None, max_grid_entries=1 << 28):
        """The rigid motion that lays `points` (n, 3) onto `mesh` (the dict of ExtractMesh or LoadPLY; without triangles a point
        cloud), by iterative closest point from `initial` (4 x 4, default identity): stages at the search radii max_distance, shrink
        * that, ... down to min_distance (default max_distance / 8), each until the step is below 10 um / 1 urad or
        iterations_per_stage steps were taken.  mode: REGISTRATION_PLANE (point to plane; the default for a mesh with triangles) or
        REGISTRATION_POINT (point to nearest point of the surface; the default for a cloud).  huber: the Huber width of the
        residuals (default: half the radius of the stage; float("inf"): none).  These defaults are provisional: they were tried on
        synthetic scenes only.
        -> dict of target_T_source (4, 4) float64, iterations, converged (the last stage ended by the convergence test), reason,
        history (a dict per step: radius, hits, used, cost, rmse, step_translation, step_rotation) and the grid of the prepared
        mesh (cell_size, grid_cells, grid_entries).  Fewer than 6 pairs or a singular system end the loop with converged False
        and the last valid transform; nothing is raised for them."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        pos = np.ascontiguousarray(mesh["positions"], np.float32).reshape(-1, 3)
        tri = mesh.get("triangles")
        tri = np.zeros((0, 3), np.uint32) if tri is None else np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
        options = np.array([max_distance, 0.0 if min_distance is None else min_distance, -1 if mode is None else int(mode), 0.0 if huber is None else huber,
                            shrink, iterations_per_stage, 0.0 if cell_size is None else cell_size, max_grid_entries], np.float64)
        start = np.ascontiguousarray(np.eye(4) if initial is None else initial, np.float64).reshape(4, 4)
        transform, status, grid = np.zeros((4, 4), np.float64), (C.c_int32 * 3)(), np.zeros(3, np.float64)
        d = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        self._check(self.L.bsh_register_points(self._ba, self.stream, len(pts), _f(pts), len(pos), _f(pos), len(tri), _u32(tri), d(options), d(start), d(transform),
                                               status, d(grid)))
        rows = np.zeros((status[0], 7), np.float64)
        self._check(self.L.bsh_registration_history(d(rows)))
        history = [dict(radius=float(r[0]), hits=int(r[1]), used=int(r[2]), cost=float(r[3]), rmse=float(r[4]), step_translation=float(r[5]),
                        step_rotation=float(r[6])) for r in rows]
        return dict(target_T_source=transform, iterations=int(status[0]), converged=bool(status[1]), reason=self.L.bsh_registration_reason(status[2]).decode(),
                    history=history, cell_size=float(grid[0]), grid_cells=int(grid[1]), grid_entries=int(grid[2]))

    def Volume(self):
        """Download of the fused volume: dict of origin (3,), voxel_size, truncation, dims (nx, ny, nz) and the arrays tsdf f32,
        count u32 of shape (nz, ny, nx) and color u8 (nz, ny, nx, 4)."""
        dims, fl = (C.c_int * 3)(), np.zeros(5, np.float32)
        self._check(self.L.bsh_volume(self._ba, self.stream, dims, _f(fl), None, None, None))
        nx, ny, nz = dims[0], dims[1], dims[2]
        tsdf, count, color = np.zeros((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.uint32), np.zeros((nz, ny, nx, 4), np.uint8)
        self._check(self.L.bsh_volume(self._ba, self.stream, dims, _f(fl), _f(tsdf), _u32(count), _u8(color)))
        return dict(origin=fl[:3].copy(), voxel_size=float(fl[3]), truncation=float(fl[4]), dims=(nx, ny, nz), tsdf=tsdf, count=count, color=color)

    def RenderVolume(self, global_T_camera, camera=None, min_depth=0.05, max_depth=50.0, step=None, min_count=1, views=("depth", "color")):
        """Views of the volume of the last FuseKeyframes from the pose global_T_camera (abi.SE3f) with `camera` (abi.Camera4f,
        pixel-corner; default: the depth camera): per pixel the first front-facing zero crossing of the interpolated volume along
        the ray, sampled every `step` metres of depth (default: the voxel size; at most 65536 steps) between min_depth and
        max_depth, over the samples seen by at least min_count keyframes.  Returns the dict of RenderModel with the entries named
        in `views` -- "depth" (h, w) uint16, "color" (h, w, 4) uint8, "normal" (h, w, 3) float32 in the camera frame, 0 where
        nothing is hit -- and "global_T_camera" (3, 4) float32, the matrix the kernel took.  Raises if nothing was fused."""
        params, w, h = self._view_camera(camera)
        out = _alloc_views(views, ("depth", "color", "normal"), h, w)
        ptr = lambda name, pointer: pointer(out[name]) if name in out else None
        out["global_T_camera"] = np.zeros((3, 4), np.float32)
        options = np.array([min_depth, max_depth, 0.0 if step is None else step], np.float32)
        self._check(self.L.bsh_render_volume(self._ba, self.stream, _f(pose7(global_T_camera)), _f(params), w, h, _f(options), int(min_count), ptr("depth", _u16),
                                             ptr("color", _u8), ptr("normal", _f), _f(out["global_T_camera"])))
        return out

    def upload_keyframe_depth(self, kf_id, depth):
        d = np.ascontiguousarray(depth, np.uint16)
        self._check(self.L.bsh_upload_keyframe_depth(self._ba, self.stream, kf_id, d.ctypes.data_as(C.POINTER(C.c_uint16))))

    def upload_keyframe_normals(self, kf_id, normals):
        d = np.ascontiguousarray(normals, np.uint16)
        self._check(self.L.bsh_upload_keyframe_normals(self._ba, self.stream, kf_id, d.ctypes.data_as(C.POINTER(C.c_uint16))))

    def set_options(self, batched_pose_optimization=True, pcg_gauge_keyframe=-1, texture_mode=abi.TEX_FIXED_POINT_1_8, scheme_end_tasks=True):
        self._check(self.L.bsh_set_options(self._ba, int(batched_pose_optimization), pcg_gauge_keyframe, texture_mode))
        self._check(self.L.bsh_set_scheme_end_tasks(self._ba, int(scheme_end_tasks)))

    def set_timings_file(self, path):
        """--save_timings: one block of BA_* lines per BA iteration (BS/direct_ba_alternating.cc:630-688); None stops."""
        self._check(self.L.bsh_set_timings_file(self._ba, path.encode() if path else None))

    def CreateSurfelsForKeyframe(self, filter_new_surfels, kf_id):
        self._check(self.L.bsh_create_surfels_for_keyframe(self._ba, self.stream, int(filter_new_surfels), kf_id))

    def set_allreduce(self, callback):
        self._check(self.L.bsh_set_allreduce(self._ba, callback, None))

    def InitComm(self, unique_id, rank, world_size):
        """RCCL communicator inside this DirectBA's kernel context (unique_id: the 128 bytes of badslam_amd.comm_unique_id() of rank 0)."""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._check(self.L.bsh_comm_init(self._ba, buf, rank, world_size))

    def DestroyComm(self):
        self._check(self.L.bsh_comm_destroy(self._ba))

    def EstimateFramePose(self, kf_id, global_T_frame_initial_estimate):
        out = np.zeros(7, np.float32)
        self._check(self.L.bsh_estimate_frame_pose(self._ba, self.stream, kf_id, _f(pose7(global_T_frame_initial_estimate)), _f(out)))
        return se3f_from7(out)

    def BundleAdjustment(self, optimize_depth_intrinsics, optimize_color_intrinsics, do_surfel_updates, optimize_poses, optimize_geometry,
                         min_iterations, max_iterations, use_pcg, active_keyframe_window_start, active_keyframe_window_end,
                         increase_ba_iteration_count, pcg_max_inner_iterations=30):
        it, conv = C.c_int(), C.c_int()
        self._check(self.L.bsh_bundle_adjustment(self._ba, self.stream, int(optimize_depth_intrinsics), int(optimize_color_intrinsics),
                                                 int(do_surfel_updates), int(optimize_poses), int(optimize_geometry), min_iterations,
                                                 max_iterations, int(use_pcg), active_keyframe_window_start, active_keyframe_window_end,
                                                 int(increase_ba_iteration_count), pcg_max_inner_iterations, C.byref(it), C.byref(conv)))
        return it.value, bool(conv.value)

    def ComputeCost(self, active_surfels_only=False):
        """The BA objective at the current poses, intrinsics and cfactors (bslam_compute_ba_cost): dict with keyframe_ids (n,),
        cost (n, 2) float32 [Tukey depth sum, kDescWeight * Huber sum of both descriptor residuals], counts (n, 2) uint32
        [depth-associated pairs, pairs with valid descriptor residuals], depth_total, descriptor_total and total (float64)."""
        cap = max(1, self.keyframe_count())
        ids, cost, counts = np.zeros(cap, np.int32), np.zeros((cap, 2), np.float32), np.zeros((cap, 2), np.uint32)
        n, totals = C.c_int(), np.zeros(2, np.float64)
        self._check(self.L.bsh_compute_cost(self._ba, self.stream, int(active_surfels_only), cap, ids.ctypes.data_as(C.POINTER(C.c_int)), _f(cost),
                                            counts.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n), totals.ctypes.data_as(C.POINTER(C.c_double))))
        k = n.value
        return dict(keyframe_ids=ids[:k], cost=cost[:k], counts=counts[:k], depth_total=float(totals[0]), descriptor_total=float(totals[1]),
                    total=float(totals[0] + totals[1]))

    def SetCostTracking(self, enable):
        """BundleAdjustment records the objective before its first and after every iteration (cost_history); off by default."""
        self._check(self.L.bsh_set_cost_tracking(self._ba, int(enable)))

    @property
    def cost_history(self):
        """(iterations + 1, 2) float64 [depth total, descriptor total] of the last BundleAdjustment call with cost tracking on."""
        n = C.c_int()
        self._check(self.L.bsh_cost_history(self._ba, 0, None, C.byref(n)))
        out = np.zeros((max(1, n.value), 2), np.float64)
        self._check(self.L.bsh_cost_history(self._ba, n.value, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)))
        return out[:n.value]

    def set_intrinsics(self, color4=None, depth4=None, a=0.0):
        c = None if color4 is None else _f(np.ascontiguousarray(color4, np.float32))
        d = None if depth4 is None else _f(np.ascontiguousarray(depth4, np.float32))
        self._check(self.L.bsh_set_intrinsics(self._ba, c, d, a))

    def cfactor(self, shape):
        out = np.zeros(shape, np.float32)
        self._check(self.L.bsh_get_cfactor(self._ba, self.stream, _f(out)))
        return out

    def intrinsics(self):
        c, d, a = np.zeros(4, np.float32), np.zeros(4, np.float32), C.c_float()
        self._check(self.L.bsh_get_intrinsics(self._ba, _f(c), _f(d), C.byref(a)))
        return c, d, a.value
