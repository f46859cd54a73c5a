"""-m gpu return codes of the keyframe-table entry points on the arguments their shared setup validates: a null context,
surfels_size above the buffer width, an empty keyframe list, no surfels, a keyframe image that does not match the camera and
a missing colour camera.  0: the call succeeds (with or without device work), -1: BSLAM_ERR_INVALID_ARGUMENT."""
import ctypes as C

import numpy as np
import pytest

from badslam_amd import abi
from tests import bso, scenes

pytestmark = pytest.mark.gpu

OK, INVALID = 0, -1
CASES = ("null_context", "size_over_width", "empty_list", "no_surfels", "image_mismatch", "no_color_camera")

# entry point -> expected code per case; a case the call has no argument for is left out
EXPECTED = {
    "assign_colors": (INVALID, INVALID, OK, OK, INVALID, INVALID),
    "debug_count_pairs": (INVALID, INVALID, INVALID, INVALID, INVALID, None),
    "accumulate_pose_estimation_coeffs": (INVALID, INVALID, None, INVALID, INVALID, INVALID),
    "accumulate_pose_coeffs_batched": (INVALID, INVALID, INVALID, INVALID, INVALID, INVALID),
    "estimate_frame_poses_batched": (INVALID, INVALID, INVALID, OK, INVALID, INVALID),
    "update_surfel_activation": (INVALID, INVALID, OK, OK, INVALID, None),
    "update_surfel_normals": (INVALID, INVALID, OK, OK, INVALID, None),
    "optimize_geometry_iteration": (INVALID, INVALID, OK, OK, INVALID, INVALID),
    "debug_association": (INVALID, INVALID, INVALID, OK, INVALID, None),
    "debug_pose_residuals": (INVALID, INVALID, INVALID, OK, INVALID, INVALID),
    "debug_ba_cost_descriptor_residuals": (INVALID, INVALID, INVALID, OK, INVALID, INVALID),
    "compute_ba_cost": (INVALID, INVALID, OK, OK, INVALID, INVALID),
    "pcg_init": (INVALID, INVALID, INVALID, OK, INVALID, INVALID),
    "pcg_step1": (INVALID, INVALID, INVALID, OK, INVALID, INVALID),
    "optimize_intrinsics": (INVALID, INVALID, INVALID, OK, INVALID, INVALID),
    "debug_optimize_intrinsics": (INVALID, INVALID, INVALID, OK, INVALID, INVALID),
    "delete_surfels_and_update_radii": (INVALID, INVALID, OK, OK, INVALID, None),
}
PARAMS = [(name, case, codes[i]) for name, codes in EXPECTED.items() for i, case in enumerate(CASES) if codes[i] is not None]


@pytest.fixture(scope="module")
def scene():
    return scenes.synthetic_scene(4, seed=5, use_depth_residuals=True, use_descriptor_residuals=True)


def call(name, scene, case):
    import torch
    import badslam_amd
    from tests.gpu_util import Hip, HipPCG, stream_ptr
    hip = Hip(scene.to_device())
    L, d = hip.L, hip.d
    ctx = None if case == "null_context" else hip.ctx.handle
    s = stream_ptr()
    color = None if case == "no_color_camera" else C.byref(scene.color_camera)
    depth = C.byref(scene.depth_camera)
    dp, sb, ab = d.depth_params(), d.surfel_buf(), d.active_buf()
    size = {"size_over_width": scene.max_surfels + 1, "no_surfels": 0}.get(case, scene.surfels_size)
    K = len(scene.keyframes)
    kfs = d.keyframe_views()
    if case == "image_mismatch":
        for k in range(K):
            kfs[k].depth.width += 1
    if case == "empty_list":
        K, kfs = 0, None
    kf = C.byref(kfs[0]) if kfs is not None else None
    out = torch.zeros((max(1, scene.max_surfels), 8), dtype=torch.float32, device=d.device)
    out_p = C.c_void_p(out.data_ptr())
    f32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    no_hook = C.cast(None, abi.ALLREDUCE_FN)

    if name == "assign_colors":
        rc = L.bslam_assign_colors(ctx, s, color, depth, C.byref(dp), K, kfs, size, C.byref(sb))
    elif name == "debug_count_pairs":
        a, b = C.c_uint64(), C.c_uint64()
        rc = L.bslam_debug_count_pairs(ctx, s, depth, C.byref(dp), K, kfs, size, C.byref(sb), C.byref(a), C.byref(b))
    elif name == "accumulate_pose_estimation_coeffs":
        v = d.keyframe_view(0)
        if case == "image_mismatch":
            v.depth.width += 1
        H, b = np.zeros(21, np.float32), np.zeros(6, np.float32)
        rc = L.bslam_accumulate_pose_estimation_coeffs(ctx, s, 1, 1, color, depth, C.byref(dp), C.byref(v.depth), C.byref(v.normals),
                                                       C.byref(v.color), C.byref(v.frame_T_global), size, C.byref(sb), 0, None, None, f32(H), f32(b))
    elif name == "accumulate_pose_coeffs_batched":
        rc = L.bslam_accumulate_pose_coeffs_batched(ctx, s, 1, 1, color, depth, C.byref(dp), K, kfs, size, C.byref(sb), None, None)
    elif name == "estimate_frame_poses_batched":
        poses = (abi.SE3f * len(scene.keyframes))()
        for k, kfr in enumerate(scene.keyframes):
            C.memmove(C.byref(poses[k]), C.byref(kfr.global_T_frame), C.sizeof(abi.SE3f))
        rc = L.bslam_estimate_frame_poses_batched(ctx, s, 1, 1, color, depth, C.byref(dp), K, kfs, size, C.byref(sb), 2, poses, None, None,
                                                  no_hook, None)
    elif name == "update_surfel_activation":
        rc = L.bslam_update_surfel_activation(ctx, s, depth, C.byref(dp), K, kfs, size, C.byref(sb), C.byref(ab))
    elif name == "update_surfel_normals":
        rc = L.bslam_update_surfel_normals(ctx, s, depth, C.byref(dp), K, kfs, size, C.byref(sb), C.byref(ab))
    elif name == "optimize_geometry_iteration":
        rc = L.bslam_optimize_geometry_iteration(ctx, s, 1, 1, color, depth, C.byref(dp), K, kfs, size, C.byref(sb), C.byref(ab))
    elif name == "debug_association":
        rc = L.bslam_debug_association(ctx, s, depth, C.byref(dp), kf, size, C.byref(sb), out_p)
    elif name == "debug_pose_residuals":
        rc = L.bslam_debug_pose_residuals(ctx, s, 1, 1, color, depth, C.byref(dp), kf, size, C.byref(sb), out_p)
    elif name == "debug_ba_cost_descriptor_residuals":
        rc = L.bslam_debug_ba_cost_descriptor_residuals(ctx, s, color, depth, C.byref(dp), kf, size, C.byref(sb), out_p)
    elif name == "compute_ba_cost":
        cost = np.zeros(2 * len(scene.keyframes), np.float32)
        rc = L.bslam_compute_ba_cost(ctx, s, 1, 1, color, depth, C.byref(dp), K, kfs, size, C.byref(sb), C.byref(ab), f32(cost), None,
                                     no_hook, None)
    elif name in ("pcg_init", "pcg_step1"):
        layout = bso.pcg_layout(scene, gauge_keyframe_id=0)
        v = HipPCG(hip, layout).vectors()
        if name == "pcg_init":
            rc = L.bslam_pcg_init(ctx, s, C.byref(layout), color, depth, C.byref(dp), K, kfs, size, C.byref(sb), C.byref(v))
        else:
            rc = L.bslam_pcg_step1(ctx, s, C.byref(layout), color, depth, C.byref(dp), K, kfs, size, C.byref(sb), C.byref(v), 1)
    elif name == "optimize_intrinsics":
        out_c, out_d, a = abi.Camera4f(), abi.Camera4f(), C.c_float(scene.a)
        rc = L.bslam_optimize_intrinsics(ctx, s, 1, 1, K, kfs, color, depth, C.byref(dp), size, C.byref(sb), C.byref(out_c), C.byref(out_d),
                                         C.byref(a))
    elif name == "debug_optimize_intrinsics":
        out_c, out_d, a = abi.Camera4f(), abi.Camera4f(), C.c_float(scene.a)
        x1 = np.zeros(5, np.float32)
        tap = abi.IntrinsicsTap(x1=x1.ctypes.data)   # every other member null
        rc = L.bslam_debug_optimize_intrinsics(ctx, s, 1, 1, K, kfs, color, depth, C.byref(dp), size, C.byref(sb), C.byref(out_c), C.byref(out_d),
                                               C.byref(a), C.byref(tap))
        assert not x1.any(), "a call that does no device work leaves the tap alone"
    elif name == "delete_surfels_and_update_radii":
        count = C.c_uint32(scene.surfels_size)
        rc = L.bslam_delete_surfels_and_update_radii(ctx, s, 1, depth, C.byref(dp), K, kfs, C.byref(count), size, C.byref(sb))
    else:
        raise AssertionError(name)
    torch.cuda.synchronize()
    message = badslam_amd.lib().bslam_last_error()
    del hip
    return rc, message


@pytest.mark.parametrize("name,case,expected", PARAMS)
def test_keyframe_table_call_return_code(scene, name, case, expected):
    rc, message = call(name, scene, case)
    assert rc == expected, (name, case, message)
