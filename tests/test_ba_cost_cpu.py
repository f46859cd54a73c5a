"""CPU checks of the BA objective entry point (bslam_compute_ba_cost): the header, the ctypes table and the built library agree,
and the float64 objective the GPU tests compare against (tests/ba_cost_util.py) is pinned to the oracle's own cost sum."""
import os
import re

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi, build
from tests import ba_cost_util, bso, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bslam_compute_ba_cost", "bslam_debug_ba_cost_descriptor_residuals")


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "badslam_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\);", text, re.S)
    assert m, f"{name} is not declared in include/badslam_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", NEW)
def test_header_abi_table_and_library_agree(name):
    build.build()
    params = _declaration(name)
    assert name in abi.SIGNATURES
    restype, argtypes = abi.SIGNATURES[name]
    assert len(argtypes) == len(params), (name, params)
    assert hasattr(badslam_amd.lib(), name), f"{name} is not exported by the built library"


def test_ba_cost_signature_and_profile_tag():
    params = _declaration("bslam_compute_ba_cost")
    assert params[11].endswith("active_surfels") and params[12] == "float* cost" and params[13] == "uint32_t* counts"
    _, argtypes = abi.SIGNATURES["bslam_compute_ba_cost"]
    assert argtypes[11] is argtypes[10] and argtypes[14] is abi.ALLREDUCE_FN
    header = open(os.path.join(ROOT, "include", "badslam_hip.h")).read()
    assert re.search(r"BSLAM_PROF_BA_COST\s*=\s*7\b", header)


def test_robust_functions():
    r = np.array([0.0, 3.0, -9.99, 10.0, 25.0])
    t = ba_cost_util.tukey_residual(r)
    assert t[0] == 0.0 and np.all(t[3:] == 100.0 / 6.0) and 0 < t[1] < t[2] < 100.0 / 6.0
    h = ba_cost_util.huber_residual(np.array([0.0, -4.0, 10.0, 30.0]))
    assert np.allclose(h, [0.0, 8.0, 50.0, 250.0])


@pytest.mark.parametrize("perturb", [False, True])
def test_float64_objective_matches_the_oracle_cost_on_a_depth_only_scene(oracle, perturb):
    """The oracle adds its Tukey terms in float, in surfel order (oracle/bslam_oracle.c: bso_accumulate_pose_estimation_coeffs):
    1e-5 relative is what that order allows."""
    scene, kf = scenes.pose_geometric_scene(seed=3)
    if perturb:
        kf.global_T_frame = bso.se3_mul(kf.global_T_frame, bso.se3_exp(np.array([0.01, -0.006, 0.004, 0.002, -0.003, 0.001], np.float32)))
    r = scene.accumulate_pose(kf, per_surfel=True, use_depth=True, use_desc=False)
    cost, counts = ba_cost_util.objective_from_probe(r["per_surfel"], True, False)
    assert counts[0] == r["count"] > 10000 and counts[1] == 0
    assert abs(cost[0] - r["cost"]) <= 1e-5 * abs(cost[0]), (cost[0], r["cost"])
    assert cost[1] == 0.0
    # the helper's scene form and mask
    c2, k2 = ba_cost_util.scene_objective(scene)
    assert np.array_equal(k2[0], counts) and c2[0, 0] == cost[0]
    mask = np.zeros(scene.surfels_size, bool)
    mask[::3] = True
    c3, k3 = ba_cost_util.scene_objective(scene, mask=mask)
    assert 0 < k3[0, 0] < counts[0] and 0.0 <= c3[0, 0] <= cost[0]
    if perturb:
        assert cost[0] > 0.0 and c3[0, 0] > 0.0
