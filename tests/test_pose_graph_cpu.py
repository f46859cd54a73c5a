"""CPU: the keyframe pose graph of loop closure (badslam_amd/host/pose_graph.cpp, BS/pose_graph_optimizer.cc with g2o's
EdgeSE3 / VertexSE3 semantics) against an independent solver -- scipy.optimize.least_squares on the same error -- and
AveragePose (BS/util.cc:110-129) known answers."""
import time

import numpy as np
import pytest
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation

from badslam_amd import build
from badslam_amd import direct_ba as dba


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()


def to_mat(p7):
    T = np.eye(4)
    T[:3, :3] = Rotation.from_quat(p7[:4]).as_matrix()
    T[:3, 3] = p7[4:]
    return T


def to_p7(T):
    q = Rotation.from_matrix(T[:3, :3]).as_quat()
    if q[3] < 0:
        q = -q
    return np.concatenate([q, T[:3, 3]])


def g2o_error(T_from, T_to, meas):
    """EdgeSE3::computeError: delta = meas^-1 from^-1 to, e = [t; q.xyz] with w >= 0."""
    d = np.linalg.inv(meas) @ np.linalg.inv(T_from) @ T_to
    q = Rotation.from_matrix(d[:3, :3]).as_quat()
    if q[3] < 0:
        q = -q
    return np.concatenate([d[:3, 3], q[:3]])


def random_pose(rng, t_scale, r_scale):
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(rng.normal(size=3) * r_scale).as_matrix()
    T[:3, 3] = rng.normal(size=3) * t_scale
    return T


def circle_path(n, radius=1.0):
    poses = []
    for i in range(n):
        a = 2 * np.pi * i / n
        T = np.eye(4)
        T[:3, :3] = Rotation.from_rotvec([0, a, 0]).as_matrix()
        T[:3, 3] = [radius * np.sin(a), 0.1 * np.sin(3 * a), radius * (1 - np.cos(a))]
        poses.append(T)
    return poses


def noisy_graph(rng, n=30, loops=((29, 0),), t_noise=0.01, r_noise=0.005):
    truth = circle_path(n)
    edges, meas = [], []
    for i in range(n - 1):
        edges.append((i, i + 1))
        meas.append(np.linalg.inv(truth[i]) @ truth[i + 1] @ random_pose(rng, t_noise, r_noise))
    for a, b in loops:
        edges.append((a, b))
        meas.append(np.linalg.inv(truth[a]) @ truth[b] @ random_pose(rng, t_noise, r_noise))
    # initial state: chained odometry (drifted)
    init = [truth[0]]
    for i in range(n - 1):
        init.append(init[-1] @ meas[i])
    return truth, init, edges, meas


def scipy_solve(init, edges, meas, fixed):
    n = len(init)
    free = [v for v in range(n) if v != fixed]

    def unpack(x):
        poses = list(init)
        for k, v in enumerate(free):
            T = np.eye(4)
            T[:3, :3] = Rotation.from_rotvec(x[6 * k + 3:6 * k + 6]).as_matrix()
            T[:3, 3] = x[6 * k:6 * k + 3]
            poses[v] = T
        return poses

    def residual(x):
        poses = unpack(x)
        return np.concatenate([g2o_error(poses[a], poses[b], m) for (a, b), m in zip(edges, meas)])

    x0 = np.concatenate([np.concatenate([init[v][:3, 3], Rotation.from_matrix(init[v][:3, :3]).as_rotvec()]) for v in free])
    sol = least_squares(residual, x0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=100000)
    sol = least_squares(residual, sol.x, jac="3-point", method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=1000)   # polish: central differences
    return unpack(sol.x), float(np.sum(sol.fun ** 2))


@pytest.mark.parametrize("seed,loops", [(1, ((29, 0),)), (2, ((29, 0), (20, 5))), (3, ((0, 29), (15, 3)))])
def test_matches_an_independent_least_squares_solver(seed, loops):
    rng = np.random.default_rng(seed)
    truth, init, edges, meas = noisy_graph(rng, loops=loops)
    p7 = np.array([to_p7(T) for T in init])
    out, chi2, info = dba.optimize_pose_graph(p7, edges, np.array([to_p7(m) for m in meas]), 0, 20)
    ref, ref_chi2 = scipy_solve(init, edges, meas, 0)
    assert np.array_equal(out[0], p7[0]), "the gauge vertex must stay bit-unchanged"
    for v in range(len(init)):
        assert np.abs(to_mat(out[v]) - ref[v]).max() <= 1e-7, v
    assert abs(chi2[-1] - ref_chi2) <= 1e-9 + 1e-6 * ref_chi2
    assert info["initial_chi2"] > chi2[-1]
    assert len(chi2) == 20 and all(np.diff(chi2[:5]) <= 1e-15)


def test_consistent_measurements_give_zero_chi2_and_the_generating_poses():
    rng = np.random.default_rng(4)
    truth = circle_path(30)
    edges = [(i, i + 1) for i in range(29)] + [(29, 0), (10, 25)]
    meas = [np.linalg.inv(truth[a]) @ truth[b] for a, b in edges]
    init = [truth[0]] + [T @ random_pose(rng, 0.05, 0.03) for T in truth[1:]]
    out, chi2, _ = dba.optimize_pose_graph(np.array([to_p7(T) for T in init]), edges, np.array([to_p7(m) for m in meas]), 0, 20)
    assert chi2[-1] < 1e-20
    for v in range(30):
        assert np.abs(to_mat(out[v]) - truth[v]).max() < 1e-9, v


def test_deleted_keyframes_are_skipped():
    rng = np.random.default_rng(5)
    truth = circle_path(12)
    drifted = [truth[0]]
    for i in range(11):
        drifted.append(drifted[-1] @ np.linalg.inv(truth[i]) @ truth[i + 1] @ random_pose(rng, 0.01, 0.004))
    exists = np.ones(12, np.int32)
    exists[[0, 4, 5]] = 0                                   # keyframe 0 deleted: the gauge is keyframe 1
    p7 = np.array([to_p7(T) for T in drifted])
    loop = np.linalg.inv(truth[11]) @ truth[1]
    out, chi2, info = dba.optimize_keyframe_pose_graph(p7, exists, [(11, 1)], [to_p7(loop)], 20)
    assert info["gauge"] == 1
    assert np.array_equal(out[1], p7[1])
    assert np.array_equal(out[[0, 4, 5]], p7[[0, 4, 5]]), "deleted keyframes are left alone"
    # same answer as the explicit graph with the odometry edge 3 -> 6 joining the neighbours of the deleted ones
    ids = [1, 2, 3, 6, 7, 8, 9, 10, 11]
    vin = [drifted[i] for i in ids]
    edges = [(k, k + 1) for k in range(len(ids) - 1)] + [(len(ids) - 1, 0)]
    meas = [np.linalg.inv(vin[a]) @ vin[b] for a, b in edges[:-1]] + [loop]
    ref, _ = scipy_solve(vin, edges, meas, 0)
    for k, i in enumerate(ids):
        assert np.abs(to_mat(out[i]) - ref[k]).max() <= 1e-7, i
    assert chi2[-1] < info["initial_chi2"]


def test_k1000_with_three_loops_is_fast_and_sparse():
    rng = np.random.default_rng(6)
    n = 1000
    loops = ((999, 0), (700, 100), (500, 250))
    truth, init, edges, meas = noisy_graph(rng, n=n, loops=loops, t_noise=0.002, r_noise=0.001)
    p7 = np.array([to_p7(T) for T in init])
    m7 = np.array([to_p7(m) for m in meas])
    t0 = time.perf_counter()
    out, chi2, info = dba.optimize_pose_graph(p7, edges, m7, 0, 20)
    dt = time.perf_counter() - t0
    assert dt < 1.0, dt
    # fill: one extra block per loop edge per eliminated vertex inside the loop, at most -> O(K * L)
    assert info["factor_blocks"] <= (n - 1) * (1 + 1 + len(loops)), info["factor_blocks"]
    assert chi2[-1] < info["initial_chi2"]
    assert abs(chi2[-1] - chi2[-2]) <= 1e-9 * chi2[-1]


def test_average_pose_known_answers():
    rng = np.random.default_rng(7)
    T = random_pose(rng, 0.5, 0.4)
    got = to_mat(dba.average_pose([to_p7(T)] * 3))
    assert np.abs(got - T).max() < 1e-12
    a, b = np.eye(4), np.eye(4)
    a[:3, :3] = Rotation.from_rotvec([0, 0, 0.3]).as_matrix()
    b[:3, :3] = Rotation.from_rotvec([0, 0, -0.3]).as_matrix()
    a[:3, 3] = [1, 2, 3]
    b[:3, 3] = [3, 0, -1]
    got = to_mat(dba.average_pose([to_p7(a), to_p7(b)]))
    assert np.abs(got[:3, :3] - np.eye(3)).max() < 1e-12
    assert np.abs(got[:3, 3] - [2, 1, 1]).max() < 1e-12


def test_fromVectorMQT_out_of_range_rotation_is_identity():
    # |q.xyz| > 1: g2o's fromCompactQuaternion returns the identity rotation; a pose graph step of that size only
    # moves the translation.  Checked through a two-vertex graph whose solve would need such a step: the result
    # must stay finite.
    p7 = np.array([[0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0]], float)
    meas = to_p7(random_pose(np.random.default_rng(8), 0.1, 2.5))
    out, chi2, _ = dba.optimize_pose_graph(p7, [(0, 1)], [meas], 0, 20)
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(chi2))
