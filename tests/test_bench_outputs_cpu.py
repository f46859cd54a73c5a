"""bench.py --dump-outputs on CPU: dump_outputs writes float32 / float64 .npy files only, at most 64 MB in all, on a fixed sample
of surfel columns, with the packed normals decoded (no GPU: the device stack is stood in for by CPU tensors)."""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import torch

import bench
from badslam_amd import abi, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fake_step(S, K, seed=1):
    rng = np.random.default_rng(seed)
    surf = np.zeros((abi.SURFEL_ATTRIBUTE_COUNT, S), np.float32)
    surf[0:3] = rng.normal(size=(3, S))
    n = rng.normal(size=(S, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    surf[3] = synthetic.s10_pack(n.astype(np.float32)).view(np.float32)
    surf[4] = rng.uniform(1e-6, 1e-4, S)
    surf[6:8] = rng.normal(size=(2, S))
    active = (rng.uniform(size=(1, S)) < 0.7).astype(np.uint8)
    dev = types.SimpleNamespace(surfels=torch.from_numpy(surf), active=torch.from_numpy(active), surfels_size=S)
    poses = (abi.SE3f * K)()
    for k in range(K):
        poses[k].q[3] = 1.0
        poses[k].t[0] = 0.1 * k
    iters = (C.c_int32 * K)(*[k % 30 for k in range(K)])
    conv = (C.c_int32 * K)(*[k % 2 for k in range(K)])
    return dev, surf, n, active, poses, iters, conv


def load_all(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_of_a_large_stack_is_a_fixed_sample_under_64_mb(tmp_path):
    S, K = bench.DUMP_SURFEL_SAMPLE + 12345, 300
    dev, surf, n, active, poses, iters, conv = fake_step(S, K)
    bench.dump_outputs(str(tmp_path / "a"), dev, poses, iters, conv)
    bench.dump_outputs(str(tmp_path / "b"), dev, poses, iters, conv)
    a, b = load_all(tmp_path / "a"), load_all(tmp_path / "b")
    assert set(a) == {"poses", "gn_iterations", "converged", "surfel_index", "surfel_positions", "surfel_normals",
                      "surfel_radius_squared", "surfel_descriptors", "surfel_active"}
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in a) <= 64 << 20
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k                       # same sample, same bytes
    idx = a["surfel_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_SURFEL_SAMPLE and np.all(np.diff(idx) > 0) and idx[-1] < S
    assert np.array_equal(a["surfel_positions"], surf[0:3, idx].T)
    assert np.array_equal(a["surfel_radius_squared"], surf[4, idx])
    assert np.array_equal(a["surfel_descriptors"], surf[6:8, idx].T)
    assert np.array_equal(a["surfel_active"], active[0, idx].astype(np.float32))
    assert np.abs(a["surfel_normals"] - n[idx]).max() <= 1.0 / 511      # the s10 fields, decoded
    assert a["poses"].shape == (K, 7) and np.array_equal(a["poses"][:, 4], (0.1 * np.arange(K)).astype(np.float32))
    assert np.array_equal(a["gn_iterations"], np.arange(K) % 30) and np.array_equal(a["converged"], np.arange(K) % 2)


def test_dump_outputs_of_a_small_stack_keeps_every_surfel(tmp_path):
    dev, surf, _, _, poses, iters, conv = fake_step(1000, 4)
    bench.dump_outputs(str(tmp_path), dev, poses, iters, conv)
    out = load_all(tmp_path)
    assert np.array_equal(out["surfel_index"], np.arange(1000))
    assert np.array_equal(out["surfel_positions"], surf[0:3].T)


def test_full_and_dump_outputs_are_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
