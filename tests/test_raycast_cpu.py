"""The surface view rule on the CPU (tests/raycast_util.py, the restatement the GPU tests compare the kernels with): the property
the block flags rest on, and what the rule yields on fields whose surface is known.

Measured with this restatement (sphere_field() 33 x 31 x 29 in voxel units seen by a 64 x 48 camera of focal length 60 from
(16, 15, -25), depth range 20 - 60; 735 pixels whose ray meets the analytic sphere):

  step   hits   hit outside   depth error against the analytic intersection, voxels   normal . radial
                              median     99th percentile     maximum                  minimum
  0.5    734    0             0.0243     0.1340              0.2413                   0.99837
  1      734    0             0.0324     0.2240              0.9093                   0.99840
  2.3    732    0             0.0458     0.4276              0.4535                   0.99843

Two-plane scene of fusion_util.plane_scene() fused at 2 cm into 60 x 50 x 40 samples and viewed from keyframe 0: 2114 hits,
plane distance of the hit points median 0.46 mm, 99th percentile 2.24 mm, maximum 4.04 mm.  The assertions are twice the
measured 99th percentile, maximum and worst deviation."""
import numpy as np
import pytest

from badslam_amd import abi
from tests import fusion_util as fu
from tests import raycast_util as ru

F = np.float32
CENTRE, RADIUS = np.array([16.3, 15.1, 14.2]), 9.7
CAMERA = abi.Camera4f(60.0, 60.0, 32.0, 24.0, 64, 48)
POSE = np.array([[1, 0, 0, 16], [0, 1, 0, 15], [0, 0, 1, -25]], F)


def test_lerps_of_corners_that_are_not_negative_are_not_negative():
    """What lets the march pass a block without a negative corner: seven nested fmaf lerps with weights in [0, 1) over corners
    none of which is < 0 never give a value < 0."""
    rng = np.random.default_rng(3)
    n = 400000
    tiny, one_less = np.nextafter(F(0), F(1)), np.nextafter(F(1), F(0))
    scale = F(10.0) ** rng.integers(-44, 38, (8, n)).astype(F)
    D = (rng.random((8, n)).astype(F) * scale).astype(F)
    D[rng.random((8, n)) < 0.2] = 0
    D[rng.random((8, n)) < 0.02] = tiny
    f = rng.random((3, n)).astype(F)
    f[rng.random((3, n)) < 0.1] = 0
    f[rng.random((3, n)) < 0.1] = one_less
    f[rng.random((3, n)) < 0.05] = tiny
    assert (f < 1).all() and (D >= 0).all()
    value = ru.value(list(D), list(f))
    assert not (value < 0).any()
    # constructed: a steep fall towards a zero corner at the largest weight, for every edge direction and magnitude
    for big in (F(3.0e38), F(1.0), F(1.0e-38), tiny):
        for corner in range(8):
            D = [F(big)] * 8
            D[corner] = F(0)
            for w in (F(0), tiny, F(0.5), one_less):
                assert not ru.value([np.array([d]) for d in D], [np.array([w])] * 3)[0] < 0


def analytic_depth(camera, pose):
    j, i = np.meshgrid(np.arange(camera.height), np.arange(camera.width), indexing="ij")
    d = np.stack([(i + 0.5 - camera.cx) / camera.fx, (j + 0.5 - camera.cy) / camera.fy, np.ones(i.shape)], -1)
    o = pose[:, 3].astype(np.float64) - CENTRE
    a, b, c = (d * d).sum(-1), 2 * (d @ o), o @ o - RADIUS ** 2
    disc = b * b - 4 * a * c
    with np.errstate(all="ignore"):
        return np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.nan), d


@pytest.fixture(scope="module")
def sphere():
    field = fu.sphere_field()
    return field, np.ones(field.shape, np.uint32)


@pytest.mark.parametrize("step, hits, p99, worst, dot", [(0.5, 734, 0.1340, 0.2413, 0.99837), (1.0, 734, 0.2240, 0.9093, 0.99840), (2.3, 732, 0.4276, 0.4535, 0.99843)])
def test_sphere(sphere, step, hits, p99, worst, dot):
    field, ones = sphere
    want, rays = analytic_depth(CAMERA, POSE)
    silhouette = ~np.isnan(want)
    assert silhouette.sum() == 735
    r = ru.raycast(ru.Volume(field, ones, None, (0, 0, 0), 1.0), POSE, CAMERA, 20.0, 60.0, step, 100.0)
    hit = r["hit"]
    error = np.abs(r["t"][hit] - want[hit])
    P = POSE[:, 3] + r["t"][..., None].astype(np.float64) * rays
    radial = (P - CENTRE) / np.linalg.norm(P - CENTRE, axis=-1, keepdims=True)
    cosine = (r["normal"].astype(np.float64) * radial).sum(-1)[hit]
    print(f"step {step}: N {r['samples']}, {hit.sum()} hits, {(hit & ~silhouette).sum()} outside, median {np.median(error):.4f}, p99 {np.percentile(error, 99):.4f}, "
          f"max {error.max():.4f}, min normal . radial {cosine.min():.5f}")
    assert not (hit & ~silhouette).any()
    assert (silhouette & ~hit).sum() <= 0.01 * silhouette.sum()
    assert hit.sum() == hits
    assert np.percentile(error, 99) <= 2 * p99 and error.max() <= 2 * worst
    assert 1.0 - cosine.min() <= 2 * (1.0 - dot)
    # the depth view is the rounded t*, the normals are unit vectors, empty pixels are zero
    assert np.array_equal(r["depth"][hit], np.trunc(F(100.0) * r["t"][hit] + F(0.5)).astype(np.uint16))
    assert np.abs(np.linalg.norm(r["normal"][hit].astype(np.float64), axis=-1) - 1).max() < 1e-6
    assert not r["depth"][~hit].any() and not r["normal"][~hit].any() and not r["color"].any()


def test_further_views_of_the_sphere(sphere):
    field, ones = sphere
    full = ru.Volume(field, ones, None, (0, 0, 0), 1.0)
    holed = ru.raycast(ru.Volume(field, fu.holed_sphere_count(field.shape), None, (0, 0, 0), 1.0), POSE, CAMERA, 20.0, 60.0, 1.0, 100.0)
    assert holed["hit"].sum() == 723                                    # the surface opens where samples are unobserved
    inside = np.array([[1, 0, 0, CENTRE[0]], [0, 1, 0, CENTRE[1]], [0, 0, 1, CENTRE[2]]], F)
    assert ru.raycast(full, inside, CAMERA, 0.5, 40.0, 1.0, 100.0)["hit"].sum() == 0          # seen from behind
    assert ru.raycast(full, POSE, CAMERA, 20.0, 28.0, 1.0, 100.0)["hit"].sum() == 0           # max_depth in front of the surface
    assert ru.sample_count(20.0, 60.0, 0.5) == 81 and ru.sample_count(20.0, 60.0, 2.3) == 18
    with pytest.raises(ValueError):
        ru.sample_count(0.05, 50.0, 0.0005)


def test_fused_planes_seen_from_a_keyframe():
    camera, keyframes = fu.plane_scene()
    dims, origin, voxel = (60, 50, 40), (-0.6, -0.5, 1.2), 0.02
    tsdf, count, color = fu.fuse(keyframes, camera, camera, np.zeros((15, 20), F), 0.0, 1.0 / 5000.0, 4, origin, voxel, dims, 0.08)
    M = keyframes[0].T.reshape(3, 4).astype(np.float64)
    pose = np.concatenate([M[:, :3].T, (-M[:, :3].T @ M[:, 3])[:, None]], 1).astype(F)
    r = ru.raycast(ru.Volume(tsdf, count, color, origin, voxel), pose, camera, 0.5, 3.0, voxel, 5000.0)
    hit = r["hit"]
    j, i = np.meshgrid(np.arange(camera.height), np.arange(camera.width), indexing="ij")
    rays = np.stack([(i + 0.5 - camera.cx) / camera.fx, (j + 0.5 - camera.cy) / camera.fy, np.ones(i.shape)], -1) @ pose[:, :3].astype(np.float64).T
    points = (pose[:, 3].astype(np.float64) + r["t"][..., None].astype(np.float64) * rays)[hit]
    distance = fu.plane_distance(points)
    print(f"{hit.sum()} hits: plane distance median {np.median(distance):.5f}, p99 {np.percentile(distance, 99):.5f}, max {distance.max():.5f}")
    assert hit.sum() > 2000
    assert np.percentile(distance, 99) <= 2 * 2.24e-3 and distance.max() <= 2 * 4.04e-3
    assert (r["color"][hit][:, 3] == 255).all() and not r["color"][~hit].any()
    # the keyframe's own depth image, where both have a value: within a voxel
    raw = keyframes[0].depth.astype(np.int64)
    both = hit & (raw > 0) & (r["depth"] > 0)
    assert both.sum() > 2000 and np.abs(r["depth"].astype(np.int64) - raw)[both].max() <= voxel * 5000.0
