"""The mesh-ray rule on the CPU (tests/mesh_rays_util.py): what the GPU comparison rests on.  The restatement agrees with a float64
Moeller-Trumbore wherever float64 is not within rounding of an edge, its slab is monotone under inclusion of boxes, no ray gets
through the edges and vertices of a closed mesh, and both entry points are declared."""
import numpy as np
import pytest

from badslam_amd import abi
from tests import mesh_rays_util as mr

F = np.float32
EDGE_BAND = 1e-4          # barycentric distance from an edge inside which float64 and the rule may decide differently
TOLERANCE_FACTOR = 4.0    # DESIGN.md 8 "Mesh rays": the bound is this factor times what plain fp32 Moeller-Trumbore reaches on the fixture


@pytest.fixture(scope="module")
def sphere():
    return mr.icosphere()


@pytest.fixture(scope="module")
def rays(sphere):
    """300 rays from inside, from outside towards the sphere, and from outside past it."""
    positions, _ = sphere
    rng = np.random.default_rng(7)
    centre = positions.mean(axis=0)
    inside = centre + rng.uniform(-0.5, 0.5, (100, 3))
    outward = rng.standard_normal((200, 3))
    outside = centre + outward / np.linalg.norm(outward, axis=1, keepdims=True) * rng.uniform(2.5, 6.0, (200, 1))
    origins = np.concatenate([inside, outside]).astype(F)
    towards = np.concatenate([rng.standard_normal((100, 3)), centre + rng.uniform(-0.8, 0.8, (100, 3)) - outside[:100], rng.standard_normal((100, 3))])
    return np.ascontiguousarray(origins, F), np.ascontiguousarray(towards * rng.uniform(0.3, 3.0, (300, 1)), F)


def plain_fp32(o, d, a, b, c):
    """Moeller-Trumbore in plain float32: the yardstick of what the format gives on the fixture."""
    o, d = o[:, None, :], d[:, None, :]
    e1, e2 = (b - a)[None], (c - a)[None]
    h = np.cross(d, e2).astype(F)
    det = (e1 * h).sum(-1, dtype=F)
    s = (o - a[None]).astype(F)
    u = ((s * h).sum(-1, dtype=F) / det).astype(F)
    q = np.cross(s, e1).astype(F)
    v = ((d * q).sum(-1, dtype=F) / det).astype(F)
    t = ((e2 * q).sum(-1, dtype=F) / det).astype(F)
    return t, u, v


def test_rule_agrees_with_float64_moller_trumbore(sphere, rays):
    positions, triangles = sphere
    origins, directions = rays
    tri = positions[triangles.astype(np.int64)]
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    accepted, t, u, v, front = mr.ray_triangle(origins, directions, a, b, c)
    hit64, t64, u64, v64, front64, edge = mr.moller_trumbore(origins, directions, a, b, c)
    clear = edge > EDGE_BAND
    assert clear.mean() > 0.99
    assert np.array_equal(accepted[clear], hit64[clear]), "the rule and float64 decide differently away from every edge"
    both = accepted & hit64 & clear
    assert both.sum() > 300
    assert np.array_equal(front[both], front64[both]), "front is not the side from which a, b, c run counter-clockwise"
    plain_t, plain_u, plain_v = plain_fp32(origins, directions, a, b, c)
    scale = np.abs(t64[both])
    deviation = lambda got, want, s: float((np.abs(got[both].astype(np.float64) - want[both]) / s).max())
    plain = max(deviation(plain_t, t64, scale), deviation(plain_u, u64, 1.0), deviation(plain_v, v64, 1.0))
    rule = max(deviation(t, t64, scale), deviation(u, u64, 1.0), deviation(v, v64, 1.0))
    print(f"largest deviation from float64: plain fp32 {plain:.3e}, the rule {rule:.3e}")
    assert 0 < plain < 1e-4
    assert rule <= TOLERANCE_FACTOR * plain


def test_closest_hit_of_the_sphere(sphere, rays):
    positions, triangles = sphere
    origins, directions = rays
    got = mr.closest_hit(origins, directions, None, positions, triangles)
    hit = np.isfinite(got["t"])
    assert hit[:100].all() and not got["front"][:100].any(), "a ray from inside hits the back of an outward-wound sphere"
    assert hit[100:200].all() and got["front"][100:200].all(), "a ray aimed at the sphere from outside hits its front"
    assert (~hit[200:]).sum() > 50
    centre, radius = positions.astype(np.float64).mean(axis=0), 1.5
    where = origins[hit].astype(np.float64) + got["t"][hit, None].astype(np.float64) * directions[hit].astype(np.float64)
    assert np.abs(np.linalg.norm(where - centre, axis=1) - radius).max() < 0.01 * radius       # on the sphere, up to the tessellation
    assert np.array_equal(mr.any_hit(origins, directions, None, positions, triangles), hit.astype(np.uint8))
    assert (got["triangle"][~hit] == mr.NO_TRIANGLE).all() and (got["uv"][~hit] == 0).all()


def test_no_ray_passes_between_triangles(sphere):
    positions, triangles = sphere
    targets = mr.edge_points(positions, triangles)[::7]
    centre = positions.mean(axis=0).astype(F)
    origins = np.broadcast_to(centre, targets.shape)
    got = mr.closest_hit(origins, (targets - centre).astype(F), None, positions, triangles)
    assert np.isfinite(got["t"]).all(), "a ray from the centre through a vertex or an edge point got out"


def test_slab_is_monotone_under_inclusion():
    rng = np.random.default_rng(19)
    n = 4000
    lo = rng.uniform(-2, 2, (n, 3)).astype(F)
    hi = (lo + rng.uniform(0, 2, (n, 3)) * (rng.uniform(0, 1, (n, 3)) > 0.2)).astype(F)        # some boxes have zero thickness
    outer_lo = (lo - rng.uniform(0, 1, (n, 3)) * (rng.uniform(0, 1, (n, 3)) > 0.3)).astype(F)
    outer_hi = (hi + rng.uniform(0, 1, (n, 3)) * (rng.uniform(0, 1, (n, 3)) > 0.3)).astype(F)
    assert (outer_lo <= lo).all() and (hi <= outer_hi).all()
    origins = rng.uniform(-3, 3, (n, 3)).astype(F)
    directions = rng.standard_normal((n, 3)).astype(F)
    directions[rng.uniform(0, 1, (n, 3)) < 0.15] = 0                                           # zero components
    directions[::50, 0] = F(1e-45)                                                             # a reciprocal that overflows
    on_plane = rng.uniform(0, 1, (n, 3)) < 0.1
    origins[on_plane] = lo[on_plane]                                                           # origins exactly on box planes
    rows = np.arange(n)
    enter_in, exit_in = (x[rows, rows] for x in mr.slab(origins, directions, lo[None], hi[None]))
    enter_out, exit_out = (x[rows, rows] for x in mr.slab(origins, directions, outer_lo[None], outer_hi[None]))
    assert not np.isnan(enter_in).any() and not np.isnan(exit_out).any()
    assert (enter_out <= enter_in).all() and (exit_in <= exit_out).all()
    assert ((enter_in <= exit_in) <= (enter_out <= exit_out)).all(), "a ray that meets the inner box meets the outer one"
    assert 0.02 < (enter_in <= exit_in).mean() < 0.95


def test_padding_moves_by_representable_floats():
    x = np.array([1.0, -1.0, 0.0, -0.0, np.inf, -np.inf, 3.4028235e38, 1e-45], F)
    up, down = mr.pad(x, mr.PAD_ULPS), mr.pad(x, -mr.PAD_ULPS)
    assert up[0] == F(1) + F(4) * np.spacing(F(1)) and down[1] == -up[0]
    assert up[2] == up[3] == F(4) * F(1e-45) and down[2] == down[3] == -F(3) * F(1e-45)               # -0 is one of the steps down
    assert up[4] == np.inf and down[4] < np.inf and down[5] == -np.inf and up[5] > -np.inf and up[6] == np.inf
    assert (down <= x).all() and (x <= up).all()


def test_both_entry_points_are_declared():
    assert "bslam_mesh_rays" in abi.SIGNATURES and "bslam_mesh_visibility" in abi.SIGNATURES
    assert len(abi.SIGNATURES["bslam_mesh_rays"][1]) == 18 and len(abi.SIGNATURES["bslam_mesh_visibility"][1]) == 20
