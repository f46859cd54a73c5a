"""-m gpu: the pieces the mesh operators share (badslam_amd/csrc/mesh_kernels.hpp: the edge runs, the union-find with a parity bit, the
compaction of an attributed mesh, the position check), through the public calls and bit for bit against the restatements of
tests/mesh_repair_util.py, tests/orient_mesh_util.py and tests/mesh_components_util.py.  The shapes are the smallest at which those
pieces can go wrong: one partly filled wave, one lane beyond a block of 256, a vertex count at which the width of the edge key steps,
a run of three, a single wave that holds a conflict and a chain of hooks on one root, and seams that straddle a wave boundary.  The
restatements alone decide what is expected; every constructed mesh is checked to give them the classes it was built for."""
import ctypes as C

import numpy as np
import pytest

from tests import mesh_components_util as mu
from tests import mesh_repair_util as ru
from tests import orient_mesh_util as ou
from tests.test_gpu_fusion import SENTINEL, bits, stream_ptr
from tests.test_gpu_mesh_components import assert_components_equal, assert_filtered_equal, gpu_components, gpu_filter
from tests.test_gpu_mesh_repair import Mesh, assert_untouched, check_topology, clean, outputs, p_
from tests.test_gpu_orient_mesh import Call, assert_equal as assert_oriented_equal, orient
from tests.test_gpu_smooth_mesh import Case, raw as raw_smooth

pytestmark = pytest.mark.gpu
F = np.float32
INVALID_ARGUMENT = -1   # BSLAM_ERR_INVALID_ARGUMENT
NONE = 0xFFFFFFFF
NAN_WITH_PAYLOAD = 0x7FC12345


@pytest.fixture(scope="module")
def gpu():
    import torch

    import badslam_amd
    from badslam_amd import build
    build.build()
    return torch, badslam_amd.lib(), badslam_amd.Context(0)


# ------------------------------------------------------------------------------------------------
# the meshes: (positions, normals, triangles)
# ------------------------------------------------------------------------------------------------
def open_strip(triangles):
    """A zigzag band of `triangles` triangles over triangles + 2 vertices in the plane z = 0, all counter-clockwise."""
    V = triangles + 2
    positions = np.array([[0.5 * i, i % 2, 0] for i in range(V)], F)
    t = np.array([(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(triangles)], np.uint32)
    return positions, np.tile(np.array([0, 0, 1], F), (V, 1)), t


def fan(V):
    """An open fan of V - 2 triangles around vertex 0; the rim 1 .. V - 1 lies on three quarters of a circle."""
    angles = 1.5 * np.pi * np.arange(V - 1) / (V - 2)
    positions = np.concatenate([np.zeros((1, 3)), np.stack([np.cos(angles), np.sin(angles), np.zeros(V - 1)], axis=1)]).astype(F)
    t = np.array([(0, k, k + 1) for k in range(1, V - 1)], np.uint32)
    return positions, np.tile(np.array([0, 0, 1], F), (V, 1)), t


def alternating_ring(n=8):
    p, nrm, t = ou.strip(n, twist=False)
    return p, nrm, ou.flip(t, np.arange(n) % 2 == 1)


def straddling():
    """56 loose triangles, then at the triangle ids 56 .. 71 the alternating ring of 8 (even ids) and the Moebius band of 8 (odd ids),
    then 8 loose triangles: the seams of both lie across the wave boundary at triangle 64 and, by sorted position, across the one at
    slot 192 (the 56 loose triangles hold the vertices 0 .. 167, so their 168 slots sort first)."""
    front, back = ou.confetti(56, 0, seed=1), ou.confetti(8, 0, seed=2)
    p, n, t = ou.concat(front, alternating_ring(), ou.strip(8, twist=True), back)
    order = list(range(56)) + [56 + k // 2 + 8 * (k % 2) for k in range(16)] + list(range(72, 80))
    return p, n, np.ascontiguousarray(t[order])


EDGE_RUN_MESHES = {"one triangle": lambda: (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F), np.tile(np.array([0, 0, 1], F), (3, 1)), np.array([[0, 1, 2]], np.uint32)),
                   "strip of 86": lambda: open_strip(86), "fan of 256 vertices": lambda: fan(256), "fan of 257 vertices": lambda: fan(257), "book": ou.book}
# name -> (unique edges, boundary, interior, non-manifold edges; patches, seams)
EDGE_RUN_CLASSES = {"one triangle": (3, 3, 0, 0, 1, 0), "strip of 86": (173, 88, 85, 0, 1, 85), "fan of 256 vertices": (509, 256, 253, 0, 1, 253),
                    "fan of 257 vertices": (511, 257, 254, 0, 1, 254), "book": (7, 6, 0, 1, 3, 0)}
PARITY_MESHES = {"Moebius band of 8": lambda: ou.strip(8, twist=True), "alternating ring of 8": alternating_ring, "both across a wave boundary": straddling}
# name -> (patches, non-orientable patches, seams, seams that disagree on input, flipped triangles by majority)
PARITY_CLASSES = {"Moebius band of 8": (1, 1, 8, 1, 0), "alternating ring of 8": (1, 0, 8, 8, 4), "both across a wave boundary": (66, 1, 16, 9, None)}


# ------------------------------------------------------------------------------------------------
# 1. the edge runs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EDGE_RUN_MESHES))
def test_edge_runs(gpu, name):
    positions, normals, triangles = EDGE_RUN_MESHES[name]()
    V = len(positions)
    edges, boundary, interior, nonmanifold, patches, seams = EDGE_RUN_CLASSES[name]
    census, want = check_topology(gpu, V, triangles, name)   # the report, edge_uses and loop_of_slot
    assert (want["unique_edges"], want["boundary_edges"], want["interior_edges"], want["nonmanifold_edges"]) == (edges, boundary, interior, nonmanifold)
    assert want["edge_uses"].max() == (3 if name == "book" else 2 if interior else 1)
    if "fan" in name:
        assert int(triangles.max()).bit_length() == (8 if "256" in name else 9), "the width of the edge key steps between the two fans"
    for mode in ou.MODES:
        expected = ou.orient(positions, normals, triangles, mode)
        assert (expected["report"]["patches"], expected["report"]["seams"], expected["report"]["nonorientable_patches"]) == (patches, seams, 0)
        assert_oriented_equal(orient(gpu, (positions, normals, triangles), mode), expected, f"{name}, {mode}")
    if name == "book":   # the edge with three uses joins nothing and stays open
        assert len(set(expected["patch_of_triangle"].tolist())) == 3 and expected["report"]["closed_patches"] == 0


# ------------------------------------------------------------------------------------------------
# 2. the union-find with a parity bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PARITY_MESHES))
def test_parity_union_find(gpu, name):
    positions, normals, triangles = PARITY_MESHES[name]()
    patches, nonorientable, seams, disagree, flipped = PARITY_CLASSES[name]
    for mode in ou.MODES:
        expected = ou.orient(positions, normals, triangles, mode)
        r = expected["report"]
        assert (r["patches"], r["nonorientable_patches"], r["seams"], r["disagreeing_seams_before"]) == (patches, nonorientable, seams, disagree)
        if mode == "majority" and flipped is not None:
            assert r["flipped_triangles"] == flipped
        assert_oriented_equal(orient(gpu, (positions, normals, triangles), mode), expected, f"{name}, {mode}")
    if name == "both across a wave boundary":
        patch = expected["patch_of_triangle"]
        assert set(patch[56:72].tolist()) == {56, 57} and patch[63] != patch[64] and patch[62] == patch[64] and patch[63] == patch[65]
    # the plain union-find over the same triangles: the vertices
    assert_components_equal(gpu_components(gpu, len(positions), triangles), mu.components(len(positions), triangles))


# ------------------------------------------------------------------------------------------------
# 3. the compaction
# ------------------------------------------------------------------------------------------------
def compaction_mesh():
    """257 vertices and 257 triangles, so that the vertex part and the triangle part of the grid both have a second block of one lane:
    19 loose triangles over the vertices 0 .. 56 and a band of 198 over the vertices 57 .. 256; as triangles the first 40 of the band
    reversed, the loose ones, the band.  Vertex 1 lies where vertex 0 does.  The last vertex and the last triangle are kept by both calls,
    and the normal of the last vertex is a NaN with a payload."""
    p, n, band = open_strip(198)
    band = band + np.uint32(57)
    loose = np.arange(57, dtype=np.uint32).reshape(19, 3)
    positions = np.concatenate([np.array([[3.0 * (v // 3), 2.0 + v % 3, 0.25 * (v % 2)] for v in range(57)], F), p + F(100)])
    positions[1] = positions[0]
    rng = np.random.default_rng(4)
    normals = rng.normal(size=(257, 3)).astype(F)
    normals.view(np.uint32)[256, 1] = NAN_WITH_PAYLOAD
    colors = rng.integers(0, 256, (257, 4), dtype=np.uint8)
    triangles = np.ascontiguousarray(np.concatenate([band[:40][:, [0, 2, 1]], loose, band]))
    assert positions.shape == (257, 3) and triangles.shape == (257, 3)
    return positions, normals, colors, triangles


@pytest.mark.parametrize("attributes", ["colours, no normals", "normals, no colours"])
def test_filter_compaction(gpu, attributes):
    positions, normals, colors, triangles = compaction_mesh()
    normals, colors = (None, colors) if attributes.startswith("colours") else (normals, None)
    want = mu.components(257, triangles)
    got = gpu_components(gpu, 257, triangles)
    assert_components_equal(got, want)
    sizes = want[1]
    assert sorted(set(sizes.tolist())) == [3, 200] and sizes[256] == 200 and sizes[0] == 3
    filtered = gpu_filter(gpu, positions, normals, colors, triangles, got[1], 4)
    assert_filtered_equal(filtered, sizes, 4, positions, normals, colors, triangles)
    assert len(filtered[0]) == 200 and len(filtered[3]) == 238
    if normals is not None:
        assert bits(filtered[1])[199, 1] == NAN_WITH_PAYLOAD
    everything = gpu_filter(gpu, positions, normals, colors, triangles, got[1], 1)
    assert_filtered_equal(everything, sizes, 1, positions, normals, colors, triangles)
    assert len(everything[0]) == 257 and len(everything[3]) == 257


@pytest.mark.parametrize("maps", [True, False])
@pytest.mark.parametrize("attributes", ["colours, no normals", "normals, no colours"])
def test_clean_compaction(gpu, attributes, maps):
    positions, normals, colors, triangles = compaction_mesh()
    normals, colors = (None, colors) if attributes.startswith("colours") else (normals, None)
    want = ru.clean(positions, normals, colors, triangles)
    # vertex 1 is welded to vertex 0, which degenerates their triangle and leaves the vertices 0 and 2 without one
    assert want["report"] == dict(welded_vertices=1, unreferenced_vertices=2, degenerate_triangles=1, duplicate_triangles=40)
    assert (want["vertex_map"][:3] == NONE).all() and want["vertex_map"][3] == 0 and want["vertex_map"][256] == 253
    assert (want["triangle_map"] == NONE).sum() == 41 and want["triangle_map"][256] == 215
    got = clean(gpu, positions, normals, colors, triangles, maps=maps)
    assert got["report"] == want["report"]
    for k in ("positions", "normals", "colors", "triangles") + (("vertex_map", "triangle_map") if maps else ()):
        assert (got[k] is None) == (want[k] is None), k
        if got[k] is not None:
            g, w = np.asarray(got[k]), np.asarray(want[k]).reshape(np.asarray(got[k]).shape)
            assert np.array_equal(bits(g), bits(w)) if g.dtype == F else np.array_equal(g, w), f"{k} differ"
    if not maps:
        assert got["vertex_map"] is None and got["triangle_map"] is None
    if normals is not None:
        assert bits(got["normals"])[253, 1] == NAN_WITH_PAYLOAD


# ------------------------------------------------------------------------------------------------
# 4. the position check
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_position_that_is_not_finite_in_the_last_vertex_is_refused(gpu, value):
    torch, L, ctx = gpu
    positions, normals, triangles = fan(257)
    positions[256, 0 if np.isnan(value) else 2] = value
    message = b": a vertex is not finite"
    m = Mesh(torch, positions, normals, None, triangles)
    out = outputs(torch, m, 257 + 2, 255 + 300, hole_of_triangle=300)
    v, t, f = C.c_uint32(SENTINEL), C.c_uint32(SENTINEL), C.c_uint32(SENTINEL)
    rc = L.bslam_fill_mesh_holes(ctx.handle, stream_ptr(torch), m.V, m.T, *m.inputs(), 4096, 257 + 2, 255 + 300, p_(out["out_positions"]), p_(out["out_normals"]),
                                 p_(out["out_colors"]), p_(out["out_indices"]), p_(out["hole_of_triangle"]), C.byref(v), C.byref(t), C.byref(f))
    assert rc == INVALID_ARGUMENT and b"bslam_fill_mesh_holes" + message in L.bslam_last_error()
    torch.cuda.synchronize()
    assert_untouched(out)
    assert (v.value, t.value, f.value) == (SENTINEL, SENTINEL, SENTINEL)
    m.assert_untouched()
    for mode in ou.MODES:
        call = Call(gpu, positions, normals, triangles)
        assert call.run(mode) == INVALID_ARGUMENT and b"bslam_orient_mesh" + message in L.bslam_last_error(), mode
        call.assert_untouched()
    case = Case(torch, positions, normals, triangles)
    assert raw_smooth(gpu, case, iterations=2) == INVALID_ARGUMENT and b"bslam_smooth_mesh" + message in L.bslam_last_error()
    torch.cuda.synchronize()
    case.assert_inputs_untouched()
    case.assert_outputs_untouched()
