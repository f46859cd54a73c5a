"""-m gpu: bslam_clean_mesh, bslam_mesh_topology and bslam_fill_mesh_holes (badslam_amd/csrc/repair_kernels.hpp) against the brute-force
restatement of tests/mesh_repair_util.py -- counts, report words, maps, per-slot arrays, indices, positions and colours bit for bit,
normals within 1e-6 (NORMAL_TOLERANCE of the normalised sums in tests/test_gpu_simplify_mesh.py): the sorts, the scans and the pointer
jumping may change no result -- and the layers above: DirectBA.CleanMesh / MeshTopology / FillHoles and tools/run_tum.py
--mesh-fill-holes --mesh-clean.  Every device array stands between guard words; outputs are filled with a sentinel first and must be
untouched at and beyond the returned counts.  The large case is the sphere of tests/fusion_util.py with two holes: 1698 vertices,
3346 triangles, 10038 slots -- several workgroups and scan tiles, and 50 boundary slots, so 7 rounds of pointer jumping; its soup
(10038 vertices) is the weld case."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi
from tests import fusion_util as fu
from tests import mesh_repair_util as ru
from tests.test_gpu_fusion import SENTINEL, bits, stream_ptr
from tests.test_gpu_mesh_components import Guarded
from tests.test_gpu_simplify_mesh import extracted   # noqa: F401  (the fixture: a DirectBA and its extracted mesh)

pytestmark = pytest.mark.gpu
F = np.float32
INVALID_ARGUMENT = -1   # BSLAM_ERR_INVALID_ARGUMENT
NORMAL_TOLERANCE = 1e-6
CASES = ru.constructed_cases()


@pytest.fixture(scope="module")
def gpu():
    import torch
    from badslam_amd import build
    build.build()
    return torch, badslam_amd.lib(), badslam_amd.Context(0)


@pytest.fixture(scope="module")
def meshes():
    """name -> (positions, normals, colors, triangles): the constructed cases, the cube as a soup, the three spheres (the last with
    colours) and the soup of the sphere with two holes."""
    rng = np.random.default_rng(3)
    out = dict(CASES)
    p, t = ru.cube()
    out["cube soup"] = ru.soup(p, None, None, t)
    for holes in (0, 1, 2):
        p, n, t = ru.sphere(holes)
        out[f"sphere {holes}"] = (p, n, rng.integers(0, 256, (len(p), 4), dtype=np.uint8) if holes == 2 else None, t)
    out["sphere 2 soup"] = ru.soup(*out["sphere 2"])
    return out


def p_(b):
    return None if b is None else b.ptr


class Mesh:
    """A mesh on the device between guard words."""

    def __init__(self, torch, positions, normals, colors, triangles):
        self.positions, self.normals, self.colors, self.triangles = ru._arrays(positions, normals, colors, triangles)
        V, T = self.V, self.T = len(self.positions), len(self.triangles)
        opt = lambda a, words: None if a is None else Guarded(torch, words, a)
        self.dev = dict(positions=Guarded(torch, 3 * V, self.positions), normals=opt(self.normals, 3 * V), colors=opt(self.colors, V),
                        indices=Guarded(torch, 3 * T, self.triangles))
        self.before = {k: b.read() for k, b in self.dev.items() if b is not None}

    def inputs(self):
        return [p_(self.dev[k]) for k in ("positions", "normals", "colors", "indices")]

    def assert_untouched(self):
        for k, was in self.before.items():
            assert np.array_equal(self.dev[k].read(), was), f"{k} was written to"


def outputs(torch, mesh, V, T, **extra):
    """Sentinel-filled outputs with room for V vertices and T triangles; extra: name -> words (None: not given)."""
    opt = lambda present, words: Guarded(torch, words) if present else None
    out = dict(out_positions=Guarded(torch, 3 * V), out_normals=opt(mesh.normals is not None, 3 * V), out_colors=opt(mesh.colors is not None, V),
               out_indices=Guarded(torch, 3 * T))
    out.update({k: None if words is None else Guarded(torch, words) for k, words in extra.items()})
    return out


def read_mesh(out, V2, T2):
    """The first V2 vertices and T2 triangles of the outputs; asserts that everything behind them is untouched."""
    o = {k: None if b is None else b.read() for k, b in out.items()}
    for k, per, n in (("out_positions", 3, V2), ("out_normals", 3, V2), ("out_colors", 1, V2), ("out_indices", 3, T2)):
        assert o[k] is None or (o[k][per * n:] == SENTINEL).all(), f"{k} was written at or beyond the returned count"
    return dict(positions=o["out_positions"][:3 * V2].view(F).reshape(V2, 3), normals=None if o["out_normals"] is None else o["out_normals"][:3 * V2].view(F).reshape(V2, 3),
                colors=None if o["out_colors"] is None else o["out_colors"][:V2].view(np.uint8).reshape(V2, 4), triangles=o["out_indices"][:3 * T2].reshape(T2, 3)), o


def assert_untouched(out):
    for k, b in out.items():
        assert b is None or (b.read() == SENTINEL).all(), f"a refused call wrote to {k}"


def assert_equal(got, want, what, keys=("positions", "colors", "triangles")):
    assert len(got["positions"]) == len(want["positions"]) and len(got["triangles"]) == len(want["triangles"]), \
        f"{what}: {len(got['positions'])} / {len(got['triangles'])} for {len(want['positions'])} / {len(want['triangles'])}"
    for k in keys:
        g, w = got[k], want[k]
        assert (g is None) == (w is None), f"{what}: {k} present in one only"
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w).reshape(np.asarray(g).shape)
        differ = bits(g) != bits(w.astype(F)) if g.dtype == F else g != w
        assert not differ.any(), f"{what}: {int(differ.sum())} {k} differ, first at {np.argwhere(differ)[0]}: {g[differ][0]!r} for {w[differ][0]!r}"
    assert (got["normals"] is None) == (want["normals"] is None), f"{what}: normals present in one only"
    if got["normals"] is not None and len(got["normals"]):
        error = np.abs(got["normals"].astype(np.float64) - want["normals"].astype(np.float64)).max()
        assert error <= NORMAL_TOLERANCE, f"{what}: normals differ by {error:.3e}"


# ------------------------------------------------------------------------------------------------
# the three calls on host arrays
# ------------------------------------------------------------------------------------------------
def clean(gpu, positions, normals, colors, triangles, flags=(1, 1, 1), maps=True, ctx=None):
    """bslam_clean_mesh -> the dict of ru.clean (maps None when not asked for)."""
    torch, L, default = gpu
    m = Mesh(torch, positions, normals, colors, triangles)
    out = outputs(torch, m, m.V, m.T, vertex_map=m.V if maps else None, triangle_map=m.T if maps else None)
    v, t, counts = C.c_uint32(SENTINEL), C.c_uint32(SENTINEL), (C.c_uint32 * 4)()
    badslam_amd.check(L.bslam_clean_mesh((ctx or default).handle, stream_ptr(torch), m.V, m.T, *m.inputs(), *[int(f) for f in flags], p_(out["out_positions"]),
                                         p_(out["out_normals"]), p_(out["out_colors"]), p_(out["out_indices"]), p_(out["vertex_map"]), p_(out["triangle_map"]),
                                         C.byref(v), C.byref(t), counts))
    m.assert_untouched()
    got, o = read_mesh(out, v.value, t.value)
    got.update(vertex_map=o["vertex_map"], triangle_map=o["triangle_map"],
               report=dict(welded_vertices=counts[0], unreferenced_vertices=counts[1], degenerate_triangles=counts[2], duplicate_triangles=counts[3]))
    return got


def check_clean(gpu, mesh, what, flags=(1, 1, 1), **kwargs):
    want = ru.clean(*mesh, weld=bool(flags[0]), remove_duplicates=bool(flags[1]), remove_unreferenced=bool(flags[2]))
    got = clean(gpu, *mesh, flags=flags, **kwargs)
    assert got["report"] == want["report"], f"{what}: {got['report']} for {want['report']}"
    assert_equal(got, want, what, keys=("positions", "colors", "triangles") + (("vertex_map", "triangle_map") if got["vertex_map"] is not None else ()))
    return got, want


def topology(gpu, V, triangles, per_slot=True, ctx=None):
    """bslam_mesh_topology -> (report dict, edge_uses (T, 3), loop_of_slot (T, 3))."""
    torch, L, default = gpu
    triangles = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    T = len(triangles)
    idx = Guarded(torch, 3 * T, triangles)
    uses, loops = (Guarded(torch, 3 * T), Guarded(torch, 3 * T)) if per_slot else (None, None)
    report = abi.MeshReport()
    badslam_amd.check(L.bslam_mesh_topology((ctx or default).handle, stream_ptr(torch), V, T, idx.ptr, C.byref(report), p_(uses), p_(loops)))
    assert np.array_equal(idx.read(), triangles.reshape(-1)), "the indices were written to"
    return report.as_dict(), None if uses is None else uses.read().reshape(T, 3), None if loops is None else loops.read().reshape(T, 3)


def check_topology(gpu, V, triangles, what, **kwargs):
    want = ru.topology(V, triangles)
    got, uses, loops = topology(gpu, V, triangles, **kwargs)
    assert got == {k: want[k] for k in ru.REPORT_FIELDS}, f"{what}: {got} for { {k: want[k] for k in ru.REPORT_FIELDS} }"
    if uses is not None:
        assert np.array_equal(uses, want["edge_uses"]), f"{what}: edge_uses differ"
        assert np.array_equal(loops, want["loop_of_slot"]), f"{what}: loop_of_slot differs"
    return got, want


def fill(gpu, positions, normals, colors, triangles, max_hole_edges, spare=(3, 5), holes=True, ctx=None):
    """bslam_fill_mesh_holes, once for the counts and once with buffers that have `spare` more room than needed -> the dict of ru.fill_holes."""
    torch, L, default = gpu
    m = Mesh(torch, positions, normals, colors, triangles)
    handle = (ctx or default).handle
    v, t, f = C.c_uint32(SENTINEL), C.c_uint32(SENTINEL), C.c_uint32(SENTINEL)
    badslam_amd.check(L.bslam_fill_mesh_holes(handle, stream_ptr(torch), m.V, m.T, *m.inputs(), max_hole_edges, 0, 0, None, None, None, None, None, C.byref(v), C.byref(t),
                                              C.byref(f)))
    V2, T2, filled = v.value, t.value, f.value
    VC, TC = V2 + spare[0], T2 + spare[1]
    out = outputs(torch, m, VC, TC, hole_of_triangle=TC - m.T if holes else None)
    badslam_amd.check(L.bslam_fill_mesh_holes(handle, stream_ptr(torch), m.V, m.T, *m.inputs(), max_hole_edges, VC, TC, p_(out["out_positions"]), p_(out["out_normals"]),
                                              p_(out["out_colors"]), p_(out["out_indices"]), p_(out["hole_of_triangle"]), C.byref(v), C.byref(t), C.byref(f)))
    assert (v.value, t.value, f.value) == (V2, T2, filled), "the counts of the two calls differ"
    m.assert_untouched()
    got, o = read_mesh(out, V2, T2)
    got["filled_holes"] = filled
    if holes:
        assert (o["hole_of_triangle"][T2 - m.T:] == SENTINEL).all(), "hole_of_triangle was written beyond the appended triangles"
        got["hole_of_triangle"] = o["hole_of_triangle"][:T2 - m.T]
    return got


def check_fill(gpu, mesh, max_hole_edges, what, **kwargs):
    want = ru.fill_holes(*mesh, max_hole_edges)
    got = fill(gpu, *mesh, max_hole_edges, **kwargs)
    assert got["filled_holes"] == want["filled_holes"], f"{what}: {got['filled_holes']} holes for {want['filled_holes']}"
    assert_equal(got, want, what, keys=("positions", "colors", "triangles") + (("hole_of_triangle",) if "hole_of_triangle" in got else ()))
    return got, want


# ------------------------------------------------------------------------------------------------
# 1. bit for bit with the restatement
# ------------------------------------------------------------------------------------------------
ALL = list(CASES) + ["cube soup", "sphere 0", "sphere 1", "sphere 2", "sphere 2 soup"]


@pytest.mark.parametrize("name", ALL)
def test_clean(gpu, meshes, name):
    got, want = check_clean(gpu, meshes[name], name)
    if name == "sphere 2 soup":
        assert (len(got["positions"]), len(got["triangles"]), got["report"]["welded_vertices"]) == (1698, 3346, 10038 - 1698)
        # the soup lists the corners in triangle order, so welding it does not give back the vertex order of the mesh, but its surface
        assert check_topology(gpu, 1698, got["triangles"], "welded soup")[0] == check_topology(gpu, 1698, meshes["sphere 2"][3], "sphere 2")[0]
    if name == "sphere 0":
        assert not any(got["report"].values()) and np.array_equal(got["triangles"], meshes[name][3])
    # idempotence on the device
    again, _ = check_clean(gpu, (got["positions"], got["normals"], got["colors"], got["triangles"]), name + ", cleaned")
    assert not any(again["report"].values()) and np.array_equal(bits(again["positions"]), bits(got["positions"])) and np.array_equal(again["triangles"], got["triangles"])


@pytest.mark.parametrize("flags", [(w, d, u) for w in (0, 1) for d in (0, 1) for u in (0, 1)])
def test_clean_flags(gpu, meshes, flags):
    seen = {}
    for name in ("one coordinate apart", "named by a dropped triangle only", "degenerate after welding", "sheet with a hole"):
        _, want = check_clean(gpu, meshes[name], f"{name} {flags}", flags=flags)
        for k, n in want["report"].items():
            seen[k] = seen.get(k, 0) + n
    assert seen["degenerate_triangles"] > 0 and (seen["welded_vertices"] > 0) == bool(flags[0]) and (seen["duplicate_triangles"] > 0) == bool(flags[1])
    assert (seen["unreferenced_vertices"] > 0) == bool(flags[2])


@pytest.mark.parametrize("attributes", ["positions alone", "normals", "colors"])
def test_clean_without_attributes_and_maps(gpu, meshes, attributes):
    for name in ("sheet with a hole", "sphere 2 soup"):
        p, n, c, t = meshes[name]
        mesh = (p, n if attributes == "normals" else None, c if attributes == "colors" else None, t)
        check_clean(gpu, mesh, f"{name}, {attributes}", maps=False)


@pytest.mark.parametrize("name", ["bow-tie", "flipped neighbour", "three on an edge", "cube soup", "sphere 0", "sphere 1", "sphere 2", "sphere 2 soup"])
def test_topology(gpu, meshes, name):
    p, _, _, t = meshes[name]
    got, want = check_topology(gpu, len(p), t, name)
    assert check_topology(gpu, len(p), t, name + ", no per-slot outputs", per_slot=False)[0] == got
    if name == "sphere 2":
        assert (got["boundary_edges"], got["loops"], got["longest_loop"], got["loop_edges"], got["euler"]) == (50, 2, 38, 50, 0)
    if name == "sphere 2 soup":
        assert (got["loops"], got["longest_loop"], got["boundary_edges"]) == (3346, 3, 10038)


@pytest.mark.parametrize("name", [n for n in CASES if len(CASES[n][3])])
def test_topology_of_the_cleaned_cases(gpu, meshes, name):
    cleaned = ru.clean(*meshes[name])
    check_topology(gpu, len(cleaned["positions"]), cleaned["triangles"], name + ", cleaned")
    # vertices that no triangle names are counted by neither side
    check_topology(gpu, len(cleaned["positions"]) + 70, cleaned["triangles"], name + ", cleaned, with unreferenced vertices")


def test_topology_of_long_open_chains_and_many_loops(gpu):
    """A strip of 300 triangles is one loop of 302; two strips that share one vertex block it and leave two open chains; pointer jumping
    needs 10 rounds for either."""
    n = 150
    strip = lambda base: [t for i in range(n) for t in ((base + 2 * i, base + 2 * i + 1, base + 2 * i + 2), (base + 2 * i + 1, base + 2 * i + 3, base + 2 * i + 2))]
    got, _ = check_topology(gpu, 2 * n + 2, strip(0), "strip")
    assert (got["loops"], got["longest_loop"], got["open_boundary_slots"]) == (1, 2 * n + 2, 0)
    joined = np.array(strip(0) + strip(2 * n + 2), np.uint32)
    joined[joined == 2 * n + 2] = 0                       # the second strip starts at the first one's vertex 0
    got, _ = check_topology(gpu, 4 * n + 4, joined, "two strips on one vertex")
    assert (got["loops"], got["blocked_vertices"], got["open_boundary_slots"]) == (0, 1, 2 * (2 * n + 2))


@pytest.mark.parametrize("attributes", ["all", "positions alone"])
@pytest.mark.parametrize("max_hole_edges", [8, 16, 64])
def test_fill_the_sphere(gpu, meshes, max_hole_edges, attributes):
    p, n, c, t = meshes["sphere 2"]
    mesh = (p, n, c, t) if attributes == "all" else (p, None, None, t)
    got, want = check_fill(gpu, mesh, max_hole_edges, f"sphere 2, {max_hole_edges}", holes=attributes == "all")
    assert got["filled_holes"] == {8: 0, 16: 1, 64: 2}[max_hole_edges]
    r, _ = check_topology(gpu, len(got["positions"]), got["triangles"], "the filled sphere")
    assert r["boundary_edges"] == {8: 50, 16: 38, 64: 0}[max_hole_edges] and r["inconsistent_edges"] == 0 and r["euler"] == {8: 0, 16: 1, 64: 2}[max_hole_edges]
    if max_hole_edges == 64:
        volume, closed = fu.signed_volume(got["positions"], got["triangles"]), fu.signed_volume(*[meshes["sphere 0"][k] for k in (0, 3)])
        assert 0.98 * closed < volume < closed


def test_fill_small_meshes(gpu, meshes):
    cleaned = ru.clean(*meshes["sheet with a hole"])
    mesh = (cleaned["positions"], cleaned["normals"], cleaned["colors"], cleaned["triangles"])
    for limit, filled in ((3, 0), (4, 1), (15, 1), (16, 2), (4096, 2)):
        assert check_fill(gpu, mesh, limit, f"sheet, {limit}")[0]["filled_holes"] == filled
    p, n, c, t = meshes["cube soup"]
    got, _ = check_fill(gpu, (p, n, c, t), 3, "cube soup")            # every triangle is a hole of its own
    assert got["filled_holes"] == 12 and len(got["triangles"]) == 48
    for name in ("bow-tie", "flipped neighbour", "three on an edge"):  # nothing but blocked vertices: nothing is filled
        assert check_fill(gpu, meshes[name], 4096, name)[0]["filled_holes"] == 0
    # zero normals on the rim of the hole give a zero normal
    zero = np.zeros_like(mesh[1])
    got, _ = check_fill(gpu, (mesh[0], zero, mesh[2], mesh[3]), 4, "sheet, zero normals")
    assert np.array_equal(bits(got["normals"][25]), bits(np.zeros(3, F)))
    assert check_fill(gpu, (np.zeros((5, 3), F), None, None, None), 10, "a point cloud")[0]["filled_holes"] == 0


def test_fill_counts_only_and_short_capacities(gpu, meshes):
    torch, L, ctx = gpu
    p, n, c, t = meshes["sphere 2"]
    m = Mesh(torch, p, n, c, t)
    for VC, TC, null in ((1700, 3396, "out_positions"), (1700, 3396, "out_indices"), (1699, 3396, None), (1700, 3395, None), (0, 0, None)):
        out = outputs(torch, m, VC, TC, hole_of_triangle=max(TC - m.T, 0))
        if null:
            out[null] = None
        v, tt, f = C.c_uint32(SENTINEL), C.c_uint32(SENTINEL), C.c_uint32(SENTINEL)
        badslam_amd.check(L.bslam_fill_mesh_holes(ctx.handle, stream_ptr(torch), m.V, m.T, *m.inputs(), 64, VC, TC, p_(out["out_positions"]), p_(out["out_normals"]),
                                                  p_(out["out_colors"]), p_(out["out_indices"]), p_(out["hole_of_triangle"]), C.byref(v), C.byref(tt), C.byref(f)))
        assert (v.value, tt.value, f.value) == (1700, 3396, 2), (VC, TC, null)
        assert_untouched(out)
    m.assert_untouched()


def test_two_calls_agree(gpu, meshes):
    mesh = meshes["sphere 2 soup"]
    a, b = clean(gpu, *mesh), clean(gpu, *mesh)
    for k in ("positions", "normals", "colors", "triangles", "vertex_map", "triangle_map"):
        assert np.array_equal(bits(a[k]) if a[k].dtype == F else a[k], bits(b[k]) if b[k].dtype == F else b[k]), k
    mesh = meshes["sphere 2"]
    a, b = fill(gpu, *mesh, 64), fill(gpu, *mesh, 64)
    for k in ("positions", "normals", "colors", "triangles", "hole_of_triangle"):
        assert np.array_equal(bits(a[k]) if a[k].dtype == F else a[k], bits(b[k]) if b[k].dtype == F else b[k]), k
    a, b = topology(gpu, len(mesh[0]), mesh[3]), topology(gpu, len(mesh[0]), mesh[3])
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_empty_mesh(gpu):
    got = clean(gpu, np.zeros((0, 3), F), None, None, None)
    assert len(got["positions"]) == 0 and len(got["triangles"]) == 0 and not any(got["report"].values())
    report, _, _ = topology(gpu, 0, np.zeros((0, 3), np.uint32))
    assert not any(report.values())
    assert fill(gpu, np.zeros((0, 3), F), None, None, None, 10, spare=(0, 0))["filled_holes"] == 0
    # vertices without triangles: nothing to weld away but duplicates, no edge, no hole
    report, _, _ = topology(gpu, 7, np.zeros((0, 3), np.uint32))
    assert not any(report.values())


def test_a_second_call_with_a_larger_mesh_grows_the_slab(gpu, meshes):
    """A context of its own, so that its first repair call is the small one; the three calls share the slab."""
    ctx = badslam_amd.Context(0)
    for name in ("sheet with a hole", "sphere 2 soup", "bow-tie"):
        check_clean(gpu, meshes[name], name, ctx=ctx)
    cleaned = ru.clean(*meshes["sheet with a hole"])
    check_topology(gpu, 25, cleaned["triangles"], "sheet", ctx=ctx)
    check_fill(gpu, meshes["sphere 2"], 64, "sphere 2", ctx=ctx)
    check_clean(gpu, meshes["sphere 1"], "sphere 1", ctx=ctx)


def test_stage_times_with_profiling_on(gpu, meshes):
    """Profiling changes no result, and a profiled call leaves its stage times.  A context of its own: the switch is the context's."""
    torch, L, _ = gpu
    ctx = badslam_amd.Context(0)

    def times(stages):
        ms = (C.c_float * 8)(*[-1.0] * 8)
        badslam_amd.check(L.bslam_repair_stage_times(ctx.handle, ms))
        ms = np.array(ms[:], np.float64)
        assert np.isfinite(ms).all() and (ms >= 0).all() and (ms[:stages] > 0).any() and (ms[stages:] == 0).all(), ms

    try:
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
        check_clean(gpu, meshes["sphere 2 soup"], "profiled", ctx=ctx)
        times(8)
        p, _, _, t = meshes["sphere 2"]
        check_topology(gpu, len(p), t, "profiled", ctx=ctx)
        times(4)
        check_fill(gpu, meshes["sphere 2"], 64, "profiled", ctx=ctx)
        times(6)
    finally:
        L.bslam_profile_enable(ctx.handle, 0)


# ------------------------------------------------------------------------------------------------
# 2. refusals: by the return code, without a fault and without a write
# ------------------------------------------------------------------------------------------------
def test_rejected_arguments_of_clean(gpu, meshes):
    torch, L, ctx = gpu
    mesh = meshes["sphere 2"]
    m = Mesh(torch, *mesh)
    V, T = m.V, m.T
    out = outputs(torch, m, V, T, vertex_map=V, triangle_map=T)
    vc, tc, counts = C.c_uint32(SENTINEL), C.c_uint32(SENTINEL), (C.c_uint32 * 4)(*[SENTINEL] * 4)
    base = dict(ctx=ctx.handle, weld=1, duplicates=1, unreferenced=1, vcount=C.byref(vc), tcount=C.byref(tc), counts=counts)
    base.update({k: b.address for k, b in m.dev.items()})
    base.update({k: b.address for k, b in out.items()})

    def run(**changes):
        a = dict(base, **changes)
        p = lambda v: None if v is None else C.c_void_p(v)
        return L.bslam_clean_mesh(a["ctx"], stream_ptr(torch), V, T, p(a["positions"]), p(a["normals"]), p(a["colors"]), p(a["indices"]), a["weld"], a["duplicates"],
                                  a["unreferenced"], p(a["out_positions"]), p(a["out_normals"]), p(a["out_colors"]), p(a["out_indices"]), p(a["vertex_map"]),
                                  p(a["triangle_map"]), a["vcount"], a["tcount"], a["counts"])

    a = base
    cases = {"null context": dict(ctx=None), "null out_vertex_count": dict(vcount=None), "null out_triangle_count": dict(tcount=None), "null counts": dict(counts=None),
             "null positions": dict(positions=None), "null indices": dict(indices=None), "null out_positions": dict(out_positions=None),
             "null out_indices": dict(out_indices=None), "weld = 2": dict(weld=2), "remove_duplicates = -1": dict(duplicates=-1), "remove_unreferenced = 3": dict(unreferenced=3),
             "misaligned positions": dict(positions=a["positions"] + 2), "misaligned normals": dict(normals=a["normals"] + 1), "misaligned colors": dict(colors=a["colors"] + 2),
             "misaligned indices": dict(indices=a["indices"] + 1), "misaligned out_positions": dict(out_positions=a["out_positions"] + 2),
             "misaligned out_indices": dict(out_indices=a["out_indices"] + 2), "misaligned vertex_map": dict(vertex_map=a["vertex_map"] + 2),
             "misaligned triangle_map": dict(triangle_map=a["triangle_map"] + 1),
             "in place: positions": dict(out_positions=a["positions"]), "in place: indices": dict(out_indices=a["indices"]),
             "triangle_map inside indices": dict(triangle_map=a["indices"] + 12 * T - 4), "vertex_map inside colors": dict(vertex_map=a["colors"] + 4 * V - 4),
             "two outputs overlap": dict(out_normals=a["out_positions"] + 12 * V - 4), "the maps are one": dict(triangle_map=a["vertex_map"]),
             "normals without out_normals": dict(out_normals=None), "out_normals without normals": dict(normals=None),
             "colors without out_colors": dict(out_colors=None), "out_colors without colors": dict(colors=None)}
    for name, changes in cases.items():
        rc = run(**changes)
        assert rc == INVALID_ARGUMENT, (name, rc, L.bslam_last_error())
    torch.cuda.synchronize()
    assert_untouched(out)
    m.assert_untouched()
    assert (vc.value, tc.value, counts[0]) == (SENTINEL, SENTINEL, SENTINEL)
    assert run() == 0 and (vc.value, tc.value, list(counts)) == (V, T, [0, 0, 0, 0])


def test_rejected_arguments_of_topology_and_fill(gpu, meshes):
    torch, L, ctx = gpu
    m = Mesh(torch, *meshes["sphere 2"])
    V, T = m.V, m.T
    uses, loops = Guarded(torch, 3 * T), Guarded(torch, 3 * T)
    report = abi.MeshReport()
    report.euler = -77
    idx = m.dev["indices"].address
    p = lambda v: None if v is None else C.c_void_p(v)
    top = lambda ctx_=ctx.handle, i=idx, r=C.byref(report), u=uses.address, l=loops.address: L.bslam_mesh_topology(ctx_, stream_ptr(torch), V, T, p(i), r, p(u), p(l))
    for name, rc in {"null context": top(ctx_=None), "null report": top(r=None), "null indices": top(i=None), "misaligned indices": top(i=idx + 2),
                     "misaligned edge_uses": top(u=uses.address + 1), "misaligned loop_of_slot": top(l=loops.address + 2), "edge_uses in place": top(u=idx),
                     "loop_of_slot inside indices": top(l=idx + 12 * T - 4), "the outputs overlap": top(l=uses.address + 12 * T - 8)}.items():
        assert rc == INVALID_ARGUMENT, (name, rc)
    assert report.euler == -77 and (uses.read() == SENTINEL).all() and (loops.read() == SENTINEL).all()
    assert top() == 0 and report.euler == 0

    VC, TC = 1700, 3396
    out = outputs(torch, m, VC, TC, hole_of_triangle=TC - T)
    vc, tc, fc = C.c_uint32(SENTINEL), C.c_uint32(SENTINEL), C.c_uint32(SENTINEL)
    base = dict(ctx=ctx.handle, limit=64, vcount=C.byref(vc), tcount=C.byref(tc), fcount=C.byref(fc))
    base.update({k: b.address for k, b in m.dev.items()})
    base.update({k: b.address for k, b in out.items()})

    def run(**changes):
        a = dict(base, **changes)
        return L.bslam_fill_mesh_holes(a["ctx"], stream_ptr(torch), V, T, p(a["positions"]), p(a["normals"]), p(a["colors"]), p(a["indices"]), a["limit"], VC, TC,
                                       p(a["out_positions"]), p(a["out_normals"]), p(a["out_colors"]), p(a["out_indices"]), p(a["hole_of_triangle"]), a["vcount"],
                                       a["tcount"], a["fcount"])

    a = base
    cases = {"null context": dict(ctx=None), "null out_vertex_count": dict(vcount=None), "null out_triangle_count": dict(tcount=None), "null filled_holes": dict(fcount=None),
             "max_hole_edges = 2": dict(limit=2), "max_hole_edges = 4097": dict(limit=4097), "max_hole_edges = 0": dict(limit=0),
             "null positions": dict(positions=None), "null indices": dict(indices=None),
             "misaligned positions": dict(positions=a["positions"] + 2), "misaligned indices": dict(indices=a["indices"] + 1),
             "misaligned out_positions": dict(out_positions=a["out_positions"] + 2), "misaligned out_colors": dict(out_colors=a["out_colors"] + 1),
             "misaligned hole_of_triangle": dict(hole_of_triangle=a["hole_of_triangle"] + 2),
             "in place: positions": dict(out_positions=a["positions"]), "in place: indices": dict(out_indices=a["indices"]),
             "hole_of_triangle inside indices": dict(hole_of_triangle=a["indices"] + 12 * T - 4), "two outputs overlap": dict(out_normals=a["out_positions"] + 12 * VC - 4),
             "normals without out_normals": dict(out_normals=None), "out_colors without colors": dict(colors=None)}
    for name, changes in cases.items():
        rc = run(**changes)
        assert rc == INVALID_ARGUMENT, (name, rc, L.bslam_last_error())
    torch.cuda.synchronize()
    assert_untouched(out)
    m.assert_untouched()
    assert (vc.value, tc.value, fc.value) == (SENTINEL, SENTINEL, SENTINEL)
    assert run() == 0 and (vc.value, tc.value, fc.value) == (VC, TC, 2)


@pytest.mark.parametrize("what", ["index = V", "index = 0xFFFFFFFF", "NaN position", "infinite position", "degenerate triangle"])
def test_device_refusals_leave_the_outputs_untouched(gpu, meshes, what):
    torch, L, ctx = gpu
    p, n, c, t = meshes["sphere 2"]
    p, t = p.copy(), t.copy()
    if what.startswith("index"):
        t[1500, 1] = len(p) if what == "index = V" else 0xFFFFFFFF
        message = b"a triangle names a vertex beyond vertex_count"
    elif what == "degenerate triangle":
        t[1500, 2] = t[1500, 0]
        message = b"a triangle repeats an index"
    else:
        p[777, 1] = np.nan if what == "NaN position" else -np.inf
        message = b"a vertex is not finite"
    m = Mesh(torch, p, n, c, t)
    V, T = m.V, m.T
    v, tt, f, counts = C.c_uint32(SENTINEL), C.c_uint32(SENTINEL), C.c_uint32(SENTINEL), (C.c_uint32 * 4)(*[SENTINEL] * 4)
    if what != "degenerate triangle":                       # cleaning drops it
        out = outputs(torch, m, V, T, vertex_map=V, triangle_map=T)
        rc = L.bslam_clean_mesh(ctx.handle, stream_ptr(torch), V, T, *m.inputs(), 1, 1, 1, p_(out["out_positions"]), p_(out["out_normals"]), p_(out["out_colors"]),
                                p_(out["out_indices"]), p_(out["vertex_map"]), p_(out["triangle_map"]), C.byref(v), C.byref(tt), counts)
        assert rc == INVALID_ARGUMENT and b"bslam_clean_mesh: " + message in L.bslam_last_error()
        assert_untouched(out)
        assert (v.value, tt.value, counts[0]) == (SENTINEL, SENTINEL, SENTINEL)
    if "position" not in what:                              # the census does not see the positions
        report = abi.MeshReport()
        report.euler = -77
        uses, loops = Guarded(torch, 3 * T), Guarded(torch, 3 * T)
        rc = L.bslam_mesh_topology(ctx.handle, stream_ptr(torch), V, T, m.dev["indices"].ptr, C.byref(report), uses.ptr, loops.ptr)
        assert rc == INVALID_ARGUMENT and b"bslam_mesh_topology: " + message in L.bslam_last_error() and report.euler == -77
        torch.cuda.synchronize()
        assert (uses.read() == SENTINEL).all(), "a refused census wrote to edge_uses"
        assert (loops.read() == SENTINEL).all(), "a refused census wrote to loop_of_slot"
    out = outputs(torch, m, V + 2, T + 50, hole_of_triangle=50)
    rc = L.bslam_fill_mesh_holes(ctx.handle, stream_ptr(torch), V, T, *m.inputs(), 64, V + 2, T + 50, p_(out["out_positions"]), p_(out["out_normals"]), p_(out["out_colors"]),
                                 p_(out["out_indices"]), p_(out["hole_of_triangle"]), C.byref(v), C.byref(tt), C.byref(f))
    assert rc == INVALID_ARGUMENT and b"bslam_fill_mesh_holes: " + message in L.bslam_last_error()
    assert_untouched(out)
    assert (v.value, tt.value, f.value) == (SENTINEL, SENTINEL, SENTINEL)
    m.assert_untouched()
    check_fill(gpu, meshes["sphere 2"], 64, "the context is fine afterwards")


# ------------------------------------------------------------------------------------------------
# 3. through DirectBA
# ------------------------------------------------------------------------------------------------
def as_dict(mesh):
    p, n, c, t = mesh
    return dict(positions=p, normals=n, colors=c, triangles=t)


def test_direct_ba_clean_after_simplify_and_decimate(extracted, meshes):   # noqa: F811
    """The sphere with one hole at cell 2.0 (in its voxel units, from the per-axis minimum of its vertices), chosen on the CPU:
    tests/simplify_mesh_util.py gives 385 vertices and 760 triangles, of which the restatement finds 5 to be duplicates -- doubled faces,
    whose edges the decimator can take neither for a boundary nor for a manifold edge.  CleanMesh of it holds no triangle twice.  The
    boundary vertices of the decimator are the ends of the edges that one triangle uses: one round of DecimateMesh on the cleaned mesh
    equals its restatement, which takes them from the same census as the repair restatement -- 23 boundary edges in one loop."""
    from tests import decimate_mesh_util as du
    from tests import simplify_mesh_util as su
    ba, _ = extracted
    sphere = as_dict(meshes["sphere 1"])
    want_simplified = su.simplify(sphere["positions"], sphere["normals"], None, sphere["triangles"], sphere["positions"].min(axis=0), 2.0)
    want = ru.clean(want_simplified["positions"], want_simplified["normals"], None, want_simplified["triangles"])
    assert (len(want_simplified["positions"]), len(want_simplified["triangles"]), want["report"]["duplicate_triangles"]) == (385, 760, 5)
    doubled = ru.topology(385, want_simplified["triangles"])
    simplified = ba.SimplifyMesh(sphere, 2.0)
    got = ba.CleanMesh(simplified)
    assert set(got) == set(sphere) | {"vertex_map", "triangle_map", "report"} and got["colors"] is None
    assert got["report"] == want["report"]
    assert_equal(got, want, "CleanMesh(SimplifyMesh)", keys=("positions", "triangles", "vertex_map", "triangle_map"))
    assert len(set(map(frozenset, got["triangles"].tolist()))) == len(got["triangles"]) == 755
    census = ru.topology(len(got["positions"]), got["triangles"])
    on_device = ba.MeshTopology(got, per_slot=True)
    assert {k: on_device[k] for k in ru.REPORT_FIELDS} == {k: census[k] for k in ru.REPORT_FIELDS} and np.array_equal(on_device["edge_uses"], census["edge_uses"])
    # the edges of the doubled faces are used four times before and, with one of each pair of faces gone, three times after
    assert (census["boundary_edges"], census["loops"]) == (23, 1) and doubled["edge_uses"].max() == 4 and census["edge_uses"].max() == 3
    # the boundary vertices by the census, and by the count of the decimation restatement (edges that one triangle uses)
    boundary = set(int(v) for row, uses in zip(got["triangles"], on_device["edge_uses"]) for k in range(3) if uses[k] == 1 for v in (row[k], row[(k + 1) % 3]))
    count = {}
    for row in got["triangles"].tolist():
        for k in range(3):
            key = (min(row[k], row[(k + 1) % 3]), max(row[k], row[(k + 1) % 3]))
            count[key] = count.get(key, 0) + 1
    assert boundary == {v for key, c in count.items() if c == 1 for v in key} and len(boundary) >= 23
    target = len(got["positions"]) // 2
    want_decimated = du.decimate(got["positions"], got["normals"], None, got["triangles"], target, max_rounds=1)
    decimated = ba.DecimateMesh(got, target_vertices=target, max_rounds=1)
    assert np.array_equal(bits(decimated["positions"]), bits(want_decimated["positions"])) and np.array_equal(decimated["triangles"], want_decimated["triangles"])
    assert np.array_equal(decimated["vertex_map"], want_decimated["vertex_map"]) and len(decimated["positions"]) < len(got["positions"])
    again = ba.CleanMesh(decimated)
    assert len(set(map(frozenset, again["triangles"].tolist()))) == len(again["triangles"])


def test_direct_ba_topology_of_an_extracted_mesh(extracted):   # noqa: F811
    ba, mesh = extracted
    got = ba.MeshTopology(mesh, per_slot=True)
    want = ru.topology(len(mesh["positions"]), mesh["triangles"])
    assert {k: got[k] for k in ru.REPORT_FIELDS} == {k: want[k] for k in ru.REPORT_FIELDS}
    assert np.array_equal(got["edge_uses"], want["edge_uses"]) and np.array_equal(got["loop_of_slot"], want["loop_of_slot"])
    undirected, directed = fu.edge_census(mesh["triangles"])
    assert got["unique_edges"] == len(undirected) and got["boundary_edges"] == int((undirected == 1).sum()) and got["interior_edges"] == int((undirected == 2).sum())
    assert got["nonmanifold_edges"] == int((undirected >= 3).sum())
    if got["nonmanifold_edges"] == 0:               # with manifold edges, a directed edge is used twice iff an interior edge is inconsistently oriented
        assert got["inconsistent_edges"] == int((directed == 2).sum())
    labels, _ = ba.MeshComponents(mesh)
    assert got["components"] == int((labels == np.arange(len(labels))).sum())
    assert got["closed"] == (got["boundary_edges"] == 0 and got["nonmanifold_edges"] == 0) and got["manifold_edges"] == (got["nonmanifold_edges"] == 0)
    assert got["oriented"] == (got["inconsistent_edges"] == 0)
    print(f"{len(mesh['positions'])} vertices, {len(mesh['triangles'])} triangles: {got['boundary_edges']} boundary edges in {got['loops']} loops, longest {got['longest_loop']}")
    assert got["boundary_edges"] > 0 and got["loops"] > 0 and set(got) >= {"components", "closed", "manifold_edges", "oriented", "euler"}


def test_direct_ba_fill_holes_then_smooth(extracted, meshes):   # noqa: F811
    ba, _ = extracted
    holed = as_dict(meshes["sphere 2"])
    rgb = dict(holed, colors=np.ascontiguousarray(holed["colors"][:, :3]))       # a LoadPLY dict: three channels
    want = ru.fill_holes(*meshes["sphere 2"], 64)
    got = ba.FillHoles(rgb, 64)
    assert set(got) == set(holed) | {"filled_holes"} and got["filled_holes"] == 2 and got["colors"].shape == (1700, 3)
    assert_equal(dict(got, colors=None), dict(want, colors=None), "FillHoles", keys=("positions", "triangles"))
    assert np.array_equal(got["colors"], want["colors"][:, :3])
    assert not ba.MeshTopology(holed)["closed"] and ba.MeshTopology(got)["closed"]
    smoothed = ba.SmoothMesh(got, iterations=3)
    after = ba.MeshTopology(smoothed)
    assert after["closed"] and after["oriented"] and after["euler"] == 2 and after["components"] == 1
    moved = np.abs(smoothed["positions"] - got["positions"]).max(axis=1) > 0
    assert moved[1698:].all(), "the vertices that close the holes have a one-ring and are smoothed with the rest"
    assert ba.FillHoles(holed, 8)["filled_holes"] == 0
    with pytest.raises(Exception, match="max_hole_edges"):
        ba.FillHoles(holed, 2)
    soup = ba.CleanMesh(as_dict(meshes["sphere 2 soup"]))
    assert (len(soup["positions"]), len(soup["triangles"])) == (1698, 3346) and ba.MeshTopology(soup)["loops"] == 2


# ------------------------------------------------------------------------------------------------
# 4. tools/run_tum.py --mesh-fill-holes --mesh-clean
# ------------------------------------------------------------------------------------------------
def test_run_tum_mesh_repair(tmp_path):
    """Five frames of the rendered sequence of tests/test_gpu_bad_slam.py, once with --mesh alone and once with --mesh-simplify-cell,
    --mesh-fill-holes 32, --mesh-clean and --surface-report: without the new flags the file is the extracted mesh, byte for byte, and
    nothing new is reported; with them the file parses and the reported census is the restatement's of the file."""
    import json

    from badslam_amd import direct_ba as dba
    from badslam_amd import png
    from tests.test_gpu_bad_slam import render_sequence
    from tools import run_tum
    cam, raw_to_float, frames, gt = render_sequence(5, seed=5)
    source = tmp_path / "source"
    (source / "rgb").mkdir(parents=True)
    (source / "depth").mkdir()
    assoc = []
    for k, (depth, rgb) in enumerate(frames):
        ts = f"{200.0 + 0.1 * k:.6f}"
        png.write_png(source / "rgb" / f"{ts}.png", rgb)
        png.write_png(source / "depth" / f"{ts}.png", depth)
        assoc.append(f"{ts} rgb/{ts}.png {ts} depth/{ts}.png")
    (source / "associated.txt").write_text("\n".join(assoc) + "\n")
    (source / "calibration.txt").write_text(f"{cam.fx} {cam.fy} {cam.cx - 0.5} {cam.cy - 0.5}\n")
    common = dict(keyframe_interval=4, ba_iterations=2, max_depth=6.0, num_scales=4, max_surfel_count=400000, mesh_voxel_size=0.04, mesh_min_count=2, mesh_min_component=50)
    plain_path, plain_report, again = tmp_path / "plain.ply", tmp_path / "plain.json", {}

    def inspect(slam, result):
        again["extracted"] = slam.ba().ExtractMesh(2, min_component_vertices=50)

    plain = run_tum.run(source, mesh=plain_path, surface_report=plain_report, inspect=inspect, **common)
    reference_path = tmp_path / "reference.ply"
    dba.SaveMeshAsPLY(reference_path, again["extracted"])
    assert plain_path.read_bytes() == reference_path.read_bytes() and not plain_report.exists()
    assert "surface" not in plain and set(plain["mesh"]) == {"path", "vertices", "triangles", "origin", "dims", "components", "removed_vertices", "removed_triangles"}

    mesh_path, report_path = tmp_path / "mesh.ply", tmp_path / "report.json"
    r = run_tum.run(source, mesh=mesh_path, mesh_simplify_cell=0.08, mesh_fill_holes=32, mesh_clean=True, surface_report=report_path, **common)
    own = dba.LoadPLY(mesh_path)
    report = json.loads(report_path.read_text())
    want = ru.topology(len(own["positions"]), own["triangles"])
    assert {k: report["mesh_topology"][k] for k in ru.REPORT_FIELDS} == {k: want[k] for k in ru.REPORT_FIELDS}
    assert report["mesh_topology"]["closed"] == (want["boundary_edges"] == 0 and want["nonmanifold_edges"] == 0) and "components" in report["mesh_topology"]
    fh, cl = report["mesh_hole_filling"], report["mesh_cleaning"]
    print(f"{fh['filled_holes']} holes filled, cleaning: {cl}, topology: {report['mesh_topology']}")
    assert fh["max_hole_edges"] == 32 and fh["vertices"] == fh["vertices_before"] + fh["filled_holes"] and fh["vertices_before"] == len(again["extracted"]["positions"])
    assert [c["after"] for c in cl] == ["simplification"] and cl[0]["vertices"] == len(own["positions"]) and cl[0]["triangles"] == len(own["triangles"])
    assert len(set(map(frozenset, own["triangles"].tolist()))) == len(own["triangles"]), "the cleaned file holds a duplicate triangle"
    assert r["mesh"]["vertices"] == len(own["positions"]) and r["mesh"]["hole_filling"] == fh and r["mesh"]["cleaning"] == cl
