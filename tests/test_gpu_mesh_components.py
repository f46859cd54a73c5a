"""-m gpu: mesh components and small-piece removal (bslam_mesh_components, bslam_filter_mesh, badslam_amd/csrc/mesh_kernels.hpp;
DirectBA.ExtractMesh(min_component_vertices, report) / MeshComponents; tools/run_tum.py --mesh-min-component) against the
sequential restatement of tests/mesh_components_util.py.  Everything is integer or a copy: labels, sizes, counts and indices must
be equal, positions, normals and colours equal bit for bit.  Never against the kernels' own output, except where a test is about
two calls agreeing.  Every device array stands between guard words, outputs are filled with a sentinel first."""
import ctypes as C

import numpy as np
import pytest

import badslam_amd
from badslam_amd import abi
from tests import fusion_util as fu
from tests import mesh_components_util as mu
from tests.test_gpu_fusion import SENTINEL, bits, pitched, stream_ptr, volume_struct

pytestmark = pytest.mark.gpu
F = np.float32
INVALID_ARGUMENT = -1   # BSLAM_ERR_INVALID_ARGUMENT
GUARD, GUARD_WORDS = 0x6B6B6B6B, 16


@pytest.fixture(scope="module")
def gpu():
    import torch
    from badslam_amd import build
    build.build()
    return torch, badslam_amd.lib(), badslam_amd.Context(0)


@pytest.fixture(scope="module")
def specks():
    """The specks mesh with colours, and the restatement's labels, sizes and count: computed once, never changed."""
    positions, normals, _, triangles = mu.specks_mesh()
    colors = np.random.default_rng(23).integers(0, 256, (len(positions), 4), dtype=np.uint8)
    return (positions, normals, colors, triangles) + mu.components(len(positions), triangles)


# ------------------------------------------------------------------------------------------------
# device plumbing
# ------------------------------------------------------------------------------------------------
class Guarded:
    """`words` 4-byte words on the device between two runs of guard words; content: an array of that many bytes, or None for the
    sentinel."""

    def __init__(self, torch, words, content=None):
        host = np.full(words + 2 * GUARD_WORDS, GUARD, np.int32)
        host[GUARD_WORDS:GUARD_WORDS + words] = SENTINEL if content is None else np.ascontiguousarray(content).reshape(-1).view(np.int32)
        self.words, self.tensor = words, torch.from_numpy(host).cuda()
        self.address = self.tensor.data_ptr() + 4 * GUARD_WORDS
        self.ptr = C.c_void_p(self.address)

    def read(self):
        """The content as uint32; asserts that the guard words are intact."""
        host = self.tensor.cpu().numpy()
        assert (host[:GUARD_WORDS] == GUARD).all() and (host[GUARD_WORDS + self.words:] == GUARD).all(), "guard words overwritten"
        return host[GUARD_WORDS:GUARD_WORDS + self.words].view(np.uint32).copy()


def raw_components(gpu, V, index_buffer, T, labels, sizes, count):
    torch, L, ctx = gpu
    return L.bslam_mesh_components(ctx.handle, stream_ptr(torch), V, T, index_buffer.ptr, labels.ptr, sizes.ptr, C.byref(count))


def gpu_components(gpu, V, triangles):
    """bslam_mesh_components of host triangles -> (labels, sizes, count)."""
    torch, L, ctx = gpu
    triangles = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    idx, labels, sizes, count = Guarded(torch, triangles.size, triangles), Guarded(torch, V), Guarded(torch, V), C.c_uint32(SENTINEL)
    badslam_amd.check(raw_components(gpu, V, idx, len(triangles), labels, sizes, count))
    assert np.array_equal(idx.read(), triangles.reshape(-1)), "the indices were written to"
    return labels.read(), sizes.read(), count.value


def assert_components_equal(got, want):
    for name, g, w in zip(("labels", "sizes"), got, want):
        differ = g != w
        assert not differ.any(), f"{name}: {int(differ.sum())} values differ, first at {np.argwhere(differ)[0]}: {g[differ][0]} for {w[differ][0]}"
    assert got[2] == want[2]


def gpu_filter(gpu, positions, normals, colors, triangles, sizes, min_vertices):
    """bslam_filter_mesh of host arrays (normals, colors: None for null) -> (positions', normals', colors', triangles'); asserts
    that inputs, guard words and every output entry at and beyond V' / T' are untouched."""
    torch, L, ctx = gpu
    V, T = len(positions), len(triangles)
    inputs = [Guarded(torch, 3 * V, positions), None if normals is None else Guarded(torch, 3 * V, normals), None if colors is None else Guarded(torch, V, colors),
              Guarded(torch, 3 * T, np.ascontiguousarray(triangles, np.uint32)), Guarded(torch, V, np.ascontiguousarray(sizes, np.uint32))]
    outputs = [Guarded(torch, 3 * V), None if normals is None else Guarded(torch, 3 * V), None if colors is None else Guarded(torch, V), Guarded(torch, 3 * T)]
    before = [None if b is None else b.read() for b in inputs]
    ptr = lambda b: None if b is None else b.ptr
    nv, nt = C.c_uint32(SENTINEL), C.c_uint32(SENTINEL)
    badslam_amd.check(L.bslam_filter_mesh(ctx.handle, stream_ptr(torch), V, T, ptr(inputs[0]), ptr(inputs[1]), ptr(inputs[2]), ptr(inputs[3]), ptr(inputs[4]),
                                          min_vertices, ptr(outputs[0]), ptr(outputs[1]), ptr(outputs[2]), ptr(outputs[3]), C.byref(nv), C.byref(nt)))
    for b, was in zip(inputs, before):
        assert b is None or np.array_equal(b.read(), was), "an input was written to"
    nv, nt = nv.value, nt.value
    assert nv <= V and nt <= T
    got = [None if b is None else b.read() for b in outputs]
    for g, used in zip(got, (3 * nv, 3 * nv, nv, 3 * nt)):
        assert g is None or (g[used:] == SENTINEL).all(), "written at or beyond the kept counts"
    return (got[0][:3 * nv].view(F).reshape(nv, 3), None if got[1] is None else got[1][:3 * nv].view(F).reshape(nv, 3),
            None if got[2] is None else got[2][:nv].view(np.uint8).reshape(nv, 4), got[3][:3 * nt].reshape(nt, 3))


def assert_filtered_equal(got, sizes, min_vertices, positions, normals, colors, triangles):
    want_t, (want_p, want_n, want_c) = mu.filter_mesh(sizes, min_vertices, triangles, positions, normals, colors)
    gp, gn, gc, gt = got
    assert gp.shape == want_p.shape and gt.shape == want_t.shape, (min_vertices, gp.shape, want_p.shape, gt.shape, want_t.shape)
    assert np.array_equal(gt, want_t)
    assert np.array_equal(bits(gp), bits(want_p))
    assert (gn is None) == (want_n is None) and (gn is None or np.array_equal(bits(gn), bits(want_n)))
    assert (gc is None) == (want_c is None) and (gc is None or np.array_equal(gc, want_c))


# ------------------------------------------------------------------------------------------------
# 1. labelling
# ------------------------------------------------------------------------------------------------
def test_specks_components(gpu, specks):
    positions, normals, colors, triangles, labels, sizes, count = specks
    assert (len(positions), len(triangles), count) == (1420, 2820, 5)
    assert_components_equal(gpu_components(gpu, len(positions), triangles), (labels, sizes, count))


@pytest.mark.parametrize("name", ["permuted strip", "strip in order", "interleaved strips"])
def test_strips(gpu, name):
    """2 x 4001 vertices in a ladder: a diameter of 4000 edges.  With the ids permuted, label propagation by pointer jumping needs
    1 728 rounds; one union launch has to do."""
    n = mu.STRIP_RUNGS
    V, triangles = {"permuted strip": (2 * n, mu.permuted_strip()), "strip in order": (2 * n, mu.strip(n)), "interleaved strips": (4 * n, mu.interleaved_strips())}[name]
    want = mu.components(V, triangles)
    assert want[2] == (2 if name == "interleaved strips" else 1) and (want[1] == 8002).all()
    assert_components_equal(gpu_components(gpu, V, triangles), want)


def test_star_and_its_hook_counts(gpu):
    """Hub V - 1 with 4 096 triangles (hub, 2 i, 2 i + 1): every hook contends for the hub's root, and the root keeps changing, down to
    vertex 0.  While profiling is on, the hooks that succeeded are counted.  Every one of them takes one root away, and the seeding
    launch ahead of the union leaves as roots the vertices smaller than all their neighbours, so their number is exact."""
    torch, L, ctx = gpu
    V, triangles = mu.star()
    want = mu.components(V, triangles)
    assert want[2] == 1 and not want[0].any()
    tested, culled = C.c_uint64(), C.c_uint64()
    try:
        badslam_amd.check(L.bslam_profile_enable(ctx.handle, 1))
        badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))     # reset
        got = gpu_components(gpu, V, triangles)
        badslam_amd.check(L.bslam_debug_cull_stats(ctx.handle, C.byref(tested), C.byref(culled)))
    finally:
        L.bslam_profile_enable(ctx.handle, 0)
    assert_components_equal(got, want)
    print(f"star: {tested.value} hooks attempted, {culled.value} failed and retried")
    smallest = np.arange(V)
    t = triangles.astype(np.int64)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        np.minimum.at(smallest, np.maximum(t[:, a], t[:, b]), np.minimum(t[:, a], t[:, b]))
    roots_behind_seeding = int((smallest == np.arange(V)).sum())
    assert roots_behind_seeding == 4096 and tested.value - culled.value == roots_behind_seeding - 1
    assert_components_equal(gpu_components(gpu, V, triangles), want)                                  # and with the counters off


def test_random_sparse(gpu):
    V, triangles = mu.random_sparse()
    want = mu.components(V, triangles)
    assert want[2] > 1000 and (want[1] == 1).sum() > 1000 and want[1].max() > 3
    got = gpu_components(gpu, V, triangles)
    assert_components_equal(got, want)
    positions = np.random.default_rng(5).standard_normal((V, 3)).astype(F)
    positions[::97] = np.array([np.nan, np.inf, -0.0], F)
    positions.view(np.uint32)[::193, 0] = 0x7FA00001                    # a signalling NaN with a payload: copied, not canonicalised
    for min_vertices in (2, 3, 4):
        assert_filtered_equal(gpu_filter(gpu, positions, None, None, triangles, want[1], min_vertices), want[1], min_vertices, positions, None, None, triangles)


@pytest.mark.parametrize("V", [0, 1, 63, 64, 65, 257])
def test_no_triangles(gpu, V):
    labels, sizes, count = gpu_components(gpu, V, np.zeros((0, 3), np.uint32))
    assert np.array_equal(labels, np.arange(V)) and (sizes == 1).all() and count == V
    positions = np.arange(3 * V, dtype=F).reshape(V, 3)
    gp, gn, gc, gt = gpu_filter(gpu, positions, None, None, np.zeros((0, 3), np.uint32), sizes, 1)
    assert np.array_equal(bits(gp), bits(positions)) and len(gt) == 0
    gp, gn, gc, gt = gpu_filter(gpu, positions, None, None, np.zeros((0, 3), np.uint32), sizes, 2)
    assert len(gp) == 0 and len(gt) == 0


def test_two_calls_agree(gpu, specks):
    positions, normals, colors, triangles, labels, sizes, count = specks
    V, tri = 2 * mu.STRIP_RUNGS, mu.permuted_strip()
    assert_components_equal(gpu_components(gpu, V, tri), gpu_components(gpu, V, tri))
    first = gpu_filter(gpu, positions, normals, colors, triangles, sizes, 49)
    second = gpu_filter(gpu, positions, normals, colors, triangles, sizes, 49)
    for a, b in zip(first, second):
        assert np.array_equal(bits(a) if a.dtype == F else a, bits(b) if b.dtype == F else b)


# ------------------------------------------------------------------------------------------------
# 2. filter
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attributes", ["normals and colours", "positions only"])
def test_specks_filter(gpu, specks, attributes):
    positions, normals, colors, triangles, labels, sizes, count = specks
    if attributes == "positions only":
        normals = colors = None
    for min_vertices, kept in ((1, (1420, 2820)), (9, (1412, 2808)), (29, (1384, 2756)), (49, (1336, 2664)), (77, (1260, 2516)), (1261, (0, 0))):
        got = gpu_filter(gpu, positions, normals, colors, triangles, sizes, min_vertices)
        assert (len(got[0]), len(got[3])) == kept
        assert_filtered_equal(got, sizes, min_vertices, positions, normals, colors, triangles)


# ------------------------------------------------------------------------------------------------
# 3. refused input
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["V", "0xFFFFFFFF"])
def test_an_index_beyond_the_vertices_is_refused_and_never_followed(gpu, specks, bad):
    torch, L, ctx = gpu
    positions, normals, colors, triangles, labels, sizes, count = specks
    V = len(positions)
    tri = triangles.copy()
    tri[1777, 1] = V if bad == "V" else 0xFFFFFFFF
    idx, out_l, out_s, n = Guarded(torch, tri.size, tri), Guarded(torch, V), Guarded(torch, V), C.c_uint32(SENTINEL)
    rc = raw_components(gpu, V, idx, len(tri), out_l, out_s, n)
    assert rc == INVALID_ARGUMENT and b"beyond vertex_count" in L.bslam_last_error()
    assert n.value == SENTINEL
    out_l.read(), out_s.read(), idx.read()                                                            # guard words intact
    tri[1777] = (V if bad == "V" else 0xFFFFFFFF, 0, 1)                                               # as the first index: the one the filter keeps by
    bufs = [Guarded(torch, 3 * V, positions), Guarded(torch, 3 * len(tri), tri), Guarded(torch, V, sizes), Guarded(torch, 3 * V), Guarded(torch, 3 * len(tri))]
    nv, nt = C.c_uint32(SENTINEL), C.c_uint32(SENTINEL)
    rc = L.bslam_filter_mesh(ctx.handle, stream_ptr(torch), V, len(tri), bufs[0].ptr, None, None, bufs[1].ptr, bufs[2].ptr, 9, bufs[3].ptr, None, None, bufs[4].ptr,
                             C.byref(nv), C.byref(nt))
    assert rc == INVALID_ARGUMENT and b"beyond vertex_count" in L.bslam_last_error()
    assert (nv.value, nt.value) == (SENTINEL, SENTINEL)
    for b in bufs:
        b.read()
    # no vertex at all: every index is beyond
    rc = raw_components(gpu, 0, Guarded(torch, 3, np.zeros(3, np.uint32)), 1, Guarded(torch, 0), Guarded(torch, 0), n)
    assert rc == INVALID_ARGUMENT
    assert_components_equal(gpu_components(gpu, V, triangles), (labels, sizes, count))                # the context is fine afterwards


def test_rejected_arguments(gpu, specks):
    torch, L, ctx = gpu
    positions, normals, colors, triangles, labels, sizes, count = specks
    V, T = len(positions), len(triangles)
    idx, out_l, out_s = Guarded(torch, 3 * T, triangles), Guarded(torch, V), Guarded(torch, V)
    n = C.c_uint32(SENTINEL)
    base = dict(ctx=ctx.handle, idx=idx.address, labels=out_l.address, sizes=out_s.address, count=C.byref(n))

    def label(**changes):
        a = dict(base, **changes)
        p = lambda v: None if v is None else C.c_void_p(v)
        return L.bslam_mesh_components(a["ctx"], stream_ptr(torch), V, T, p(a["idx"]), p(a["labels"]), p(a["sizes"]), a["count"])

    for name, changes in {"null context": dict(ctx=None), "null indices": dict(idx=None), "null labels": dict(labels=None), "null sizes": dict(sizes=None),
                          "null count": dict(count=None), "misaligned indices": dict(idx=idx.address + 2), "misaligned labels": dict(labels=out_l.address + 1),
                          "misaligned sizes": dict(sizes=out_s.address + 2), "labels are sizes": dict(sizes=out_l.address),
                          "labels overlap sizes": dict(labels=out_s.address - 4 * (V - 1)), "labels inside indices": dict(labels=idx.address + 12 * T - 4),
                          "sizes are indices": dict(sizes=idx.address)}.items():
        rc = label(**changes)
        assert rc == INVALID_ARGUMENT, (name, rc, L.bslam_last_error())
    torch.cuda.synchronize()
    assert (out_l.read() == SENTINEL).all() and (out_s.read() == SENTINEL).all() and n.value == SENTINEL
    assert np.array_equal(idx.read(), triangles.reshape(-1))
    assert label() == 0 and n.value == count

    ins = dict(positions=Guarded(torch, 3 * V, positions), normals=Guarded(torch, 3 * V, normals), colors=Guarded(torch, V, colors), indices=idx,
               sizes=Guarded(torch, V, sizes))
    outs = dict(out_positions=Guarded(torch, 3 * V), out_normals=Guarded(torch, 3 * V), out_colors=Guarded(torch, V), out_indices=Guarded(torch, 3 * T))
    nv, nt = C.c_uint32(SENTINEL), C.c_uint32(SENTINEL)
    fbase = dict(ctx=ctx.handle, min_vertices=49, nv=C.byref(nv), nt=C.byref(nt), **{k: b.address for k, b in {**ins, **outs}.items()})

    def filt(**changes):
        a = dict(fbase, **changes)
        p = lambda v: None if v is None else C.c_void_p(v)
        return L.bslam_filter_mesh(a["ctx"], stream_ptr(torch), V, T, p(a["positions"]), p(a["normals"]), p(a["colors"]), p(a["indices"]), p(a["sizes"]),
                                   a["min_vertices"], p(a["out_positions"]), p(a["out_normals"]), p(a["out_colors"]), p(a["out_indices"]), a["nv"], a["nt"])

    a = fbase
    cases = {"null context": dict(ctx=None), "null positions": dict(positions=None), "null indices": dict(indices=None), "null sizes": dict(sizes=None),
             "null out_positions": dict(out_positions=None), "null out_indices": dict(out_indices=None), "null vertex count": dict(nv=None),
             "null triangle count": dict(nt=None), "normals without out_normals": dict(out_normals=None), "out_normals without normals": dict(normals=None),
             "colors without out_colors": dict(out_colors=None), "out_colors without colors": dict(colors=None), "min_vertices 0": dict(min_vertices=0),
             "misaligned positions": dict(positions=a["positions"] + 2), "misaligned normals": dict(normals=a["normals"] + 1),
             "misaligned colors": dict(colors=a["colors"] + 2), "misaligned indices": dict(indices=a["indices"] + 2), "misaligned sizes": dict(sizes=a["sizes"] + 3),
             "misaligned out_positions": dict(out_positions=a["out_positions"] + 2), "misaligned out_normals": dict(out_normals=a["out_normals"] + 2),
             "misaligned out_colors": dict(out_colors=a["out_colors"] + 1), "misaligned out_indices": dict(out_indices=a["out_indices"] + 2),
             "in place: positions": dict(out_positions=a["positions"]), "in place: normals": dict(out_normals=a["normals"]),
             "in place: colors": dict(out_colors=a["colors"]), "in place: indices": dict(out_indices=a["indices"]),
             "out_positions overlaps sizes": dict(out_positions=a["sizes"] + 4 * (V - 1)), "out_indices overlaps positions": dict(out_indices=a["positions"] - 12 * T + 4),
             "two outputs overlap": dict(out_normals=a["out_positions"] + 12 * V - 4), "out_colors inside out_indices": dict(out_colors=a["out_indices"] + 8)}
    for name, changes in cases.items():
        rc = filt(**changes)
        assert rc == INVALID_ARGUMENT, (name, rc, L.bslam_last_error())
    torch.cuda.synchronize()
    for b in outs.values():
        assert (b.read() == SENTINEL).all(), "a refused call wrote to an output"
    assert (nv.value, nt.value) == (SENTINEL, SENTINEL)
    assert filt() == 0 and (nv.value, nt.value) == (1336, 2664)
    # two inputs may share memory: only outputs are exclusive
    assert filt(normals=a["positions"]) == 0


# ------------------------------------------------------------------------------------------------
# 4. the chain on the device
# ------------------------------------------------------------------------------------------------
def test_extract_label_filter_on_the_device(gpu, specks):
    """The specks field in pitched volume buffers -> bslam_extract_mesh -> bslam_mesh_components -> bslam_filter_mesh at 49, no host
    copy in between: equals the chain of restatements."""
    torch, L, ctx = gpu
    positions, normals, _, triangles, labels, sizes, count = specks
    field = mu.specks_field()
    nz, ny, nx = field.shape
    vol = volume_struct((nx, ny, nz), (0.0, 0.0, 0.0), 1.0)
    t_t, t_b = pitched(torch, field.reshape(nz * ny, nx).view(np.int32), 5)
    c_t, c_b = pitched(torch, np.ones((nz * ny, nx), np.int32), 3)
    V, T = len(positions), len(triangles)
    pos, nrm, idx, lab, siz = Guarded(torch, 3 * V), Guarded(torch, 3 * V), Guarded(torch, 3 * T), Guarded(torch, V), Guarded(torch, V)
    out_pos, out_nrm, out_idx = Guarded(torch, 3 * V), Guarded(torch, 3 * V), Guarded(torch, 3 * T)
    nv, nt, n = C.c_uint32(), C.c_uint32(), C.c_uint32()
    badslam_amd.check(L.bslam_extract_mesh(ctx.handle, stream_ptr(torch), C.byref(vol), C.byref(t_b), C.byref(c_b), None, 1, V, T, pos.ptr, nrm.ptr, None, idx.ptr,
                                           C.byref(nv), C.byref(nt)))
    assert (nv.value, nt.value) == (V, T)
    badslam_amd.check(L.bslam_mesh_components(ctx.handle, stream_ptr(torch), V, T, idx.ptr, lab.ptr, siz.ptr, C.byref(n)))
    badslam_amd.check(L.bslam_filter_mesh(ctx.handle, stream_ptr(torch), V, T, pos.ptr, nrm.ptr, None, idx.ptr, siz.ptr, 49, out_pos.ptr, out_nrm.ptr, None, out_idx.ptr,
                                          C.byref(nv), C.byref(nt)))
    assert_components_equal((lab.read(), siz.read(), n.value), (labels, sizes, count))
    assert (nv.value, nt.value) == (1336, 2664)
    want_t, (want_p,) = mu.filter_mesh(sizes, 49, triangles, positions)
    assert np.array_equal(out_idx.read()[:3 * 2664].reshape(-1, 3), want_t)
    assert np.array_equal(out_pos.read()[:3 * 1336], bits(want_p).reshape(-1))
    keep = sizes >= 49
    got_n = out_nrm.read()[:3 * 1336].view(F).reshape(-1, 3)
    assert np.array_equal(bits(got_n), nrm.read().reshape(-1, 3)[keep])                               # a copy of what extraction wrote
    assert np.abs(got_n.astype(np.float64) - normals[keep]).max() <= 1e-6                             # which is the restatement's, as test_gpu_fusion has it
    for b in (out_pos, out_nrm):
        assert (b.read()[3 * 1336:] == SENTINEL).all()
    assert (out_idx.read()[3 * 2664:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------
# 5. through DirectBA
# ------------------------------------------------------------------------------------------------
PATCHES = ((2, 110, 150), (2, 60, 10), (0, 20, 30), (1, 5, 150))        # (keyframe, row, column) of 6 x 6 pixels
PATCH_IN_FRONT = 1500                                                   # raw depth units: 0.3 m at 1 / 5000
VOLUME_ORIGIN = (-1.5091177225112915, -1.153994083404541, 1.4357331991195679)
VOLUME_DIMS = (150, 118, 69)


def test_clean_up_through_direct_ba():
    """Three 160 x 120 keyframes of tests/scenes.py as test_gpu_fusion.py uses them, with four 6 x 6 patches of depth overwritten by
    a value 0.3 m in front of the surface under their centre (almost four truncations: detached), fused at 2 cm into a fixed volume
    (the box of the surfels, its near side 0.4 m closer, padded by the truncation).

    Measured beforehand on the CPU, with the restatements on these images and the oracle's pose matrices: 24 217 vertices, 47 682
    triangles, 14 components of 23 962 (98.9 %), 121, 90, 20, 15 vertices and nine single vertices in no triangle.  The patch of
    keyframe 0 and most of the others' are averaged away by the keyframes that see free space there; what stays lies at the
    image borders of keyframes 1 and 2.  At min_component_vertices = 64 the 20, the 15 and the nine go: 44 vertices."""
    from badslam_amd.direct_ba import DirectBA
    from tests import bso, scenes
    cam = bso.make_camera(131.25, 131.25, 80.0, 60.0, 160, 120)
    scene = scenes.synthetic_scene(3, width=160, height=120, cell=2, camera=cam)
    for k, y, x in PATCHES:
        depth = scene.keyframes[k].depth
        assert not (int(depth[y + 3, x + 3]) & fu.INVALID_DEPTH_BIT)
        depth[y:y + 6, x:x + 6] = int(depth[y + 3, x + 3]) - PATCH_IN_FRONT
    ba = DirectBA(scene.max_surfels, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, 0.8, 1, 1, 1, scene.color_camera, scene.depth_camera, 0, True, False)
    for kf in scene.keyframes:
        ba.AddKeyframe(kf.id, max(kf.min_depth, 1e-3), max(kf.max_depth, 1e-2), kf.depth, kf.normals, kf.radius, kf.color, kf.global_T_frame)
    for kf in scene.keyframes:
        ba.CreateSurfelsForKeyframe(False, kf.id)
    voxel, truncation, origin = 0.02, 0.08, np.array(VOLUME_ORIGIN, F)
    ba.FuseKeyframes(origin, voxel, VOLUME_DIMS, truncation)
    keyframes = []
    for k in range(3):
        depth, _, _, color, _, _ = ba.keyframe_images(k, 120, 160)
        T = ba.RenderModel(ba.keyframe_pose(k), views=("depth",))["camera_T_global"]
        keyframes.append(fu.Keyframe(depth, color, T))
    _, depth4, a = ba.intrinsics()
    camera = abi.Camera4f(*[float(v) for v in depth4], 160, 120)
    volume = fu.fuse(keyframes, camera, camera, ba.cfactor(scene.cfactor.shape), 0.0, scene.raw_to_float_depth, scene.cell, origin, voxel, VOLUME_DIMS, truncation)
    wp, wn, wc, wt = fu.extract_mesh(*volume, origin, voxel, 1)
    labels, sizes, count = mu.components(len(wp), wt)
    per_component = np.sort(sizes[labels == np.arange(len(wp))])[::-1]
    print(f"{len(wp)} vertices, {len(wt)} triangles, {count} components: {per_component.tolist()}")
    assert count >= 3 and per_component[0] >= 0.95 * len(wp)
    assert (len(wp), len(wt), count) == (24217, 47682, 14) and per_component[:5].tolist() == [23962, 121, 90, 20, 15]

    # without the option: today's call, bit for bit, by either route
    today = ba.ExtractMesh(1)
    assert np.array_equal(today["triangles"], wt) and np.array_equal(bits(today["positions"]), bits(wp)) and np.array_equal(today["colors"], wc)
    for other in (ba.ExtractMesh(1, min_component_vertices=0), ba.ExtractMesh(1, min_component_vertices=1), ba.ExtractMesh(1, min_component_vertices=1, report=True)[0]):
        for key in ("positions", "normals", "colors", "triangles"):
            assert np.array_equal(other[key].view(np.uint8), today[key].view(np.uint8)), key

    N = 64
    mesh, report = ba.ExtractMesh(1, min_component_vertices=N, report=True)
    want_t, (want_p, want_c) = mu.filter_mesh(sizes, N, wt, wp, wc)
    assert np.array_equal(mesh["triangles"], want_t) and np.array_equal(bits(mesh["positions"]), bits(want_p)) and np.array_equal(mesh["colors"], want_c)
    assert np.array_equal(bits(mesh["normals"]), bits(today["normals"][sizes >= N]))
    assert report["components"] == count and np.array_equal(report["sizes_descending"], per_component)
    assert report["removed_vertices"] == len(wp) - len(want_p) == 44 and report["removed_triangles"] == len(wt) - len(want_t)
    plain = ba.ExtractMesh(1, min_component_vertices=N)
    for key in ("positions", "normals", "colors", "triangles"):
        assert np.array_equal(plain[key].view(np.uint8), mesh[key].view(np.uint8)), key

    # the caller's own mesh: one label per remaining piece, and the unfiltered mesh's labels
    got_labels, got_sizes = ba.MeshComponents(mesh)
    assert_components_equal((got_labels, got_sizes, 3), mu.components(len(want_p), want_t))
    assert len(np.unique(got_labels)) == 3 and sorted(np.unique(got_sizes).tolist()) == [90, 121, 23962]
    got_labels, got_sizes = ba.MeshComponents(today)
    assert_components_equal((got_labels, got_sizes, count), (labels, sizes, count))
    everything, all_report = ba.ExtractMesh(1, min_component_vertices=len(wp) + 1, report=True)
    assert len(everything["positions"]) == 0 and len(everything["triangles"]) == 0 and all_report["removed_vertices"] == len(wp)
    ba.close()


# ------------------------------------------------------------------------------------------------
# 6. the tool
# ------------------------------------------------------------------------------------------------
def test_run_tum_mesh_min_component(tmp_path):
    """tools/run_tum.py --mesh --mesh-min-component on five frames of the rendered sequence of tests/test_gpu_bad_slam.py: the file
    parses and holds the restatement's filter of the mesh ExtractMesh gives in the same run.  Seen on this sequence at 4 cm and
    min_count 2: 4 473 vertices in 3 components, two of them single vertices in no triangle, which the filter removes."""
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
    seen = {}

    def inspect(slam, result):
        seen["mesh"] = slam.ba().ExtractMesh(2)

    N = 50
    mesh_path = tmp_path / "model.ply"
    r = run_tum.run(source, keyframe_interval=4, ba_iterations=2, max_depth=6.0, num_scales=4, max_surfel_count=400000, mesh=mesh_path, mesh_voxel_size=0.04,
                    mesh_min_count=2, mesh_min_component=N, inspect=inspect)
    full = seen["mesh"]
    labels, sizes, count = mu.components(len(full["positions"]), full["triangles"])
    want_t, (want_p, want_n, want_c) = mu.filter_mesh(sizes, N, full["triangles"], full["positions"], full["normals"], full["colors"])
    print(f"{len(full['positions'])} vertices in {count} components, {len(want_p)} kept at {N}")
    vertices, faces, _ = fu.read_ply(mesh_path)
    assert len(vertices) == r["mesh"]["vertices"] == len(want_p) > 1000 and len(faces) == r["mesh"]["triangles"] == len(want_t) > 1000
    assert r["mesh"]["components"] == count and r["mesh"]["removed_vertices"] == len(full["positions"]) - len(want_p)
    assert r["mesh"]["removed_triangles"] == len(full["triangles"]) - len(want_t)
    assert np.array_equal(bits(np.stack([vertices["x"], vertices["y"], vertices["z"]], 1)), bits(want_p))
    assert np.array_equal(bits(np.stack([vertices["nx"], vertices["ny"], vertices["nz"]], 1)), bits(want_n))
    assert np.array_equal(np.stack([vertices["red"], vertices["green"], vertices["blue"]], 1), want_c[:, :3])
    assert np.array_equal(faces, want_t.astype(np.int32))
    assert run_tum.arg_parser().parse_args(["x"]).mesh_min_component == 0
