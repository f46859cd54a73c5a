"""The mesh orientation rule itself (include/badslam_hip.h "Mesh orientation"), on the restatement of tests/orient_mesh_util.py: what
the three modes do to meshes whose right answer is known by construction.  tests/test_gpu_orient_mesh.py holds the device to the same
restatement bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import fusion_util as fu
from tests import mesh_repair_util as ru
from tests import orient_mesh_util as ou

F = np.float32


@pytest.fixture(scope="module")
def spheres():
    return {holes: ou.sphere(holes) for holes in (0, 2)}


def check_consistent(V, triangles):
    assert ru.topology(V, triangles)["inconsistent_edges"] == 0


def test_sphere_with_a_seeded_30_percent_flipped(spheres):
    p, n, t = spheres[0]
    assert fu.signed_volume(p, t) > 0, "the extracted sphere is wound counter-clockwise seen from outside"
    mask = ou.seeded_mask(len(t), 0.3, 1)
    for mode in ou.MODES:
        got = ou.orient(p, n, ou.flip(t, mask), mode)
        assert np.array_equal(got["triangles"], t) and np.array_equal(got["flipped"].astype(bool), mask), mode
        r = got["report"]
        assert (r["patches"], r["orientable_patches"], r["closed_patches"], r["disagreeing_seams_after"], r["flipped_triangles"]) == (1, 1, 1, 0, int(mask.sum())), mode
        assert r["seams"] == 3 * len(t) // 2 and r["disagreeing_seams_before"] > 0 and r["fallback_patches"] == 0
        assert r["inverted_patches"] == (0 if mask[0] == 0 else 1)
        check_consistent(len(p), got["triangles"])


def test_majority_with_70_percent_flipped_gives_the_mirror_winding(spheres):
    p, n, t = spheres[0]
    mask = ou.seeded_mask(len(t), 0.7, 2)
    got = ou.orient(p, n, ou.flip(t, mask), "majority")
    assert np.array_equal(got["triangles"], ou.flip(t, np.ones(len(t), bool))) and got["report"]["flipped_triangles"] == int((~mask).sum())
    # the other two modes know which side is out
    for mode in ("normals", "volume"):
        assert np.array_equal(ou.orient(p, n, ou.flip(t, mask), mode)["triangles"], t), mode


def test_a_tie_keeps_the_winding_of_the_first_triangle():
    positions = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], F)
    for quad in ([[0, 1, 2], [1, 2, 3]], [[0, 2, 1], [1, 3, 2]]):
        got = ou.orient(positions, None, quad, "majority")
        assert got["triangles"][0].tolist() == quad[0] and got["flipped"].tolist() == [0, 1] and got["report"]["inverted_patches"] == 0
        check_consistent(4, got["triangles"])


def test_cube_inside_out():
    p, n, t = ou.cube()
    inside_out = ou.flip(t, np.ones(12, bool))
    volume = ou.orient(p, n, inside_out, "volume")
    assert volume["report"]["flipped_triangles"] == 12 and volume["report"]["inverted_patches"] == 1 and np.array_equal(volume["triangles"], t)
    majority = ou.orient(p, n, inside_out, "majority")
    assert majority["report"]["flipped_triangles"] == 0 and np.array_equal(majority["triangles"], inside_out)
    assert np.array_equal(ou.orient(p, n, inside_out, "normals")["triangles"], t)


def test_cube_with_five_flipped():
    p, n, t = ou.cube()
    mask = ou.seeded_mask(12, 5 / 12, 3)
    assert mask.sum() == 5
    for mode in ou.MODES:
        got = ou.orient(p, n, ou.flip(t, mask), mode)
        assert np.array_equal(got["triangles"], t) and got["report"]["flipped_triangles"] == 5 and got["report"]["closed_patches"] == 1, mode


def test_open_sphere_all_flipped(spheres):
    p, n, t = spheres[2]
    inward = ou.flip(t, np.ones(len(t), bool))
    got = ou.orient(p, n, inward, "normals")
    assert np.array_equal(got["triangles"], t) and got["report"]["inverted_patches"] == 1 and got["report"]["closed_patches"] == 0
    assert np.array_equal(ou.orient(p, -n, inward, "normals")["triangles"], inward)
    volume = ou.orient(p, n, inward, "volume")
    assert volume["report"]["fallback_patches"] == 1 and np.array_equal(volume["triangles"], inward)
    # zero normals vote for neither side: the majority decides
    zero = ou.orient(p, np.zeros_like(n), inward, "normals")
    assert zero["report"]["fallback_patches"] == 1 and np.array_equal(zero["triangles"], inward)


def test_moebius_band_comes_back_unchanged():
    p, n, t = ou.strip(16, twist=True)
    assert len(t) == 16
    for mode in ou.MODES:
        for triangles in (t, ou.flip(t, ou.seeded_mask(16, 0.5, 4))):
            got = ou.orient(p, n, triangles, mode)
            r = got["report"]
            assert np.array_equal(got["triangles"], triangles) and not got["flipped"].any() and (got["patch_of_triangle"] == 0).all()
            assert (r["patches"], r["orientable_patches"], r["nonorientable_patches"], r["flipped_triangles"]) == (1, 0, 1, 0)
            assert r["disagreeing_seams_after"] == r["disagreeing_seams_before"] > 0 and r["seams"] == 16 and r["fallback_patches"] == 0
    ring = ou.orient(*ou.strip(16, twist=False), "majority")
    assert ring["report"]["nonorientable_patches"] == 0 and ring["report"]["disagreeing_seams_before"] == 0 and not ring["flipped"].any()


def test_book_is_three_patches():
    p, n, t = ou.book()
    got = ou.orient(p, n, t, "majority")
    assert got["patch_of_triangle"].tolist() == [0, 1, 2] and got["report"]["patches"] == 3 and got["report"]["seams"] == 0 and np.array_equal(got["triangles"], t)
    assert got["report"]["closed_patches"] == 0


def parts(spheres):
    p, n, t = spheres[0]
    cp, cn, ct = ou.cube()
    mp, mn, mt = ou.strip(16, twist=True)
    return [(p, n, ou.flip(t, ou.seeded_mask(len(t), 0.3, 1))), (mp, mn, ou.flip(mt, ou.seeded_mask(16, 0.5, 4))), (cp, cn, ou.flip(ct, np.ones(12, bool))), ou.book(),
            ou.confetti(5, 4, seed=6), (spheres[2][0], spheres[2][1], ou.flip(spheres[2][2], np.ones(len(spheres[2][2]), bool)))]


@pytest.mark.parametrize("mode", ou.MODES)
def test_concat_equals_the_parts(spheres, mode):
    meshes = parts(spheres)
    whole = ou.orient(*ou.concat(*meshes), mode)
    base, vertices, total = 0, 0, dict.fromkeys(ou.REPORT_FIELDS, 0)
    for p, n, t in meshes:
        part = ou.orient(p, n, t, mode)
        rows = slice(base, base + len(t))
        assert np.array_equal(whole["patch_of_triangle"][rows], part["patch_of_triangle"] + base)
        assert np.array_equal(whole["flipped"][rows], part["flipped"])
        assert np.array_equal(whole["triangles"][rows], part["triangles"] + vertices)
        for k, v in part["report"].items():
            total[k] += v
        base, vertices = base + len(t), vertices + len(p)
    assert whole["report"] == total


@pytest.mark.parametrize("mode", ou.MODES)
def test_orienting_twice_flips_nothing(spheres, mode):
    p, n, t = ou.concat(*parts(spheres))
    once = ou.orient(p, n, t, mode)
    twice = ou.orient(p, n, once["triangles"], mode)
    assert twice["report"]["flipped_triangles"] == 0 and np.array_equal(twice["triangles"], once["triangles"])
    assert np.array_equal(twice["patch_of_triangle"], once["patch_of_triangle"])


def test_refusals_of_the_restatement():
    p, n, t = ou.cube()
    bad = t.copy()
    bad[3, 1] = 8
    with pytest.raises(ValueError, match="beyond vertex_count"):
        ou.orient(p, n, bad)
    bad = t.copy()
    bad[3, 1] = bad[3, 0]
    with pytest.raises(ValueError, match="repeats an index"):
        ou.orient(p, n, bad)
    with pytest.raises(ValueError, match="needs normals"):
        ou.orient(p, None, t, "normals")
    empty = ou.orient(p, n, np.zeros((0, 3), np.uint32), "volume")
    assert not any(empty["report"].values()) and len(empty["triangles"]) == 0


def test_the_call_is_declared_in_every_layer():
    """The C ABI, its ctypes signature, the host class, the Python method and the tool's flag."""
    import inspect
    import os

    from badslam_amd import abi
    from badslam_amd import direct_ba as dba
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "badslam_hip.h")).read()
    assert "int bslam_orient_mesh(" in header and "typedef struct bslam_orient_report" in header
    restype, argtypes = abi.SIGNATURES["bslam_orient_mesh"]
    assert restype is C.c_int and len(argtypes) == 12
    assert tuple(name for name, _ in abi.OrientReport._fields_) == ou.REPORT_FIELDS and C.sizeof(abi.OrientReport) == 40
    assert tuple(abi.ORIENT_MODES) == ou.MODES and list(abi.ORIENT_MODES.values()) == [0, 1, 2]
    assert list(inspect.signature(dba.DirectBA.OrientMesh).parameters) == ["self", "mesh", "mode", "recompute_normals", "report"]
    assert "bsh_orient_mesh" in open(os.path.join(root, "badslam_amd", "host", "c_api.cpp")).read()
    from tools import run_tum
    assert "mesh_orient" in inspect.signature(run_tum.run).parameters
