"""LoadPLY (badslam_amd/host/io.cpp, bsh_load_ply): what the project's two writers produce loads back bit for bit; ascii, double
coordinates, polygons, extra properties and elements written by the test; truncated and malformed files raise.  No GPU."""
import struct

import numpy as np
import pytest

from badslam_amd import direct_ba as dba

F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def mesh():
    rng = np.random.default_rng(9)
    V, T = 57, 91
    positions = rng.standard_normal((V, 3)).astype(F)
    positions[3] = [-0.0, 1e-42, 3.4e38]                                # a negative zero, a denormal, a huge value
    return dict(positions=positions, normals=rng.standard_normal((V, 3)).astype(F), colors=rng.integers(0, 256, (V, 4), dtype=np.uint8),
                triangles=rng.integers(0, V, (T, 3)).astype(np.uint32))


def test_the_mesh_writer_loads_back(tmp_path, mesh):
    dba.SaveMeshAsPLY(tmp_path / "mesh.ply", mesh)
    got = dba.LoadPLY(tmp_path / "mesh.ply")
    assert np.array_equal(bits(got["positions"]), bits(mesh["positions"])) and np.array_equal(bits(got["normals"]), bits(mesh["normals"]))
    assert np.array_equal(got["colors"], mesh["colors"][:, :3]) and np.array_equal(got["triangles"], mesh["triangles"])
    assert got["triangles"].dtype == np.uint32 and got["positions"].dtype == F


@pytest.mark.parametrize("attributes", ["all", "positions only", "colours only"])
def test_the_point_cloud_writer_loads_back(tmp_path, mesh, attributes):
    colors = mesh["colors"][:, :3] if attributes != "positions only" else None
    normals = mesh["normals"] if attributes == "all" else None
    dba.SavePointCloudAsPLY(tmp_path / "cloud.ply", mesh["positions"], colors, normals)
    got = dba.LoadPLY(tmp_path / "cloud.ply")
    assert np.array_equal(bits(got["positions"]), bits(mesh["positions"])) and got["triangles"].shape == (0, 3)
    assert (got["colors"] is None) == (colors is None) and (colors is None or np.array_equal(got["colors"], colors))
    assert (got["normals"] is None) == (normals is None) and (normals is None or np.array_equal(bits(got["normals"]), bits(normals)))


def test_ascii_with_a_quad_a_pentagon_and_extras(tmp_path):
    text = """ply
format ascii 1.0
comment written by the test
element vertex 5
property float x
property float y
property float z
property float quality
property list uchar int neighbours
element edge 2
property int a
property int b
element face 4
property uchar flag
property list uchar uint vertex_indices
end_header
0 0 0 0.5 2 1 2
1 0 0 0.25 0
1 1 0 1e-3 1 4
0 1 0 7 3 0 1 2
0.5 0.5 1.25 -1 0
0 1
1 2
9 3 0 1 2
8 4 0 1 2 3
7 5 0 1 2 3 4
6 2 0 1
"""
    (tmp_path / "a.ply").write_text(text)
    got = dba.LoadPLY(tmp_path / "a.ply")
    assert np.array_equal(got["positions"], np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1.25]], F))
    assert got["normals"] is None and got["colors"] is None
    assert got["triangles"].tolist() == [[0, 1, 2], [0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [0, 3, 4]]      # fans; the two-vertex face gives nothing


def binary_ply(header_lines, body):
    return ("\n".join(["ply", "format binary_little_endian 1.0"] + header_lines + ["end_header"]) + "\n").encode() + body


def test_binary_with_double_coordinates_other_index_types_and_extras(tmp_path):
    header = ["element camera 1", "property float fx", "property list ushort double samples", "element vertex 3", "property double x", "property double y",
              "property double z", "property uchar red", "property uchar green", "property uchar blue", "property short label", "element face 2",
              "property list int ushort vertex_index", "property double area"]
    body = struct.pack("<fH2d", 525.0, 2, 1.0, 2.0)
    xyz = [(0.1, 0.2, 0.3), (1e-50, -2.5, 1e300), (4.0, 5.0, 6.0)]
    for i, p in enumerate(xyz):
        body += struct.pack("<3d3Bh", *p, 10 * i, 20 * i, 30 * i, -i)
    body += struct.pack("<i3Hd", 3, 0, 1, 2, 0.5) + struct.pack("<i4Hd", 4, 2, 1, 0, 2, 0.25)
    (tmp_path / "b.ply").write_bytes(binary_ply(header, body))
    got = dba.LoadPLY(tmp_path / "b.ply")
    with np.errstate(over="ignore"):
        assert np.array_equal(bits(got["positions"]), bits(np.array(xyz, np.float64).astype(F)))               # rounded to float once; 1e300 -> inf
    assert got["colors"].tolist() == [[0, 0, 0], [10, 20, 30], [20, 40, 60]] and got["normals"] is None
    assert got["triangles"].tolist() == [[0, 1, 2], [2, 1, 0], [2, 0, 2]]


def test_truncated_and_malformed_files_raise(tmp_path, mesh):
    dba.SaveMeshAsPLY(tmp_path / "mesh.ply", mesh)
    whole = (tmp_path / "mesh.ply").read_bytes()
    start = whole.index(b"end_header\n") + len(b"end_header\n")
    V, T = len(mesh["positions"]), len(mesh["triangles"])
    assert len(whole) == start + 27 * V + 13 * T
    bad = {"cut in the faces": whole[:-1], "cut in the last vertex": whole[:start + 27 * V - 5], "cut behind the header": whole[:start],
           "cut in the header": whole[:start - 4], "empty": b"", "not a ply": b"plx\n" + whole[4:],
           "big endian": whole.replace(b"binary_little_endian", b"binary_big_endian"), "unknown type": whole.replace(b"property float x", b"property real x"),
           "no x": whole.replace(b"property float x", b"property float u"), "negative count": whole.replace(b"element face %d" % T, b"element face -1"),
           "a count the file cannot hold": whole.replace(b"element face %d" % T, b"element face 4000000000"),
           "no count": whole.replace(b"element vertex %d" % V, b"element vertex"), "a property before any element": whole.replace(b"element vertex %d\n" % V, b"", 1),
           "an index beyond the vertices": whole[:start + 27 * V + 1] + struct.pack("<i", V) + whole[start + 27 * V + 5:],
           "a negative index": whole[:start + 27 * V + 1] + struct.pack("<i", -1) + whole[start + 27 * V + 5:],
           "a list count beyond the file": whole[:start + 27 * V] + b"\xff" + whole[start + 27 * V + 1:],
           "no format": whole.replace(b"format binary_little_endian 1.0\n", b""), "an unknown header line": whole.replace(b"end_header", b"elemant x 1\nend_header")}
    for name, data in bad.items():
        (tmp_path / "bad.ply").write_bytes(data)
        with pytest.raises(dba.DirectBAError):
            dba.LoadPLY(tmp_path / "bad.ply")
            pytest.fail(f"{name}: loaded")
    ascii_bad = {"a word that is no number": "0 0 zero\n", "too few values": "0 0\n"}
    for name, row in ascii_bad.items():
        (tmp_path / "bad.ply").write_text("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n" + row)
        with pytest.raises(dba.DirectBAError):
            dba.LoadPLY(tmp_path / "bad.ply")
            pytest.fail(f"{name}: loaded")
    with pytest.raises(dba.DirectBAError):
        dba.LoadPLY(tmp_path / "there is no such file.ply")
    (tmp_path / "bad.ply").write_bytes(whole)                             # and the intact file still loads
    assert len(dba.LoadPLY(tmp_path / "bad.ply")["triangles"]) == T
