"""A Python float64 restatement of the rule of include/badslam_hip.h "Mesh smoothing" (bslam_smooth_mesh,
badslam_amd/csrc/smooth_kernels.hpp): sets and dictionaries over the live triangles, Python floats (IEEE doubles, one rounding per
operation, nothing fused) for everything that decides a bit.  No sort of pairs, no head flags, no scan.  Also the meshes the
smoothing tests share; the builders are those of simplify_mesh_util and decimate_mesh_util."""
import math

import numpy as np

from tests import decimate_mesh_util as du
from tests import simplify_mesh_util as su

F = np.float32
Refused = du.Refused
MODES = {"fixed": 0, "rim": 1, "free": 2}
plane, noisy_plane, uv_sphere, fan, tetrahedron, octahedron, three_wings = su.plane, du.noisy_plane, su.uv_sphere, du.fan, du.tetrahedron, du.octahedron, du.three_wings


def check_parameters(iterations, lambda_, mu, mode):
    """The refusals without a launch that do not concern pointers."""
    lambda_, mu = float(F(lambda_)), float(F(mu))
    if not (math.isfinite(lambda_) and 0.0 < lambda_ <= 1.0):
        raise Refused("lambda must be finite and lie in (0, 1]")
    if not (math.isfinite(mu) and -1.0 <= mu <= 0.0):
        raise Refused("mu must be finite and lie in [-1, 0]")
    if mode not in (0, 1, 2):
        raise Refused("boundary_mode must be 0 (fixed), 1 (rim) or 2 (free)")
    if not 0 <= iterations <= 65535:
        raise Refused("more than 65535 iterations")


def topology(V, triangles):
    """-> (live triangles as tuples, uses {(v, u): c(v, u)}, boundary set) of rule 1 and 2."""
    live = [tuple(int(i) for i in t) for t in triangles if len({int(i) for i in t}) == 3]
    uses = {}
    for t in live:
        for v in t:
            for u in t:
                if u != v:
                    uses[(v, u)] = uses.get((v, u), 0) + 1
    boundary = {v for (v, u), c in uses.items() if c == 1}
    return live, uses, boundary


def stencils(V, triangles, mode):
    """S(v) for every v, each an ascending list (rule 3)."""
    live, uses, boundary = topology(V, triangles)
    nbr = {}
    for (v, u) in uses:
        nbr.setdefault(v, set()).add(u)
    out = []
    for v in range(V):
        n = sorted(nbr.get(v, ()))
        if v in boundary and mode == 0:
            n = []
        elif v in boundary and mode == 1:
            n = [u for u in n if uses[(v, u)] == 1]
        out.append(n)
    return out


def vertex_normals(pos, normals, V, triangles):
    """Rule 6 over the positions `pos` (tuples of Python floats) -> (V, 3) f32."""
    live = [tuple(int(i) for i in t) for t in triangles if len({int(i) for i in t}) == 3]
    g = [(0.0, 0.0, 0.0)] * V
    has = [False] * V
    for t in live:                                                               # ascending triangle id
        n = du.face_normal(pos[t[0]], pos[t[1]], pos[t[2]])
        for v in t:
            g[v] = (g[v][0] + n[0], g[v][1] + n[1], g[v][2] + n[2])
            has[v] = True
    out = np.zeros((V, 3), F)
    for v in range(V):
        ss = (g[v][0] * g[v][0] + g[v][1] * g[v][1]) + g[v][2] * g[v][2]
        if has[v] and ss > 0.0:
            length = math.sqrt(ss)
            out[v] = [du.f32(x / length) for x in g[v]]
        elif normals is not None:
            out[v] = normals[v]
    return out


def smooth(positions, normals, triangles, iterations=10, lambda_=0.5, mu=-0.53, mode=0, want_normals=True):
    """-> (positions (V, 3) f32, normals (V, 3) f32 or None).  normals and triangles may be None; mode 0 fixed, 1 rim, 2 free."""
    check_parameters(iterations, lambda_, mu, mode)
    positions = np.ascontiguousarray(positions, F).reshape(-1, 3)
    V = len(positions)
    triangles = np.zeros((0, 3), np.uint32) if triangles is None else np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    if (triangles >= V).any():
        raise Refused("a triangle names a vertex beyond vertex_count")
    if not np.isfinite(positions).all():
        raise Refused("a vertex is not finite")
    if normals is not None:
        normals = np.ascontiguousarray(normals, F).reshape(-1, 3)
    lambda_, mu = float(F(lambda_)), float(F(mu))                                 # the fp32 parameters, widened
    S = stencils(V, triangles, mode)
    pos = [tuple(float(x) for x in p) for p in positions]                        # the fp32 values, widened
    factors = [lambda_] if mu == 0.0 else [lambda_, mu]
    for _ in range(iterations):
        for f in factors:
            new = []
            for v in range(V):
                if not S[v]:
                    new.append(pos[v])
                    continue
                moved = []
                for a in range(3):
                    s = pos[S[v][0]][a]
                    for u in S[v][1:]:
                        s = s + pos[u][a]
                    m = s / float(len(S[v]))
                    moved.append(du.f32(pos[v][a] + f * (m - pos[v][a])))
                new.append(tuple(moved))
            pos = new
    out = np.array(pos, np.float64).reshape(-1, 3).astype(F)
    return out, (vertex_normals(pos, normals, V, triangles) if want_normals else None)


# ------------------------------------------------------------------------------------------------
# meshes
# ------------------------------------------------------------------------------------------------
def noisy_sphere(segments=48, rings=24, sigma=0.02, seed=0, centre=(1.3, 1.1, 1.2)):
    """uv_sphere(48, 24) -- 1 106 vertices -- with every radius scaled by 1 + normal(0, sigma).  -> (positions, clean positions,
    outward unit normals, triangles, centre)."""
    clean, normals, triangles = uv_sphere(segments, rings, 1.0, centre)
    c = np.asarray(centre, np.float64)
    scale = 1.0 + np.random.default_rng(seed).normal(0.0, sigma, len(clean))
    noisy = (c + (clean.astype(np.float64) - c) * scale[:, None]).astype(F)
    return noisy, clean, normals, triangles, c


def radii(positions, centre):
    return np.linalg.norm(positions.astype(np.float64) - centre, axis=1)


def rim_of(n):
    """The ids of the outer vertices of plane(n)."""
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return np.flatnonzero(((i == 0) | (j == 0) | (i == n - 1) | (j == n - 1)).reshape(-1))


def zero_fan():
    """Vertex 0 sits in two triangles of opposite orientation and equal area: its fan sums to zero.  Vertex 5 has no triangle."""
    positions = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [4, 4, 4]], F)
    triangles = np.array([[0, 1, 2], [0, 4, 3]], np.uint32)
    return positions, triangles
