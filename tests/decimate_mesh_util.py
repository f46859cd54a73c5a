"""A NumPy / Python float64 restatement of the edge-collapse rule of include/badslam_hip.h "Mesh decimation" (bslam_decimate_mesh,
badslam_amd/csrc/decimate_kernels.hpp), brute force: dictionaries and sets over the live triangles, Python floats (IEEE doubles, one
rounding per operation, nothing fused) for every decision.  No sort of pairs, no head flags, no scans, no atomics.  Also the
meshes the decimation tests share."""
import math
import struct

import numpy as np

from tests import simplify_mesh_util as su

F = np.float32
GOLDEN = 0x9E3779B1
NO_KEY = (1 << 64) - 1


class Refused(ValueError):
    """What the library answers with BSLAM_ERR_INVALID_ARGUMENT behind its launches."""


def cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def face_normal(a, b, c):
    return cross(sub(b, a), sub(c, a))


def plane_quadric(n, a):
    """The ten products of the plane (n, d = -n . a)."""
    d = -dot(n, a)
    x, y, z = n
    return [x * x, x * y, x * z, x * d, y * y, y * z, y * d, z * z, z * d, d * d]


def quadric_cost(q, p):
    xx, xy, xz, xd, yy, yz, yd, zz, zd, dd = q
    x, y, z = p
    sq = ((xx * x) * x + (yy * y) * y) + (zz * z) * z
    cr = ((xy * x) * y + (xz * x) * z) + (yz * y) * z
    li = (xd * x + yd * y) + zd * z
    return (sq + 2.0 * cr) + (2.0 * li + dd)


def f32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return float(F(x))


def float_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def decimate(positions, normals, colors, triangles, target_vertices, boundary_weight=1.0, max_cost=None, max_rounds=0, trace=None):
    """-> dict of positions (V', 3) f32, normals or None, colors (V', 4) u8 or None, triangles (T', 3) u32, vertex_map (V,) u32, rounds.
    trace (a list) receives the number of collapses of every round."""
    positions = np.ascontiguousarray(positions, F).reshape(-1, 3)
    V = len(positions)
    triangles = np.zeros((0, 3), np.uint32) if triangles is None else np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    if (triangles >= V).any():
        raise Refused("a triangle names a vertex beyond vertex_count")
    if not np.isfinite(positions).all():
        raise Refused("a vertex is not finite")
    max_cost = math.inf if max_cost is None else float(F(max_cost))
    w = float(F(boundary_weight))
    pos = [tuple(float(x) for x in p) for p in positions]                       # the fp32 values, widened
    nrm = None if normals is None else [tuple(float(x) for x in n) for n in np.ascontiguousarray(normals, F).reshape(-1, 3)]
    col = None if colors is None else [tuple(int(x) for x in c) for c in np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)]
    tris = [tuple(int(i) for i in t) for t in triangles if len({int(i) for i in t}) == 3]

    # 1 .. 3: the vertex quadrics, once
    Q = [[0.0] * 10 for _ in range(V)]
    for t in tris:                                                               # ascending triangle id
        k = plane_quadric(face_normal(pos[t[0]], pos[t[1]], pos[t[2]]), pos[t[0]])
        for v in t:
            Q[v] = [a + b for a, b in zip(Q[v], k)]
    uses = {}
    for t in tris:
        for e in range(3):
            key = (min(t[e], t[(e + 1) % 3]), max(t[e], t[(e + 1) % 3]))
            uses[key] = uses.get(key, 0) + 1
    for t in tris:                                                               # ascending triangle id, edges 0, 1, 2
        n = face_normal(pos[t[0]], pos[t[1]], pos[t[2]])
        for e in range(3):
            a, b = t[e], t[(e + 1) % 3]
            if uses[(min(a, b), max(a, b))] != 1:
                continue
            ev = sub(pos[b], pos[a])
            ee = (ev[0] * ev[0] + ev[1] * ev[1]) + ev[2] * ev[2]
            if not ee > 0.0:
                continue
            k = [(x * w) / ee for x in plane_quadric(cross(ev, n), pos[a])]
            for v in (a, b):
                Q[v] = [x + y for x, y in zip(Q[v], k)]

    parent = list(range(V))
    live = V
    rounds = 0
    while live > target_vertices and (max_rounds == 0 or rounds < max_rounds):
        rounds += 1
        count, fan, nbr = {}, {}, {}
        for t in tris:
            for e in range(3):
                a, b = t[e], t[(e + 1) % 3]
                key = (min(a, b), max(a, b))
                count[key] = count.get(key, 0) + 1
                nbr.setdefault(a, set()).add(b)
                nbr.setdefault(b, set()).add(a)
            for v in t:
                fan.setdefault(v, []).append(t)
        boundary = {v for (lo, hi), c in count.items() if c == 1 for v in (lo, hi)}
        candidates = []                                                          # (key, lo, hi, choice)
        for rank, (lo, hi) in enumerate(sorted(count)):
            c = count[(lo, hi)]
            if c > 2:
                continue
            common = nbr[lo] & nbr[hi]
            if len(common) + (1 if lo in boundary and hi in boundary else 0) != c + (1 if c == 1 else 0):
                continue
            if any(x not in boundary and len(fan[x]) == 3 for x in common):
                continue
            q = [a + b for a, b in zip(Q[lo], Q[hi])]
            mid = tuple(f32((a + b) * 0.5) for a, b in zip(pos[lo], pos[hi]))
            places = (pos[lo], pos[hi], mid)
            costs = [quadric_cost(q, p) for p in places]
            choice = 0
            if costs[1] < costs[0]:
                choice = 1
            if costs[2] < costs[choice]:
                choice = 2
            cost = costs[choice]
            if cost != cost:
                continue
            cost32 = f32(cost if cost > 0.0 else 0.0)
            if not (cost32 < math.inf and cost32 <= max_cost):
                continue
            p = places[choice]
            flips = False
            for v, other in ((lo, hi), (hi, lo)):
                for t in fan[v]:
                    if other in t:
                        continue
                    old = face_normal(pos[t[0]], pos[t[1]], pos[t[2]])
                    moved = [p if i == v else pos[i] for i in t]
                    if not dot(old, face_normal(*moved)) > 0.0:
                        flips = True
            if flips:
                continue
            candidates.append(((float_bits(cost32) << 32) | ((rank * GOLDEN) & 0xFFFFFFFF), lo, hi, choice))
        m1 = {}
        for key, lo, hi, _ in candidates:
            m1[lo] = min(m1.get(lo, NO_KEY), key)
            m1[hi] = min(m1.get(hi, NO_KEY), key)
        m2 = {v: min([m1.get(v, NO_KEY)] + [m1.get(x, NO_KEY) for x in nbr[v]]) for v in nbr}
        selected = sorted(c for c in candidates if c[0] == m2[c[1]] and c[0] == m2[c[2]])[:live - target_vertices]
        if trace is not None:
            trace.append(len(selected))
        if not selected:
            break
        for key, lo, hi, choice in selected:
            q = [a + b for a, b in zip(Q[lo], Q[hi])]
            if choice == 1:
                pos[lo] = pos[hi]
                if nrm is not None:
                    nrm[lo] = nrm[hi]
                if col is not None:
                    col[lo] = col[hi]
            elif choice == 2:
                pos[lo] = tuple(f32((a + b) * 0.5) for a, b in zip(pos[lo], pos[hi]))
                if nrm is not None:
                    s = tuple(a + b for a, b in zip(nrm[lo], nrm[hi]))
                    ss = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
                    ok = all(math.isfinite(x) for x in nrm[lo] + nrm[hi]) and ss > 0.0
                    nrm[lo] = tuple(f32(x / math.sqrt(ss)) for x in s) if ok else (0.0, 0.0, 0.0)
                if col is not None:
                    col[lo] = tuple((a + b + 1) // 2 for a, b in zip(col[lo], col[hi]))
            Q[lo] = q
            parent[hi] = lo
        live -= len(selected)
        tris = [t for t in (tuple(parent[i] for i in t) for t in tris) if len(set(t)) == 3]

    def root(v):
        while parent[v] != v:
            v = parent[v]
        return v

    roots = [root(v) for v in range(V)]
    kept = sorted(set(roots))
    new_id = {v: i for i, v in enumerate(kept)}
    out = dict(positions=np.array([pos[v] for v in kept], np.float64).reshape(-1, 3).astype(F), normals=None, colors=None,
               triangles=np.array([[new_id[i] for i in t] for t in tris], np.uint32).reshape(-1, 3),
               vertex_map=np.array([new_id[r] for r in roots], np.uint32).reshape(-1), rounds=rounds)
    if nrm is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            out["normals"] = np.array([nrm[v] for v in kept], np.float64).reshape(-1, 3).astype(F)
    if col is not None:
        out["colors"] = np.array([col[v] for v in kept], np.uint8).reshape(-1, 4)
    return out


# ------------------------------------------------------------------------------------------------
# meshes
# ------------------------------------------------------------------------------------------------
plane, uv_sphere, face_normals, edge_counts = su.plane, su.uv_sphere, su.face_normals, su.edge_counts


def bumpy_plane(n=25):
    """plane(25) with z = 0.5 + 3 exp(-r^2 / 8) around (12.25, 12.25)."""
    positions, triangles = plane(n)
    p = positions.astype(np.float64)
    r2 = (p[:, 0] - 12.25) ** 2 + (p[:, 1] - 12.25) ** 2
    p[:, 2] = 0.5 + 3.0 * np.exp(-r2 / 8.0)
    return p.astype(F), triangles


def roof_height(x):
    return 1.0 - 0.5 * np.abs(np.asarray(x, np.float64) - 10.25)


def roof(n=21):
    """plane(21) with z = 1 - 0.5 |x - 10.25|: two planes that meet in a crease along y; every value is exact in fp32."""
    positions, triangles = plane(n)
    positions[:, 2] = roof_height(positions[:, 0]).astype(F)
    return positions, triangles


def noisy_plane(n, seed=0, amplitude=0.05):
    positions, triangles = plane(n)
    positions[:, 2] += np.random.default_rng(seed).uniform(-amplitude, amplitude, n * n).astype(F)
    return positions, triangles


def fan(valence=70):
    """A closed fan of `valence` triangles around vertex 0 on a shallow cone."""
    a = 2.0 * np.pi * np.arange(valence) / valence
    rim = np.stack([np.cos(a), np.sin(a), np.full(valence, -0.25) + 0.01 * np.cos(5 * a)], axis=1)
    positions = np.concatenate([[[0.0, 0.0, 0.0]], rim]).astype(F)
    k = np.arange(valence)
    triangles = np.stack([np.zeros(valence, np.int64), 1 + k, 1 + (k + 1) % valence], axis=1).astype(np.uint32)
    return positions, triangles


def tetrahedron():
    positions = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    return positions, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.uint32)


def octahedron():
    positions = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F)
    return positions, np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.uint32)


def three_wings():
    """Three triangles on the edge (0, 1), a strip beside them, two input-degenerate triangles and two vertices in no triangle."""
    positions = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0.2], [0.5, 0, 1], [2, 0, 0], [2, 1, 0], [3, 0.5, 0.1], [7, 7, 7], [8, 8, 8]], F)
    triangles = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [2, 2, 5], [1, 5, 6], [1, 6, 2], [5, 7, 6], [6, 6, 6]], np.uint32)
    return positions, triangles


def attributes(V, seed=0):
    rng = np.random.default_rng(seed)
    n = rng.standard_normal((V, 3))
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F), rng.integers(0, 256, (V, 4), dtype=np.uint8)


def mesh_area(positions, triangles):
    return 0.5 * np.linalg.norm(face_normals(positions, triangles), axis=1).sum()
