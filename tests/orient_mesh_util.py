"""Restatement of the mesh orientation rule of include/badslam_hip.h "Mesh orientation" (bslam_orient_mesh): dictionaries and a
breadth-first walk per patch from its smallest triangle id -- no sort, no union-find.  Everything is integer but the two votes, which
are Python float (float64) expressions of one triangle each in the written order; the volume sum is a Python int.  So the device has
to reproduce every bit.  A mesh here is (positions (V, 3) f32, normals (V, 3) f32 or None, triangles (T, 3) u32)."""
import math
from collections import deque

import numpy as np

from tests import mesh_repair_util as ru

F = np.float32
MODES = ("majority", "normals", "volume")
REPORT_FIELDS = ("patches", "orientable_patches", "nonorientable_patches", "closed_patches", "seams", "disagreeing_seams_before", "disagreeing_seams_after",
                 "flipped_triangles", "inverted_patches", "fallback_patches")


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def seams_of(triangles):
    """-> (uses per slot, [(triangle a, triangle b, disagrees)] of the edges with exactly two uses, a < b as slots)."""
    corners = [int(i) for i in np.asarray(triangles).reshape(-1)]
    slots_of = {}
    for h in range(len(corners)):
        a, b = corners[h], corners[3 * (h // 3) + (h % 3 + 1) % 3]
        slots_of.setdefault((min(a, b), max(a, b)), []).append(h)
    uses = [0] * len(corners)
    seams = []
    for slots in slots_of.values():
        for h in slots:
            uses[h] = len(slots)
        if len(slots) == 2:
            seams.append((slots[0] // 3, slots[1] // 3, int(corners[slots[0]] == corners[slots[1]])))
    return uses, seams


def orient(positions, normals, triangles, mode="majority"):
    """-> dict of triangles (T, 3) u32, flipped (T,) u8, patch_of_triangle (T,) u32 and report."""
    if mode not in MODES:
        raise ValueError("mode must be 'majority', 'normals' or 'volume'")
    positions, normals, _, triangles = ru._arrays(positions, normals, None, triangles)
    if mode == "normals" and normals is None:
        raise ValueError("mode 1 (normals) needs normals")
    ru._check(positions, triangles)
    for a, b, c in triangles.tolist():
        if a == b or a == c or b == c:
            raise ValueError("a triangle repeats an index")
    T = len(triangles)
    report = dict.fromkeys(REPORT_FIELDS, 0)
    if T == 0 or len(positions) == 0:
        return dict(triangles=triangles.copy(), flipped=np.zeros(T, np.uint8), patch_of_triangle=np.zeros(T, np.uint32), report=report)
    uses, seams = seams_of(triangles)
    joined = [[] for _ in range(T)]
    for a, b, d in seams:
        joined[a].append((b, d))
        joined[b].append((a, d))
    P = positions.astype(np.float64).tolist()
    N = None if normals is None else normals.astype(np.float64).tolist()
    if mode == "volume":
        c = tuple(float(x) for x in positions.min(axis=0))
        D = max(float(hi) - float(lo) for lo, hi in zip(positions.min(axis=0), positions.max(axis=0)))
        k = 58 - 3 * math.frexp(D)[1] - T.bit_length() if D > 0.0 else None
    patch, flip0 = [-1] * T, [0] * T
    flipped = np.zeros(T, np.uint8)
    conflict = set()
    for first in range(T):
        if patch[first] != -1:
            continue
        members, queue = [], deque([first])
        patch[first] = first
        while queue:
            t = queue.popleft()
            members.append(t)
            for other, d in joined[t]:
                if patch[other] == -1:
                    patch[other], flip0[other] = first, flip0[t] ^ d
                    queue.append(other)
        orientable = all(flip0[t] ^ flip0[other] == d for t in members for other, d in joined[t])
        closed = all(uses[3 * t + k_] == 2 for t in members for k_ in range(3))
        report["patches"] += 1
        report["closed_patches"] += int(closed)
        if not orientable:
            report["nonorientable_patches"] += 1
            conflict.add(first)
            continue
        report["orientable_patches"] += 1
        ones = sum(flip0[t] for t in members)
        majority = ones > len(members) - ones
        corners = lambda t: (int(triangles[t, 0]), int(triangles[t, 1 + flip0[t]]), int(triangles[t, 2 - flip0[t]]))
        if mode == "majority":
            invert = majority
        elif mode == "normals":
            plus = minus = 0
            for t in members:
                i0, i1, i2 = corners(t)
                n = tuple((N[i0][a] + N[i1][a]) + N[i2][a] for a in range(3))
                vote = _dot(_cross(_sub(P[i1], P[i0]), _sub(P[i2], P[i0])), n)
                plus, minus = plus + int(vote > 0.0), minus + int(vote < 0.0)
            fallback = plus == minus
            invert = majority if fallback else minus > plus
            report["fallback_patches"] += int(fallback)
        else:
            total = 0
            if k is not None:
                for t in members:
                    i0, i1, i2 = corners(t)
                    total += round(math.ldexp(_dot(_sub(P[i0], c), _cross(_sub(P[i1], c), _sub(P[i2], c))), k))   # round(): to nearest, ties to even
                assert abs(total) < 2 ** 61
            fallback = not closed or total == 0
            invert = majority if fallback else total < 0
            report["fallback_patches"] += int(fallback)
        report["inverted_patches"] += int(invert)
        for t in members:
            flipped[t] = flip0[t] ^ int(invert)
    out = flip(triangles, flipped.astype(bool))
    report["seams"] = len(seams)
    report["disagreeing_seams_before"] = sum(d for _, _, d in seams)
    report["disagreeing_seams_after"] = sum(d for a, _, d in seams if patch[a] in conflict)
    report["flipped_triangles"] = int(flipped.sum())
    assert report["disagreeing_seams_after"] == sum(d for _, _, d in seams_of(out)[1])
    return dict(triangles=out, flipped=flipped, patch_of_triangle=np.array(patch, np.uint32), report=report)


# ----------------------------------------------------------------------------- inputs

def flip(triangles, mask):
    """The triangles with (a, b, c) written as (a, c, b) where mask is set."""
    out = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3).copy()
    mask = np.asarray(mask, bool)
    out[mask] = out[mask][:, [0, 2, 1]]
    return out


def seeded_mask(count, share, seed):
    """A mask over `count` triangles with round(share * count) set, chosen by `seed`."""
    mask = np.zeros(count, bool)
    mask[np.random.default_rng(seed).permutation(count)[:int(round(share * count))]] = True
    return mask


def shuffle(triangles, seed):
    """The triangles under a seeded permutation of their ids -> (triangles, order): row i of the result is row order[i] of the input."""
    triangles = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    order = np.random.default_rng(seed).permutation(len(triangles))
    return np.ascontiguousarray(triangles[order]), order


def strip(n, twist):
    """A band of n (even) triangles closed into a ring of n / 2 quads; twist=True closes it with a half turn: a Moebius band.  Bottom
    vertex i is 2 i, top vertex i is 2 i + 1; the normals point along the band's own normal at the first row of every quad."""
    m = n // 2
    assert n == 2 * m and m >= 3
    positions, normals = np.zeros((2 * m, 3)), np.zeros((2 * m, 3))
    for i in range(m):
        u = 2.0 * math.pi * i / m
        half = 0.5 * u if twist else 0.0
        centre = np.array([math.cos(u), math.sin(u), 0.0]) * 4.0
        across = math.sin(half) * np.array([math.cos(u), math.sin(u), 0.0]) + math.cos(half) * np.array([0.0, 0.0, 1.0])
        along = np.array([-math.sin(u), math.cos(u), 0.0])
        positions[2 * i], positions[2 * i + 1] = centre - 0.5 * across, centre + 0.5 * across
        normals[2 * i] = normals[2 * i + 1] = np.cross(along, across)
    bottom = lambda i: 2 * i if i < m else (1 if twist else 0)
    top = lambda i: 2 * i + 1 if i < m else (0 if twist else 1)
    triangles = [t for i in range(m) for t in ((bottom(i), bottom(i + 1), top(i)), (bottom(i + 1), top(i + 1), top(i)))]
    return positions.astype(F), normals.astype(F), np.array(triangles, np.uint32)


def book():
    """Three triangles on one spine edge: the edge joins nothing."""
    positions = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], F)
    normals = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, -1], [0, 1, 0]], F)
    return positions, normals, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.uint32)


def confetti(n_single, n_pairs, seed=0):
    """Disjoint pieces on a grid in the plane z = 0 with normals +z: n_single triangles, then n_pairs quads of two triangles, the second
    of which is flipped for a seeded half of them; a seeded half of all pieces is drawn clockwise."""
    rng = np.random.default_rng(seed)
    positions, triangles = [], []
    for piece in range(n_single + n_pairs):
        x, y, base = 3.0 * (piece % 32), 3.0 * (piece // 32), len(positions)
        positions += [[x, y, 0], [x + 1, y, 0], [x, y + 1, 0]]
        first = [base, base + 1, base + 2]
        second = None
        if piece >= n_single:
            positions.append([x + 1, y + 1, 0])
            second = [base + 1, base + 3, base + 2]
            if rng.integers(2):
                second = [second[0], second[2], second[1]]
        if rng.integers(2):
            first = [first[0], first[2], first[1]]
            second = None if second is None else [second[0], second[2], second[1]]
        triangles += [first] if second is None else [first, second]
    positions = np.array(positions, F)
    return positions, np.tile(np.array([0, 0, 1], F), (len(positions), 1)), np.array(triangles, np.uint32)


def cube():
    """mesh_repair_util.cube() with normals that point away from its centre."""
    positions, triangles = ru.cube()
    return positions, (positions - F(0.5)).astype(F), triangles


def sphere(holes=0):
    return ru.sphere(holes)


def concat(*meshes):
    """The meshes side by side: vertex ids are offset, triangle ids follow one another."""
    offset, positions, normals, triangles = 0, [], [], []
    for p, n, t in meshes:
        positions.append(np.asarray(p, F).reshape(-1, 3))
        normals.append(np.zeros((len(p), 3), F) if n is None else np.asarray(n, F).reshape(-1, 3))
        triangles.append(np.asarray(t, np.uint32).reshape(-1, 3) + np.uint32(offset))
        offset += len(p)
    return np.concatenate(positions), np.concatenate(normals), np.concatenate(triangles)
