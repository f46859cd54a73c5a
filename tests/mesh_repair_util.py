"""Brute-force restatement of the mesh repair rules of include/badslam_hip.h "Mesh repair" (bslam_clean_mesh, bslam_mesh_topology,
bslam_fill_mesh_holes): dictionaries and explicit walks, one vertex, triangle or slot at a time -- no sort, no scan, no pointer
jumping.  Everything is integer but the centroid of a hole, which is a Python float (float64) sum in the order of the walk, so the
device has to reproduce every bit.  A slot is 3 t + k: corner k of triangle t and the half-edge from corner k to corner (k + 1) % 3."""
import math

import numpy as np

from tests import fusion_util as fu

F = np.float32
NONE = 0xFFFFFFFF
REPORT_FIELDS = ("referenced_vertices", "unique_edges", "boundary_edges", "interior_edges", "nonmanifold_edges", "inconsistent_edges", "blocked_vertices", "loops",
                 "longest_loop", "loop_edges", "open_boundary_slots", "euler")


def _arrays(positions, normals, colors, triangles):
    positions = np.ascontiguousarray(positions, F).reshape(-1, 3)
    normals = None if normals is None else np.ascontiguousarray(normals, F).reshape(-1, 3)
    colors = None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 4)
    triangles = np.zeros((0, 3), np.uint32) if triangles is None else np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    return positions, normals, colors, triangles


def _check(positions, triangles):
    if len(triangles) and int(triangles.max()) >= len(positions):
        raise ValueError("a triangle names a vertex beyond vertex_count")
    if not np.isfinite(positions).all():
        raise ValueError("a vertex is not finite")


def clean(positions, normals, colors, triangles, weld=True, remove_duplicates=True, remove_unreferenced=True):
    """-> dict of positions, normals, colors, triangles, vertex_map, triangle_map and report."""
    positions, normals, colors, triangles = _arrays(positions, normals, colors, triangles)
    _check(positions, triangles)
    V, T = len(positions), len(triangles)
    rep = list(range(V))
    if weld:
        first = {}
        for v in range(V):
            # equal as floats: +0.0 stands for -0.0, every other value for its bits
            key = tuple(int(np.array(0.0 if c == 0 else c, F).view(np.uint32)) for c in positions[v])
            rep[v] = first.setdefault(key, v)
    kept_triangles, seen, degenerate, duplicate = [], set(), 0, 0
    for t in range(T):
        a, b, c = (rep[int(i)] for i in triangles[t])
        if a == b or a == c or b == c:
            degenerate += 1
            continue
        if remove_duplicates:
            key = frozenset((a, b, c))
            if key in seen:
                duplicate += 1
                continue
            seen.add(key)
        kept_triangles.append(t)
    named = set()
    for t in kept_triangles:
        named.update(rep[int(i)] for i in triangles[t])
    representatives = [v for v in range(V) if rep[v] == v]
    kept_vertices = [v for v in representatives if not remove_unreferenced or T == 0 or v in named]
    new_id = {v: n for n, v in enumerate(kept_vertices)}
    vertex_map = np.array([new_id.get(rep[v], NONE) for v in range(V)], np.uint32).reshape(V)
    triangle_map = np.full(T, NONE, np.uint32)
    triangle_map[kept_triangles] = np.arange(len(kept_triangles), dtype=np.uint32)
    out_triangles = np.array([[new_id[rep[int(i)]] for i in triangles[t]] for t in kept_triangles], np.uint32).reshape(-1, 3)
    take = lambda a: None if a is None else a[kept_vertices].copy()
    return dict(positions=take(positions), normals=take(normals), colors=take(colors), triangles=out_triangles, vertex_map=vertex_map, triangle_map=triangle_map,
                report=dict(welded_vertices=V - len(representatives), unreferenced_vertices=len(representatives) - len(kept_vertices), degenerate_triangles=degenerate,
                            duplicate_triangles=duplicate))


def _boundary(triangles):
    """Edge uses per slot, the boundary slots, and per vertex the boundary slots that start and that end there."""
    corners = [int(i) for i in triangles.reshape(-1)]
    E = len(corners)
    origin = lambda h: corners[h]
    end = lambda h: corners[3 * (h // 3) + (h % 3 + 1) % 3]
    slots_of = {}
    for h in range(E):
        slots_of.setdefault((min(origin(h), end(h)), max(origin(h), end(h))), []).append(h)
    uses = [0] * E
    for slots in slots_of.values():
        for h in slots:
            uses[h] = len(slots)
    boundary = [h for h in range(E) if uses[h] == 1]
    starts, ends = {}, {}
    for h in boundary:
        starts.setdefault(origin(h), []).append(h)
        ends.setdefault(end(h), []).append(h)
    return origin, end, slots_of, uses, boundary, starts, ends


def topology(vertex_count, triangles):
    """-> dict of the report's fields, edge_uses (T, 3), loop_of_slot (T, 3) and loop_slots: a list of the slots of every loop in walk order
    from its smallest slot, in ascending loop id."""
    triangles = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    T = len(triangles)
    if T and int(triangles.max()) >= vertex_count:
        raise ValueError("a triangle names a vertex beyond vertex_count")
    for a, b, c in triangles.tolist():
        if a == b or a == c or b == c:
            raise ValueError("a triangle repeats an index")
    origin, end, slots_of, uses, boundary, starts, ends = _boundary(triangles)
    inconsistent = sum(1 for slots in slots_of.values() if len(slots) == 2 and origin(slots[0]) == origin(slots[1]))
    passable = lambda v: len(starts.get(v, ())) == 1 and len(ends.get(v, ())) == 1
    touched = set(starts) | set(ends)
    loop_of_slot = [NONE] * (3 * T)
    loops, open_slots = [], 0
    for h in boundary:
        walk, cur, closed = [], h, False
        while len(walk) <= len(boundary):
            walk.append(cur)
            v = end(cur)
            if not passable(v):
                break
            cur = starts[v][0]
            if cur == h:
                closed = True
                break
        if not closed:
            open_slots += 1
            continue
        loop_of_slot[h] = min(walk)
        if h == min(walk):
            loops.append(walk)
    counts = [len(s) for s in slots_of.values()]
    referenced = len(set(int(i) for i in triangles.reshape(-1)))
    lengths = [len(walk) for walk in loops]
    return dict(referenced_vertices=referenced, unique_edges=len(slots_of), boundary_edges=counts.count(1), interior_edges=counts.count(2),
                nonmanifold_edges=sum(1 for c in counts if c >= 3), inconsistent_edges=inconsistent, blocked_vertices=sum(1 for v in touched if not passable(v)),
                loops=len(loops), longest_loop=max(lengths, default=0), loop_edges=sum(lengths), open_boundary_slots=open_slots,
                euler=referenced - len(slots_of) + T, edge_uses=np.array(uses, np.uint32).reshape(T, 3), loop_of_slot=np.array(loop_of_slot, np.uint32).reshape(T, 3),
                loop_slots=loops)


def fill_holes(positions, normals, colors, triangles, max_hole_edges):
    """-> dict of positions, normals, colors, triangles, filled_holes and hole_of_triangle (for the appended triangles)."""
    positions, normals, colors, triangles = _arrays(positions, normals, colors, triangles)
    _check(positions, triangles)
    if not 3 <= max_hole_edges <= 4096:
        raise ValueError("max_hole_edges must lie in [3, 4096]")
    V = len(positions)
    corners = triangles.reshape(-1)
    new_positions, new_normals, new_colors, new_triangles, hole_of_triangle = [], [], [], [], []
    for walk in topology(V, triangles)["loop_slots"]:
        n = len(walk)
        if n > max_hole_edges:
            continue
        hole, centre = len(new_positions), V + len(new_positions)
        p, g, c = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0, 0, 0, 0]
        for h in walk:
            a, b = int(corners[h]), int(corners[3 * (h // 3) + (h % 3 + 1) % 3])
            for axis in range(3):
                p[axis] = p[axis] + float(positions[a, axis])
                if normals is not None:
                    g[axis] = g[axis] + float(normals[a, axis])
            if colors is not None:
                for ch in range(4):
                    c[ch] += int(colors[a, ch])
            new_triangles.append((b, a, centre))
            hole_of_triangle.append(hole)
        new_positions.append([F(s / float(n)) for s in p])
        gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        new_normals.append([F(s / math.sqrt(gg)) for s in g] if gg > 0.0 and math.isfinite(gg) else [F(0)] * 3)
        new_colors.append([(s + n // 2) // n for s in c])
    add = lambda a, rows, dtype, width: None if a is None else np.concatenate([a, np.array(rows, dtype).reshape(-1, width)])
    return dict(positions=add(positions, new_positions, F, 3), normals=add(normals, new_normals, F, 3), colors=add(colors, new_colors, np.uint8, 4),
                triangles=add(triangles, new_triangles, np.uint32, 3), filled_holes=len(new_positions), hole_of_triangle=np.array(hole_of_triangle, np.uint32))


# ----------------------------------------------------------------------------- inputs

def soup(positions, normals, colors, triangles):
    """Every corner a vertex of its own, as an STL converter writes a mesh."""
    positions, normals, colors, triangles = _arrays(positions, normals, colors, triangles)
    flat = triangles.reshape(-1).astype(np.int64)
    take = lambda a: None if a is None else np.ascontiguousarray(a[flat])
    return take(positions), take(normals), take(colors), np.arange(len(flat), dtype=np.uint32).reshape(-1, 3)


def cube():
    """The unit cube: 8 vertices, 12 triangles, counter-clockwise seen from outside."""
    positions = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], F)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    triangles = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.uint32)
    return positions, triangles


def sphere(holes=0):
    """fusion_util.sphere_field() extracted: holes = 0 with every sample observed, 1 with holed_sphere_count, 2 with a second, smaller
    block unobserved as well -> positions, normals, triangles."""
    field = fu.sphere_field()
    count = np.ones(field.shape, np.uint32) if holes == 0 else fu.holed_sphere_count(field.shape)
    if holes == 2:
        count[16, 15, 5:8] = 0
    positions, normals, _, triangles = fu.extract_mesh(field, count, None, (0, 0, 0), 1.0, 1)
    return positions, normals, triangles


def constructed_cases():
    """Small meshes, one per thing that can go wrong -> {name: (positions, normals, colors, triangles)}; normals and colours are
    random but fixed."""
    rng = np.random.default_rng(11)
    grid = lambda n: np.array([[x, y, 0.25 * x * y] for y in range(n) for x in range(n)], F)
    square = grid(2)
    cases = {
        "bow-tie": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], F), [[0, 1, 2], [0, 3, 4]]),
        "flipped neighbour": (square, [[0, 1, 2], [1, 2, 3]]),
        "three on an edge": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], F), [[0, 1, 2], [1, 0, 3], [0, 1, 4]]),
        "rotated and flipped duplicates": (square, [[0, 1, 2], [1, 2, 0], [0, 2, 1], [1, 3, 2]]),
        "degenerate after welding": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0], [1, 1, 0]], F), [[0, 1, 3], [0, 1, 2], [3, 4, 2]]),
        "one coordinate apart": (np.array([[1, 2, 3], [1.5, 2, 3], [1, 2.5, 3], [1, 2, 3.5], [1, 2, 3], [0.0, 5, 5], [-0.0, 5, 5], [1, -0.0, 0.0], [1, 0.0, -0.0]], F),
                                 [[0, 1, 2], [4, 2, 3], [5, 6, 0], [7, 8, 1], [5, 7, 3]]),
        "named by a dropped triangle only": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [6, 6, 6]], F), [[0, 1, 2], [3, 3, 1], [0, 1, 2]]),
        "point cloud with duplicates": (np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [2, 0, 0], [1, 0, 0], [-0.0, 0, 0]], F), None),
    }
    # a 5 x 5 sheet with the middle cell missing (a hole of 4), one triangle doubled with the other orientation, and a stray vertex
    n, tri = 5, []
    for y in range(n - 1):
        for x in range(n - 1):
            if (x, y) != (2, 2):
                a = y * n + x
                tri += [[a, a + 1, a + n], [a + 1, a + n + 1, a + n]]
    cases["sheet with a hole"] = (np.concatenate([grid(n), np.array([[9, 9, 9]], F)]), tri + [[1, 0, 5]])
    out = {}
    for name, (positions, triangles) in cases.items():
        V = len(positions)
        out[name] = (positions, rng.standard_normal((V, 3)).astype(F), rng.integers(0, 256, (V, 4), dtype=np.uint8),
                     np.zeros((0, 3), np.uint32) if triangles is None else np.array(triangles, np.uint32))
    return out
