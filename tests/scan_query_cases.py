"""Cases of the scan grid's build, inside test, ray walk and closest-point backward (csrc/grid_kernels.hip: bf_grid_count / scan /
fill / pack, bf_inside_mesh, bf_intersect, bf_nearest_backward), shared by tests/test_scan_query_cases.py (CPU: every case is what it
claims to be and well posed) and tests/test_gpu_scan_queries.py (MI355X: the kernels against oracle/mesh_oracle.py on them).

A case is a scan (verts float32[NV,3], faces int32[NF,3]) plus its queries.  The number of vertices sets the grid (set_mesh's step is
the cube root of box volume / NV, MO.grid_params), so a case carries vertices no face uses to land on the grid it wants.

  grid-size cases   the prefix sum of bf_grid_scan_kernel takes cells + 1 ints in chunks of 4096: one full chunk, one element into the
                    second, into the third, a tiny grid, a one-triangle scan whose grid is one cell thick
  stretched_body    a body scan six times as long: all six ray directions of the inside test occur, walks of 5 cells
  rollover          17 triangles above one another: the inside test's 15-deep memory forgets the first and counts it twice
  ties / ties_open  a lattice cube in an n x n x n grid, n odd: a query per cell, so every tie between the six distances to the wall
                    occurs; queries on cell walls, on and off the grid's outer faces.  A closed mesh answers the same along every
                    ray, so the tie ORDER shows on the six cubes that lack one face: the ray through the hole counts nothing
  ray families      uniform, axis-parallel, one zero component, in a cell wall's plane, off the grid and missing it, from 30 m at a
                    triangle with direction norms 1e-3 / 1 / 1e3, from the grid's outer faces, zero directions
  backward cases    one lattice triangle with eight queries in each of its seven Voronoi regions, a segment, a point, bad face ids

A ray is kept only if MO.ray_grazing (float64, the mesh and the grid alone - nothing a device returns) says the float32 walk cannot
differ from the brute force on it: candidates are drawn from a seeded stream and the grazing ones passed over, which is choosing the
seed ray by ray.  Nothing here touches a GPU.
"""
import functools

import numpy as np

from bodyfitting_amd import synthetic as S
from oracle import mesh_oracle as MO

SCAN_CHUNK = 4096                     # ints per pass of bf_grid_scan_kernel
MEMORY = 15                           # hits bf_inside_mesh_kernel remembers (the reference's visited[16])
BODY_FRAME = 3                        # S.make_scan_problem frame of the body cases (test_inside_mesh_matches_the_restated_rule's)
STRETCH = (6.0, 1.0, 1.1)
DIRECTIONS = ("-x", "+x", "-y", "+y", "-z", "+z")     # the order in which the inside test breaks ties

# name -> (box far corner, vertices, grid, cells + 1)
GRID_CASES = {
    "one_chunk": ((14.5, 12.5, 20.5), 3716, (15, 13, 21), 4096),
    "chunk_plus_one": ((15.5, 15.5, 15.5), 3724, (16, 16, 16), 4097),
    "third_chunk": ((31.5, 15.5, 15.5), 7568, (32, 16, 16), 8193),
    "tiny": ((3.5, 2.5, 1.5), 13, (4, 3, 2), 25),
}
ONE_TRIANGLE = "one_triangle"         # 3 vertices: a 3 x 2 x 1 grid
ONE_TRIANGLE_GRID = (3, 2, 1)
N_SMALL = 300                         # random small triangles of a chunk case


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def grid_of(verts):
    """(step float, dims int64[3], origin float32[3]) of the scan's grid, as set_mesh computes them"""
    return MO.grid_params(np.array(verts, np.float32))          # (a copy: torch will not wrap a read-only array quietly)


def cell_lists(verts, faces):
    step, dims, origin = grid_of(verts)
    return MO.insert_grid_surface(verts, faces, step, origin, dims)


@functools.lru_cache(maxsize=None)
def model690():
    return S.make_model("smpl", seed=0, nv=690)


# ----------------------------------------------------------------------------------------------------------------------------
# grid sizes
# ----------------------------------------------------------------------------------------------------------------------------

def _pad_to(verts, nv, ext, rng):
    """`verts` plus unreferenced random vertices inside the box, nv rows in all"""
    n = nv - len(verts)
    assert n >= 0, (nv, len(verts))
    return np.concatenate([verts, rng.uniform(0.0, 1.0, (n, 3)) * np.asarray(ext)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def grid_case(name):
    """-> (verts, faces, queries): triangles over many cells, triangles with a corner on a corner of the box (the highest cell
    coordinate a vertex can have: grid_box's clamp), one small triangle inside each cell around every chunk edge of the prefix sum
    and N_SMALL random small ones (as many as the vertex count allows on the tiny grid), then padding."""
    if name == ONE_TRIANGLE:
        v = np.array([[0, 0, 0], [2.2, 0.3, 0.2], [0.5, 1.7, 0.9]], np.float32)
        f = np.array([[0, 1, 2]], np.int32)
        rng = np.random.default_rng(77)
        q = rng.uniform(v.min(0) - 0.2, v.max(0) + 0.2, (40, 3)).astype(np.float32)
        return _freeze(v, f, q)
    ext, nv, dims, _ = GRID_CASES[name]
    ext = np.asarray(ext, np.float64)
    rng = np.random.default_rng(1000 + nv)
    q = rng.uniform(-0.3, ext + 0.3, (40, 3)).astype(np.float32)
    if nv < 100:
        # 13 vertices cannot carry 300 triangles of their own: the box's eight corners and five points inside it, the triangles by
        # index - across the grid, at every corner, and 40 random triples
        v = np.concatenate([np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)]) * ext,
                            rng.uniform(0.1, 0.9, (nv - 8, 3)) * ext]).astype(np.float32)
        f = [[0, 7, 8], [1, 6, 9], [2, 5, 10], [3, 4, 11], [8, 9, 10], [10, 11, 12], [0, 8, 12], [7, 9, 11]]
        f += [sorted(rng.choice(nv, 3, replace=False).tolist()) for _ in range(40)]
        assert tuple(grid_of(v)[1]) == dims
        return _freeze(v, np.asarray(f, np.int32), q)
    box = np.array([[0, 0, 0], ext], np.float64)
    step, num, origin = grid_of(_pad_to(box, nv, ext, np.random.default_rng(0)))   # box and count decide the grid, nothing else
    assert tuple(num) == dims
    verts, faces = [box[0], box[1]], []

    def add(tri, first=None):
        i = len(verts)
        ids = ([first] if first is not None else []) + list(range(i, i + len(tri)))
        verts.extend(tri)
        faces.append(ids)

    # over many cells: the whole grid, a slab, a sliver along the long diagonal
    add([[ext[0], 0.2, 0.1], [0.3, ext[1], ext[2]]], first=0)
    add([[0.0, ext[1], 0.0], [ext[0], 0.0, ext[2]]], first=1)
    add([[0.1, 0.1, 0.1], [ext[0] - 0.1, 0.2, 0.3], [0.2, ext[1] - 0.1, 0.4]])
    add([[0.2, 0.3, 0.2], [0.3, 0.2, 0.2]], first=1)
    # a corner on each of the other six corners of the box
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                if cx == cy == cz:
                    continue
                c = np.array([cx, cy, cz]) * ext
                inward = np.where(np.array([cx, cy, cz]) == 1, -1.0, 1.0)
                add([c, c + inward * [1.3, 0.2, 0.4], c + inward * [0.3, 1.1, 0.6]])
    # one triangle inside each cell around every chunk edge: element e of the scanned array is cell e - 1
    cells = sorted({e - 1 + k for e in range(SCAN_CHUNK, int(np.prod(dims)) + 1, SCAN_CHUNK) for k in (-2, -1, 0, 1, 2)
                    if 0 <= e - 1 + k < int(np.prod(dims))})
    for c in cells:
        ijk = np.array([c // (dims[1] * dims[2]), (c // dims[2]) % dims[1], c % dims[2]], np.float64)
        mid = np.clip(origin.astype(np.float64) + step * (ijk + 0.5), 0.05, ext - 0.15)
        add([mid + [0.1, 0, 0], mid + [0, 0.1, 0], mid + [0, 0, 0.1]])
    for _ in range(N_SMALL):
        mid = rng.uniform(0.0, 1.0, 3) * ext
        add(np.clip(mid + rng.normal(0.0, 0.45, (3, 3)), 0.0, ext))
    v = _pad_to(np.asarray(verts, np.float64), nv, ext, rng)
    return _freeze(v, np.asarray(faces, np.int32), q)


GRID_CASE_NAMES = tuple(GRID_CASES) + (ONE_TRIANGLE,)


# ----------------------------------------------------------------------------------------------------------------------------
# body scans
# ----------------------------------------------------------------------------------------------------------------------------

BODIES = ("body", "stretched_body", "stretched_body_big")


@functools.lru_cache(maxsize=None)
def body(name):
    """-> (verts, faces, queries) of "body" (the 690-vertex scan of frame BODY_FRAME), "stretched_body" (times STRETCH: a 9 x 9 x 10
    grid) and "stretched_body_big" (subdivided twice first).  300 near-surface plus 200 uniform queries; 200 in all on the big one,
    whose oracle is a Python loop over ~50 triangles per cell."""
    _, sv, sf = S.make_scan_problem(model690(), BODY_FRAME)
    if name == "stretched_body_big":
        sv, sf = S.subdivide_mesh(sv, sf, 2)
        sv = sv.astype(np.float32)
    if name != "body":
        sv = (sv * np.asarray(STRETCH, np.float32)).astype(np.float32)
    rng = np.random.default_rng(21)
    near, uni = (120, 80) if name == "stretched_body_big" else (300, 200)
    sigma = 0.03 * (np.asarray(STRETCH) if name != "body" else np.ones(3))
    q = np.concatenate([sv[rng.integers(0, len(sv), near)] + rng.normal(0, 1.0, (near, 3)) * sigma,
                        rng.uniform(sv.min(0) - 0.1, sv.max(0) + 0.1, (uni, 3))]).astype(np.float32)
    return _freeze(sv, np.asarray(sf, np.int32), q)


# ----------------------------------------------------------------------------------------------------------------------------
# the 15-deep memory rolling over
# ----------------------------------------------------------------------------------------------------------------------------

ROLLOVER_MIRRORS = tuple(DIRECTIONS)          # the direction of the designed ray
ROLLOVER_BOX = (6.5, 6.5, 3.5)                # 148 vertices: a 7 x 7 x 4 grid
ROLLOVER_DESIGNED = np.array([-1.0, 1.0, -1.0, 1.0, 1.0], np.float32)
ROLLOVER_UNLIMITED = np.array([1.0, 1.0, -1.0, -1.0, 1.0], np.float32)      # the same queries with a memory that never forgets
ROLLOVER_16_DEEP = np.array([-1.0, 1.0, -1.0, -1.0, 1.0], np.float32)       # ... and with one slot more than the rule has


@functools.lru_cache(maxsize=None)
def rollover(mirror="-z"):
    """-> (verts, faces, queries, designed): the construction for the -z ray, turned so that its ray runs along `mirror`.
    Triangle 0 lies in z-cells 0 and 1; triangles 1..16 sit above one another in z-cell 1 over its middle.  Query 0 looks down from
    above all 17: cell 1 lists triangle 0 first, 16 more hits push it out of the 15 remembered, cell 0 lists it again - 18 counted,
    -1, where the 17 distinct triangles would give +1.  Queries 1 and 2 (below the stack; in it) count 1 and 8: +1 and -1.  Query 3
    sits under the topmost triangle: triangle 0 and 15 more, exactly one hit more than the memory holds, so triangle 0 is counted
    again (17, +1) where a 16-deep memory would keep it (16, -1); query 4, one triangle lower, stays within the memory (15, +1).
    The queries after these five are random ones on which a 15-deep and an unlimited memory agree."""
    tris = [[(1, 1, .2), (6, 2, .9), (2, 6, .5)]] + [[(2.9, 3.0, z), (3.6, 3.1, z), (3.1, 3.8, z)] for z in 0.8 + 0.05 * np.arange(1, 17)]
    v = np.asarray(tris, np.float64).reshape(-1, 3)
    rng = np.random.default_rng(148)
    box = np.asarray(ROLLOVER_BOX)
    v = np.concatenate([v, [[0, 0, 0], box], rng.uniform(0, 1, (148 - 53, 3)) * box])
    q = np.concatenate([[[3.2, 3.3, 1.7], [3.2, 3.3, 0.7], [3.2, 3.3, 1.2], [3.2, 3.3, 1.575], [3.2, 3.3, 1.525]], rng.uniform(-0.2, 1.0, (40, 3)) * (box + 0.2)])
    axis, plus = "xyz".index(mirror[1]), mirror[0] == "+"
    if plus:                                                    # reflect in the box's middle plane: the ray turns round
        v[:, 2], q[:, 2] = box[2] - v[:, 2], box[2] - q[:, 2]
    perm = {0: [2, 0, 1], 1: [1, 2, 0], 2: [0, 1, 2]}[axis]     # new coordinate `axis` is the old z
    v, q = v[:, perm], q[:, perm]
    f = np.arange(51, dtype=np.int32).reshape(17, 3)
    return _freeze(v.astype(np.float32), f, q.astype(np.float32), ROLLOVER_DESIGNED)


# ----------------------------------------------------------------------------------------------------------------------------
# ties between the six directions, cell walls, the grid's outer faces
# ----------------------------------------------------------------------------------------------------------------------------

TIES_N = 5
TIES_BOX = (4.5, 4.5, 4.5)                    # 91 vertices: a 5 x 5 x 5 grid
TIES_NV = 91
CUBE_LO, CUBE_HI = 1.0, 4.0                   # the lattice cube: cells 1..3 have their middle inside it, cells 0 and 4 outside
_OFFSET = np.array([0.13, 0.07, -0.11])       # off the cell's middle: off the cube's face diagonals, where the crossing rule is degenerate


def _cube(without=None):
    """the cube's 8 corners and 12 outward triangles, two per face in DIRECTIONS order; `without` leaves one face out"""
    c = np.array([[x, y, z] for x in (CUBE_LO, CUBE_HI) for y in (CUBE_LO, CUBE_HI) for z in (CUBE_LO, CUBE_HI)], np.float64)
    quads = {"-x": (0, 1, 3, 2), "+x": (4, 6, 7, 5), "-y": (0, 4, 5, 1), "+y": (2, 3, 7, 6), "-z": (0, 2, 6, 4), "+z": (1, 5, 7, 3)}
    f = [t for d in DIRECTIONS if d != without for t in ((quads[d][0], quads[d][1], quads[d][2]), (quads[d][0], quads[d][2], quads[d][3]))]
    return c, np.asarray(f, np.int32)


def first_minimum(to_end):
    """the direction the inside test takes: the FIRST smallest of the six distances (its scan keeps a direction unless another is
    strictly nearer)"""
    return int(np.argmin(np.asarray(to_end)))


@functools.lru_cache(maxsize=None)
def ties(without=None):
    """-> (verts, faces, queries, designed float32[Q] with 0 where nothing is designed, kinds str[Q]).
    kinds: "cell" one query per cell of the grid (every tie pattern); "wall" on an interior cell wall, "face0" on the grid's low outer
    face (in the grid: cell 0), "faceN-" the last float32 before the high outer face and "faceN" the first one on it (off the grid),
    "off" just off the grid.  designed: a "cell" query inside the cube answers +1 - unless its ray leaves through the missing face
    `without` - and one outside -1; everything off the grid -1."""
    corners, f = _cube(without)
    rng = np.random.default_rng(91)
    box = np.asarray(TIES_BOX)
    v = np.concatenate([corners, [[0, 0, 0], box], rng.uniform(0, 1, (TIES_NV - 10, 3)) * box]).astype(np.float32)
    step, num, origin = grid_of(v)
    assert tuple(num) == (TIES_N,) * 3
    st, org = np.float32(step), origin.astype(np.float32)
    q, designed, kinds = [], [], []
    for i in range(TIES_N):
        for j in range(TIES_N):
            for k in range(TIES_N):
                cell = np.array([i, j, k])
                q.append(org.astype(np.float64) + float(st) * (cell + 0.5) + _OFFSET)
                inside = bool(np.all((cell >= 1) & (cell <= 3)))
                to_end = [i, TIES_N - 1 - i, j, TIES_N - 1 - j, k, TIES_N - 1 - k]
                designed.append(1.0 if inside and DIRECTIONS[first_minimum(to_end)] != without else -1.0)
                kinds.append("cell")

    def xf(x, d):
        return (np.float32(x) - org[d]) / st

    others = [org.astype(np.float64) + float(st) * (np.array(c) + 0.5) + _OFFSET for c in ((2, 2, 2), (1, 3, 2), (0, 2, 4), (3, 1, 1))]
    for d in range(3):
        for base in others:
            for w in range(1, TIES_N):                          # interior walls
                p = base.copy(); p[d] = np.float32(org[d] + st * np.float32(w)); q.append(p); designed.append(0.0); kinds.append("wall")
            p = base.copy(); p[d] = org[d]; q.append(p); designed.append(0.0); kinds.append("face0")
            hi = np.float32(org[d] + st * np.float32(TIES_N))
            while xf(hi, d) >= TIES_N:
                hi = np.nextafter(hi, np.float32(-np.inf))
            while xf(np.nextafter(hi, np.float32(np.inf)), d) < TIES_N:
                hi = np.nextafter(hi, np.float32(np.inf))
            p = base.copy(); p[d] = hi; q.append(p); designed.append(0.0); kinds.append("faceN-")
            p = base.copy(); p[d] = np.nextafter(hi, np.float32(np.inf)); q.append(p); designed.append(-1.0); kinds.append("faceN")
            for off in (np.nextafter(org[d], np.float32(-np.inf)), org[d] - np.float32(0.3), hi + np.float32(0.3)):
                p = base.copy(); p[d] = off; q.append(p); designed.append(-1.0); kinds.append("off")
    return _freeze(v, f, np.asarray(q, np.float32), np.asarray(designed, np.float32), np.asarray(kinds))


# ----------------------------------------------------------------------------------------------------------------------------
# rays
# ----------------------------------------------------------------------------------------------------------------------------

RAY_FAMILIES = ("uniform", "axis", "one_zero", "wall_plane", "outside_miss", "far", "outer_face", "zero")
MISS_BY_CONSTRUCTION = ("outside_miss", "zero")
FAR = 30.0
FAR_NORMS = (1e-3, 1.0, 1e3)
N_RAYS = 96                                   # per family (a multiple of 6: axis x sign, norms x aim)


def _candidates(family, verts, faces, rng, n):
    """n candidate rays -> (origins, directions, in-plane axis per ray or -1)"""
    step, num, origin = grid_of(verts)
    st, org = np.float32(step), origin.astype(np.float32)
    lo, hi = verts.min(0).astype(np.float64), verts.max(0).astype(np.float64)
    glo, ghi = org.astype(np.float64), org.astype(np.float64) + float(st) * num
    plane = np.full(n, -1)
    inside = np.concatenate([rng.uniform(lo - 0.05, hi + 0.05, (n - n // 2, 3)),
                             verts[rng.integers(0, len(verts), n // 2)] + rng.normal(0, 0.05, (n // 2, 3))])
    toward = verts[rng.integers(0, len(verts), n)] + rng.normal(0, 0.1, (n, 3))
    if family == "uniform":
        o, d = rng.uniform(lo - 0.3, hi + 0.3, (n, 3)), rng.normal(size=(n, 3))
        d[::2] = toward[::2] - o[::2]                            # every other one towards the body: a thin shape in its box
    elif family == "axis":
        o, d = inside, np.zeros((n, 3))
        d[np.arange(n), np.arange(n) % 3] = np.where((np.arange(n) // 3) % 2 == 0, 1.0, -1.0) * rng.uniform(0.2, 5.0, n)
    elif family == "one_zero":
        o, d = inside, rng.normal(size=(n, 3))
        d[np.arange(n), np.arange(n) % 3] = 0.0
    elif family == "wall_plane":
        o, d = inside, rng.normal(size=(n, 3))
        plane = np.arange(n) % 3
        wall = np.clip(np.floor((o[np.arange(n), plane] - glo[plane]) / float(st)) + rng.integers(0, 2, n), 1, num[plane] - 1)
        o[np.arange(n), plane] = (org[plane] + st * wall.astype(np.float32)).astype(np.float32)
        d[np.arange(n), plane] = 0.0
    elif family == "outside_miss":                              # beyond one face of the grid, going away from it or along it
        o, d = rng.uniform(glo, ghi, (n, 3)), rng.normal(size=(n, 3))
        k, far_side = np.arange(n) % 3, (np.arange(n) // 3) % 2 == 1
        o[np.arange(n), k] = np.where(far_side, ghi[k] + rng.uniform(0.01, 2.0, n), glo[k] - rng.uniform(0.01, 2.0, n))
        away = np.where(far_side, 1.0, -1.0) * np.abs(d[np.arange(n), k])
        d[np.arange(n), k] = np.where((np.arange(n) // 6) % 2 == 0, away, 0.0)
    elif family == "far":                                       # from 30 m: two in three at a triangle's centroid, the others past the body
        aim = verts[faces[rng.integers(0, len(faces), n)]].astype(np.float64).mean(1)
        loose = np.arange(n) % 3 == 2
        aim[loose] = rng.uniform(glo, ghi, (n, 3))[loose]
        u = rng.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        o = aim + FAR * u
        d = -u * np.asarray(FAR_NORMS)[(np.arange(n) // 3) % 3][:, None]
    elif family == "outer_face":
        o, d = rng.uniform(glo, ghi, (n, 3)), rng.normal(size=(n, 3))
        k, far_side = np.arange(n) % 3, (np.arange(n) // 3) % 2 == 1
        o = o.astype(np.float32)
        o[np.arange(n), k] = np.where(far_side, (org[k] + st * num[k].astype(np.float32)).astype(np.float32), org[k])
        d[::2] = toward[::2] - o[::2]
    elif family == "zero":
        o, d = inside, np.zeros((n, 3))
        d[n // 2:] = rng.uniform(-1.5e-5, 1.5e-5, (n - n // 2, 3))          # squared norm below the rule's 1e-9
    else:
        raise KeyError(family)
    return np.asarray(o, np.float32), np.asarray(d, np.float32), plane


def grazing(verts, faces, o, d, plane=None):
    """MO.ray_grazing on the scan's own grid; rays in a cell wall's plane (plane[r] = its axis) by that function's in-plane rule"""
    step, num, origin = grid_of(verts)
    out = np.zeros(len(o), bool)
    plane = np.full(len(o), -1) if plane is None else np.asarray(plane)
    for k in (-1, 0, 1, 2):
        m = plane == k
        if m.any():
            out[m] = MO.ray_grazing(verts, faces, o[m], d[m], step, origin, num, in_plane_axis=None if k < 0 else k)
    return out


@functools.lru_cache(maxsize=None)
def rays(scan, family, n=N_RAYS):
    """-> (origins float32[n,3], directions float32[n,3], in-plane axis int[n]) of one family on body(scan): the first n candidates of
    the family's seeded stream that are not grazing."""
    verts, faces, _ = body(scan)
    rng = np.random.default_rng(500 + 17 * RAY_FAMILIES.index(family) + BODIES.index(scan))
    keep_o, keep_d, keep_p, have = [], [], [], 0
    for _ in range(8):
        o, d, p = _candidates(family, verts, faces, rng, n)
        ok = ~grazing(verts, faces, o, d, p)
        keep_o.append(o[ok]); keep_d.append(d[ok]); keep_p.append(p[ok])
        have += int(ok.sum())
        if have >= n:
            break
    assert have >= n, (scan, family, have)
    return _freeze(np.concatenate(keep_o)[:n], np.concatenate(keep_d)[:n], np.concatenate(keep_p)[:n])


# ----------------------------------------------------------------------------------------------------------------------------
# the closest point's backward
# ----------------------------------------------------------------------------------------------------------------------------

REGIONS = ("face", "edge0", "edge1", "edge2", "corner0", "corner1", "corner2")      # edge i is opposite corner i
BACKWARD_FACES = {"lattice": 0, "segment": 1, "point": 2}


@functools.lru_cache(maxsize=None)
def backward_case():
    """-> dict: verts, faces (a lattice triangle, a segment, a point; padding gives the scan a volume), and per query the face id,
    the coefficients MO.closest_rule returns for it (float64 rule on the lattice: clamped ones exact zeros), the incoming gradient
    and `group`: one of REGIONS for the 7 x 8 queries on the lattice triangle, "segment" / "point" (the rule's own coefficients:
    one zero), "segment_flat" / "point_flat" (three non-zero coefficients on a triangle without area: the kernel's nn > 0 guard)."""
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0],
                  [0, 10, 0], [2, 10, 0], [4, 10, 0],
                  [8, 8, 3], [8, 8, 3], [8, 8, 3],
                  [-6, -6, -5], [12, 14, 9]], np.float32)
    f = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.int32)
    rng = np.random.default_rng(56)
    # eight queries per Voronoi region of triangle 0, in its plane's coordinates (u, v) plus a height: corner regions lie behind both
    # edges at the corner, edge regions beside the edge's interior
    plane = {"face": lambda r: (0.4 + 2.8 * r[0] * (1 - r[1]), 0.4 + 2.8 * r[1] * (1 - r[0]) * 0.9),
             "edge0": lambda r: (2 + 2 * (r[0] - 0.5) + 1 + r[1], 2 - 2 * (r[0] - 0.5) + 1 + r[1]),
             "edge1": lambda r: (-0.5 - 2 * r[1], 0.5 + 3 * r[0]),
             "edge2": lambda r: (0.5 + 3 * r[0], -0.5 - 2 * r[1]),
             "corner0": lambda r: (-0.3 - 2 * r[0], -0.3 - 2 * r[1]),
             "corner1": lambda r: (4.5 + 2 * r[0] + 2 * r[1], -0.3 - 2 * r[1]),
             "corner2": lambda r: (-0.3 - 2 * r[0], 4.5 + 2 * r[0] + 2 * r[1])}
    q, ids, group = [], [], []
    for name in REGIONS:
        for _ in range(8):
            r = rng.uniform(0.05, 0.95, 2)
            x, y = plane[name](r)
            q.append([x, y, rng.uniform(-2, 2)]); ids.append(0); group.append(name)
    for name, fid in (("segment", 1), ("point", 2)):
        for _ in range(8):
            q.append(v[f[fid]].mean(0) + rng.normal(0, 1, 3)); ids.append(fid); group.append(name)
    q, ids, group = np.asarray(q, np.float32), np.asarray(ids, np.int32), np.asarray(group)
    rel = v[f[ids]].astype(np.float64) - q.astype(np.float64)[:, None]
    bary = MO.closest_rule(rel[:, 0], rel[:, 1], rel[:, 2])[0].astype(np.float32)
    flat = np.isin(group, ("segment", "point"))
    q = np.concatenate([q, q[flat]]); ids = np.concatenate([ids, ids[flat]])
    group = np.concatenate([group, np.char.add(group[flat], "_flat")])
    bary = np.concatenate([bary, np.tile(np.array([[0.25, 0.5, 0.25]], np.float32), (int(flat.sum()), 1))])
    g = rng.normal(size=q.shape).astype(np.float32)
    out = {"verts": v, "faces": f, "queries": q, "ids": ids, "bary": bary, "dnearest": g, "group": group}
    _freeze(*out.values())
    return out
