"""CPU: the cases of tests/scan_query_cases.py are what they claim to be, with the oracle alone - the grids and the chunk edges of the
prefix sum, the six directions and the long walks of the inside test, the inside answers against a float64 winding number, the memory
that rolls over, the designed tie answers, and that no ray is one on which a float32 walk may differ from the brute force.  With this
the GPU file (tests/test_gpu_scan_queries.py) compares exactly, with no filter and no slack.  Run with -s for the figures."""
import numpy as np
import pytest

import scan_query_cases as Q
from oracle import mesh_oracle as MO


def _oracle_inside(verts, faces, q, memory=Q.MEMORY):
    step, dims, origin = Q.grid_of(verts)
    tri_num, tri_idx = Q.cell_lists(verts, faces)
    return MO.inside_mesh(verts, faces, q, step, origin, dims, tri_num, tri_idx, memory=memory)


@pytest.mark.parametrize("name", Q.GRID_CASE_NAMES)
def test_grid_size_cases_land_on_their_grids(name):
    """cells + 1 - what bf_grid_scan_kernel scans - is 4096, 4097, 8193, 25 and 7, and the cells on both sides of every chunk edge
    hold triangles, so a lost or doubled carry changes a start that is in use"""
    v, f, _ = Q.grid_case(name)
    _, dims, _ = Q.grid_of(v)
    if name == Q.ONE_TRIANGLE:
        assert tuple(dims) == Q.ONE_TRIANGLE_GRID and len(v) == 3 and len(f) == 1 and dims.min() == 1
        return
    ext, nv, grid, n_scan = Q.GRID_CASES[name]
    assert len(v) == nv and tuple(dims) == grid and int(dims.prod()) + 1 == n_scan
    np.testing.assert_array_equal(v.min(0), 0)
    np.testing.assert_array_equal(v.max(0), np.asarray(ext, np.float32))
    assert {tuple(c) for c in v[f].reshape(-1, 3)} >= {(x, y, z) for x in (0, ext[0]) for y in (0, ext[1]) for z in (0, ext[2])}
    tri_num, tri_idx = Q.cell_lists(v, f)
    count = np.diff(np.concatenate([[0], tri_num]))                      # count[c] is element c + 1 of the scanned array
    span = (v[f].max(1) - v[f].min(1)).max(1)
    print(name, "grid", dims, "scan length", n_scan, "entries", len(tri_idx), "longest list", count.max(), "cells in use", (count > 0).mean())
    assert (span > 0.9 * max(ext)).sum() >= 2                            # triangles over many cells
    if nv < 100:
        return
    assert len(f) >= Q.N_SMALL + 10 and (span < 3.0).sum() >= Q.N_SMALL
    for edge in range(Q.SCAN_CHUNK, n_scan + 1, Q.SCAN_CHUNK):           # elements edge - 1 | edge lie in different chunks
        elements = [e for e in (edge - 2, edge - 1, edge, edge + 1) if 1 <= e < n_scan]
        assert all(count[e - 1] > 0 for e in elements), (edge, count[edge - 4:edge + 2])
        assert len({int(count[e - 1]) for e in range(edge - 8, min(edge + 8, n_scan))}) > 1          # and not all the same
    assert n_scan % Q.SCAN_CHUNK == {"one_chunk": 0, "chunk_plus_one": 1, "third_chunk": 1}[name]


def test_stretched_body_takes_every_direction_and_long_walks():
    v, f, q = Q.body("stretched_body")
    step, dims, origin = Q.grid_of(v)
    direction, cells, _ = MO.inside_walks(q, step, origin, dims)
    per_direction = np.bincount(direction[direction >= 0], minlength=6)
    print("stretched_body grid", dims, "queries per direction", per_direction, "longest walk", cells.max())
    assert tuple(dims) == (9, 9, 10) and per_direction.min() >= 20 and cells.max() >= 4
    v, f, q = Q.body("stretched_body_big")
    step, dims, origin = Q.grid_of(v)
    direction, cells, _ = MO.inside_walks(q, step, origin, dims)
    print("stretched_body_big grid", dims, "queries per direction", np.bincount(direction[direction >= 0], minlength=6), "longest walk", cells.max())
    assert len(q) <= 200 and len(f) > 20000 and np.bincount(direction[direction >= 0], minlength=6).min() >= 10 and cells.max() >= 8


@pytest.mark.parametrize("case", ["stretched_body", "ties"])
def test_the_inside_rule_is_the_truth_on_closed_meshes(case):
    """the rule's answer = the sign of the float64 winding number, on EVERY query on the grid"""
    v, f, q = Q.body(case) if case != "ties" else Q.ties()[:3]
    step, dims, origin = Q.grid_of(v)
    on_grid = MO.inside_walks(q, step, origin, dims)[0] >= 0
    rule = _oracle_inside(v, f, q)
    w = MO.winding_number(v, f, q[on_grid])
    print(case, "on the grid", on_grid.sum(), "inside", (rule > 0).sum(), "winding numbers off an integer by", np.abs(w - np.round(w)).max())
    assert np.abs(w - np.round(w)).max() < 1e-9
    np.testing.assert_array_equal(rule[on_grid] > 0, np.abs(w) > 0.5)
    assert (rule[~on_grid] == -1).all() and (rule > 0).sum() >= 25 and (rule[on_grid] < 0).sum() >= 25


@pytest.mark.parametrize("mirror", Q.ROLLOVER_MIRRORS)
def test_rollover_is_where_the_memory_forgets(mirror):
    v, f, q, designed = Q.rollover(mirror)
    step, dims, origin = Q.grid_of(v)
    direction, cells, _ = MO.inside_walks(q, step, origin, dims)
    want_dims = [7, 7, 7]
    want_dims["xyz".index(mirror[1])] = 4
    assert len(v) == 148 and len(f) == 17 and list(dims) == want_dims
    n = len(designed)
    assert n == 5 and (direction[:n] == Q.DIRECTIONS.index(mirror)).all() and cells[0] == 2
    short, full = _oracle_inside(v, f, q), _oracle_inside(v, f, q, memory=None)
    np.testing.assert_array_equal(short[:n], designed)
    np.testing.assert_array_equal(full[:n], Q.ROLLOVER_UNLIMITED)        # 17 and 16 distinct triangles above queries 0 and 3
    np.testing.assert_array_equal(_oracle_inside(v, f, q[:n], memory=16), Q.ROLLOVER_16_DEEP)
    assert (designed != Q.ROLLOVER_UNLIMITED).sum() == 2 and (designed != Q.ROLLOVER_16_DEEP).sum() == 1
    np.testing.assert_array_equal(short[n:], full[n:])
    assert (direction[n:] >= 0).sum() >= 20


@pytest.mark.parametrize("without", (None,) + Q.DIRECTIONS)
def test_ties_cover_every_pattern_and_answer_as_designed(without):
    v, f, q, designed, kinds = Q.ties(without)
    step, dims, origin = Q.grid_of(v)
    direction, _, to_end = MO.inside_walks(q, step, origin, dims)
    cell = kinds == "cell"
    assert len(v) == Q.TIES_NV and tuple(dims) == (Q.TIES_N,) * 3 and cell.sum() == Q.TIES_N ** 3
    patterns = {tuple(np.nonzero(t == t.min())[0]) for t in to_end[cell]}
    two = {(a, b) for a in range(6) for b in range(a + 1, 6) if a // 2 != b // 2}
    three = {(a, b, c) for a in (0, 1) for b in (2, 3) for c in (4, 5)}
    assert patterns >= two | three | {tuple(range(6))} | {(a,) for a in range(6)}
    for t, d in zip(to_end[cell], direction[cell]):
        assert d == Q.first_minimum(t) == min(np.nonzero(t == t.min())[0])
    assert (direction[np.isin(kinds, ("cell", "wall", "face0", "faceN-"))] >= 0).all()               # xf == 0 is on the grid ...
    assert (direction[np.isin(kinds, ("faceN", "off"))] == -1).all()                                  # ... xf == num is off it
    for d in range(3):                                                   # the outer-face queries sit on the very last float32
        xf = (q[:, d] - origin[d]) / np.float32(step)
        up = (np.nextafter(q[:, d], np.float32(np.inf)) - origin[d]) / np.float32(step)
        assert (xf == 0).sum() >= 4 and ((xf < Q.TIES_N) & (up >= Q.TIES_N)).sum() >= 4      # one float32 further is off the grid
    rule = _oracle_inside(v, f, q)
    has = designed != 0
    np.testing.assert_array_equal(rule[has], designed[has])
    if without is not None:                                              # the hole is seen: and only by the rays that take it
        closed = Q.ties()[3]
        flipped = np.nonzero(designed != closed)[0]
        # (of the 27 cells inside the cube, the first minimum is -x for 10, +x for 9, -y and +y for 3 each, -z and +z for one)
        assert len(flipped) == {"-x": 10, "+x": 9, "-y": 3, "+y": 3, "-z": 1, "+z": 1}[without]
        assert (direction[flipped] == Q.DIRECTIONS.index(without)).all()
        tied = [i for i in flipped if (to_end[i] == to_end[i].min()).sum() > 1]
        later = [i for i in np.nonzero(cell & (closed > 0) & (designed > 0))[0] if Q.DIRECTIONS.index(without) in np.nonzero(to_end[i] == to_end[i].min())[0]]
        print("without", without, ":", len(flipped), "answers turn,", len(tied), "of them at a tie;", len(later), "ties pass the hole by")
        # (-x comes first and loses no tie; +-z come last and win none inside the cube)
        assert (len(later) >= 1 or without == "-x") and (len(tied) >= 1 or without[1] == "z")


@pytest.mark.parametrize("scan", Q.BODIES)
@pytest.mark.parametrize("family", Q.RAY_FAMILIES)
def test_no_ray_is_grazing_and_families_hit_and_miss(scan, family):
    v, f, _ = Q.body(scan)
    o, d, plane = Q.rays(scan, family)
    assert len(o) == Q.N_RAYS and np.isfinite(o).all() and np.isfinite(d).all()
    assert not Q.grazing(v, f, o, d, plane).any()
    step, dims, origin = Q.grid_of(v)
    far_corner = origin + np.float32(step) * dims.astype(np.float32)
    outside = np.any((o < origin) | (o > far_corner), 1)
    zeros = (d == 0).sum(1)
    if family == "axis":
        assert (zeros == 2).all() and {(k, s) for k, s in zip(np.argmax(d != 0, 1), np.sign(d).sum(1))} == {(k, s) for k in range(3) for s in (-1, 1)}
    if family == "one_zero":
        assert (zeros == 1).all()
    if family == "wall_plane":
        k = plane
        xf = (o[np.arange(len(o)), k] - origin[k]) / np.float32(step)
        assert (plane >= 0).all() and (d[np.arange(len(o)), k] == 0).all() and np.abs(xf - np.round(xf)).max() < 1e-5
    else:
        assert (plane == -1).all()
    if family == "outside_miss":
        assert outside.all()
    if family == "far":
        dist = np.linalg.norm(o - (origin + far_corner) / 2, axis=1)
        norms = np.linalg.norm(d, axis=1)
        assert outside.all() and dist.min() > 20 and all((np.abs(norms / n - 1) < 1e-3).sum() >= Q.N_RAYS // 4 for n in Q.FAR_NORMS)
    if family == "outer_face":
        on_face = (o == origin) | (o == far_corner)
        assert on_face.any(1).all() and on_face.any(0).all() and not outside.any()
    if family == "zero":
        assert (zeros == 3).sum() >= 10 and ((d * d).sum(1) < 1e-9).all() and (zeros < 3).sum() >= 10
    want = MO.intersects_any(v, f, o, d)
    print(scan, family, "hits", int(want.sum()), "of", len(want))
    if family in Q.MISS_BY_CONSTRUCTION:
        assert not want.any()
    else:
        assert 0.1 * len(want) <= want.sum() <= 0.9 * len(want)


def test_ray_grazing_flags_what_it_should():
    """the criterion itself, on one triangle in a 4 x 4 x 4 grid of step 1 at the origin: a clean hit, a hit 3e-6 inside an edge, a hit
    on a grid plane, a miss, a triangle behind the origin (twice), and a ray in a wall's plane with and without the in-plane rule"""
    v = np.array([[0.3, 0.3, 1.5], [3.3, 0.4, 1.5], [0.4, 3.3, 1.5]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    grid = (1.0, np.zeros(3, np.float32), np.array([4, 4, 4]))
    o = np.array([[1.2, 1.3, 3.5], [1.2, 0.330003, 3.5], [1.0, 1.3, 3.5], [3.2, 3.3, 3.5], [1.2, 1.3, 0.5], [1.2, 1.3, 3.5]], np.float32)
    d = np.array([[0, 0, -1]] * 5 + [[0, 0, 1]], np.float32)
    np.testing.assert_array_equal(MO.ray_grazing(v, f, o, d, *grid), [False, True, True, False, False, False])
    o2, d2 = np.array([[1.2, 2.0, 3.5]], np.float32), np.array([[0.1, 0, -1]], np.float32)            # in the plane y = 2
    assert MO.ray_grazing(v, f, o2, d2, *grid).all()
    assert not MO.ray_grazing(v, f, o2, d2, *grid, in_plane_axis=1).any()
    m = 2 * 15 * 2.0 ** -24 * 4
    assert 1e-6 < m < 1e-5                                               # the margin at this size: a few float32 ulps of the grid


def test_backward_cases_lie_in_their_regions():
    c = Q.backward_case()
    zeros = (c["bary"] == 0).sum(1)
    for g in Q.REGIONS:
        m = c["group"] == g
        assert m.sum() == 8 and (c["ids"][m] == 0).all()
        assert (zeros[m] == {"f": 0, "e": 1, "c": 2}[g[0]]).all()
        if g[0] == "e":
            assert (c["bary"][m][:, int(g[-1])] == 0).all()
        if g[0] == "c":
            assert (c["bary"][m][:, int(g[-1])] == 1).all()
    tri = c["verts"][c["faces"]].astype(np.float64)
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert area[0] == 16 and area[1] == 0 and area[2] == 0 and np.ptp(tri[1], 0).max() == 4 and np.ptp(tri[2], 0).max() == 0
    assert (zeros[c["group"] == "segment"] >= 1).all() and (zeros[c["group"] == "segment"] == 1).sum() >= 4
    assert (zeros[c["group"] == "point"] == 1).all()
    assert (zeros[np.isin(c["group"], ("segment_flat", "point_flat"))] == 0).all()
    want = MO.nearest_backward(c["verts"], c["faces"], c["queries"], c["ids"], c["bary"], c["dnearest"])
    assert np.isfinite(want).all()
    flat = np.isin(c["group"], ("segment_flat", "point_flat"))
    np.testing.assert_array_equal(want[flat], c["dnearest"][flat].astype(np.float64))      # no plane to project onto: the identity
    np.testing.assert_array_equal(want[c["group"] == "point"], 0)
