"""The scan grid's build (bf_grid_count / scan / fill / pack), bf_inside_mesh_kernel, bf_intersect_kernel and bf_nearest_backward_kernel
on the cases of tests/scan_query_cases.py, against oracle/mesh_oracle.py - exactly: tests/test_scan_query_cases.py shows on the CPU that
the cases are well posed (the grids sit on the prefix sum's chunk edges, no ray is grazing, the designed answers are the rule's), so
nothing here is filtered and nothing has slack but the backward's float32 rounding.  Run with -s for the figures."""
import numpy as np
import pytest

import scan_query_cases as Q
from bodyfitting_amd import native as N
from oracle import mesh_oracle as MO

pytestmark = pytest.mark.gpu


def _grid(scan, verts):
    """the device's grid, held against set_mesh's as test_gpu_scan.test_grid_matches_set_mesh holds it"""
    dims, origin, step = scan.grid_info()
    step_o, dims_o, origin_o = MO.grid_params(np.array(verts))
    assert step == pytest.approx(step_o, rel=1e-6)
    np.testing.assert_array_equal(dims, dims_o)
    np.testing.assert_allclose(origin, origin_o, atol=1e-6)
    return dims, origin, step


def _inside(verts, faces, q):
    """-> (device answers, oracle answers on the DEVICE's grid and lists, directions walked)"""
    scan = N.Scan(verts, faces)
    try:
        dims, origin, step = _grid(scan, verts)
        tri_num, tri_idx = scan.grid_lists()
        got = scan.inside_mesh(q)
    finally:
        scan.close()
    want = MO.inside_mesh(verts, faces, q, step, origin, dims, tri_num, tri_idx)
    return got, want, MO.inside_walks(q, step, origin, dims)[0]


@pytest.mark.parametrize("name", Q.GRID_CASE_NAMES)
def test_grid_build_on_the_prefix_sums_chunk_edges(name):
    """cells + 1 = 4096 (one full chunk of bf_grid_scan_kernel), 4097 (one element in the second), 8193 (the carry taken twice), 25
    and 7: the cell lists are insert_grid_surface's, entry for entry, and a second build gives the same bytes"""
    v, f, q = Q.grid_case(name)
    scan = N.Scan(v, f)
    dims, origin, step = _grid(scan, v)
    tri_num, tri_idx = scan.grid_lists()
    tn_o, ti_o = MO.insert_grid_surface(v, f, step, origin, dims)
    print(name, "grid", dims, "scan length", int(np.prod(dims)) + 1, "entries", len(tri_idx))
    if name != Q.ONE_TRIANGLE:
        assert tuple(dims) == Q.GRID_CASES[name][2] and int(np.prod(dims)) + 1 == Q.GRID_CASES[name][3]
    np.testing.assert_array_equal(tri_num, tn_o)
    np.testing.assert_array_equal(tri_idx, ti_o)
    again = N.Scan(v, f)
    tn2, ti2 = again.grid_lists()
    assert tn2.tobytes() == tri_num.tobytes() and ti2.tobytes() == tri_idx.tobytes()
    # the queries of the case, on a grid of this size (one cell thick for the single triangle: every z distance is a tie at 0)
    got = scan.inside_mesh(q)
    np.testing.assert_array_equal(got, MO.inside_mesh(v, f, q, step, origin, dims, tri_num, tri_idx))
    again.close(); scan.close()


@pytest.mark.parametrize("case", ["stretched_body", "stretched_body_big"])
def test_inside_mesh_along_all_six_directions(case):
    v, f, q = Q.body(case)
    got, want, direction = _inside(v, f, q)
    print(case, "queries per direction", np.bincount(direction[direction >= 0], minlength=6), "inside", int((got > 0).sum()), "differ", int((got != want).sum()))
    np.testing.assert_array_equal(got, want)
    assert np.bincount(direction[direction >= 0], minlength=6).min() >= 10 and (got > 0).sum() >= 20 and (got < 0).sum() >= 20


@pytest.mark.parametrize("mirror", Q.ROLLOVER_MIRRORS)
def test_inside_mesh_forgets_after_fifteen_hits(mirror):
    """the 15-deep memory of the rule (the reference's visited[16]) rolls over: 18 counted where 17 triangles are crossed, 17 where 16"""
    v, f, q, designed = Q.rollover(mirror)
    got, want, direction = _inside(v, f, q)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[:len(designed)], designed)
    np.testing.assert_array_equal(got[:len(designed)], [-1, 1, -1, 1, 1])
    assert (direction[:len(designed)] == Q.DIRECTIONS.index(mirror)).all()


@pytest.mark.parametrize("without", (None,) + Q.DIRECTIONS)
def test_inside_mesh_breaks_ties_in_the_rules_order(without):
    """a query in every cell of a 5 x 5 x 5 grid around a lattice cube, closed and with each face left out in turn: inside the cube the
    answer is +1 unless the FIRST nearest wall in the order -x +x -y +y -z +z lies beyond the missing face; queries on cell walls and
    on the grid's outer faces (the low one is on the grid, the high one off it)"""
    v, f, q, designed, kinds = Q.ties(without)
    got, want, direction = _inside(v, f, q)
    np.testing.assert_array_equal(got, want)
    has = designed != 0
    np.testing.assert_array_equal(got[has], designed[has])
    centre = 2 * 25 + 2 * 5 + 2                                          # the six-way tie takes -x
    assert kinds[centre] == "cell" and got[centre] == (-1 if without == "-x" else 1)
    assert (got[np.isin(kinds, ("faceN", "off"))] == -1).all() and (direction[kinds == "face0"] >= 0).all()


@pytest.mark.parametrize("scan_name", Q.BODIES)
def test_intersects_any_is_the_brute_force_on_every_family(scan_name):
    """no ray of any family differs from the brute force over all triangles, in either direction"""
    v, f, _ = Q.body(scan_name)
    scan = N.Scan(v, f)
    _grid(scan, v)
    for family in Q.RAY_FAMILIES:
        o, d, _ = Q.rays(scan_name, family)
        got = scan.intersects_any(o, d)
        want = MO.intersects_any(v, f, o, d)
        print(scan_name, family, "hits", int(want.sum()), "of", len(want), "| false hits", int((got & ~want).sum()), "missed", int((want & ~got).sum()))
        np.testing.assert_array_equal(got, want, err_msg=family)
        if family in Q.MISS_BY_CONSTRUCTION:
            assert not got.any()
    scan.close()


def test_nearest_points_backward_by_region_and_on_its_guards():
    """bf_nearest_backward_kernel on one lattice triangle, eight queries in each Voronoi region; on a segment and a point (the
    `ee > 0` and `nn > 0` guards) and on face ids outside the mesh"""
    c = Q.backward_case()
    scan = N.Scan(c["verts"], c["faces"])
    got = scan.nearest_points_backward(c["ids"], c["bary"], c["dnearest"])
    want = MO.nearest_backward(c["verts"], c["faces"], c["queries"], c["ids"], c["bary"], c["dnearest"])
    assert np.isfinite(got).all()
    zeros = (c["bary"] == 0).sum(1)
    for g in np.unique(c["group"]):
        m = c["group"] == g
        scale = np.abs(want[m]).max()
        print(g, "worst error", float(np.abs(got[m] - want[m]).max()), "of", float(scale))
        np.testing.assert_allclose(got[m], want[m], rtol=0, atol=2e-5 * scale, err_msg=g)
        if g.startswith("edge") or g == "face":
            assert scale > 0.1
    np.testing.assert_array_equal(got[zeros == 2], 0)                    # corners: the closest point does not move
    np.testing.assert_array_equal(got[c["group"] == "point"], 0)         # an edge without length
    flat = np.isin(c["group"], ("segment_flat", "point_flat"))
    np.testing.assert_array_equal(got[flat], c["dnearest"][flat])        # a face without area: nothing to project out
    seg = (c["group"] == "segment") & (zeros == 1)
    assert seg.sum() >= 4 and np.abs(got[seg]).max() > 0.1 and (got[seg][:, 1:] == 0).all()         # along the segment's x direction only
    for bad in (-1, len(c["faces"]), 2 ** 31 - 1, -2 ** 31):
        ids = np.full(len(c["ids"]), bad, np.int64).astype(np.int32)
        np.testing.assert_array_equal(scan.nearest_points_backward(ids, c["bary"], c["dnearest"]), 0)
    scan.close()
