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


# ------------------------------------------------------------------------------------------------------------------------------
# The one-shot host entry points (host arrays in, host arrays out, nothing kept): bf_smpl_forward, bf_model_forward, bf_scan_nearest,
# bf_scan_nearest_hinted, bf_scan_inside, bf_scan_intersects, bf_scan_nearest_backward and the two bf_nearest_selftest_*.  Their
# buffers may be blocks another call has used before: block edges of the 256-thread launches, a smaller call behind a larger one,
# the route counters and the refusals.  Everything on the 690-vertex model and the 690-vertex scan.
# ------------------------------------------------------------------------------------------------------------------------------

EDGE = (255, 256, 257)                    # both sides of a 256-thread block
INVALID = -1                              # BF_ERR_INVALID
COUNTERS = ("host_calls", "dev_calls", "allocations", "stream_switches")


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint8)


def _same_words(got, want, what):
    """bit for bit (as uint32: -0.0 is not +0.0, a NaN is its payload)"""
    g, w = _words(got), _words(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), f"{what}: {int((g != w).sum())} of {g.size} words differ"


@pytest.fixture(scope="module")
def dev690():
    from bodyfitting_amd import synthetic as S
    dev = N.DeviceModel(Q.model690(), S.make_gmm(seed=0), device=0)
    yield dev
    dev.close()


@pytest.fixture(scope="module")
def body_scan():
    v, f, q = Q.body("body")
    scan = N.Scan(v, f)
    yield scan, v, f, q
    scan.close()


def _smpl_inputs(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 0.7, (n, 10)).astype(np.float32), rng.normal(0, 0.8, (n, 3)).astype(np.float32),
            rng.normal(0, 0.3, (n, 69)).astype(np.float32))


def _packed(n, seed):
    """packed parameters [n, 86] of _smpl_inputs(n, seed) with a similarity that is NOT the identity: bf_model_forward ignores it"""
    betas, orient, pose = _smpl_inputs(n, seed)
    rng = np.random.default_rng(seed + 1)
    transl, scale = rng.normal(0, 0.5, (n, 3)).astype(np.float32), rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
    return np.concatenate([transl, scale, pose, betas, orient], 1)


def _rays(n):
    o, d = zip(*[Q.rays("body", family)[:2] for family in ("uniform", "axis", "one_zero")])
    return np.ascontiguousarray(np.concatenate(o)[:n]), np.ascontiguousarray(np.concatenate(d)[:n])


def test_inside_mesh_and_intersects_any_on_both_sides_of_a_block(body_scan):
    """n = 255, 256, 257 against the oracles of this file: the restated inside rule on the device's own grid, the brute force over
    all triangles"""
    scan, v, f, q = body_scan
    dims, origin, step = _grid(scan, v)
    tri_num, tri_idx = scan.grid_lists()
    inside = MO.inside_mesh(v, f, q[:EDGE[-1]], step, origin, dims, tri_num, tri_idx)
    o, d = _rays(EDGE[-1])
    hits = MO.intersects_any(v, f, o, d)
    assert (inside > 0).sum() >= 20 and (inside < 0).sum() >= 20 and hits.sum() >= 20 and (~hits).sum() >= 20
    for n in EDGE:
        np.testing.assert_array_equal(scan.inside_mesh(q[:n]), inside[:n], err_msg=f"inside_mesh n={n}")
        np.testing.assert_array_equal(scan.intersects_any(o[:n], d[:n]), hits[:n], err_msg=f"intersects_any n={n}")


def test_nearest_points_backward_on_both_sides_of_a_block():
    """the 88 queries of the backward case repeated up to n = 255, 256, 257: the oracle's gradient in the band of
    test_nearest_points_backward_by_region_and_on_its_guards (2e-5 of the group's largest entry; exact zeros stay exact)"""
    c = Q.backward_case()
    scan = N.Scan(c["verts"], c["faces"])
    want = MO.nearest_backward(c["verts"], c["faces"], c["queries"], c["ids"], c["bary"], c["dnearest"])
    for n in EDGE:
        i = np.arange(n) % len(c["ids"])
        got = scan.nearest_points_backward(c["ids"][i], c["bary"][i], c["dnearest"][i])
        assert got.shape == (n, 3) and np.isfinite(got).all()
        for g in np.unique(c["group"]):
            m = c["group"][i] == g
            np.testing.assert_allclose(got[m], want[i][m], rtol=0, atol=2e-5 * np.abs(want[c["group"] == g]).max(), err_msg=f"n={n} {g}")
    scan.close()


@pytest.mark.parametrize("n", [1, 16])
def test_forward_packed_is_forward_on_the_same_parameters(dev690, n):
    """bf_model_forward (packed parameters, the similarity ignored) against bf_smpl_forward on the same betas and thetas, at 1 frame and
    at BF_MFMA_MIN_FRAMES frames.  Rule applied: bit for bit - the two calls agree in every word of vertices and joints
    (the 3e-6 band of the suite's other forward_packed tests is against the float64 oracle and is not needed between the two)."""
    betas, orient, pose = _smpl_inputs(n, 40 + n)
    verts, joints, _ = dev690.forward(betas, orient, pose)
    pv, pj = dev690.forward_packed(_packed(n, 40 + n))
    print(f"n={n}: vertices max |diff| {np.abs(pv - verts).max():.3g} ({int((_words(pv) != _words(verts)).sum())} words), "
          f"joints max |diff| {np.abs(pj - joints).max():.3g} ({int((_words(pj) != _words(joints)).sum())} words)")
    _same_words(pv, verts, f"n={n} vertices")
    _same_words(pj, joints, f"n={n} joints")


def _one_shot_entries(dev, scan_ctx):
    """name -> call(size, seed) -> tuple of result arrays; sizes: (small, large)"""
    scan, v, f, q = scan_ctx
    lib = N._lib.load()
    c = Q.backward_case()

    def points(n, seed):
        rng = np.random.default_rng(seed)
        return np.ascontiguousarray(v[rng.integers(0, len(v), n)] + rng.normal(0, 0.02, (n, 3)), np.float32)

    def rays(n, seed):
        rng = np.random.default_rng(seed)
        return points(n, seed), rng.normal(size=(n, 3)).astype(np.float32)

    def backward(n, seed):
        i = np.random.default_rng(seed).integers(0, len(c["ids"]), n)
        return scan_b.nearest_points_backward(c["ids"][i], c["bary"][i], c["dnearest"][i]),

    def quot(n, seed):
        rng = np.random.default_rng(seed)
        num, den = rng.normal(0, 3, n).astype(np.float32), rng.uniform(0.1, 3.0, n).astype(np.float32)
        out = np.empty(n, np.float32)
        N._lib.check(lib.bf_nearest_selftest_quot(0, n, N._lib.fptr(num), N._lib.fptr(den), N._lib.fptr(out)), "selftest_quot")
        _same_words(out, num / den, f"quot n={n}")
        return out,

    def rule(n, seed):
        patches = np.random.default_rng(seed).normal(0, 1, (n, 9)).astype(np.float32)
        dist, coeff = np.empty(n, np.float32), np.empty((n, 3), np.float32)
        N._lib.check(lib.bf_nearest_selftest_rule(0, n, N._lib.fptr(patches), 1, N._lib.fptr(dist), N._lib.fptr(coeff)), "selftest_rule")
        return dist, coeff

    scan_b = N.Scan(c["verts"], c["faces"])
    entries = {
        "bf_smpl_forward": (lambda n, s: dev.forward(*_smpl_inputs(n, s)), (3, 16)),
        "bf_model_forward": (lambda n, s: dev.forward_packed(_packed(n, s)), (3, 16)),
        "bf_scan_nearest": (lambda n, s: scan.nearest_points(points(n, s)), (5, 257)),
        "bf_scan_nearest_hinted": (lambda n, s: scan.nearest_points_hinted(points(n, s), hint=points(n, s + 1)), (5, 257)),
        "bf_scan_inside": (lambda n, s: (scan.inside_mesh(points(n, s)),), (5, 257)),
        "bf_scan_intersects": (lambda n, s: (scan.intersects_any(*rays(n, s)),), (5, 257)),
        "bf_scan_nearest_backward": (backward, (5, 257)),
        "bf_nearest_selftest_quot": (quot, (5, 300)),
        "bf_nearest_selftest_rule": (rule, (5, 300)),
    }
    return entries, scan_b


ONE_SHOT = ("bf_smpl_forward", "bf_model_forward", "bf_scan_nearest", "bf_scan_nearest_hinted", "bf_scan_inside", "bf_scan_intersects",
            "bf_scan_nearest_backward", "bf_nearest_selftest_quot", "bf_nearest_selftest_rule")


@pytest.mark.parametrize("name", ONE_SHOT)
def test_a_smaller_call_behind_a_larger_one_reads_nothing_stale(dev690, body_scan, name):
    """small, LARGE (other data), small, small: the three small results are the same words - a buffer that held the larger call's
    data is written before it is read - and the counters move as they should: bf_smpl_forward and bf_scan_nearest count one host
    call each, the others count nothing, and no host-route call counts a device call, an allocation or a stream switch"""
    entries, scan_b = _one_shot_entries(dev690, body_scan)
    try:
        call, (small, large) = entries[name]
        want = call(small, 7)
        call(large, 8)
        before = N.dev_route_stats()
        second = call(small, 7)
        after = N.dev_route_stats()
        third = call(small, 7)
        for k, (a, b, w) in enumerate(zip(second, third, want)):
            _same_words(a, w, f"{name} output {k}: behind the larger call")
            _same_words(b, w, f"{name} output {k}: the call after that")
        counted = 1 if name in ("bf_smpl_forward", "bf_scan_nearest") else 0
        assert after["host_calls"] == before["host_calls"] + counted, (name, before, after)
        assert all(after[k] == before[k] for k in COUNTERS[1:]), (name, before, after)
    finally:
        scan_b.close()


def test_without_a_hint_the_nearest_buffer_is_not_read(body_scan):
    """a hinted call, then the same points without a hint: nearest_points' bits (the kernel may not take what the buffer held for a
    guess); a NaN hint and a far-off hint give nearest_points' bits too"""
    scan, v, f, q = body_scan
    for n in (5, 257):
        rng = np.random.default_rng(90 + n)
        pts = np.ascontiguousarray(v[rng.integers(0, len(v), n)] + rng.normal(0, 0.02, (n, 3)), np.float32)
        want = scan.nearest_points(pts)
        hints = {"a good guess": want[0], "NaN": np.full((n, 3), np.nan, np.float32), "far off": pts + np.float32(50.0),
                 "a wrong guess": np.ascontiguousarray(want[0][::-1])}
        for what, hint in hints.items():
            got = scan.nearest_points_hinted(pts, hint=hint)
            bare = scan.nearest_points_hinted(pts, hint=None)
            for k, name in enumerate(("nearest", "face ids", "coefficients")):
                _same_words(got[k], want[k], f"n={n} hint {what}: {name}")
                _same_words(bare[k], want[k], f"n={n} no hint behind {what}: {name}")
        timed = scan.nearest_points_hinted(pts, hint=want[0], reps=3)
        assert len(timed) == 4 and timed[3] > 0.0
        for k in range(3):
            _same_words(timed[k], want[k], f"n={n} three timed repeats")


def test_the_one_shot_entries_refuse_bad_arguments(dev690, body_scan):
    """a NULL handle, n = 0 and each required pointer NULL in turn: BF_ERR_INVALID, "<entry>: bad argument", no counter moved; an
    output that is optional may be NULL (bf_smpl_forward runs with all three NULL)"""
    import ctypes as C
    scan, v, f, q = body_scan
    lib = N._lib.load()
    F, I = N._lib.fptr, N._lib.iptr
    a = np.zeros(3 * 690 * 3, np.float32)
    i32 = np.zeros(16, np.int32)
    u8 = np.zeros(16, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
    m, s = dev690._h, scan._h
    good = {
        "bf_smpl_forward": (lib.bf_smpl_forward, [m, 1, F(a), F(a), F(a), None, None, None], (0, 2, 3, 4)),
        "bf_model_forward": (lib.bf_model_forward, [m, 1, F(a), None, None], (0, 2)),
        "bf_scan_inside": (lib.bf_scan_inside, [s, 1, F(a), F(a)], (0, 2, 3)),
        "bf_scan_intersects": (lib.bf_scan_intersects, [s, 1, F(a), F(a), u8], (0, 2, 3, 4)),
        "bf_scan_nearest": (lib.bf_scan_nearest, [s, 1, F(a), None, None, None], (0, 2)),
        "bf_scan_nearest_hinted": (lib.bf_scan_nearest_hinted, [s, 1, F(a), None, None, None, None, 0, None], (0, 2)),
        "bf_scan_nearest_backward": (lib.bf_scan_nearest_backward, [s, 1, I(i32), F(a), F(a), F(a)], (0, 2, 3, 4, 5)),
        "bf_nearest_selftest_quot": (lib.bf_nearest_selftest_quot, [0, 1, F(a), F(a), F(a)], (2, 3, 4)),
        "bf_nearest_selftest_rule": (lib.bf_nearest_selftest_rule, [0, 1, F(a), 1, F(a), F(a)], (2, 4, 5)),
    }
    assert set(good) == set(ONE_SHOT)
    before = N.dev_route_stats()
    for name, (fn, args, required) in good.items():
        bad = [args[:1] + [0] + args[2:], args[:1] + [-1] + args[2:]] + [args[:k] + [None] + args[k + 1:] for k in required]
        for b in bad:
            assert fn(*b) == INVALID, (name, b)
            assert lib.bf_last_error() == name.encode() + b": bad argument", (name, lib.bf_last_error())
    assert N.dev_route_stats() == before, "a refused call was counted"
    for name, (fn, args, _) in good.items():
        assert fn(*args) == 0, (name, lib.bf_last_error())
    after = N.dev_route_stats()
    assert after["host_calls"] == before["host_calls"] + 2 and all(after[k] == before[k] for k in COUNTERS[1:]), (before, after)
