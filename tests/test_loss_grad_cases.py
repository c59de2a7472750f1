"""Every case of the gradient sweep (tests/loss_grad_cases.py) is well posed - proven here on the CPU oracle, so that
tests/test_gpu_loss_grad_sweep.py never has to leave a case, a view, a joint or a parameter out:

  * every loss joint is more than 0.2 m in front of every present camera (the reference guards neither the near plane nor a
    point behind the camera, loss.py:22-43);
  * the fp64 gradient is finite and no block is identically zero unless the case declares it;
  * torch's float32 autograd of the same oracle agrees with float64 to 1e-5 of each block's maximum - a case where the
    reference's own float32 arithmetic is worse than that would be ill conditioned and gets rebuilt, not banded;
  * axis C: the neck sweep reaches exactly the rows 0..78 and every yaw stays clear of a rounding boundary;
  * axis D: the GMM arg-min is the intended component with more than 0.5 to the runner-up (float32 cannot flip it);
  * axis R: the swept angles reach every quadrant of the fit kernel's sine / cosine on every model kind, its wrap (n >= 4, n >= 8),
    both sides of u = 1e-3 and an angle whose float32 cosine is 1; SMPL-X yaws stay 1e-3 degrees from a rounding boundary;
  * axis H: the oracle's float32 and float64 loops from the case's point agree to 1e-5 after the ten steps.
"""
import functools
import warnings

import numpy as np
import pytest
import torch

import loss_grad_cases as LC

CASES = LC.all_cases()
IDS = [c.id for c in CASES]


@functools.lru_cache(maxsize=None)
def _oracles(i):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)         # (float() of a tensor that requires grad, inside the oracle)
        return LC.oracle(CASES[i], torch.float64), LC.oracle(CASES[i], torch.float32)


def test_the_sweep_covers_every_axis():
    per_axis = {a: [c for c in CASES if c.axis == a] for a, _ in LC.AXES}
    assert all(len(v) > 0 for v in per_axis.values())
    # A: every view count of the sparse kernel on both instances, plus the largest accepted one
    for kind in ("smpl", "kid"):
        assert {c.n_views for c in per_axis["A"] if c.kind == kind and c.size == "small"} >= set(LC.VIEWS_A) | {LC.V_MAX[kind]}
    assert {c.n_views for c in per_axis["B"] if c.size == "small"} == set(LC.VIEWS_B) | {LC.V_MAX["smplx"]}
    # every axis runs its first and last case on the full-size models too
    for a, cases in per_axis.items():
        assert any(c.size == "full" for c in cases), a
    # H: one case per view-count regime of A and B, two contour rows >= 40, two GMM components, the all-at-once hypers
    loops = LC.loop_cases()
    assert {c.axis for c in loops} == {"A", "B", "C", "D", "E", "R"}
    va = {c.n_views for c in loops if c.axis == "A"}
    assert min(va) <= 16 and any(16 < v <= 48 for v in va) and any(v > 48 for v in va)
    vb = {c.n_views for c in loops if c.axis == "B"}
    assert any(v <= 118 for v in vb) and any(v >= 119 for v in vb)
    assert sum(c.axis == "C" for c in loops) >= 2 and sum(c.axis == "D" for c in loops) >= 2
    assert any(c.axis == "E" and len(c.hyper) == len(LC.HYPER_KEYS) for c in loops)
    # R: properties of the INPUTS, in the float32 terms of the fit kernel's sincos_small and rodrigues_fwd (a = ||theta + 1e-8||,
    # u = a * a, n = rint(a * 0.636619772)), read off the cases' own parameters
    def numbers(cases):
        got = []
        for c in cases:
            full = np.concatenate([c.params["global_orient"], c.params["pose"]] + ([np.zeros(3), c.params["leye_pose"]] if c.kind == "smplx" else []))
            for j, th in c.swept.items():
                assert np.array_equal(full[3 * j:3 * j + 3], th), (c.id, j)              # the case carries the swept vector unchanged
                got.append(LC.sweep_numbers(full[3 * j:3 * j + 3]))
        return got
    for kind in ("smpl", "kid", "smplx"):
        assert {n & 3 for _, _, n, _ in numbers(c for c in per_axis["R"] if c.kind == kind)} == {0, 1, 2, 3}, kind
        assert any(n >= 4 for _, _, n, _ in numbers(c for c in per_axis["R"] if c.kind == kind)), kind
    for kind in ("smpl", "smplx"):
        small = numbers(c for c in per_axis["R"] if c.kind == kind and c.size == "small")
        assert any(n >= 8 for _, _, n, _ in small), kind
        assert any(u < np.float32(1e-3) for _, u, _, _ in small) and any(np.float32(1e-3) <= u < np.float32(1.01e-3) for _, u, _, _ in small), kind
        assert any(cos_a == 1.0 and a != 0.0 for a, _, _, cos_a in small), kind          # 1 - cos a has no bits left
        # exact coordinate axes, one of them with a negative zero; the general direction; the angles of R_ALL_AXES_AT on all four
        vecs = [th for c in per_axis["R"] if c.kind == kind for th in c.swept.values()]
        assert any(np.count_nonzero(th) == 1 and np.signbit(th[th == 0.0]).any() for th in vecs) and any(np.count_nonzero(th) == 3 for th in vecs)
    for a in LC.R_ALL_AXES_AT:
        assert {s.axis for s in LC.sweep() if s.a == a} == set(LC.R_AXIS_NAMES), a
    # the loops: a leaf in quadrant 3, a root whose steps cross the wrap at 2 pi, a spine joint whose steps cross u = 1e-3
    assert sorted((c.kind, c.name.split("-")[0], c.name.rsplit("-", 1)[1]) for c in loops if c.axis == "R") == \
        [("smpl", "2pi", "root"), ("smpl", "4.7", "leaf"), ("smplx", "0.0318", "spine")]
    # no swept rotation on the knees and elbows but the one declared pair
    for c in per_axis["R"]:
        assert all(j not in (4, 5, 18, 19) for j in c.swept) or "knee" in c.name, c.id


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_case_is_well_posed(i):
    c = CASES[i]
    o64, o32 = _oracles(i)
    d = LC.depths(c, o64["joints"])
    assert d.shape[0] >= 1 and d.min() > LC.MIN_DEPTH, f"a loss joint {d.min():.2f} m from a camera plane"
    for k in c.blocks:
        g64, g32 = o64["grads"][k], o32["grads"][k]
        assert np.isfinite(g64).all() and np.isfinite(g32).all(), k
        _, M, err32 = LC.band(g64, g32, c.base)
        if k in c.zero_blocks:
            assert M == 0.0 and err32 == 0.0, k
        else:
            assert M > 0.0, f"{k} is identically zero"
            assert err32 <= 1e-5 * M, f"{k}: float32 autograd is {err32 / M:.1e} of the block's maximum from float64"
    for n in LC.TERMS:
        assert np.isfinite(o64["terms"][n])
    if c.axis == "D":
        m, gap = LC.gmm_gap(c)
        assert f"component{m}" in c.name and gap > 0.5, (m, gap)
    if c.axis == "C":
        y = LC.neck_yaw_degrees(c)
        frac = abs(y - 0.5 - round(y - 0.5))                  # distance of -yaw * 180 / pi from the nearest half-integer
        assert frac >= (0.1 if c.name.startswith("chain") else 0.24), (y, frac)
        assert 0 <= o64["row"] <= 78 and o32["row"] == o64["row"]


def test_neck_sweep_reaches_every_contour_row():
    rows = {}
    for i, c in enumerate(CASES):
        if c.axis == "C" and c.size == "small" and c.name.startswith("neck"):
            rows[int(c.name[4:])] = _oracles(i)[0]["row"]
    assert set(rows.values()) == set(range(79))
    assert all(1 <= rows[d] <= 39 for d in range(-45, 0)) and rows[-45] == 39 and rows[-40] == 39          # the clamp at 39
    assert all(40 <= rows[d] <= 78 for d in range(1, 45)) and rows[0] == 0
    chain = [_oracles(i)[0]["row"] for i, c in enumerate(CASES) if c.axis == "C" and c.name.startswith("chain")]
    assert len(chain) == 3 and max(chain) >= 40


def test_axis_r_contour_rows_stay_clear_of_a_rounding_boundary():
    """a swept root or spine joint turns the neck: -yaw of every SMPL-X case of axis R sits 1e-3 degrees or more (ROW_MARGIN of
    tests/test_gpu_smplx_autograd.py) from a rounding boundary of the contour row, and float32 picks the float64 row"""
    n = 0
    for i, c in enumerate(CASES):
        if c.axis == "R" and c.kind == "smplx":
            y = LC.neck_yaw_degrees(c)
            assert abs(y - 0.5 - round(y - 0.5)) >= 1e-3, (c.id, y)
            o64, o32 = _oracles(i)
            assert 0 <= o64["row"] <= 78 and o32["row"] == o64["row"], c.id
            n += 1
    assert n > 30


@pytest.mark.parametrize("c", LC.loop_cases(), ids=[c.id for c in LC.loop_cases()])
def test_loop_start_is_well_conditioned(c):
    """ten Adam steps from the case's point: the oracle loop in float32 and in float64 end within 1e-5 of each other"""
    a, b = LC.oracle_loop(c, 10, double=True), LC.oracle_loop(c, 10, double=False)
    for k in c.blocks:
        assert np.isfinite(np.asarray(a[k])).all()
        np.testing.assert_allclose(np.asarray(b[k], np.float64), np.asarray(a[k], np.float64), rtol=0, atol=1e-5, err_msg=k)


def test_oracle_keywords_default_to_the_reference_literals():
    """the keyword arguments added for the sweep change nothing when left alone, and each of them reaches its term"""
    c = next(x for x in CASES if x.axis == "E" and x.kind == "smpl" and x.name == "default-hyper")
    m, g = LC.model(c.kind, c.size), LC.gmm_bufs()
    from oracle import smplify_oracle as O
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        base = O.loss_and_grad(m, g, c.problem, c.params)
        same = O.loss_and_grad(m, g, c.problem, c.params, constant_scale=c.problem["constant_scale"], sigma=O.SIGMA,
                               pose_prior_weight=O.POSE_PRIOR_WEIGHT, angle_prior_weight=O.ANGLE_PRIOR_WEIGHT,
                               shape_prior_weight=O.SHAPE_PRIOR_WEIGHT)
        twice = O.loss_and_grad(m, g, c.problem, c.params, pose_prior_weight=2 * O.POSE_PRIOR_WEIGHT,
                                angle_prior_weight=2 * O.ANGLE_PRIOR_WEIGHT, shape_prior_weight=2 * O.SHAPE_PRIOR_WEIGHT)
    assert base[0] == same[0] and all(np.array_equal(base[2][k], same[2][k]) for k in base[2])
    for n in LC.TERMS[1:]:
        assert twice[1][n] == pytest.approx(4 * base[1][n], rel=1e-12)
    assert twice[1]["reprojection_loss"] == base[1]["reprojection_loss"]
    with pytest.raises(TypeError):
        O.loss_and_grad(m, g, c.problem, c.params, sigm=1.0)


def test_analytic_loop_oracle_takes_the_same_keywords():
    """oracle/analytic.py drives axis H's SMPL loops: with the all-at-once hypers its gradient is float64 autograd's (1e-9 of each block)"""
    from oracle import analytic as A
    c = next(x for x in CASES if x.axis == "E" and x.kind == "smpl" and x.name == "all-at-once")
    m = LC.model(c.kind, c.size)
    kw = c.oracle_keywords()
    cs = kw.pop("constant_scale")
    _, terms, grads, _ = A.loss_grad(A.build_fit_tables(m), LC.gmm_bufs(), A.build_views(c.problem), c.params, cs, c.problem["imsize"], **kw)
    o64, _ = _oracles(CASES.index(c))
    for n in LC.TERMS:
        assert terms[n] == pytest.approx(o64["terms"][n], rel=1e-10)
    for k in c.blocks:
        np.testing.assert_allclose(grads[k], o64["grads"][k], rtol=0, atol=1e-9 * np.abs(o64["grads"][k]).max(), err_msg=k)
