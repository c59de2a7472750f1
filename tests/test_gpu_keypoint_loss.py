"""bf_keypoint_loss (native.keypoint_loss), the drop-in `smplify.loss.multiview_keypoint_loss` and `smplify.prior.MaxMixturePrior`
on the MI355X.

Oracle: float64 torch autograd of oracle.smplify_oracle.multiview_keypoint_loss with respect to joints, pose and betas
(keypoint_loss_cases.oracle), started from the float32 values the kernel receives, so the difference is arithmetic only.  Points,
cameras and keypoints come from tests/loss_grad_cases.py; LG.oracle(case)["joints"] rounded to float32 are the world-space joints.
Band, the project's own: per gradient block max(5e-6 M, 8 err32), per term relative max(3e-6, 8 rel32), err32 /
rel32 the error of torch's float32 autograd of the same oracle at the same point.  Every check prints its worst position inside
the band before it asserts; nothing is skipped or filtered.

The worst position over the whole file is printed when its last test has run; it has not been recorded from a device run yet."""
import numpy as np
import pytest
import torch

import keypoint_loss_cases as KC
import loss_grad_cases as LG
from conftest import load_golden
from bodyfitting_amd import _lib, assets
from bodyfitting_amd import native as N
from bodyfitting_amd import synthetic as S
from bodyfitting_amd.keypoints import pack_keypoints_smplx
from oracle import smplify_oracle as O

pytestmark = pytest.mark.gpu
FIT_TOL = 1e-4
BLOCKS = ("djoints", "dposes", "dbetas")
HYPER_KEYS = ("sigma", "pose_prior_weight", "angle_prior_weight", "shape_prior_weight", "imsize")
WORST = {"block": 0.0, "term": 0.0}


@pytest.fixture(scope="module")
def gmm_dev():
    g = N.Gmm(*LG.gmm_bufs(), device=0)
    yield g
    g.close()


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    print(f"\nworst position inside the band over this file: gradient block {WORST['block']:.2f}, term {WORST['term']:.2f}")


# ----------------------------------------------------------------------------------------------------------------------------
# from a case of tests/loss_grad_cases.py to the arrays of one problem
# ----------------------------------------------------------------------------------------------------------------------------

def _case(kind, frame, V, tag):
    pr = LG.problem(kind, "small", frame, V)
    return LG.Case("K", f"{tag}-V{V}", kind, "small", pr, LG.point(kind, pr, ("K", tag, V)))


def _problem(case, absent=()):
    """-> dict(joints[R,3], w2c[V,4,4], K[V,3,3], kp[V,R,3], present[V], divisor, pose, betas, hyper) in float32.  `absent`: views
    marked absent for the kernel - their cameras and keypoints stay in the arrays, the kernel must not read them into the result."""
    pr = case.problem
    ref = LG.oracle(case)
    joints = np.asarray(ref["joints"], np.float32)
    assert LG.depths(case, joints).min() > LG.MIN_DEPTH
    # the arg-min component must be the same in float32 and float64: a quadratic form of a few hundred carries ~1e-6 of itself in
    # float32 rounding, i.e. below 1e-3; ten times that is asked of the runner-up's distance
    assert LG.gmm_gap(case)[1] > 0.01
    # (smplify.py:131-135: the cameras are inverted by torch in float32)
    w2c = torch.inverse(torch.as_tensor(np.asarray(pr["c2ws"]), dtype=torch.float32)).numpy()
    rows = joints.shape[0]
    kp = np.zeros((len(pr["keypoints"]), rows, 3), np.float32)
    for v, k in enumerate(pr["keypoints"]):
        if k is not None:
            kp[v] = pack_keypoints_smplx(k) if case.kind == "smplx" else np.asarray(k["pose"], np.float32)
    hyper = {k: float(v) for k, v in case.hyper.items() if k in HYPER_KEYS}
    hyper["imsize"] = float(pr["imsize"])
    return {"joints": joints, "w2c": w2c, "K": np.asarray(pr["Ks"], np.float32), "kp": kp,
            "present": np.array([k is not None and v not in absent for v, k in enumerate(pr["keypoints"])], np.uint8), "divisor": len(pr["use_frames"]),
            "pose": np.asarray(case.params["pose"], np.float32), "betas": np.asarray(case.params["betas"], np.float32)[:10], "hyper": hyper}


def _inp(problems, gmm=True, hyper=None, dterms=None, poses=True, betas=True):
    """n problems of equal sizes -> the arguments of KC.oracle / native.keypoint_loss"""
    st = lambda k: np.stack([p[k] for p in problems])          # noqa: E731
    inp = {"joints": st("joints"), "w2c": st("w2c"), "K": st("K"), "keypoints": st("kp"), "present": st("present"),
           "divisor": np.array([p["divisor"] for p in problems], np.int32), "poses": st("pose") if poses else None,
           "betas": st("betas") if betas else None, "gmm": (LG.gmm_bufs() if gmm is True else gmm) if gmm else None,
           "hyper": dict(problems[0]["hyper"] if hyper is None else hyper), "dterms": dterms}
    return inp


def _run(inp, gmm_dev, want=N.KP_LOSS_OUTPUTS):
    return N.keypoint_loss(inp["joints"], w2c=inp["w2c"], K=inp["K"], keypoints=inp["keypoints"], present=inp["present"],
                           divisor=inp["divisor"], poses=inp["poses"], betas=inp["betas"], gmm=gmm_dev if inp["gmm"] else None,
                           hyper=N.make_hyper(**inp["hyper"]), dterms=inp["dterms"], want=want)


def _check(name, inp, gmm_dev, got=None):
    got = _run(inp, gmm_dev) if got is None else got
    o64, o32 = KC.oracle(inp, torch.float64), KC.oracle(inp, torch.float32)
    worst_b, worst_t, fails = 0.0, 0.0, []
    n = len(o64["terms"])
    for i in range(n):
        for b in BLOCKS:
            if o64[b].shape[1] == 0:
                continue
            assert got[b].dtype == np.float32 and got[b].shape == o64[b].shape and np.isfinite(got[b]).all(), (name, b)
            band, M, err32 = LG.band(o64[b][i], o32[b][i])
            err = float(np.abs(got[b][i].astype(np.float64) - o64[b][i]).max())
            pos = err / band if band > 0 else (0.0 if err == 0 else np.inf)
            worst_b = max(worst_b, pos)
            if not err <= band:
                fails.append((i, b, err, band, M, err32))
        for t, term in enumerate(KC.TERMS):
            t64, t32, g = float(o64["terms"][i, t]), float(o32["terms"][i, t]), float(got["terms"][i, t])
            rel = LG.term_band(t64, t32)
            err = abs(g - t64)
            pos = err / (rel * abs(t64)) if t64 != 0 else (0.0 if err == 0 else np.inf)
            worst_t = max(worst_t, pos)
            if not err <= rel * abs(t64):
                fails.append((i, term, g, t64, rel))
    print(f"{name}: worst gradient block at {worst_b:.2f} of its band, worst term at {worst_t:.2f}")
    WORST["block"], WORST["term"] = max(WORST["block"], worst_b), max(WORST["term"], worst_t)
    assert not fails, (name, fails[:4])
    return got, o64


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ----------------------------------------------------------------------------------------------------------------------------
# views
# ----------------------------------------------------------------------------------------------------------------------------

# 512 threads, rows padded to 32: 16 view slots at 25 rows, 3 at 135 - both sides of every edge, one past two full rounds, and the
# 64-view staging chunk's edge inside 144
VIEWS = [("smpl", V) for V in (1, 2, 3, 15, 16, 17, 33, 48, 144)] + [("smplx", V) for V in (1, 2, 3, 4, 7, 48, 144)]


@pytest.mark.parametrize("kind,V", VIEWS)
def test_view_counts(gmm_dev, kind, V):
    _check(f"{kind} V={V}", _inp([_problem(_case(kind, 2, V, "views"))]), gmm_dev)


@pytest.mark.parametrize("kind,V", [("smpl", 17), ("smplx", 4), ("smplx", 7)])
def test_absent_views(gmm_dev, kind, V):
    for tag, missing in (("first", (0,)), ("last", (V - 1,)), ("every-second", tuple(range(0, V, 2))), ("odd", tuple(range(1, V, 2)))):
        _check(f"{kind} V={V} {tag} absent", _inp([_problem(_case(kind, 3, V, tag), missing)]), gmm_dev)


@pytest.mark.parametrize("kind", ["smpl", "smplx"])
def test_all_views_absent_and_no_views(gmm_dev, kind):
    V = 5
    p = _problem(_case(kind, 3, V, "none"), tuple(range(V)))
    # a joint at depth 0 in an absent view: skipped, not projected
    p["joints"][0] = -(p["w2c"][2, :3, :3].T @ p["w2c"][2, :3, 3])
    got, _ = _check(f"{kind} all absent", _inp([p]), gmm_dev)
    assert got["terms"][0, 0] == 0.0 and not _bits(got["djoints"]).any()
    none = N.keypoint_loss(p["joints"][None], poses=p["pose"][None], betas=p["betas"][None], gmm=gmm_dev)
    assert none["terms"][0, 0] == 0.0 and not _bits(none["djoints"]).any()
    for k in ("dposes", "dbetas"):
        np.testing.assert_array_equal(_bits(none[k]), _bits(got[k]))
    np.testing.assert_array_equal(_bits(none["terms"]), _bits(got["terms"]))
    empty = N.keypoint_loss(p["joints"][None], w2c=np.zeros((1, 0, 4, 4)), K=np.zeros((1, 0, 3, 3)), keypoints=np.zeros((1, 0, len(p["joints"]), 3)),
                            divisor=[3], poses=p["pose"][None], betas=p["betas"][None], gmm=gmm_dev)
    np.testing.assert_array_equal(_bits(empty["terms"]), _bits(got["terms"]))


# ----------------------------------------------------------------------------------------------------------------------------
# rows
# ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def x8():
    return _problem(_case("smplx", 1, 8, "rows"))


@pytest.mark.parametrize("rows", [1, 25, 31, 32, 33, 135, 256])
def test_row_counts(gmm_dev, x8, rows):
    p = dict(x8)
    if rows <= 135:
        p["joints"], p["kp"] = x8["joints"][:rows], x8["kp"][:, :rows]
    else:
        # 121 more rows: the first 121 joints moved by a few centimetres, with their keypoints
        shift = np.random.default_rng(5).normal(0, 0.03, (rows - 135, 3)).astype(np.float32)
        p["joints"] = np.concatenate([x8["joints"], x8["joints"][:rows - 135] + shift])
        p["kp"] = np.concatenate([x8["kp"], x8["kp"][:, :rows - 135]], 1)
    _check(f"rows={rows}", _inp([p]), gmm_dev)


def test_group_with_zero_confidences_gets_bit_zero_rows(gmm_dev, x8):
    p = dict(x8, kp=x8["kp"].copy())
    p["kp"][:, 25:46, 2] = 0.0
    got, _ = _check("left hand at zero confidence", _inp([p]), gmm_dev)
    assert not _bits(got["djoints"][0, 25:46]).any() and np.abs(got["djoints"][0, :25]).min() > 0


# ----------------------------------------------------------------------------------------------------------------------------
# problems
# ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def seventeen():
    out = []
    for f in range(17):
        missing = tuple(v for v in range(5) if (f >> v) & 1 and f % 6 != 5)        # a different presence pattern per problem
        out.append(_problem(_case("smpl", f, 5, f"n{f}"), missing))
    return out


@pytest.mark.parametrize("n", [1, 2, 5, 17])
def test_problem_counts_each_equal_to_its_own_call(gmm_dev, seventeen, n):
    inp = _inp(seventeen[:n])
    got, _ = _check(f"n={n}", inp, gmm_dev)
    for i in range(n):
        one = _run(_inp([seventeen[i]]), gmm_dev)
        for k in N.KP_LOSS_OUTPUTS:
            np.testing.assert_array_equal(_bits(got[k][i]), _bits(one[k][0]), err_msg=f"problem {i} {k}")


def test_problem_counts_smplx(gmm_dev):
    ps = [_problem(_case("smplx", f, 4, f"nx{f}"), (f % 4,) if f else ()) for f in range(3)]
    got, _ = _check("smplx n=3", _inp(ps), gmm_dev)
    for i in range(3):
        one = _run(_inp([ps[i]]), gmm_dev)
        for k in N.KP_LOSS_OUTPUTS:
            np.testing.assert_array_equal(_bits(got[k][i]), _bits(one[k][0]))


# ----------------------------------------------------------------------------------------------------------------------------
# priors, hypers, dterms, outputs
# ----------------------------------------------------------------------------------------------------------------------------

def _lg_cases(axis_fn, kinds, pick):
    return [c for c in axis_fn() if c.size == "small" and c.kind in kinds and pick(c)]


@pytest.mark.parametrize("kind", ["smpl", "smplx"])
def test_each_gmm_component_as_the_minimum(gmm_dev, kind):
    cases = _lg_cases(LG.axis_d, (kind,), lambda c: True)
    assert len(cases) == 16                                   # eight components, each with its priors-only variant
    for c in cases:
        m, gap = LG.gmm_gap(c)
        assert f"component{m}" in c.name and gap > 0.5
        p = _problem(c)
        assert len(p["pose"]) == (63 if kind == "smplx" else 69)
        _check(c.id, _inp([p]), gmm_dev)


def test_one_component_gmm_no_gmm_and_priors_only(gmm_dev, x8):
    p = _problem(_case("smpl", 4, 3, "gmm"))
    one = S.gmm_buffers(S.make_gmm(seed=3, n_comp=1))
    g1 = N.Gmm(*one, device=0)
    try:
        inp = _inp([p], gmm=one)
        _check("one component", inp, g1, got=_run(inp, g1))
    finally:
        g1.close()
    got, _ = _check("no gmm", _inp([p], gmm=None), gmm_dev)
    assert not _bits(got["terms"][:, 1]).any()
    for q in (p, x8):
        pri = N.keypoint_loss(None, poses=q["pose"][None], betas=q["betas"][None], gmm=gmm_dev)
        inp = _inp([dict(q, present=np.zeros_like(q["present"]))])
        full = _run(inp, gmm_dev)
        for k in ("dposes", "dbetas"):
            np.testing.assert_array_equal(_bits(pri[k]), _bits(full[k]))
        _check("priors only", inp, gmm_dev, got=full)


@pytest.mark.parametrize("name", [n for n, _ in LG.HYPER_SWEEP if not n.startswith("cscale")])
def test_hypers(gmm_dev, name):
    cases = [c for c in LG.axis_e() if c.name == name]
    assert len(cases) == len(LG.HYPER_MODELS)
    for c in cases:
        p = _problem(c)
        assert set(p["hyper"]) - {"imsize"} == set(c.hyper) - {"constant_scale", "imsize"}
        _check(c.id, _inp([p]), gmm_dev)


def test_angle_dofs_and_betas_at_their_extremes(gmm_dev):
    cases = _lg_cases(LG.axis_f, ("smpl", "smplx"), lambda c: (c.name.startswith("angles") or c.name.startswith("betas")) and "priors-only" not in c.name)
    assert len([c for c in cases if c.kind == "smpl" and c.name.startswith("angles")]) == 16          # all sign patterns at +-1.5 rad
    assert len([c for c in cases if c.name.startswith("betas")]) == 6
    for c in cases:
        _check(c.id, _inp([_problem(c)]), gmm_dev)


def test_non_unit_dterms(gmm_dev, seventeen, x8):
    rng = np.random.default_rng(11)
    d = rng.uniform(-2.0, 3.0, (5, 4)).astype(np.float32)
    d[1] = [0.0, 1.0, 0.0, 1.0]
    _check("dterms n=5", _inp(seventeen[:5], dterms=d), gmm_dev)
    _check("dterms smplx", _inp([x8], dterms=np.array([[0.5, -1.5, 2.0, 0.25]], np.float32)), gmm_dev)


def test_null_outputs_in_every_combination_and_determinism(gmm_dev, seventeen):
    inp = _inp(seventeen[:3])
    full = _run(inp, gmm_dev)
    again = _run(inp, gmm_dev)
    for k in N.KP_LOSS_OUTPUTS:
        np.testing.assert_array_equal(_bits(full[k]), _bits(again[k]), err_msg=k)
    for mask in range(16):
        want = tuple(k for i, k in enumerate(N.KP_LOSS_OUTPUTS) if (mask >> i) & 1)
        got = _run(inp, gmm_dev, want=want)
        assert set(got) == set(want)
        for k in want:
            np.testing.assert_array_equal(_bits(got[k]), _bits(full[k]), err_msg=f"{want} {k}")
    # no poses / no betas: that prior is off and its term 0
    got, _ = _check("no poses", _inp(seventeen[:2], poses=False), gmm_dev, got=dict(_run(_inp(seventeen[:2], poses=False), gmm_dev, want=("terms", "djoints", "dbetas")),
                                                                                     dposes=np.zeros((2, 0), np.float32)))
    assert not got["terms"][:, 1:3].any()
    got, _ = _check("no betas", _inp(seventeen[:2], betas=False), gmm_dev, got=dict(_run(_inp(seventeen[:2], betas=False), gmm_dev, want=("terms", "djoints", "dposes")),
                                                                                     dbetas=np.zeros((2, 0), np.float32)))
    assert not got["terms"][:, 3].any()


def test_optional_outputs_of_one_problem_with_two_views_and_one_row(gmm_dev):
    """n = 1, two views, one joint row (the fewest of test_row_counts): the 16 subsets of (terms, djoints, dposes, dbetas).  Every
    output asked for holds the bits of the all-outputs call; the empty subset succeeds and counts once on the host route"""
    p = _problem(_case("smpl", 2, 2, "views"))            # (test_view_counts' two-view problem)
    p["joints"], p["kp"] = p["joints"][:1], p["kp"][:, :1]
    inp = _inp([p])
    full = _run(inp, gmm_dev)
    assert all(np.isfinite(full[k]).all() for k in N.KP_LOSS_OUTPUTS) and full["djoints"].any()
    for mask in range(16):
        want = tuple(k for i, k in enumerate(N.KP_LOSS_OUTPUTS) if (mask >> i) & 1)
        before = N.dev_route_stats()["host_calls"]
        got = _run(inp, gmm_dev, want=want)
        assert N.dev_route_stats()["host_calls"] == before + 1, want
        assert set(got) == set(want)
        for k in want:
            assert got[k].tobytes() == full[k].tobytes(), (want, k)


def test_limits_return_their_error_codes(gmm_dev, seventeen):
    p = seventeen[0]
    V = len(p["w2c"])

    def code(**kw):
        args = dict(joints=p["joints"][None], w2c=p["w2c"][None], K=p["K"][None], keypoints=p["kp"][None], divisor=[V], poses=p["pose"][None],
                    betas=p["betas"][None], gmm=gmm_dev)
        args.update(kw)
        joints = args.pop("joints")
        with pytest.raises(_lib.BodyfitError) as e:
            N.keypoint_loss(joints, **args)
        return str(e.value)

    assert "(-3)" in code(joints=np.zeros((1, 257, 3)), keypoints=np.zeros((1, V, 257, 3)))          # BF_ERR_UNSUPPORTED
    assert "(-3)" in code(betas=np.zeros((1, 17)))
    assert "(-3)" in code(poses=np.zeros((1, 129)), gmm=None)
    assert "(-1)" in code(poses=np.zeros((1, 55)))                                                    # BF_ERR_INVALID
    assert "(-1)" in code(poses=np.zeros((1, 70)))                                                    # above the GMM's 69
    assert "(-1)" in code(divisor=[0])
    for kw in (dict(poses=None, want=("dposes",)), dict(betas=None, want=("dbetas",))):      # (refused before the library is called)
        with pytest.raises(ValueError):
            N.keypoint_loss(p["joints"][None], **kw)
    for M, D in ((17, 69), (8, 129)):
        with pytest.raises(_lib.BodyfitError, match=r"\(-3\)"):
            N.Gmm(np.zeros((M, D)), np.zeros((M, D, D)), np.ones(M))
    with pytest.raises(_lib.BodyfitError, match=r"\(-1\)"):
        N.Gmm(np.zeros((2, 69)), np.zeros((2, 69, 69)), np.array([1.0, 0.0]))
    # the largest sizes are accepted: 256 rows is test_row_counts; 16 components of 128 dimensions, 16 betas
    rng = np.random.default_rng(2)
    A = rng.normal(0, 0.2, (16, 128, 128))
    big = (rng.normal(0, 0.3, (16, 128)).astype(np.float32), (A @ A.transpose(0, 2, 1) + np.eye(128)).astype(np.float32),
           rng.uniform(0.1, 1.0, 16).astype(np.float32))
    g = N.Gmm(*big)
    try:
        q = dict(p, pose=rng.normal(0, 0.3, 128).astype(np.float32), betas=rng.normal(0, 1, 16).astype(np.float32))
        inp = _inp([q], gmm=big)
        _check("16 x 128 GMM, 16 betas", inp, g, got=_run(inp, g))
    finally:
        g.close()


def test_gradient_of_a_precision_matrix_that_is_not_symmetric(gmm_dev, seventeen):
    """autograd's 0.5 (P + P^T) d, not P d: the float32 inverse of a covariance is symmetric only to rounding, so the test skews one"""
    means, prec, w = (np.array(a) for a in LG.gmm_bufs())
    rng = np.random.default_rng(4)
    prec = (prec + 0.05 * np.abs(prec).mean() * rng.normal(size=prec.shape)).astype(np.float32)
    g = N.Gmm(means, prec, w)
    try:
        inp = _inp(seventeen[:2], gmm=(means, prec, w))
        _check("skewed precisions", inp, g, got=_run(inp, g))
    finally:
        g.close()


# ----------------------------------------------------------------------------------------------------------------------------
# the torch path and the prior alone
# ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def prior(gmm, monkeypatch):
    monkeypatch.setattr(assets, "_GMM", {"gmm": gmm})
    from bodyfitting_amd.prior import MaxMixturePrior
    p = MaxMixturePrior(prior_folder="prior", num_gaussians=8, dtype=torch.float32).to(torch.device("cpu"))      # smplify.py:46
    yield p
    for g in p._on_device.values():
        g.close()


def _dicts(case, p):
    return [k if p["present"][v] else None for v, k in enumerate(case.problem["keypoints"])]


@pytest.mark.parametrize("kind", ["smpl", "smplx"])
def test_torch_path_is_bit_equal_to_the_native_call(prior, kind):
    from bodyfitting_amd.loss import multiview_keypoint_loss
    case = _case(kind, 7, 5, "torch")
    p = _problem(case, (2,))
    hyper = dict(sigma=80.0, pose_prior_weight=3.0, angle_prior_weight=9.0, shape_prior_weight=4.0, imsize=512)
    x = [torch.tensor(p["joints"][None], requires_grad=True), torch.tensor(p["pose"][None], requires_grad=True),
         torch.tensor(p["betas"][None], requires_grad=True)]
    total, losses = multiview_keypoint_loss(torch.tensor(p["w2c"]), torch.tensor(p["K"]), _dicts(case, p), *x, case.problem["use_frames"], prior,
                                            use_hand_face=kind == "smplx", **hyper)
    assert total.dtype == torch.float32 and total.shape == ()
    want = N.keypoint_loss(p["joints"][None], w2c=p["w2c"][None], K=p["K"][None], keypoints=p["kp"][None], present=p["present"][None],
                           divisor=[p["divisor"]], poses=p["pose"][None], betas=p["betas"][None], gmm=prior._on_device[0],
                           hyper=N.make_hyper(**hyper))
    for i, k in enumerate(KC.TERMS):
        np.testing.assert_array_equal(_bits(np.float32(np.asarray(losses[k]).reshape(-1)[0])), _bits(want["terms"][0, i]))
    assert float(total) == float(torch.tensor(want["terms"]).sum())
    total.backward()
    for xi, k in zip(x, BLOCKS):
        np.testing.assert_array_equal(_bits(xi.grad.numpy().reshape(want[k].shape)), _bits(want[k]), err_msg=k)
    # numpy in: floats out, the same values
    t2, l2 = multiview_keypoint_loss(p["w2c"], p["K"], _dicts(case, p), *[t.detach().numpy() for t in x], case.problem["use_frames"], prior,
                                     use_hand_face=kind == "smplx", **hyper)
    assert isinstance(t2, float) and l2["reprojection_loss"] == float(want["terms"][0, 0])


@pytest.mark.parametrize("B", [1, 3])
def test_max_mixture_prior_alone(prior, B):
    rng = np.random.default_rng(B)
    means = np.asarray(LG.gmm_bufs()[0], np.float64)
    pose = (means[[1, 4, 6][:B]] + rng.normal(0, 0.05, (B, 69))).astype(np.float32)
    x = torch.tensor(pose, requires_grad=True)
    got = prior(x, None)
    assert got.shape == (B,) and got.dtype == torch.float32
    w = torch.tensor(rng.uniform(0.5, 2.0, B).astype(np.float32))
    (got * w).sum().backward()
    ref = {}
    for dtype in (torch.float64, torch.float32):
        y = torch.tensor(pose, dtype=dtype, requires_grad=True)
        v = O.gmm_merged_nll(y, *O.to_torch_gmm(LG.gmm_bufs(), dtype))
        g, = torch.autograd.grad((v * w.to(dtype)).sum(), y)
        ref[dtype] = (v.detach().numpy().astype(np.float64), g.numpy().astype(np.float64))
    for i in range(B):
        t64, t32 = ref[torch.float64][0][i], ref[torch.float32][0][i]
        assert abs(float(got[i]) - t64) <= LG.term_band(t64, t32) * abs(t64), (i, float(got[i]), t64)
        band, M, err32 = LG.band(ref[torch.float64][1][i], ref[torch.float32][1][i])
        err = float(np.abs(x.grad.numpy()[i].astype(np.float64) - ref[torch.float64][1][i]).max())
        print(f"B={B} row {i}: gradient at {err / band:.2f} of its band")
        assert err <= band, (i, err, band)
    np.testing.assert_array_equal(prior(pose, None), got.detach().numpy())


# ----------------------------------------------------------------------------------------------------------------------------
# the reference loop with BOTH halves on the HIP path: O.fit / O.fit_smplx with the model's forward swapped for the drop-in
# model (as tests/test_gpu_smpl_autograd.py does) and the loss swapped for the drop-in loss
# ----------------------------------------------------------------------------------------------------------------------------

PARAMS = ("global_transl", "scale", "pose", "betas", "global_orient")


def _swap_loss(monkeypatch, prior, raw_keypoints, use_frames):
    from bodyfitting_amd.loss import multiview_keypoint_loss
    calls = []

    def shim(w2cs, Ks, kps, model_joints, poses, betas, n_use_frames, gmm, imsize=512, use_hand_face=False, **kw):
        # (the oracle hands over packed keypoint tensors; the drop-in takes the OpenPose dicts the reference's loop holds)
        assert n_use_frames == len(use_frames) and not kw
        calls.append(1)
        return multiview_keypoint_loss(w2cs, Ks, raw_keypoints, model_joints, poses, betas, use_frames, prior, imsize=imsize,
                                       use_hand_face=use_hand_face)

    monkeypatch.setattr(O, "multiview_keypoint_loss", shim)
    return calls


@pytest.fixture
def smpl_dropin(smpl_model, gmm, monkeypatch):
    monkeypatch.setattr(assets, "_MODELS", {("smpl", "neutral"): smpl_model})
    monkeypatch.setattr(assets, "_GMM", {"gmm": gmm})
    monkeypatch.setattr(assets, "_DEVICE_MODELS", {})
    from bodyfitting_amd.smpl import SMPL
    smpl = SMPL(gender="neutral").to(torch.device("cpu"))          # (smplify.py:51-56's construction line)
    yield smpl
    for d in list(assets._DEVICE_MODELS.values()):
        d.close()


def _fit_smpl(monkeypatch, smpl_dropin, prior, smpl_model, gmm_bufs, prob, iters, snapshots):
    def forward(m, betas, global_orient, body_pose):
        out = smpl_dropin(betas=betas, global_orient=global_orient, body_pose=body_pose)
        return {"vertices": out.vertices, "joints": out.joints, "joints_ori": out.joints_ori, "full_pose": out.full_pose}
    monkeypatch.setattr(O, "smpl_forward", forward)
    calls = _swap_loss(monkeypatch, prior, prob["keypoints"], prob["use_frames"])
    res = O.fit(smpl_model, gmm_bufs, prob, iters, snapshots=snapshots)
    assert len(calls) == iters
    return res


def test_loop_on_the_hip_model_and_the_hip_loss_holds_cfg1(monkeypatch, smpl_dropin, prior, smpl_model, gmm_bufs):
    g = load_golden("cfg1_1view_50it.npz")
    prob = S.make_problem(smpl_model, frame=0, n_views=1)
    res = _fit_smpl(monkeypatch, smpl_dropin, prior, smpl_model, gmm_bufs, prob, 50, (1, 10, 50))
    worst = max(float(np.abs(res["snapshots"][k][n] - g[f"it{k}_{n}"]).max()) for k in (1, 10, 50) for n in PARAMS)
    print("cfg1: largest distance from the golden", worst)
    for k in (1, 10, 50):
        for n in PARAMS:
            np.testing.assert_allclose(res["snapshots"][k][n], g[f"it{k}_{n}"], rtol=0, atol=FIT_TOL, err_msg=f"it{k} {n}")


def test_loop_on_the_hip_model_and_the_hip_loss_holds_cfg2_frame0(monkeypatch, smpl_dropin, prior, smpl_model, gmm_bufs):
    g = load_golden("cfg2_48view_100it_f0.npz")
    prob = S.make_problem(smpl_model, frame=0, n_views=48)
    res = _fit_smpl(monkeypatch, smpl_dropin, prior, smpl_model, gmm_bufs, prob, 100, (1, 2, 10, 50, 100))
    worst = max(float(np.abs(res["snapshots"][k][n] - g[f"it{k}_{n}"]).max()) for k in (1, 2, 10, 50, 100) for n in PARAMS)
    print("cfg2 frame 0: largest distance from the golden", worst)
    for k in (1, 2, 10, 50, 100):
        for n in PARAMS:
            np.testing.assert_allclose(res["snapshots"][k][n], g[f"it{k}_{n}"], rtol=0, atol=FIT_TOL, err_msg=f"it{k} {n}")
    np.testing.assert_allclose(res["global_transl"], g["final_global_transl"], atol=FIT_TOL)


JOINT_MAPPER = dict(use_hands=True, use_face=True, use_face_contour=True, openpose_format="coco25")


@pytest.fixture
def smplx_dropin(gmm, monkeypatch):
    model = S.make_model("smplx", seed=0)
    dev = N.DeviceModel(model, gmm, device=0)
    monkeypatch.setattr(assets, "_MODELS", {("smplx", "neutral"): model})
    monkeypatch.setattr(assets, "_GMM", {"gmm": gmm})
    monkeypatch.setattr(assets, "_DEVICE_MODELS", {("smplx", "neutral", 0): dev})
    from bodyfitting_amd import smplx as X
    mapper = X.JointMapper(X.smpl_to_openpose("smplx", **JOINT_MAPPER))
    obj = X.create(model_path="data", model_type="smplx", joint_mapper=mapper, ext="npz", gender="neutral", use_face_contour=True,
                   dtype=torch.float32).to(torch.device("cpu"))                      # smplify.py:59-80
    yield model, obj
    dev.close()


def test_loop_on_the_hip_model_and_the_hip_loss_holds_the_smplx_golden(monkeypatch, smplx_dropin, prior, gmm_bufs):
    model, body = smplx_dropin

    def forward(m, betas, global_orient, body_pose, leye_pose, reye_pose, left_hand_pose, right_hand_pose, jaw_pose=None, expression=None,
                mapped=True):
        out = body(betas=betas, global_orient=global_orient, body_pose=body_pose, leye_pose=leye_pose, reye_pose=reye_pose,
                   left_hand_pose=left_hand_pose, right_hand_pose=right_hand_pose, jaw_pose=jaw_pose, return_full_pose=True)
        return {"vertices": out.vertices, "joints": out.joints, "full_pose": out.full_pose, "dyn_row": torch.as_tensor(body.dyn_row)}

    monkeypatch.setattr(O, "smplx_forward", forward)
    g = load_golden("smplx_8view_40it.npz")
    prob = S.make_problem_smplx(model, frame=0, n_views=8)
    calls = _swap_loss(monkeypatch, prior, prob["keypoints"], prob["use_frames"])
    res = O.fit_smplx(model, gmm_bufs, prob, 40, snapshots=(1, 2, 10, 40))
    assert len(calls) == 40
    worst = max(float(np.abs(res["snapshots"][k][n] - g[f"it{k}_{n}"]).max()) for k in (1, 2, 10, 40) for n in O.SMPLX_PARAMS)
    print("smplx: largest distance from the golden", worst)
    for k in (1, 2, 10, 40):
        for n in O.SMPLX_PARAMS:
            np.testing.assert_allclose(res["snapshots"][k][n], g[f"it{k}_{n}"], rtol=0, atol=FIT_TOL, err_msg=f"it{k} {n}")
    np.testing.assert_allclose(res["joints"], g["joints"], rtol=0, atol=FIT_TOL)
