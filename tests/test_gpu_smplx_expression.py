"""SMPL-X expression coefficients through the HIP forward and its VJP on the MI355X: bf_smplx_forward_expr / bf_smplx_vjp_expr
(DeviceModel.forward_smplx / vjp_smplx with `expression`) against the float64 oracle's smplx forward and its torch autograd, the
call without expression, all three skinning widths, another number of coefficients, determinism, the refusals, and the loop the
feature serves: Adam on expression and jaw against the 68 face landmarks through the drop-in object.

Parameters are those of tests/test_gpu_smplx_autograd.py (the same draws for the same seed, so its contour-row margins hold here: the
row depends on the pose alone) with expression ~ N(0, 0.7) drawn behind them; frame 0's expression is exactly zero.  The synthetic
expression directions are dense over the vertices: max |Jx| is 0.05 and a vertex moves up to 0.077, so the vertex and the joint half
of the mathematics both carry.

Band of the VJP (the convention of tests/test_gpu_smpl_autograd.py): max|HIP - fp64| <= 4 * max|torch fp32 - fp64| + 1e-6 * max|fp64|
per gradient block, all nine blocks.  Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

from bodyfitting_amd import _lib, assets
from bodyfitting_amd import native as N
from bodyfitting_amd import synthetic as S
from oracle import smplify_oracle as O
from width_variants import Variants

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 3, 5, 8, 9, 17, 64)        # the 1-, 2-, 4- and 8-frame instances of the mesh reverse and their tails
CASES = ("vertices", "joints", "joints_all", "full_pose", "all")
INPUTS = ("betas", "global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose", "expression")
COT_ARG = {"vertices": "dverts", "joints": "djoints", "joints_all": "djoints_all", "full_pose": "dfull_pose"}
ROW_MARGIN = 1e-3                         # degrees between -yaw and the nearest rounding boundary of the contour row
ATOL = 3e-6
FIT_TOL = 1e-4
BF_ERR_INVALID, BF_ERR_UNSUPPORTED = -1, -3      # include/bodyfit.h


def _params(n, seed, ne=10):
    """tests/test_gpu_smplx_autograd.py: _params, draw for draw, then expression ~ N(0, 0.7) with frame 0 exactly zero"""
    rng = np.random.default_rng(seed)
    p = {"betas": rng.normal(0, 0.7, (n, 10)), "global_orient": rng.normal(0, 0.8, (n, 3)), "body_pose": rng.normal(0, 0.3, (n, 63)),
         "jaw_pose": rng.normal(0, 0.2, (n, 3)), "leye_pose": rng.normal(0, 0.2, (n, 3)), "reye_pose": rng.normal(0, 0.2, (n, 3)),
         "left_hand_pose": rng.normal(0, 0.4, (n, 6)), "right_hand_pose": rng.normal(0, 0.4, (n, 6))}
    p["expression"] = rng.normal(0, 0.7, (n, ne))
    p = {k: v.astype(np.float32) for k, v in p.items()}
    for k in ("jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose", "expression"):
        p[k][0] = 0.0
    if n > 1:
        p["global_orient"][1] = np.array([0.6, -0.48, 0.64], np.float32) * 3.13
        p["body_pose"][1, 45:48] = np.array([-0.28, 0.96, 0.0], np.float32) * 3.1
        p["jaw_pose"][1] = np.array([0.8, 0.0, -0.6], np.float32) * 3.12
        p["left_hand_pose"][1] = np.array([1.2, -0.9, 1.0, 0.8, -1.1, 0.7], np.float32)
        p["right_hand_pose"][1] = np.array([-1.0, 1.1, -0.8, 0.9, 1.2, -0.7], np.float32)
    return p


def _oracle(m, p, dtype, grad=False, mapped=False):
    x = {k: torch.tensor(p[k], dtype=dtype, requires_grad=grad) for k in INPUTS}
    out = O.smplx_forward(m, x["betas"], x["global_orient"], x["body_pose"], x["leye_pose"], x["reye_pose"], x["left_hand_pose"],
                          x["right_hand_pose"], jaw_pose=x["jaw_pose"], expression=x["expression"], mapped=mapped)
    return x, out


def row_margin(m64, ref):
    """degrees between -yaw of the oracle's neck chain and the nearest rounding boundary of the contour row, per frame"""
    n = ref["full_pose"].shape[0]
    R = O.batch_rodrigues(ref["full_pose"].detach().reshape(-1, 3)).view(n, -1, 3, 3)
    rel = torch.eye(3, dtype=torch.float64).unsqueeze(0).expand(n, -1, -1)
    for j in m64["neck_kin_chain"]:
        rel = torch.bmm(R[:, int(j)], rel)
    deg = (-torch.atan2(-rel[:, 2, 0], torch.sqrt(rel[:, 0, 0] ** 2 + rel[:, 1, 0] ** 2)) * 180.0 / np.pi).numpy()
    return np.abs(deg - np.floor(deg) - 0.5)


def _check_rows(m64, ref, got_rows):
    """dyn_row of the device == the fp64 oracle's for EVERY frame; the inputs must sit away from a rounding boundary"""
    margin = row_margin(m64, ref)
    assert (margin >= ROW_MARGIN).all(), ("a frame sits on a rounding boundary of the contour row: pick another seed", margin.min())
    assert got_rows.dtype == np.int32
    np.testing.assert_array_equal(got_rows, ref["dyn_row"].numpy())


def _cotangents(n, dev, seed):
    rng = np.random.default_rng(seed + 100)
    return {"vertices": rng.normal(0, 1, (n, dev.n_verts, 3)).astype(np.float32),
            "joints": rng.normal(0, 1, (n, dev.n_joint_map, 3)).astype(np.float32),
            "joints_all": rng.normal(0, 1, (n, dev.n_joints_all, 3)).astype(np.float32),
            "full_pose": rng.normal(0, 1, (n, 3 * dev.n_joints)).astype(np.float32)}


def _torch_grads(model, dtype, p, cot):
    """per case: torch autograd of O.smplx_forward in `dtype` -> the nine gradient blocks as float64 numpy"""
    m = O.to_torch_model(model, dtype)
    x, out = _oracle(m, p, dtype, grad=True, mapped=False)
    xm, mapped = _oracle(m, p, dtype, grad=True, mapped=True)
    res = {}
    for case in CASES:
        keys = ("vertices", "joints", "joints_all", "full_pose") if case == "all" else (case,)
        g = [np.zeros(p[k].shape) for k in INPUTS]
        for k in keys:
            src, xs = (mapped["joints"], xm) if k == "joints" else (out["joints" if k == "joints_all" else k], x)
            gk = torch.autograd.grad((src * torch.as_tensor(cot[k], dtype=dtype)).sum(), [xs[i] for i in INPUTS], retain_graph=True,
                                     allow_unused=True)
            g = [a if b is None else a + b.detach().numpy().astype(np.float64) for a, b in zip(g, gk)]
        res[case] = g
    return res


def _band_check(name, got, f32, f64):
    err = float(np.abs(got.astype(np.float64) - f64).max())
    ref_err = float(np.abs(f32 - f64).max())
    band = 4 * ref_err + 1e-6 * float(np.abs(f64).max())
    share = err / band if band > 0 else 0.0
    print(f"{name}: {share:.3f} of the band (error {err:.3g}, torch fp32's {ref_err:.3g}, max |g| {float(np.abs(f64).max()):.3g})")
    assert err <= band, (name, err, ref_err, band)
    return share


def _forward_against_oracle(dev, model, p):
    m64 = O.to_torch_model(model, torch.float64)
    got = dev.forward_smplx(**p)
    _, ref = _oracle(m64, p, torch.float64, mapped=False)
    _, ref_m = _oracle(m64, p, torch.float64, mapped=True)
    _check_rows(m64, ref, got["dyn_row"])
    for name, want in (("vertices", ref["vertices"]), ("joints", ref_m["joints"]), ("joints_all", ref["joints"]), ("full_pose", ref["full_pose"])):
        print(f"{name}: max |HIP - fp64| {float(np.abs(got[name] - want.numpy()).max()):.3g}")
    np.testing.assert_allclose(got["vertices"], ref["vertices"].numpy(), rtol=0, atol=ATOL)
    np.testing.assert_allclose(got["joints"], ref_m["joints"].numpy(), rtol=0, atol=ATOL)
    np.testing.assert_allclose(got["joints_all"], ref["joints"].numpy(), rtol=0, atol=ATOL)
    np.testing.assert_allclose(got["full_pose"], ref["full_pose"].numpy(), rtol=0, atol=ATOL)
    # expression moved the mesh and the chain joints (the frames past the first: frame 0's is zero)
    if len(p["betas"]) > 1:
        plain = dev.forward_smplx(**{k: v for k, v in p.items() if k != "expression"})
        assert float(np.abs(plain["vertices"][1:] - got["vertices"][1:]).max()) > 1e-2
        assert float(np.abs(plain["joints_all"][1:, :55] - got["joints_all"][1:, :55]).max()) > 1e-3


def _vjp_against_autograd(dev, model, n, seed, ne=10):
    p = _params(n, seed, ne)
    cot = _cotangents(n, dev, seed)
    m64 = O.to_torch_model(model, torch.float64)
    _check_rows(m64, _oracle(m64, p, torch.float64)[1], dev.forward_smplx(**p)["dyn_row"])
    g64 = _torch_grads(model, torch.float64, p, cot)
    g32 = _torch_grads(model, torch.float32, p, cot)
    worst = 0.0
    for case in CASES:
        kw = {COT_ARG[k]: cot[k] for k in COT_ARG if case in (k, "all")}
        got = dev.vjp_smplx(**p, **kw)
        assert len(got) == 9
        for i, name in enumerate(INPUTS):
            assert got[i].dtype == np.float32 and got[i].shape == g64[case][i].shape
            worst = max(worst, _band_check(f"n={n} {case} d{name}", got[i], g32[case][i], g64[case][i]))
    print(f"n={n}: worst error at {worst:.2f} of the band")


@pytest.fixture(scope="module")
def full():
    model = S.make_model("smplx", seed=0)
    dev = N.DeviceModel(model, S.make_gmm(seed=0), device=0)
    assert dev.n_expression == 10 and dev.n_verts == 10475           # 40 tiles of the expression kernels + 235 vertices
    yield model, dev
    dev.close()


@pytest.fixture(scope="module")
def small():
    model = S.make_model("smplx", seed=0, nv=1200)        # 38 tiles: the split single-frame instance of the mesh reverse
    dev = N.DeviceModel(model, S.make_gmm(seed=0), device=0)
    assert dev.n_expression == 10 and dev.n_verts == 1200
    yield model, dev
    dev.close()


@pytest.fixture(scope="module")
def variants(gmm):
    v = Variants(gmm)
    yield v
    v.close()


@pytest.mark.parametrize("n", [1, 5])
def test_forward_matches_the_oracle(full, n):
    model, dev = full
    _forward_against_oracle(dev, model, _params(n, 300 + n))


def test_forward_without_expression_is_the_old_call_and_zeros_change_no_value(full):
    model, dev = full
    p = _params(5, 305)
    del p["expression"]
    plain = dev.forward_smplx(**p)
    none = dev.forward_smplx(**p, expression=None)
    zeros = dev.forward_smplx(**p, expression=np.zeros((5, 10), np.float32))
    for k in ("vertices", "joints", "joints_all", "full_pose", "dyn_row"):
        assert plain[k].tobytes() == none[k].tobytes(), k
        np.testing.assert_array_equal(zeros[k], plain[k], err_msg=k)
    # the reverse too: None is the eight-gradient call, bit for bit
    cot = _cotangents(5, dev, 305)
    a = dev.vjp_smplx(**p, dverts=cot["vertices"], djoints_all=cot["joints_all"])
    b = dev.vjp_smplx(**p, dverts=cot["vertices"], djoints_all=cot["joints_all"], expression=None)
    assert len(a) == 8 and len(b) == 8
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_vjp_small_model_matches_fp64_autograd(small, n):
    model, dev = small
    _vjp_against_autograd(dev, model, n, seed=50 + n)


@pytest.mark.parametrize("n", [1, 9, 64])
def test_vjp_full_model_matches_fp64_autograd(full, n):
    model, dev = full
    _vjp_against_autograd(dev, model, n, seed=n)


@pytest.mark.parametrize("name", ["smplx_B8", "smplx_BD"])
def test_skinning_widths_forward_and_vjp(variants, name):
    """v_nnz 8 and 0 (dense rows): the expression kernels' other two skinning paths"""
    model, dev = variants.get(name)
    assert dev.n_expression == 10
    _forward_against_oracle(dev, model, _params(3, 403))
    _vjp_against_autograd(dev, model, 3, seed=403)


def test_three_expression_coefficients(small):
    """shapedirs[:, :, :13]: a model with three expression directions - no hard-coded 10, no padding read as a coefficient"""
    model = dict(small[0], shapedirs=np.ascontiguousarray(small[0]["shapedirs"][:, :, :13]))
    dev = N.DeviceModel(model, S.make_gmm(seed=0), device=0)
    try:
        assert dev.n_expression == 3
        _forward_against_oracle(dev, model, _params(2, 52, ne=3))
        _vjp_against_autograd(dev, model, 2, seed=52, ne=3)
    finally:
        dev.close()


def test_extra_regressor_joints_follow_the_updated_vertices(small):
    """An SMPL-X-kind model WITH J_regressor_extra rows (the ABI allows it; tests/test_gpu_smplx.py has one): the mesh pass sums those
    joints per tile in front of the expression's vertex delta, so they are formed again behind it.  Rows over two tiles each, mapped
    into the 135 joints; forward and VJP at n = 3."""
    model = dict(small[0])
    nv = model["v_template"].shape[0]
    rng = np.random.default_rng(11)
    reg = np.zeros((3, nv), np.float32)
    for r in range(3):
        ids = rng.choice(nv, size=12, replace=False)
        w = rng.uniform(0.2, 1.0, size=12)
        reg[r, ids] = w / w.sum()
    model["J_regressor_extra"] = reg
    jm = np.asarray(model["joint_map"]).copy()
    jm[jm >= 76] += 3                                  # all-joints layout: chain 55 | selector 21 | extra 3 | landmarks
    jm[[1, 8, 15]] = [76, 77, 78]
    model["joint_map"] = jm
    dev = N.DeviceModel(model, S.make_gmm(seed=0), device=0)
    try:
        assert dev.n_expression == 10 and dev.n_joints_all == 147
        p = _params(3, 53)
        _forward_against_oracle(dev, model, p)
        plain = dev.forward_smplx(**{k: v for k, v in p.items() if k != "expression"})
        assert float(np.abs(plain["joints_all"][1:, 76:79] - dev.forward_smplx(**p)["joints_all"][1:, 76:79]).max()) > 1e-3
        _vjp_against_autograd(dev, model, 3, seed=53)
    finally:
        dev.close()


def test_vjp_is_deterministic_and_dexpression_is_optional(full):
    model, dev = full
    n = 9
    p = _params(n, 7)
    cot = _cotangents(n, dev, 7)
    kw = {COT_ARG[k]: cot[k] for k in COT_ARG}
    a = dev.vjp_smplx(**p, **kw)
    b = dev.vjp_smplx(**p, **kw)
    c = dev.vjp_smplx(**p, **kw, want_dexpression=False)            # dexpression = NULL
    assert len(a) == 9 and c[8] is None
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(a[:8], c[:8]):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("n", [1, 3])
def test_vjp_optional_gradients_at_the_c_abi(small, n):
    """bf_smplx_vjp_expr on this file's small model with one gradient asked for and every other NULL: dbetas only, dglobal_orient
    only, the left hand only, dexpression only.  The one asked for holds the bits of the all-gradients call; none asked for succeeds"""
    _, dev = small
    p = _params(n, 140 + n)
    cot = _cotangents(n, dev, 140 + n)
    full = dev.vjp_smplx(**p, **{COT_ARG[k]: cot[k] for k in COT_ARG})
    assert len(full) == 9 and all(np.isfinite(g).all() for g in full) and full[6].any() and full[8].any()
    par = _lib.SmplxParams(*[_lib.fptr(p[k]) for k in INPUTS[:8]])
    cots = _lib.SmplxCotangents(*[_lib.fptr(cot[k]) for k in ("vertices", "joints", "joints_all", "full_pose")])

    def call(which):
        out = [np.full_like(g, np.nan) if i in which else None for i, g in enumerate(full)]
        dst = _lib.SmplxGrads(*[_lib.fptr(o) for o in out[:8]])
        before = N.dev_route_stats()["host_calls"]
        rc = dev._lib.bf_smplx_vjp_expr(dev._h, n, C.byref(par), _lib.fptr(p["expression"]), C.byref(cots), C.byref(dst), _lib.fptr(out[8]))
        assert rc == 0 and N.dev_route_stats()["host_calls"] == before + 1, which
        return out

    for which in ((0,), (1,), (6,), (8,), ()):
        for i, got in enumerate(call(which)):
            if i in which:
                assert got.tobytes() == full[i].tobytes(), (which, i)


def test_refusals_at_the_c_abi_and_in_python(small, dev_model, monkeypatch):
    lib = dev_model._lib
    dirs = np.ascontiguousarray(small[0]["shapedirs"][:, :, 10:], np.float32)
    z = {"betas": np.zeros((1, 10), np.float32), "global_orient": np.zeros((1, 3), np.float32), "body_pose": np.zeros((1, 63), np.float32)}
    par = _lib.SmplxParams(*[_lib.fptr(z[k]) for k in ("betas", "global_orient", "body_pose")])
    out, cotz, gr = _lib.SmplxOutputs(), _lib.SmplxCotangents(), _lib.SmplxGrads()
    expr = np.full((1, 10), 0.1, np.float32)
    # an SMPL model
    assert dev_model.n_expression == 0 and lib.bf_model_n_expression(dev_model._h) == 0
    smpl_dirs = np.zeros((dev_model.n_verts, 3, 10), np.float32)
    assert lib.bf_model_set_expression(dev_model._h, 10, _lib.fptr(smpl_dirs)) == BF_ERR_UNSUPPORTED
    assert b"SMPL-X-kind" in lib.bf_last_error()
    assert lib.bf_smplx_forward_expr(dev_model._h, 1, C.byref(par), _lib.fptr(expr), C.byref(out)) == BF_ERR_UNSUPPORTED
    assert lib.bf_smplx_vjp_expr(dev_model._h, 1, C.byref(par), _lib.fptr(expr), C.byref(cotz), C.byref(gr), None) == BF_ERR_UNSUPPORTED
    with pytest.raises(_lib.BodyfitError):
        dev_model.forward_smplx(**z, expression=expr)
    # an SMPL-X model registered with its 10 shape directions only: no directions attached
    bare = N.DeviceModel(dict(small[0], shapedirs=np.ascontiguousarray(small[0]["shapedirs"][:, :, :10])), S.make_gmm(seed=0), device=0)
    try:
        assert bare.n_expression == 0 and lib.bf_model_n_expression(bare._h) == 0
        assert lib.bf_smplx_forward_expr(bare._h, 1, C.byref(par), _lib.fptr(expr), C.byref(out)) == BF_ERR_UNSUPPORTED
        assert b"bf_model_set_expression" in lib.bf_last_error()
        dexpr = np.zeros((1, 10), np.float32)
        assert lib.bf_smplx_vjp_expr(bare._h, 1, C.byref(par), _lib.fptr(expr), C.byref(cotz), C.byref(gr), _lib.fptr(dexpr)) == BF_ERR_UNSUPPORTED
        assert b"bf_model_set_expression" in lib.bf_last_error()
        with pytest.raises(_lib.BodyfitError, match="expression"):
            bare.forward_smplx(**z, expression=expr)
        with pytest.raises(_lib.BodyfitError, match="expression"):
            bare.vjp_smplx(**z, dverts=np.zeros((1, 1200, 3), np.float32), expression=expr)
        # the drop-in on it behaves as before: zeros pass and are ignored, anything else is refused
        monkeypatch.setattr(assets, "_MODELS", {("smplx", "neutral"): small[0]})
        monkeypatch.setattr(assets, "_DEVICE_MODELS", {("smplx", "neutral", 0): bare})
        from bodyfitting_amd import smplx as X
        body = X.create(model_type="smplx", use_face_contour=True, num_expression_coeffs=10)
        assert body._dev is bare and body.num_expression_coeffs == 0
        plain = body(**z)
        np.testing.assert_array_equal(body(**z, expression=np.zeros((1, 10), np.float32)).vertices, plain.vertices)
        with pytest.raises(ValueError, match="expression"):
            body(**z, expression=expr)
        # n_expr 0 and 17, then a first and a second attachment
        big = np.zeros((1200, 3, 17), np.float32)
        assert lib.bf_model_set_expression(bare._h, 0, _lib.fptr(dirs)) == BF_ERR_UNSUPPORTED
        assert lib.bf_model_set_expression(bare._h, 17, _lib.fptr(big)) == BF_ERR_UNSUPPORTED
        assert lib.bf_model_n_expression(bare._h) == 0
        assert lib.bf_model_set_expression(bare._h, 10, _lib.fptr(dirs)) == 0
        assert lib.bf_model_n_expression(bare._h) == 10
        assert lib.bf_model_set_expression(bare._h, 10, _lib.fptr(dirs)) == BF_ERR_INVALID
        # ... and the directions attached by hand are the ones a model dict with 20 columns brings
        bare.n_expression = 10
        got, want = bare.forward_smplx(**z, expression=expr), small[1].forward_smplx(**z, expression=expr)
        assert got["vertices"].tobytes() == want["vertices"].tobytes() and got["joints_all"].tobytes() == want["joints_all"].tobytes()
    finally:
        bare.close()


def _landmark_loop(forward, psi0, jaw0, steps=30):
    """Adam(lr=1e-2) on expression and jaw against the target landmarks; forward(psi, jaw) -> the summed squared landmark distance.
    -> (final psi, final jaw, the losses, was expression.grad there after the first backward)"""
    psi, jaw = psi0.clone().requires_grad_(True), jaw0.clone().requires_grad_(True)
    opt = torch.optim.Adam([psi, jaw], lr=1e-2)
    losses, had_grad = [], None
    for _ in range(steps):
        opt.zero_grad()
        loss = forward(psi, jaw)
        loss.backward()
        if had_grad is None:
            had_grad = psi.grad is not None
        losses.append(float(loss.detach()))
        opt.step()
    with torch.no_grad():
        losses.append(float(forward(psi, jaw)))
    return psi.detach().double().numpy(), jaw.detach().double().numpy(), losses, had_grad


def test_adam_on_expression_and_jaw_against_the_face_landmarks(small, monkeypatch):
    """The loop a user writes on the drop-in: target = the fp64 oracle's 68 landmarks at a drawn expression and jaw pose, start at
    zero, 30 Adam steps through smplx.create(...) - the final coefficients stay within FIT_TOL of the same loop through the fp64
    oracle (torch fp32 through the oracle stays 1.4e-6 from it)."""
    model, dev = small
    monkeypatch.setattr(assets, "_MODELS", {("smplx", "neutral"): model})
    monkeypatch.setattr(assets, "_DEVICE_MODELS", {("smplx", "neutral", 0): dev})
    from bodyfitting_amd import smplx as X
    body = X.create(model_path="data", model_type="smplx", use_face_contour=True, num_expression_coeffs=10, dtype=torch.float32)
    assert body._dev is dev and body.num_expression_coeffs == 10
    rng = np.random.default_rng(900)
    fixed = {"betas": rng.normal(0, 0.7, (1, 10)), "global_orient": rng.normal(0, 0.8, (1, 3)), "body_pose": rng.normal(0, 0.3, (1, 63))}
    fixed = {k: v.astype(np.float32) for k, v in fixed.items()}
    psi_t, jaw_t = rng.normal(0, 0.7, (1, 10)).astype(np.float32), rng.normal(0, 0.2, (1, 3)).astype(np.float32)
    m64 = O.to_torch_model(model, torch.float64)
    f64 = {k: torch.tensor(v, dtype=torch.float64) for k, v in fixed.items()}
    zeros = lambda w: torch.zeros(1, w, dtype=torch.float64)       # noqa: E731

    def oracle(psi, jaw):
        return O.smplx_forward(m64, f64["betas"], f64["global_orient"], f64["body_pose"], zeros(3), zeros(3), zeros(6), zeros(6), jaw_pose=jaw,
                               expression=psi, mapped=False)

    ref = oracle(torch.tensor(psi_t, dtype=torch.float64), torch.tensor(jaw_t, dtype=torch.float64))
    margin = row_margin(m64, ref)
    assert (margin >= ROW_MARGIN).all(), margin
    target = ref["joints"][:, -68:].detach()
    want_psi, want_jaw, want_losses, _ = _landmark_loop(lambda psi, jaw: (oracle(psi, jaw)["joints"][:, -68:] - target).square().sum(),
                                                        torch.zeros(1, 10, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.float64))
    f32 = {k: torch.tensor(v) for k, v in fixed.items()}
    target32 = target.float()
    got_psi, got_jaw, losses, had_grad = _landmark_loop(
        lambda psi, jaw: (body(**f32, expression=psi, jaw_pose=jaw).joints[:, -68:] - target32).square().sum(),
        torch.zeros(1, 10), torch.zeros(1, 3))
    print(f"loss {losses[0]:.6g} -> {losses[-1]:.6g} (fp64 oracle loop: {want_losses[0]:.6g} -> {want_losses[-1]:.6g}); "
          f"max |expression - fp64 loop| {float(np.abs(got_psi - want_psi).max()):.3g}, jaw {float(np.abs(got_jaw - want_jaw).max()):.3g}; "
          f"moved: expression {float(np.abs(got_psi).max()):.3g}, jaw {float(np.abs(got_jaw).max()):.3g}")
    assert had_grad, "expression.grad is None after the first backward: the input was ignored"
    assert losses[-1] < losses[0]
    np.testing.assert_allclose(got_psi, want_psi, rtol=0, atol=FIT_TOL)
    np.testing.assert_allclose(got_jaw, want_jaw, rtol=0, atol=FIT_TOL)
