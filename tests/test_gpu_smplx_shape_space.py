"""SMPL-X with more than 10 betas and more than 16 expression coefficients on the MI355X: bf_model_set_shape_space and the kernels of
shape_ext_kernels.hip behind DeviceModel.forward_smplx / vjp_smplx, against the float64 oracle's smplx forward and its torch autograd.

Models: the 1,200-vertex synthetic SMPL-X model widened once to (300, 100) (synthetic.widen_shape_space) and cut to each shape space,
so every space shares its columns with the others.  Parameters: tests/test_gpu_smplx_expression.py's draws for the same seed - the
contour row depends on the pose alone, so its row margins hold here - with the betas beyond the tenth and the expression beyond the
tenth ~ N(0, 0.7) drawn behind them from a generator of their own; frame 0's expression stays exactly zero.

Forward: ATOL = 3e-6, the project's.  VJP: max|HIP - fp64| <= 4 * max|torch fp32 - fp64| + 1e-6 * max|fp64| per gradient block, all
nine blocks, every cotangent case.  Every test prints its figures before it asserts.
The wide kernels walk the directions for blocks of 8 frames (BF_EXT_FB): 1, 8, 9 and 64 frames are a lone frame, a full block, a
block with a one-frame tail and eight blocks."""
import ctypes as C

import numpy as np
import pytest
import torch

from bodyfitting_amd import _lib, assets
from bodyfitting_amd import native as N
from bodyfitting_amd import synthetic as S
from oracle import smplify_oracle as O
from test_gpu_smplx_expression import (ATOL, CASES, COT_ARG, FIT_TOL, INPUTS, ROW_MARGIN, _band_check, _check_rows, _cotangents, row_margin)
from test_gpu_smplx_expression import _params as _base_params
from width_variants import Variants

pytestmark = pytest.mark.gpu
BF_ERR_INVALID, BF_ERR_UNSUPPORTED = -1, -3      # include/bodyfit.h
# (10,17): the first width the kernels behind bf_model_set_expression refuse; (16,10): 16 directions - those kernels behind the pack;
# (26,48) / (26,49): 64 and 65 directions, the two sides of a wave; (300,0): betas alone, expression=None
SPACES = [(10, 17), (16, 10), (16, 50), (26, 48), (26, 49), (300, 100), (300, 0)]
WIDE = {(10, 17): True, (16, 10): False, (16, 50): True, (26, 48): True, (26, 49): True, (300, 100): True, (300, 0): True}


def _params(n, seed, nb, ne):
    """the draws of tests/test_gpu_smplx_expression.py, then betas[:, 10:] and expression[:, 10:] from a generator of their own"""
    p = _base_params(n, seed, 10)
    rng = np.random.default_rng(seed + 77000)
    more_b, more_e = rng.normal(0, 0.7, (n, 290)).astype(np.float32), rng.normal(0, 0.7, (n, 90)).astype(np.float32)
    more_e[0] = 0.0
    p["betas"] = np.ascontiguousarray(np.concatenate([p["betas"], more_b], axis=1)[:, :nb])
    p["expression"] = np.ascontiguousarray(np.concatenate([p["expression"], more_e], axis=1)[:, :ne])
    if ne == 0:
        del p["expression"]
    return p


def _oracle(m, p, dtype, grad=False, mapped=False):
    x = {k: torch.tensor(p[k], dtype=dtype, requires_grad=grad) for k in INPUTS if k in p}
    out = O.smplx_forward(m, x["betas"], x["global_orient"], x["body_pose"], x["leye_pose"], x["reye_pose"], x["left_hand_pose"],
                          x["right_hand_pose"], jaw_pose=x["jaw_pose"], expression=x.get("expression"), mapped=mapped)
    return x, out


def _torch_grads(model, dtype, p, cot):
    """per case: torch autograd of O.smplx_forward in `dtype` -> the gradient blocks (eight, or nine with expression) as float64 numpy"""
    m = O.to_torch_model(model, dtype)
    names = [k for k in INPUTS if k in p]
    x, out = _oracle(m, p, dtype, grad=True, mapped=False)
    xm, mapped = _oracle(m, p, dtype, grad=True, mapped=True)
    res = {}
    for case in CASES:
        keys = ("vertices", "joints", "joints_all", "full_pose") if case == "all" else (case,)
        g = [np.zeros(p[k].shape) for k in names]
        for k in keys:
            src, xs = (mapped["joints"], xm) if k == "joints" else (out["joints" if k == "joints_all" else k], x)
            gk = torch.autograd.grad((src * torch.as_tensor(cot[k], dtype=dtype)).sum(), [xs[i] for i in names], retain_graph=True,
                                     allow_unused=True)
            g = [a if b is None else a + b.detach().numpy().astype(np.float64) for a, b in zip(g, gk)]
        res[case] = g
    return res


def _forward_against_oracle(dev, model, p):
    m64 = O.to_torch_model(model, torch.float64)
    got = dev.forward_smplx(**p)
    _, ref = _oracle(m64, p, torch.float64, mapped=False)
    _, ref_m = _oracle(m64, p, torch.float64, mapped=True)
    _check_rows(m64, ref, got["dyn_row"])
    pairs = (("vertices", ref["vertices"]), ("joints", ref_m["joints"]), ("joints_all", ref["joints"]), ("full_pose", ref["full_pose"]))
    for name, want in pairs:
        print(f"{name}: max |HIP - fp64| {float(np.abs(got[name] - want.numpy()).max()):.3g}")
    for name, want in pairs:
        np.testing.assert_allclose(got[name], want.numpy(), rtol=0, atol=ATOL, err_msg=name)
    return got


def _vjp_against_autograd(dev, model, p, seed):
    n = len(p["betas"])
    names = [k for k in INPUTS if k in p]
    cot = _cotangents(n, dev, seed)
    g64 = _torch_grads(model, torch.float64, p, cot)
    g32 = _torch_grads(model, torch.float32, p, cot)
    worst = 0.0
    for case in CASES:
        kw = {COT_ARG[k]: cot[k] for k in COT_ARG if case in (k, "all")}
        got = dev.vjp_smplx(**p, **kw)
        assert len(got) == len(names)
        for i, name in enumerate(names):
            assert got[i].dtype == np.float32 and got[i].shape == g64[case][i].shape, (name, got[i].shape)
            worst = max(worst, _band_check(f"n={n} {case} d{name}", got[i], g32[case][i], g64[case][i]))
    print(f"n={n}: worst error at {worst:.2f} of the band")


@pytest.fixture(scope="module")
def base():
    return S.make_model("smplx", seed=0, nv=1200)


@pytest.fixture(scope="module")
def spaces(base):
    """(nb, ne) -> (model dict, DeviceModel), made on first use, all cut from one (300, 100) widening"""
    big = S.widen_shape_space(base, 300, 100, seed=0)
    made = {}

    def get(nb, ne):
        if (nb, ne) not in made:
            model = S.widen_shape_space(big, nb, ne)
            dev = N.DeviceModel(model, S.make_gmm(seed=0), device=0)
            assert (dev.n_betas, dev.n_core_betas, dev.n_expression, dev.n_verts) == (nb, 10, ne, 1200)
            assert dev.shape_ext_wide == WIDE[(nb, ne)]
            made[(nb, ne)] = (model, dev)
        return made[(nb, ne)]

    yield get
    for _, dev in made.values():
        dev.close()


@pytest.mark.parametrize("nb,ne", SPACES)
def test_shape_spaces_forward_and_all_gradient_blocks(spaces, nb, ne):
    """n = 9: a full frame block and a one-frame tail"""
    model, dev = spaces(nb, ne)
    p = _params(9, 59, nb, ne)
    got = _forward_against_oracle(dev, model, p)
    # the coefficients beyond the core ten moved the mesh
    core = dict(p, betas=np.ascontiguousarray(np.pad(p["betas"][:, :10], ((0, 0), (0, nb - 10)))))
    if ne:
        core["expression"] = np.zeros_like(p["expression"])
    assert float(np.abs(dev.forward_smplx(**core)["vertices"][1:] - got["vertices"][1:]).max()) > 1e-2
    _vjp_against_autograd(dev, model, p, 59)


@pytest.mark.parametrize("n", [1, 8, 64])
def test_frame_counts_at_16_50(spaces, n):
    model, dev = spaces(16, 50)
    p = _params(n, 50 + n, 16, 50)
    _forward_against_oracle(dev, model, p)
    _vjp_against_autograd(dev, model, p, 50 + n)


@pytest.mark.parametrize("n", [7, 17])
def test_frame_counts_at_300_100(spaces, n):
    """below a frame block, and two blocks with a tail, at the full width"""
    model, dev = spaces(300, 100)
    seed = {7: 55, 17: 67}[n]                  # (every frame at least 0.009 degrees from a rounding boundary of the contour row; _check_rows asserts it)
    p = _params(n, seed, 300, 100)
    _forward_against_oracle(dev, model, p)
    _vjp_against_autograd(dev, model, p, seed)


def test_full_size_model_at_16_50():
    """10,475 vertices: 41 tiles of the wide kernels, the last with 235 vertices; n = 2"""
    model = S.widen_shape_space(S.make_model("smplx", seed=0), 16, 50, seed=0)
    dev = N.DeviceModel(model, S.make_gmm(seed=0), device=0)
    try:
        assert (dev.n_verts, dev.n_betas, dev.n_expression, dev.shape_ext_wide) == (10475, 16, 50, True)
        p = _params(2, 52, 16, 50)
        _forward_against_oracle(dev, model, p)
        _vjp_against_autograd(dev, model, p, 52)
    finally:
        dev.close()


@pytest.fixture(scope="module")
def variants(gmm):
    v = Variants(gmm)
    yield v
    v.close()


@pytest.mark.parametrize("name", ["smplx_B8", "smplx_BD"])
def test_skinning_widths(variants, name):
    """v_nnz 8 and 0 (dense rows): for_each_bone's other two paths in the wide kernels, n = 3"""
    model = S.widen_shape_space(variants.get(name)[0], 16, 50, seed=0)
    dev = N.DeviceModel(model, S.make_gmm(seed=0), device=0)
    try:
        assert dev.shape_ext_wide
        p = _params(3, 403, 16, 50)
        _forward_against_oracle(dev, model, p)
        _vjp_against_autograd(dev, model, p, 403)
    finally:
        dev.close()


def test_extra_regressor_joints_follow_the_updated_vertices(base):
    """a model with J_regressor_extra rows (tests/test_gpu_smplx_expression.py's): their per-tile sums are formed again behind the
    wide vertex delta; n = 3"""
    model = S.widen_shape_space(base, 16, 50, seed=0)
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
        assert dev.n_joints_all == 147 and dev.shape_ext_wide
        p = _params(3, 53, 16, 50)
        _forward_against_oracle(dev, model, p)
        _vjp_against_autograd(dev, model, p, 53)
    finally:
        dev.close()


def test_switch_sends_the_default_model_through_the_wide_kernels(base, monkeypatch):
    """BF_SHAPE_EXT_WIDE=1, read at the attachment: the (10, 10) model on the wide kernels meets the same tolerances; the forward adds
    in the narrow kernels' order, so its bits are theirs"""
    narrow = N.DeviceModel(base, S.make_gmm(seed=0), device=0)
    monkeypatch.setenv("BF_SHAPE_EXT_WIDE", "1")
    wide = N.DeviceModel(base, S.make_gmm(seed=0), device=0)
    monkeypatch.delenv("BF_SHAPE_EXT_WIDE")
    try:
        assert not narrow.shape_ext_wide and wide.shape_ext_wide and (wide.n_betas, wide.n_expression) == (10, 10)
        for n, seed in ((1, 51), (9, 59)):
            p = _params(n, seed, 10, 10)
            got = _forward_against_oracle(wide, base, p)
            assert got["vertices"].tobytes() == narrow.forward_smplx(**p)["vertices"].tobytes()
            _vjp_against_autograd(wide, base, p, seed)
    finally:
        narrow.close()
        wide.close()


def test_equal_inputs_give_equal_bits_and_gradients_are_optional(spaces):
    """two identical calls; then bf_smplx_vjp_expr with dbetas only and dexpression only: the bits of the all-gradients call"""
    _, dev = spaces(16, 50)
    n = 9
    p = _params(n, 7, 16, 50)
    cot = _cotangents(n, dev, 7)
    kw = {COT_ARG[k]: cot[k] for k in COT_ARG}
    a, b = dev.vjp_smplx(**p, **kw), dev.vjp_smplx(**p, **kw)
    assert len(a) == 9 and a[0].shape == (n, 16) and a[8].shape == (n, 50) and a[0][:, 10:].any() and a[8][:, 10:].any()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    f1, f2 = dev.forward_smplx(**p), dev.forward_smplx(**p)
    assert all(f1[k].tobytes() == f2[k].tobytes() for k in f1)
    c = dev.vjp_smplx(**p, **kw, want_dexpression=False)
    assert c[8] is None and all(x.tobytes() == y.tobytes() for x, y in zip(a[:8], c[:8]))
    par = _lib.SmplxParams(*[_lib.fptr(p[k]) for k in INPUTS[:8]])
    cots = _lib.SmplxCotangents(*[_lib.fptr(cot[k]) for k in ("vertices", "joints", "joints_all", "full_pose")])
    for which in ((0,), (8,), (1,), ()):
        out = [np.full_like(g, np.nan) if i in which else None for i, g in enumerate(a)]
        dst = _lib.SmplxGrads(*[_lib.fptr(o) for o in out[:8]])
        rc = dev._lib.bf_smplx_vjp_expr(dev._h, n, C.byref(par), _lib.fptr(p["expression"]), C.byref(cots), C.byref(dst), _lib.fptr(out[8]))
        assert rc == 0, which
        for i in which:
            assert out[i].tobytes() == a[i].tobytes(), (which, i)


def test_refusals_at_the_c_abi(base, dev_model):
    lib = dev_model._lib
    wide = S.widen_shape_space(base, 16, 50, seed=0)
    dirs = np.ascontiguousarray(wide["shapedirs"][:, :, 10:], np.float32)                # [NV, 3, 56]
    big = np.zeros((1200, 3, 400), np.float32)
    core = dict(base, shapedirs=np.ascontiguousarray(base["shapedirs"][:, :, :10]))

    def bare():
        dev = N.DeviceModel(core, S.make_gmm(seed=0), device=0)
        assert (dev.n_betas, dev.n_expression, lib.bf_model_n_betas(dev._h)) == (10, 0, 10)
        return dev

    # an SMPL model
    assert lib.bf_model_set_shape_space(dev_model._h, 16, 50, _lib.fptr(np.zeros((dev_model.n_verts, 3, 56), np.float32))) == BF_ERR_UNSUPPORTED
    assert b"SMPL-X-kind" in lib.bf_last_error()
    assert lib.bf_model_n_betas(dev_model._h) == dev_model.n_betas and lib.bf_model_n_betas(None) == 0
    m = bare()
    try:
        # the ranges: 10..300 betas, 0..100 expression coefficients, at least one direction; NULL
        for nb, ne in ((9, 10), (301, 10), (16, -1), (16, 101), (10, 0)):
            assert lib.bf_model_set_shape_space(m._h, nb, ne, _lib.fptr(big)) == BF_ERR_UNSUPPORTED, (nb, ne)
        assert lib.bf_model_set_shape_space(m._h, 16, 50, None) == BF_ERR_INVALID
        assert (lib.bf_model_n_betas(m._h), lib.bf_model_n_expression(m._h)) == (10, 0)
        # attached once; then neither call again
        assert lib.bf_model_set_shape_space(m._h, 16, 50, _lib.fptr(dirs)) == 0
        assert (lib.bf_model_n_betas(m._h), lib.bf_model_n_expression(m._h), lib.bf_model_shape_ext_wide(m._h)) == (16, 50, 1)
        assert lib.bf_model_set_shape_space(m._h, 16, 50, _lib.fptr(dirs)) == BF_ERR_INVALID
        assert lib.bf_model_set_expression(m._h, 10, _lib.fptr(dirs)) == BF_ERR_INVALID
        # dexpression without expression; expression == NULL is zero coefficients
        m.n_betas, m.n_expression = 16, 50
        p = _params(2, 52, 16, 50)
        par = _lib.SmplxParams(*[_lib.fptr(p[k]) for k in INPUTS[:8]])
        cot = _cotangents(2, m, 52)
        cots = _lib.SmplxCotangents(_lib.fptr(cot["vertices"]), None, None, None)
        dexpr = np.zeros((2, 50), np.float32)
        assert lib.bf_smplx_vjp_expr(m._h, 2, C.byref(par), None, C.byref(cots), C.byref(_lib.SmplxGrads()), _lib.fptr(dexpr)) == BF_ERR_INVALID
        zero = dict(p, expression=np.zeros((2, 50), np.float32))
        none = {k: v for k, v in p.items() if k != "expression"}
        assert m.forward_smplx(**none)["vertices"].tobytes() == m.forward_smplx(**zero)["vertices"].tobytes()
        a, b = m.vjp_smplx(**none, dverts=cot["vertices"]), m.vjp_smplx(**zero, dverts=cot["vertices"])
        assert len(a) == 8 and a[0].shape == (2, 16) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b[:8]))
    finally:
        m.close()
    m = bare()
    try:
        # the other order
        assert lib.bf_model_set_expression(m._h, 10, _lib.fptr(np.ascontiguousarray(base["shapedirs"][:, :, 10:]))) == 0
        assert lib.bf_model_set_shape_space(m._h, 16, 50, _lib.fptr(dirs)) == BF_ERR_INVALID
        assert (lib.bf_model_n_betas(m._h), lib.bf_model_n_expression(m._h), lib.bf_model_shape_ext_wide(m._h)) == (10, 10, 0)
    finally:
        m.close()


def test_device_route_gives_the_host_routes_bits(tmp_path):
    """(16, 50) on GPU tensors, in a fresh process that imports torch first (tests/shape_space_child.py): the host route's bits at 1, 9
    and 65 frames, and a repeated call adds no workspace allocation"""
    import conftest
    import shape_space_child
    if conftest.FRESH is None:
        pytest.skip("no fork server")
    out = str(tmp_path / "out.npz")
    proc = conftest.FRESH.Process(target=shape_space_child.same_bits, args=(out,))
    proc.start()
    proc.join(300)
    if proc.is_alive():
        proc.terminate()
        pytest.fail("the child hung")
    err = tmp_path / "out.npz.err"
    assert proc.exitcode == 0, "exit code %s\n%s" % (proc.exitcode, err.read_text() if err.exists() else "")


def _loop(forward, betas0, psi0, steps=30):
    """Adam(lr=1e-2) on betas and expression; forward(betas, psi) -> the loss.  -> (betas, psi, the losses, both had a gradient)"""
    betas, psi = betas0.clone().requires_grad_(True), psi0.clone().requires_grad_(True)
    opt = torch.optim.Adam([betas, psi], lr=1e-2)
    losses, had = [], None
    for _ in range(steps):
        opt.zero_grad()
        loss = forward(betas, psi)
        loss.backward()
        if had is None:
            had = betas.grad is not None and psi.grad is not None and bool(betas.grad[:, 10:].any()) and bool(psi.grad[:, 10:].any())
        losses.append(float(loss.detach()))
        opt.step()
    with torch.no_grad():
        losses.append(float(forward(betas, psi)))
    return betas.detach().double().numpy(), psi.detach().double().numpy(), losses, had


@pytest.mark.parametrize("nb,ne", [(16, 50), (300, 100)])
def test_adam_on_betas_and_expression_against_the_vertices(spaces, monkeypatch, nb, ne):
    """The loop a user writes: smplx.create(num_betas=, num_expression_coeffs=), target = the fp64 oracle's vertices at coefficients
    ~ N(0, 0.7), betas and expression from zero, 30 Adam steps - the final coefficients stay within FIT_TOL of the same loop through the
    fp64 oracle (torch fp32 through the oracle ends 1.4e-6 from it)."""
    model, dev = spaces(nb, ne)
    monkeypatch.setattr(assets, "_MODELS", {("smplx", "neutral"): model})
    monkeypatch.setattr(assets, "_DEVICE_MODELS", {("smplx", "neutral", 0): dev})
    from bodyfitting_amd import smplx as X
    body = X.create(model_path="data", model_type="smplx", use_face_contour=True, num_betas=nb, num_expression_coeffs=ne, dtype=torch.float32)
    assert body._dev is dev and (body.num_betas, body.num_expression_coeffs) == (nb, ne)
    rng = np.random.default_rng(900)
    fixed = {"global_orient": rng.normal(0, 0.8, (1, 3)).astype(np.float32), "body_pose": rng.normal(0, 0.3, (1, 63)).astype(np.float32)}
    betas_t, psi_t = rng.normal(0, 0.7, (1, nb)), rng.normal(0, 0.7, (1, ne))
    m64 = O.to_torch_model(model, torch.float64)
    f64 = {k: torch.tensor(v, dtype=torch.float64) for k, v in fixed.items()}
    zeros = lambda w: torch.zeros(1, w, dtype=torch.float64)       # noqa: E731

    def oracle(betas, psi):
        return O.smplx_forward(m64, betas, f64["global_orient"], f64["body_pose"], zeros(3), zeros(3), zeros(6), zeros(6), expression=psi,
                               mapped=False)

    ref = oracle(torch.tensor(betas_t), torch.tensor(psi_t))
    assert (row_margin(m64, ref) >= ROW_MARGIN).all()
    target = ref["vertices"].detach()
    want_b, want_p, want_losses, _ = _loop(lambda b, e: (oracle(b, e)["vertices"] - target).square().sum(), zeros(nb), zeros(ne))
    f32 = {k: torch.tensor(v) for k, v in fixed.items()}
    target32 = target.float()
    got_b, got_p, losses, had = _loop(lambda b, e: (body(**f32, betas=b, expression=e).vertices - target32).square().sum(),
                                      torch.zeros(1, nb), torch.zeros(1, ne))
    print(f"({nb},{ne}) loss {losses[0]:.6g} -> {losses[-1]:.6g} (fp64 oracle loop: {want_losses[0]:.6g} -> {want_losses[-1]:.6g}); "
          f"max |betas - fp64 loop| {float(np.abs(got_b - want_b).max()):.3g}, expression {float(np.abs(got_p - want_p).max()):.3g}; "
          f"moved: betas {float(np.abs(got_b).max()):.3g}, expression {float(np.abs(got_p).max()):.3g}")
    assert had, "a gradient is missing or zero beyond the tenth coefficient after the first backward"
    assert losses[-1] < losses[0]
    np.testing.assert_allclose(got_b, want_b, rtol=0, atol=FIT_TOL)
    np.testing.assert_allclose(got_p, want_p, rtol=0, atol=FIT_TOL)
