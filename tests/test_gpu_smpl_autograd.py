"""The differentiable drop-in models.smpl.SMPL on the MI355X: bf_smpl_vjp (DeviceModel.vjp) against float64 torch autograd of the
oracle's smplx forward, its determinism, the torch path's parity with the numpy path, and the oracle's restatement of the reference
loop (smplify.py:177-213, torch Adam) run with its SMPL forward swapped for the HIP model under torch autograd.

Band of the VJP (the convention of tests/test_gpu_hmr.py): max|HIP - fp64| <= 4 * max|torch fp32 - fp64| + 1e-6 * max|fp64|."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from bodyfitting_amd import _lib, assets, model_files
from bodyfitting_amd import native as N
from bodyfitting_amd import synthetic as S
from oracle import smplify_oracle as O

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 3, 5, 8, 9, 17, 64)        # the 1-, 2-, 4- and 8-frame instances of the mesh reverse and their tails
CASES = ("vertices", "joints", "joints_ori", "all")
PARAMS = ("global_transl", "scale", "pose", "betas", "global_orient")
FIT_TOL = 1e-4


def _params(n, nb, seed):
    rng = np.random.default_rng(seed)
    betas = rng.normal(0, 0.7, (n, nb)).astype(np.float32)
    orient = rng.normal(0, 0.8, (n, 3)).astype(np.float32)
    pose = rng.normal(0, 0.3, (n, 69)).astype(np.float32)
    orient[0] = 0.0                       # theta = 0: the Rodrigues singular point (angle = ||1e-8||)
    pose[0] = 0.0
    if n > 1:                             # |theta| near pi
        orient[1] = np.array([0.6, -0.48, 0.64], np.float32) * 3.13
        pose[1, 0:3] = np.array([0.0, 0.8, -0.6], np.float32) * 3.14
        pose[1, 45:48] = np.array([-0.28, 0.96, 0.0], np.float32) * 3.1
    return betas, orient, pose


def _cotangents(n, dev, seed):
    rng = np.random.default_rng(seed + 100)
    return {"vertices": rng.normal(0, 1, (n, dev.n_verts, 3)).astype(np.float32),
            "joints": rng.normal(0, 1, (n, dev.n_joint_map, 3)).astype(np.float32),
            "joints_ori": rng.normal(0, 1, (n, dev.n_joints + dev.n_selector, 3)).astype(np.float32)}


def _torch_grads(model, dtype, betas, orient, pose, cot):
    """per case: torch autograd of O.smpl_forward in `dtype` -> (dbetas, dorient, dpose) as float64 numpy"""
    m = O.to_torch_model(model, dtype)
    x = [torch.tensor(a, dtype=dtype, requires_grad=True) for a in (betas, orient, pose)]
    out = O.smpl_forward(m, *x)
    res = {}
    for case in CASES:
        keys = ("vertices", "joints", "joints_ori") if case == "all" else (case,)
        total = sum((out[k] * torch.as_tensor(cot[k], dtype=dtype)).sum() for k in keys)
        g = torch.autograd.grad(total, x, retain_graph=True, allow_unused=True)
        res[case] = [np.zeros(xi.shape) if gi is None else gi.detach().numpy().astype(np.float64) for gi, xi in zip(g, x)]
    return res


def _band_check(name, got, f32, f64):
    err = float(np.abs(got.astype(np.float64) - f64).max())
    ref_err = float(np.abs(f32 - f64).max())
    band = 4 * ref_err + 1e-6 * float(np.abs(f64).max())
    assert err <= band, (name, err, ref_err, band)
    return err / band


def _vjp_against_autograd(dev, model, n, seed):
    betas, orient, pose = _params(n, dev.n_betas, seed)
    cot = _cotangents(n, dev, seed)
    g64 = _torch_grads(model, torch.float64, betas, orient, pose, cot)
    g32 = _torch_grads(model, torch.float32, betas, orient, pose, cot)
    worst = 0.0
    for case in CASES:
        kw = {"dverts": None, "djoints": None, "djoints_ori": None}
        for k, arg in (("vertices", "dverts"), ("joints", "djoints"), ("joints_ori", "djoints_ori")):
            if case in (k, "all"):
                kw[arg] = cot[k]
        got = dev.vjp(betas, orient, pose, **kw)
        for i, name in enumerate(("dbetas", "dglobal_orient", "dbody_pose")):
            assert got[i].dtype == np.float32 and got[i].shape == g64[case][i].shape
            worst = max(worst, _band_check(f"n={n} {case} {name}", got[i], g32[case][i], g64[case][i]))
    print(f"n={n}: worst error at {worst:.2f} of the band")


@pytest.fixture(scope="module")
def small():
    model = S.make_model("smpl", seed=0, nv=690)          # 22 tiles: the split single-frame path of the mesh reverse
    dev = N.DeviceModel(model, S.make_gmm(seed=0), device=0)
    yield model, dev
    dev.close()


@pytest.fixture(scope="module")
def kid():
    model = S.make_model("smpl", seed=0)
    kid = model_files.kid_model(model, S.make_kid_template(model))
    dev = N.DeviceModel(kid, S.make_gmm(seed=0), device=0)
    yield kid, dev
    dev.close()


@pytest.mark.parametrize("n", SIZES)
def test_vjp_full_model_matches_fp64_autograd(dev_model, smpl_model, n):
    _vjp_against_autograd(dev_model, smpl_model, n, seed=n)


@pytest.mark.parametrize("n", SIZES)
def test_vjp_small_model_matches_fp64_autograd(small, n):
    model, dev = small
    _vjp_against_autograd(dev, model, n, seed=50 + n)


@pytest.mark.parametrize("n", SIZES)
def test_vjp_kid_model_matches_fp64_autograd(kid, n):
    model, dev = kid
    assert dev.n_betas == 11
    _vjp_against_autograd(dev, model, n, seed=90 + n)


@pytest.mark.parametrize("n", [1, 3])
def test_vjp_optional_gradients_at_the_c_abi(small, n):
    """bf_smpl_vjp on the 690-vertex model with one gradient asked for and the others NULL: dbetas only, dglobal_orient only,
    dbody_pose only.  The one asked for holds the bits of the all-gradients call; none asked for succeeds and counts once"""
    _, dev = small
    betas, orient, pose = _params(n, dev.n_betas, 130 + n)
    cot = _cotangents(n, dev, 130 + n)
    full = dev.vjp(betas, orient, pose, cot["vertices"], cot["joints"], cot["joints_ori"])
    assert all(np.isfinite(g).all() and g.any() for g in full)

    def call(which):
        out = [np.full_like(g, np.nan) if i in which else None for i, g in enumerate(full)]
        before = N.dev_route_stats()["host_calls"]
        rc = dev._lib.bf_smpl_vjp(dev._h, n, _lib.fptr(betas), _lib.fptr(orient), _lib.fptr(pose), _lib.fptr(cot["vertices"]),
                                  _lib.fptr(cot["joints"]), _lib.fptr(cot["joints_ori"]), *[_lib.fptr(o) for o in out])
        assert rc == 0 and N.dev_route_stats()["host_calls"] == before + 1, which
        return out

    for which in ((0,), (1,), (2,), ()):
        for i, got in enumerate(call(which)):
            assert (got is None) == (i not in which)
            if got is not None:
                assert got.tobytes() == full[i].tobytes(), (which, i)


def test_vjp_is_deterministic_and_refuses_smplx(dev_model):
    n = 9
    betas, orient, pose = _params(n, 10, 7)
    cot = _cotangents(n, dev_model, 7)
    a = dev_model.vjp(betas, orient, pose, cot["vertices"], cot["joints"], cot["joints_ori"])
    b = dev_model.vjp(betas, orient, pose, cot["vertices"], cot["joints"], cot["joints_ori"])
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    model = S.make_model("smplx", seed=0, nv=1200)
    dev = N.DeviceModel(model, S.make_gmm(seed=0), device=0)
    try:
        with pytest.raises(_lib.BodyfitError):
            dev.vjp(np.zeros((1, 10)), np.zeros((1, 3)), np.zeros((1, 3 * (dev.n_joints - 1))), np.zeros((1, dev.n_verts, 3)))
    finally:
        dev.close()


@pytest.fixture
def dropin(smpl_model, gmm, monkeypatch):
    monkeypatch.setattr(assets, "_MODELS", {("smpl", "neutral"): smpl_model})
    monkeypatch.setattr(assets, "_GMM", {"gmm": gmm})
    monkeypatch.setattr(assets, "_DEVICE_MODELS", {})
    from bodyfitting_amd.smpl import SMPL
    smpl = SMPL(gender="neutral").to(torch.device("cpu"))          # (smplify.py:51-56's construction line)
    yield smpl
    for d in list(assets._DEVICE_MODELS.values()):
        d.close()


def test_torch_path_matches_numpy_path_and_the_vjp(dropin):
    n = 5
    betas, orient, pose = _params(n, 10, 11)
    ref = dropin(betas=betas, global_orient=orient, body_pose=pose)
    x = [torch.tensor(a, requires_grad=True) for a in (betas, orient, pose)]
    out = dropin(betas=x[0], global_orient=x[1], body_pose=x[2])
    for k in ("vertices", "joints", "joints_ori"):
        assert getattr(out, k).dtype == torch.float32
        np.testing.assert_array_equal(getattr(out, k).detach().numpy(), getattr(ref, k))
    cot = _cotangents(n, dropin._dev, 11)
    total = sum((getattr(out, k) * torch.as_tensor(cot[k])).sum() for k in ("vertices", "joints", "joints_ori"))
    total.backward()
    want = dropin._dev.vjp(betas, orient, pose, cot["vertices"], cot["joints"], cot["joints_ori"])
    for xi, w in zip(x, want):
        np.testing.assert_array_equal(xi.grad.numpy(), w)


def _fit_through_dropin(monkeypatch, dropin, smpl_model, gmm_bufs, prob, iters, snapshots):
    def shim(m, betas, global_orient, body_pose):
        out = dropin(betas=betas, global_orient=global_orient, body_pose=body_pose)
        return {"vertices": out.vertices, "joints": out.joints, "joints_ori": out.joints_ori, "full_pose": out.full_pose}
    monkeypatch.setattr(O, "smpl_forward", shim)
    return O.fit(smpl_model, gmm_bufs, prob, iters, snapshots=snapshots)


def test_oracle_loop_on_the_hip_model_holds_cfg1(monkeypatch, dropin, smpl_model, gmm_bufs):
    g = load_golden("cfg1_1view_50it.npz")
    prob = S.make_problem(smpl_model, frame=0, n_views=1)
    res = _fit_through_dropin(monkeypatch, dropin, smpl_model, gmm_bufs, prob, 50, (1, 10, 50))
    for k in (1, 10, 50):
        for n in PARAMS:
            np.testing.assert_allclose(res["snapshots"][k][n], g[f"it{k}_{n}"], rtol=0, atol=FIT_TOL, err_msg=f"it{k} {n}")


@pytest.mark.parametrize("frame", [0, 1, 2, 3])
def test_oracle_loop_on_the_hip_model_holds_cfg2(monkeypatch, dropin, smpl_model, gmm_bufs, frame):
    g = load_golden(f"cfg2_48view_100it_f{frame}.npz")
    prob = S.make_problem(smpl_model, frame=frame, n_views=48)
    res = _fit_through_dropin(monkeypatch, dropin, smpl_model, gmm_bufs, prob, 100, (1, 2, 10, 50, 100))
    for k in (1, 2, 10, 50, 100):
        for n in PARAMS:
            np.testing.assert_allclose(res["snapshots"][k][n], g[f"it{k}_{n}"], rtol=0, atol=FIT_TOL, err_msg=f"it{k} {n}")
    # rtn_dict's global_transl = t * s: frame 3's is the ill-conditioned one, banded as tests/test_gpu_parity.py does
    band = FIT_TOL
    err = float(np.abs(res["global_transl"] - g["final_global_transl"]).max())
    if frame == 3:
        import ref_drift as RD
        sens = load_golden("sens_cfg2_48view_100it.npz")
        owns = [float(np.abs(sens[f"{v}_f3_final_global_transl"] - g["final_global_transl"]).max()) for v in RD.VARIANTS]
        own = max(owns)
        assert 1e-4 < own < 3e-4, own
        band = max(FIT_TOL, RD.K * own)
        print("cfg2 frame 3 global_transl:", RD.position(err, owns))
    np.testing.assert_allclose(res["global_transl"], g["final_global_transl"], atol=band)


# --------------------------------------------------------------------------------------------------------------------------------
# the joint-angle sweep through the reverse of the chain (tests/model_sweep_cases.py): vjp_rodrigues from 1e-6 rad to beyond 4 pi
# --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["smpl", "kid"])
def test_vjp_over_the_angle_sweep_matches_fp64_autograd_frame_by_frame(kind):
    """every angle, axis and joint set of axis R as the frames of one batch of the 690-vertex model, cotangents "all" and "joints":
    _band_check's band per FRAME and gradient block, and once more on the pose-gradient row of every swept joint against that row's
    own float64 maximum and float32 error (a block-wide maximum would wave a lone small joint's error through)"""
    import model_sweep_cases as MS
    model = MS.model(kind)
    dev = N.DeviceModel(model, S.make_gmm(seed=0), device=0)
    try:
        p, n = MS.params(kind), len(MS.frames(kind))
        cot = _cotangents(n, dev, 400)
        args = (p["betas"], p["global_orient"], p["body_pose"])
        g64 = _torch_grads(model, torch.float64, *args, cot)
        g32 = _torch_grads(model, torch.float32, *args, cot)
        for case in ("all", "joints"):
            kw = {arg: cot[k] if case in (k, "all") else None for k, arg in (("vertices", "dverts"), ("joints", "djoints"), ("joints_ori", "djoints_ori"))}
            got = dev.vjp(*args, **kw)
            MS.check_vjp(kind, case, ["betas", "global_orient", "body_pose"], got, g32[case], g64[case])
        MS.report(kind)
    finally:
        dev.close()
