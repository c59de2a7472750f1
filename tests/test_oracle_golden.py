"""The oracle restatement against goldens produced by the imported reference (oracle/gen_golden.py)."""
import numpy as np
import pytest
import torch

import ref_drift as RD
from conftest import load_golden
from bodyfitting_amd import synthetic as S
from oracle import smplify_oracle as O

PARAMS = ("global_transl", "scale", "pose", "betas", "global_orient")


def test_model_generator_is_stable(smpl_model):
    g = load_golden("cfg2_48view_100it_f0.npz")
    assert S.model_digest(smpl_model) == str(g["model_digest"])


def test_cfg1_one_view_50_iters(smpl_model, gmm_bufs):
    """BASELINE config 1: 1 frame, 1 view, 50 iterations of the reference loop."""
    torch.set_num_threads(1)
    g = load_golden("cfg1_1view_50it.npz")
    prob = S.make_problem(smpl_model, frame=0, n_views=1)
    trace = []
    res = O.fit(smpl_model, gmm_bufs, prob, 50, snapshots=(1, 10, 50), trace=trace)
    for k in (1, 10, 50):
        for n in PARAMS:
            np.testing.assert_allclose(res["snapshots"][k][n], g[f"it{k}_{n}"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(res["joints"], g["joints"], atol=5e-6)
    np.testing.assert_allclose(res["vertices"][::53], g["vertices_sample"], atol=5e-6)
    assert trace[-1][0] < trace[0][0]        # the objective went down


def test_cfg2_48_views_100_iters(smpl_model, gmm_bufs):
    """BASELINE config 2 against the reference: parameters after 1/2/10/50/100 Adam steps."""
    torch.set_num_threads(1)
    g = load_golden("cfg2_48view_100it_f1.npz")
    prob = S.make_problem(smpl_model, frame=1, n_views=48)
    res = O.fit(smpl_model, gmm_bufs, prob, 100, snapshots=(1, 2, 10, 50, 100))
    for k in (1, 2, 10, 50, 100):
        for n in PARAMS:
            np.testing.assert_allclose(res["snapshots"][k][n], g[f"it{k}_{n}"], rtol=0, atol=5e-6)
    np.testing.assert_allclose(res["global_transl"], g["final_global_transl"], atol=5e-6)
    np.testing.assert_allclose(res["full_pose"], g["full_pose"], atol=5e-6)


def test_ragged_views(smpl_model, gmm_bufs):
    """views without a detection are skipped but still counted in the divisor (loss.py:157,197)."""
    torch.set_num_threads(1)
    g = load_golden("ragged_8view_20it.npz")
    prob = S.make_problem(smpl_model, frame=5, n_views=8, missing_views=tuple(g["missing_views"]))
    res = O.fit(smpl_model, gmm_bufs, prob, 20, snapshots=(1, 20))
    for k in (1, 20):
        for n in PARAMS:
            np.testing.assert_allclose(res["snapshots"][k][n], g[f"it{k}_{n}"], rtol=0, atol=2e-6)


def test_loss_terms_and_gradient(smpl_model, gmm_bufs):
    """the four-term dict of loss.py:219-224 and the autograd gradient, fp32 reference vs fp64 oracle."""
    g = load_golden("loss_terms_f0.npz")
    prob = S.make_problem(smpl_model, frame=0, n_views=48)
    params = {k: g[f"param_{k}"].astype(np.float64) for k in PARAMS}
    loss, terms, grads, joints, verts = O.loss_and_grad(smpl_model, gmm_bufs, prob, params)
    assert loss == pytest.approx(float(g["loss"]), rel=1e-6)
    for k, v in terms.items():
        assert v == pytest.approx(float(g[f"term_{k}"]), rel=1e-6)
    for k in PARAMS:
        scale = np.abs(grads[k]).max()
        np.testing.assert_allclose(grads[k], g[f"grad_{k}"], atol=2e-6 * scale)
    np.testing.assert_allclose(joints, g["joints"], atol=5e-6)


def test_known_answers(smpl_model):
    """identity pose => vertices == v_template + S beta; joints regress from the shaped mesh."""
    m = O.to_torch_model(smpl_model, torch.float64)
    betas = torch.linspace(-1, 1, 10, dtype=torch.float64)[None]
    out = O.smpl_forward(m, betas, torch.zeros(1, 3, dtype=torch.float64), torch.zeros(1, 69, dtype=torch.float64))
    shaped = m["v_template"] + torch.einsum("l,mkl->mk", betas[0], m["shapedirs"])
    np.testing.assert_allclose(out["vertices"][0].numpy(), shaped.numpy(), atol=1e-7)
    J = m["J_regressor"] @ shaped
    np.testing.assert_allclose(out["joints_ori"][0, :24].numpy(), J.numpy(), atol=1e-7)
    # GMoF -> r^2 for sigma -> inf; zero residual -> zero loss
    r = torch.tensor([0.5, -2.0], dtype=torch.float64)
    assert torch.allclose(O.gmof(r, 1e9), r * r, rtol=1e-9)
    assert float(O.gmof(torch.zeros(1), 100.0)) == 0.0
    # single camera at identity => closed-form pinhole projection
    pts = torch.tensor([[[0.1, -0.2, 2.0]]], dtype=torch.float64)
    K = torch.tensor([[500.0, 0, 256], [0, 500, 256], [0, 0, 1]], dtype=torch.float64)
    uv = O.perspective_projection(pts, torch.eye(3, dtype=torch.float64)[None], torch.zeros(1, 3, dtype=torch.float64), K)
    np.testing.assert_allclose(uv[0, 0].numpy(), [256 + 500 * 0.05, 256 - 500 * 0.1], atol=1e-9)


@pytest.mark.parametrize("variant", ("base",) + RD.SCAN_VARIANTS)
def test_cfg5_goldens_match_todays_generator(variant):
    """config 5 as stated (oracle/gen_golden.py cfg5_goldens) is held on the GPU against these files, whose scan is not stored but
    regenerated: each one must still describe today's model and frame-0 scan, and hold every snapshot the GPU test reads"""
    g = load_golden(RD.CFG5 % variant)
    model = S.make_model("smplx", seed=0)
    _, sv, sf = S.make_scan_problem_smplx(model, frame=0, n_views=48)
    assert str(g["model_digest"]) == S.model_digest(model)
    assert str(g["scan_digest"]) == S.scan_digest(sv, sf)
    assert int(g["num_iters"]) == 300 and int(g["n_views"]) == 48 and int(g["frame"]) == 0
    want = {f"it{k}_{n}" for k in (1, 100, 101, 102, 103, 300) for n in O.SMPLX_PARAMS}
    want |= {f"it{k}_loss_{n}" for k in (1, 100, 101, 102, 103, 300)
             for n in ("total", "reprojection_loss", "pose_prior_loss", "angle_prior_loss", "shape_prior_loss")}
    want |= {f"it{k}_loss_pc_loss" for k in (102, 103, 300)}               # (the scan loss is active from step 102 on)
    want |= {f"disp{k}_sample" for k in (1, 10, 300)} | {"vertices", "joints", "full_pose", "displacement", "wall_s", "threads"}
    assert want <= set(g.files), sorted(want - set(g.files))
    assert not {f"it{k}_loss_pc_loss" for k in (1, 100, 101)} & set(g.files)
    nv = model["v_template"].shape[0]
    assert g["vertices"].shape == (nv, 3) and g["displacement"].shape == (nv, 3) and g["joints"].shape == (135, 3)
    for k in O.SMPLX_PARAMS:
        assert np.isfinite(g[f"it300_{k}"]).all()
