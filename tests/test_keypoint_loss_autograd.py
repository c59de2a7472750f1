"""`smplify.loss.multiview_keypoint_loss` and `smplify.prior.MaxMixturePrior` of the drop-in packages (bodyfitting_amd/loss.py,
bodyfitting_amd/prior.py) on the CPU: signatures, import names, buffers, the autograd Function, what is accepted and what is
refused - with `native.keypoint_loss` / `native.Gmm` replaced by a float64 stand-in over oracle.smplify_oracle (the HIP kernel
itself is held to the same oracle in tests/test_gpu_keypoint_loss.py)."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import keypoint_loss_cases as KC
from bodyfitting_amd import assets, native
from bodyfitting_amd import synthetic as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACE_MAPPING = list(range(17, 17 + 51)) + list(range(0, 17))          # loss.py:20, spelled out


@pytest.fixture
def L(monkeypatch, gmm):
    """bodyfitting_amd.loss with the stand-in behind the native call, float64 let through (gradcheck needs it)"""
    from bodyfitting_amd import loss, prior
    monkeypatch.setattr(native, "keypoint_loss", KC.stand_in_keypoint_loss)
    monkeypatch.setattr(native, "Gmm", KC.StandInGmm)
    monkeypatch.setattr(assets, "_GMM", {"gmm": gmm})
    monkeypatch.setattr(prior, "_require_float32", lambda who, name, x: None)
    return loss


@pytest.fixture
def prior(L):
    from bodyfitting_amd.prior import MaxMixturePrior
    return MaxMixturePrior()


def _smpl_inputs(seed=0, n_views=4, absent=(1,), dtype=torch.float64):
    sc = KC.scene(49, n_views, seed)
    rng = np.random.default_rng(seed + 7)
    keypoints = [None if v in absent else {"pose": sc["kp"][v][:25]} for v in range(n_views)]
    x = [torch.tensor(sc["joints"], dtype=dtype, requires_grad=True), torch.tensor(rng.normal(0, 0.2, (1, 69)), dtype=dtype, requires_grad=True),
         torch.tensor(rng.normal(0, 0.6, (1, 10)), dtype=dtype, requires_grad=True)]
    return sc, keypoints, x


def _smplx_inputs(seed=1, n_views=3, dtype=torch.float64):
    """view 0: all four groups, view 1: no left hand and no face, view 2: absent"""
    sc = KC.scene(135, n_views, seed)
    rng = np.random.default_rng(seed + 7)
    keypoints = []
    for v in range(n_views):
        face70 = np.zeros((70, 3), np.float32)
        face70[FACE_MAPPING] = sc["kp"][v][67:135]
        face70[68:] = rng.uniform(0, 500, (2, 3))                          # the pupils: never read
        k = {"pose": sc["kp"][v][:25], "hand_left": sc["kp"][v][25:46], "hand_right": sc["kp"][v][46:67], "face": face70}
        if v == 1:
            del k["hand_left"], k["face"]
        keypoints.append(None if v == 2 else k)
    x = [torch.tensor(sc["joints"], dtype=dtype, requires_grad=True), torch.tensor(rng.normal(0, 0.2, (1, 63)), dtype=dtype, requires_grad=True),
         torch.tensor(rng.normal(0, 0.6, (1, 10)), dtype=dtype, requires_grad=True)]
    return sc, keypoints, x


def _literal(sc, keypoints, joints, poses, betas, n_use, gmm_bufs, use_hand_face, imsize=512, sigma=100, wp=4.78, wa=15.2, ws=5):
    """loss.py:139-224 restated line by line in float64 torch - the hands' and the face's confidences keep their trailing axis, as
    in the reference, so every joint of such a group is weighted by the group's summed squared confidences"""
    from oracle import smplify_oracle as O

    def rep(cord, k, squeeze):
        k = torch.tensor(np.asarray(k, np.float64))
        conf = k[:, 2] if squeeze else k[:, 2:3]
        err = O.gmof((k[:, :2] - cord) / (imsize / 1024), sigma)
        return ((conf ** 2) * err.sum(-1)).sum(-1)

    body, hand, face = [], [], []
    for i in range(n_use):
        k = keypoints[i]
        if k is None:
            continue
        w = torch.tensor(sc["w2c"][i], dtype=torch.float64)
        uv = O.perspective_projection(joints, w[None, :3, :3], w[None, :3, 3], torch.tensor(sc["K"][i], dtype=torch.float64))[0]
        body.append(rep(uv[:25], k["pose"], True))
        if use_hand_face:
            if "hand_left" in k:
                hand.append(rep(uv[25:46], k["hand_left"], False))
            if "hand_right" in k:
                hand.append(rep(uv[46:67], k["hand_right"], False))
            if "face" in k:
                face.append(rep(uv[67:], np.asarray(k["face"])[FACE_MAPPING], False))
    loss_2d = torch.stack(body).sum() / n_use
    if use_hand_face:
        loss_2d = loss_2d + torch.cat(hand).sum() / n_use + torch.cat(face).sum() / n_use
        poses = torch.cat([poses, torch.zeros_like(poses[:, :6])], -1)
    terms = [loss_2d, wp ** 2 * O.gmm_merged_nll(poses, *O.to_torch_gmm(gmm_bufs, torch.float64)), wa ** 2 * O.angle_prior(poses).sum(-1),
             ws ** 2 * (betas ** 2).sum(-1)]
    return torch.stack([t.reshape(()) for t in terms])


def test_signatures_are_the_references():
    from bodyfitting_amd.loss import multiview_keypoint_loss
    from bodyfitting_amd.prior import MaxMixturePrior
    sig = [(p.name, p.default) for p in inspect.signature(multiview_keypoint_loss).parameters.values()]
    E = inspect.Parameter.empty
    assert sig == [("w2cs", E), ("Ks", E), ("keypoints", E), ("model_joints", E), ("poses", E), ("betas", E), ("use_frames", E),
                   ("pose_prior", E), ("sigma", 100), ("shape_prior_weight", 5), ("angle_prior_weight", 15.2), ("output", "sum"),
                   ("debug", False), ("imsize", 512), ("pose_prior_weight", 4.78), ("use_hand_face", False), ("output_folder", None),
                   ("verts", None), ("device", None)]                      # (the reference's list, loss.py:139-141, plus `device`)
    init = inspect.signature(MaxMixturePrior.__init__).parameters
    assert [(p.name, str(p.default), p.kind) for p in init.values()] == [
        ("self", str(E), inspect.Parameter.POSITIONAL_OR_KEYWORD), ("prior_folder", "prior", inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("num_gaussians", "6", inspect.Parameter.POSITIONAL_OR_KEYWORD), ("dtype", str(torch.float32), inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("epsilon", "1e-16", inspect.Parameter.POSITIONAL_OR_KEYWORD), ("use_merged", "True", inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("kwargs", str(E), inspect.Parameter.VAR_KEYWORD)]                 # prior.py:102-105
    for name in ("forward", "merged_log_likelihood"):
        assert list(inspect.signature(getattr(MaxMixturePrior, name)).parameters) == ["self", "pose", "betas"]


def test_dropin_packages_resolve_by_the_reference_import_names():
    """`from smplify.loss import multiview_keypoint_loss`, `from smplify.prior import MaxMixturePrior` (smplify.py's import lines)
    with dropin/ first on sys.path, in a child process; importing them does not import torch"""
    code = """
import os, sys
import bodyfitting_amd
root = os.path.dirname(bodyfitting_amd.__file__)
sys.path.insert(0, os.path.join(root, "dropin"))
from smplify.loss import multiview_keypoint_loss
from smplify.prior import MaxMixturePrior
import smplify.loss as SL
import bodyfitting_amd.loss as L, bodyfitting_amd.prior as P
assert multiview_keypoint_loss is L.multiview_keypoint_loss and MaxMixturePrior is P.MaxMixturePrior
assert SL.__file__.startswith(os.path.join(root, "dropin")), SL.__file__
assert SL.SKELETON_LENGTH == 25 and SL.HANDS_LENGTH == 42 and SL.FACE_LENGTH == 68 and len(SL.FACE_MAPPING) == 68
for name in ("perspective_projection", "gmof", "angle_prior", "reprojection_loss", "multview_mask_loss", "extract_countours"):
    assert getattr(SL, name) is getattr(L, name), name
assert "torch" not in sys.modules
print("ok")
"""
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=REPO, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


def test_prior_buffers_to_and_refusals(prior, gmm):
    from bodyfitting_amd.prior import MaxMixturePrior
    means, precisions, nll_weights = S.gmm_buffers(gmm)
    np.testing.assert_array_equal(prior.means, means)
    np.testing.assert_array_equal(prior.precisions, precisions)
    np.testing.assert_array_equal(np.asarray(prior.nll_weights).reshape(-1), nll_weights)
    assert prior.means.dtype == np.float32 and prior.random_var_dim == 69
    assert prior.to(torch.device("cpu")) is prior and prior.to("cpu", dtype=torch.float32) is prior
    assert MaxMixturePrior(prior_folder="prior", num_gaussians=8, dtype=torch.float32) is not None      # smplify.py:46's line
    with pytest.raises(ValueError):
        MaxMixturePrior(use_merged=False)
    for bad in (torch.float64, torch.float16, np.float64):
        with pytest.raises(ValueError):
            MaxMixturePrior(dtype=bad)


def test_prior_alone_is_the_merged_likelihood_and_differentiable(prior, gmm_bufs):
    from oracle import smplify_oracle as O
    rng = np.random.default_rng(3)
    pose = torch.tensor(np.asarray(gmm_bufs[0], np.float64)[[0, 3, 7]] + rng.normal(0, 0.05, (3, 69)), requires_grad=True)
    got = prior(pose, None)
    assert got.shape == (3,)
    want = O.gmm_merged_nll(pose, *O.to_torch_gmm(gmm_bufs, torch.float64))
    torch.testing.assert_close(got, want, atol=1e-9, rtol=1e-12)
    assert torch.autograd.gradcheck(lambda p: prior(p, None), (pose,), eps=1e-6, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(prior.forward(pose, None), prior.merged_log_likelihood(pose, None))
    # numpy in, numpy out; 63 dofs are zero-padded
    a = prior(pose.detach().numpy(), None)
    assert isinstance(a, np.ndarray) and a.shape == (3,)
    np.testing.assert_allclose(a, want.detach().numpy(), rtol=1e-12)
    p63 = pose.detach()[:, :63]
    torch.testing.assert_close(prior(p63, None), O.gmm_merged_nll(torch.cat([p63, torch.zeros(3, 6, dtype=p63.dtype)], -1),
                                                                     *O.to_torch_gmm(gmm_bufs, torch.float64)), atol=1e-9, rtol=1e-12)


def test_smpl_value_gradcheck_and_an_absent_view(L, prior, gmm_bufs):
    sc, keypoints, x = _smpl_inputs()
    use_frames = [10, 11, 12, 13]

    def f(j, p, b):
        return L.multiview_keypoint_loss(torch.tensor(sc["w2c"]), sc["K"], keypoints, j, p, b, use_frames, prior)[0]

    total, losses = L.multiview_keypoint_loss(torch.tensor(sc["w2c"]), sc["K"], keypoints, *x, use_frames, prior)
    want = _literal(sc, keypoints, x[0], x[1], x[2], 4, gmm_bufs, False)
    assert total.shape == () and set(losses) == set(KC.TERMS)
    torch.testing.assert_close(total, want.sum(), rtol=1e-6, atol=0)
    for k, w in zip(KC.TERMS, want):
        assert isinstance(losses[k], np.ndarray) or np.isscalar(losses[k])
        np.testing.assert_allclose(np.asarray(losses[k]).reshape(-1)[0], float(w), rtol=1e-6)
    assert torch.autograd.gradcheck(f, tuple(x), eps=1e-6, atol=1e-4, rtol=1e-5)
    # the 24 joints behind the first 25 get exact zeros
    x[0].grad = None
    total.backward()
    assert x[0].grad.shape == (1, 49, 3) and not x[0].grad[:, 25:].any() and x[0].grad[:, :25].abs().min() > 0
    # only the first len(use_frames) entries are looked at (loss.py:156), and every group is divided by len(use_frames)
    two = L.multiview_keypoint_loss(torch.tensor(sc["w2c"]), sc["K"], keypoints, *x, [0, 1], prior)[1]
    want2 = _literal(sc, keypoints, x[0], x[1], x[2], 2, gmm_bufs, False)
    np.testing.assert_allclose(two["reprojection_loss"], float(want2[0]), rtol=1e-6)


def test_smplx_value_gradcheck_missing_groups_and_face_order(L, prior, gmm_bufs):
    sc, keypoints, x = _smplx_inputs()
    use_frames = [0, 1, 2]

    def f(j, p, b):
        return L.multiview_keypoint_loss(list(torch.tensor(sc["w2c"])), list(sc["K"]), keypoints, j, p, b, use_frames, prior,
                                         use_hand_face=True, sigma=60, imsize=1024, pose_prior_weight=2.0, shape_prior_weight=3.0,
                                         angle_prior_weight=7.0)[0]

    total = f(*x)
    want = _literal(sc, keypoints, x[0], x[1], x[2], 3, gmm_bufs, True, imsize=1024, sigma=60, wp=2.0, wa=7.0, ws=3.0)
    torch.testing.assert_close(total, want.sum(), rtol=1e-6, atol=0)
    assert torch.autograd.gradcheck(f, tuple(x), eps=1e-6, atol=1e-4, rtol=1e-5)
    # a face given in the wrong order is a different loss: FACE_MAPPING is applied
    shuffled = [None if k is None else dict(k) for k in keypoints]
    shuffled[0]["face"] = np.ascontiguousarray(keypoints[0]["face"][::-1])
    other = L.multiview_keypoint_loss(list(torch.tensor(sc["w2c"])), list(sc["K"]), shuffled, *x, use_frames, prior, use_hand_face=True,
                                      sigma=60, imsize=1024, pose_prior_weight=2.0, shape_prior_weight=3.0, angle_prior_weight=7.0)[0]
    assert abs(float(other) - float(total)) > 1e-3 * abs(float(total))


def test_gradients_reach_only_inputs_that_ask(L, prior):
    sc, keypoints, x = _smpl_inputs(seed=2)
    x[1].requires_grad_(False)
    total, _ = L.multiview_keypoint_loss(torch.tensor(sc["w2c"]), sc["K"], keypoints, *x, [0, 1, 2, 3], prior)
    total.backward()
    assert x[0].grad is not None and x[2].grad is not None and x[1].grad is None
    assert x[0].grad.shape == x[0].shape and x[2].grad.shape == x[2].shape
    y = [t.detach() for t in x]
    total, _ = L.multiview_keypoint_loss(torch.tensor(sc["w2c"]), sc["K"], keypoints, *y, [0, 1, 2, 3], prior)
    assert not total.requires_grad
    with pytest.raises(RuntimeError):                                      # once differentiable
        z = [t.detach().requires_grad_(True) for t in x]
        t2, _ = L.multiview_keypoint_loss(torch.tensor(sc["w2c"]), sc["K"], keypoints, *z, [0, 1, 2, 3], prior)
        g, = torch.autograd.grad(t2, z[0], create_graph=True)
        g.sum().backward()


class ReferenceLikePrior(torch.nn.Module):
    """the shape of the reference's own module: buffers as tensors, nll_weights [1, M]"""

    def __init__(self, bufs):
        super().__init__()
        self.register_buffer("means", torch.tensor(bufs[0]))
        self.register_buffer("precisions", torch.tensor(bufs[1]))
        self.register_buffer("nll_weights", torch.tensor(bufs[2]).unsqueeze(0))


def test_the_three_kinds_of_pose_prior(L, prior, gmm_bufs):
    from oracle import smplify_oracle as O
    sc, keypoints, x = _smpl_inputs(seed=4, absent=())
    args = (torch.tensor(sc["w2c"]), sc["K"], keypoints, *x, [0, 1, 2, 3])
    own, _ = L.multiview_keypoint_loss(*args, prior)
    ref_like = ReferenceLikePrior(gmm_bufs)
    before = KC.StandInGmm.created
    a, _ = L.multiview_keypoint_loss(*args, ref_like)
    b, _ = L.multiview_keypoint_loss(*args, ref_like)
    assert KC.StandInGmm.created == before + 1                             # uploaded once per object and device
    torch.testing.assert_close(a, own, rtol=1e-12, atol=0)
    torch.testing.assert_close(b, own, rtol=1e-12, atol=0)
    # any other callable: evaluated in torch outside the kernel, weighted and added
    calls = []

    def generic(p, betas):
        calls.append((tuple(p.shape), betas))
        return O.gmm_merged_nll(p, *O.to_torch_gmm(gmm_bufs, torch.float64))

    c, losses = L.multiview_keypoint_loss(*args, generic)
    assert calls == [((1, 69), None)]
    torch.testing.assert_close(c, own, rtol=1e-6, atol=0)          # (4.78 ** 2 in double here, from the float32 hyper in the call)
    np.testing.assert_allclose(losses["pose_prior_loss"], 4.78 ** 2 * float(generic(x[1], None)), rtol=1e-6)
    assert torch.autograd.gradcheck(lambda j, p, bb: L.multiview_keypoint_loss(args[0], args[1], keypoints, j, p, bb, [0, 1, 2, 3], generic)[0],
                                    tuple(x), eps=1e-6, atol=1e-4, rtol=1e-5)
    # with use_hand_face it sees the 63 dofs zero-padded to 69
    scx, kpx, xx = _smplx_inputs(seed=5)
    calls.clear()
    L.multiview_keypoint_loss(torch.tensor(scx["w2c"]), scx["K"], kpx, *xx, [0, 1, 2], generic, use_hand_face=True)
    assert calls == [((1, 69), None)]
    with pytest.raises(ValueError):
        L.multiview_keypoint_loss(*args, 3.0)


def test_refusals(monkeypatch, gmm):
    from bodyfitting_amd import loss as L
    from bodyfitting_amd.prior import MaxMixturePrior
    monkeypatch.setattr(native, "keypoint_loss", KC.stand_in_keypoint_loss)
    monkeypatch.setattr(native, "Gmm", KC.StandInGmm)
    monkeypatch.setattr(assets, "_GMM", {"gmm": gmm})
    prior = MaxMixturePrior()
    sc, keypoints, x = _smpl_inputs(seed=6, dtype=torch.float32)
    w2c, K, frames = torch.tensor(sc["w2c"]), sc["K"], [0, 1, 2, 3]
    assert L.multiview_keypoint_loss(w2c, K, keypoints, *x, frames, prior, debug=True, output_folder="out", verts=x[0])[0].shape == ()
    with pytest.raises(ValueError, match="batch"):
        L.multiview_keypoint_loss(w2c, K, keypoints, x[0].repeat(2, 1, 1), x[1].repeat(2, 1), x[2].repeat(2, 1), frames, prior)
    with pytest.raises(ValueError, match="output"):
        L.multiview_keypoint_loss(w2c, K, keypoints, *x, frames, prior, output="reprojection")
    with pytest.raises(ValueError, match="no view"):
        L.multiview_keypoint_loss(w2c, K, [None] * 4, *x, frames, prior)
    with pytest.raises(ValueError, match="requires grad"):
        L.multiview_keypoint_loss(w2c.clone().requires_grad_(True), K, keypoints, *x, frames, prior)
    with pytest.raises(ValueError, match="requires grad"):
        L.multiview_keypoint_loss(w2c, [torch.tensor(k, requires_grad=True) for k in K], keypoints, *x, frames, prior)
    with pytest.raises(ValueError, match="requires grad"):
        kg = [None if k is None else {"pose": torch.tensor(k["pose"], requires_grad=True)} for k in keypoints]
        L.multiview_keypoint_loss(w2c, K, kg, *x, frames, prior)
    for i in range(3):
        y = [t.double() if k == i else t for k, t in enumerate(x)]
        with pytest.raises(ValueError, match="float32"):
            L.multiview_keypoint_loss(w2c, K, keypoints, *y, frames, prior)
    # with use_hand_face: a group that no view has
    scx, kpx, xx = _smplx_inputs(seed=7, dtype=torch.float32)
    assert L.multiview_keypoint_loss(torch.tensor(scx["w2c"]), scx["K"], kpx, *xx, [0, 1, 2], prior, use_hand_face=True)[0].shape == ()
    for group in (("hand_left", "hand_right"), ("face",)):
        cut = [None if k is None else {n: a for n, a in k.items() if n not in group} for k in kpx]
        with pytest.raises(ValueError, match=group[0][:4]):
            L.multiview_keypoint_loss(torch.tensor(scx["w2c"]), scx["K"], cut, *xx, [0, 1, 2], prior, use_hand_face=True)
    one_hand = [None if k is None else {n: a for n, a in k.items() if n != "hand_left"} for k in kpx]
    L.multiview_keypoint_loss(torch.tensor(scx["w2c"]), scx["K"], one_hand, *xx, [0, 1, 2], prior, use_hand_face=True)


def test_numpy_in_gives_floats_out(L, prior):
    sc, keypoints, x = _smpl_inputs(seed=8, dtype=torch.float32)
    arrays = [t.detach().numpy() for t in x]
    total, losses = L.multiview_keypoint_loss(sc["w2c"], sc["K"], keypoints, *arrays, [0, 1, 2, 3], prior)
    t2, l2 = L.multiview_keypoint_loss(torch.tensor(sc["w2c"]), sc["K"], keypoints, *x, [0, 1, 2, 3], prior)
    assert isinstance(total, float) and all(isinstance(v, float) for v in losses.values()) and set(losses) == set(KC.TERMS)
    np.testing.assert_allclose(total, float(t2), rtol=1e-12)
    for k in KC.TERMS:
        np.testing.assert_allclose(losses[k], np.asarray(l2[k]).reshape(-1)[0], rtol=1e-12)


def test_small_functions_and_stubs():
    from bodyfitting_amd import loss as L
    from oracle import smplify_oracle as O
    rng = np.random.default_rng(9)
    pts, rot, t, K = rng.normal(0, 0.3, (2, 7, 3)), np.stack([np.eye(3)] * 2), np.array([[0, 0, 3.0], [0.1, 0, 4.0]]), np.array(
        [[500.0, 0, 256], [0, 500, 256], [0, 0, 1]])
    want = O.perspective_projection(torch.tensor(pts), torch.tensor(rot), torch.tensor(t), torch.tensor(K))
    torch.testing.assert_close(L.perspective_projection(torch.tensor(pts), torch.tensor(rot), torch.tensor(t), torch.tensor(K)), want)
    np.testing.assert_allclose(L.perspective_projection(pts, rot, t, K), want.numpy(), rtol=1e-12)
    x = rng.normal(0, 50, (5, 2))
    np.testing.assert_allclose(L.gmof(x, 100), O.gmof(torch.tensor(x), 100).numpy(), rtol=1e-12)
    pose = rng.normal(0, 0.4, (2, 69))
    np.testing.assert_allclose(L.angle_prior(pose), O.angle_prior(torch.tensor(pose)).numpy(), rtol=1e-12)
    torch.testing.assert_close(L.angle_prior(torch.tensor(pose)), O.angle_prior(torch.tensor(pose)))
    cord, gt, conf = rng.normal(0, 9, (6, 2)), rng.normal(0, 9, (6, 2)), rng.uniform(size=6)
    np.testing.assert_allclose(L.reprojection_loss(cord, gt, conf, 0.5, 100),
                               float(O.reprojection_loss(torch.tensor(cord), torch.tensor(gt), torch.tensor(conf), 0.5, 100)), rtol=1e-12)
    for name in ("multview_mask_loss", "extract_countours", "point_cloud_loss_mesh_grid", "normal_loss_mesh_grid",
                 "normal_laplacian_smoothness", "point_cloud_loss_chamfer_naive"):
        with pytest.raises(NotImplementedError, match="SMPLify"):
            getattr(L, name)(None, None)
