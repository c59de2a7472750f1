"""`expression` as the ninth input of the drop-in SMPLX's torch path, on the CPU: a stand-in device model with expression directions
(n_expression = 10) whose forward_smplx / vjp_smplx are oracle.smplify_oracle.smplx_forward(..., expression=, mapped=False) and its
torch autograd in float64.  The HIP model's own forward / vjp with expression are held to the same oracle in
tests/test_gpu_smplx_expression.py.

The drop-in takes `expression` in the device model's dtype only.  The HIP model computes in float32; the stand-in of the gradient
checks computes in float64 and says so (`dtype`), which is what lets torch.autograd.gradcheck run on it; the refusals are tested
on a stand-in that - like the HIP model - computes in float32."""
import numpy as np
import pytest
import torch

from bodyfitting_amd import assets
from bodyfitting_amd import synthetic as S
from oracle import smplify_oracle as O

NV = 1200
NE = 10
INPUTS = ("betas", "global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose")
ALL = INPUTS + ("expression",)
WIDTHS = (10, 3, 63, 3, 3, 3, 6, 6, NE)


class StandInDevice:
    """DeviceModel's forward_smplx / vjp_smplx interface, with expression directions, over the fp64 torch oracle; records the
    arguments of its calls."""
    n_expression = NE

    def __init__(self, model, dtype=np.float64):
        self.m = O.to_torch_model(model, torch.float64)
        self.dtype = dtype                      # what it takes `expression` in (DeviceModel.dtype: float32)
        self.n_betas, self.n_hand_pca, self.n_joints = 10, model["left_hand_components"].shape[0], model["J_regressor"].shape[0]
        self.forward_args, self.vjp_args = [], []

    def _inputs(self, arrays, expression, grad=False):
        n = np.asarray(arrays[0]).reshape(-1, 10).shape[0]
        return [torch.tensor(np.zeros((n, w)) if a is None else np.asarray(a, np.float64).reshape(n, w), requires_grad=grad)
                for a, w in zip(tuple(arrays) + (expression,), WIDTHS)]

    def _forward(self, x, with_expr):
        b, go, bp, jaw, le, re, lh, rh, ex = x
        out = O.smplx_forward(self.m, b, go, bp, le, re, lh, rh, jaw_pose=jaw, expression=ex if with_expr else None, mapped=False)
        return {"vertices": out["vertices"], "joints_all": out["joints"], "joints": out["joints"][:, self.m["joint_map"]],
                "full_pose": out["full_pose"], "dyn_row": out["dyn_row"]}

    def forward_smplx(self, *arrays, **kw):
        self.forward_args.append((len(arrays), dict(kw)))
        assert len(arrays) == 8 and set(kw) <= {"expression"}
        out = self._forward(self._inputs(arrays, kw.get("expression")), "expression" in kw)
        return {k: v.numpy().astype(np.int32) if k == "dyn_row" else v.numpy() for k, v in out.items()}

    def vjp_smplx(self, *arrays, dverts=None, djoints=None, djoints_all=None, dfull_pose=None, **kw):
        self.vjp_args.append((len(arrays), dict(kw)))
        assert len(arrays) == 8 and set(kw) <= {"expression"}
        with torch.enable_grad():                 # (called from inside a backward, where grad mode is off)
            x = self._inputs(arrays, kw.get("expression"), grad=True)
            out = self._forward(x, "expression" in kw)
            total = sum((out[k] * torch.as_tensor(np.asarray(d, np.float64))).sum()
                        for k, d in (("vertices", dverts), ("joints", djoints), ("joints_all", djoints_all), ("full_pose", dfull_pose))
                        if d is not None)
            g = torch.autograd.grad(total, x, allow_unused=True)
        g = tuple((gi if gi is not None else torch.zeros_like(xi)).numpy() for gi, xi in zip(g, x))
        return g if "expression" in kw else g[:8]       # eight gradients without expression, nine with - dexpression last


@pytest.fixture(scope="module")
def small_model():
    model = S.make_model("smplx", seed=0, nv=NV)
    assert model["shapedirs"].shape[2] == 10 + NE
    return model


def _dropin(small_model, monkeypatch, dtype):
    stand_in = StandInDevice(small_model, dtype)
    monkeypatch.setattr(assets, "_MODELS", {("smplx", "neutral"): small_model})
    monkeypatch.setattr(assets, "get_device_model", lambda *a, **k: stand_in)
    from bodyfitting_amd import smplx
    return smplx


@pytest.fixture
def X(small_model, monkeypatch):
    """bodyfitting_amd.smplx on a float64 stand-in device model"""
    return _dropin(small_model, monkeypatch, np.float64)


@pytest.fixture
def X32(small_model, monkeypatch):
    """... on one that, like the HIP model, takes float32"""
    return _dropin(small_model, monkeypatch, np.float32)


def _params(n, seed=0, grad=True):
    rng = np.random.default_rng(seed)
    scale = dict(zip(ALL, (0.7, 0.8, 0.3, 0.2, 0.2, 0.2, 0.5, 0.5, 0.7)))
    return {k: torch.tensor(rng.normal(0, scale[k], (n, w)), dtype=torch.float64, requires_grad=grad) for k, w in zip(ALL, WIDTHS)}


def test_gradcheck_over_all_nine_inputs(X):
    body = X.create(model_type="smplx", use_face_contour=True)
    assert body.num_expression_coeffs == NE

    def f(*x):
        out = body(**dict(zip(ALL, x)), return_full_pose=True)
        return out.vertices, out.joints, out.full_pose

    p = _params(2)
    assert torch.autograd.gradcheck(f, tuple(p[k] for k in ALL), eps=1e-6, atol=1e-6, rtol=1e-5, fast_mode=True)
    # expression, jaw and eyes exactly zero: the usual start of a loop
    z = {k: torch.zeros_like(v, requires_grad=True) if k in ("expression", "jaw_pose", "leye_pose", "reye_pose") else v
         for k, v in _params(1, 3).items()}
    assert torch.autograd.gradcheck(f, tuple(z[k] for k in ALL), eps=1e-6, atol=1e-6, rtol=1e-5, fast_mode=True)
    assert all(n == 8 and "expression" in kw for n, kw in body._dev.forward_args + body._dev.vjp_args)


def test_expression_gets_a_gradient_only_when_it_requires_one(X, small_model):
    body = X.create(model_type="smplx", use_face_contour=True)
    p = _params(2, seed=1)
    p["expression"].requires_grad_(False)
    out = body(**p)
    out.joints.square().sum().backward()
    assert p["expression"].grad is None and p["betas"].grad is not None and out.expression is p["expression"]
    # a zeros tensor that requires grad is an input like any other: its gradient is the oracle's, not None
    q = _params(1, seed=2)
    q["expression"] = torch.zeros(1, NE, dtype=torch.float64, requires_grad=True)
    body(**q).joints.square().sum().backward()
    assert q["expression"].grad is not None and q["expression"].grad.shape == (1, NE)
    r = {k: v.detach().clone().requires_grad_(True) for k, v in q.items()}
    m = O.to_torch_model(small_model, torch.float64)
    ref = O.smplx_forward(m, r["betas"], r["global_orient"], r["body_pose"], r["leye_pose"], r["reye_pose"], r["left_hand_pose"],
                          r["right_hand_pose"], jaw_pose=r["jaw_pose"], expression=r["expression"], mapped=False)
    ref["joints"].square().sum().backward()
    assert float(r["expression"].grad.abs().max()) > 0
    torch.testing.assert_close(q["expression"].grad, r["expression"].grad, atol=1e-12, rtol=0)
    # only expression requires grad
    s = _params(1, seed=3, grad=False)
    s["expression"].requires_grad_(True)
    body(**s).vertices.sum().backward()
    assert s["expression"].grad is not None and all(s[k].grad is None for k in INPUTS)


def test_numpy_path_equals_torch_path(X):
    body = X.create(model_type="smplx", use_face_contour=True)
    p = _params(2, seed=5, grad=False)
    arrays = {k: v.numpy() for k, v in p.items()}
    a = body(**arrays, return_full_pose=True)
    b = body(**p, return_full_pose=True)
    for k in ("vertices", "joints", "full_pose"):
        assert isinstance(getattr(a, k), np.ndarray) and isinstance(getattr(b, k), torch.Tensor), k
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k).numpy())
    assert a.expression is arrays["expression"] and b.expression is p["expression"]
    # expression moves the mesh: the same call without it differs
    c = body(**{k: v for k, v in arrays.items() if k != "expression"})
    assert float(np.abs(c.vertices - a.vertices).max()) > 1e-3
    # expression alone as a tensor takes the torch path
    d = body(**{k: v for k, v in arrays.items() if k != "expression"}, expression=p["expression"])
    assert isinstance(d.vertices, torch.Tensor)
    np.testing.assert_array_equal(d.vertices.numpy(), a.vertices)


def test_expression_none_makes_the_eight_argument_device_call(X):
    body = X.create(model_type="smplx", use_face_contour=True)
    p = _params(1, seed=6)
    del p["expression"]
    out = body(**p, expression=None)
    out.joints.sum().backward()
    assert out.expression is None
    body(**{k: v.detach().numpy() for k, v in p.items()})
    assert body._dev.forward_args == [(8, {}), (8, {})] and body._dev.vjp_args == [(8, {})]


def test_wrong_width_dtype_and_coefficient_count_are_refused(X32, small_model, monkeypatch):
    body = X32.create(model_type="smplx", use_face_contour=True, num_expression_coeffs=NE)
    p = {k: v.float() for k, v in _params(2, seed=7, grad=False).items()}
    good = p.pop("expression")
    assert body(**p, expression=good).joints.shape == (2, 144, 3)
    assert body(**{k: v.numpy() for k, v in p.items()}, expression=good.numpy()).joints.shape == (2, 144, 3)
    for bad in (torch.zeros(2, 7), torch.zeros(2, NE + 1), torch.zeros(1, NE), torch.zeros(2 * NE), good.double(), torch.zeros(2, NE, dtype=torch.float64),
                torch.zeros(2, NE, dtype=torch.float16)):
        with pytest.raises(ValueError, match="expression"):
            body(**p, expression=bad)
        with pytest.raises(ValueError, match="expression"):
            body(**{k: v.numpy() for k, v in p.items()}, expression=bad.numpy())
    with pytest.raises(ValueError, match="num_expression_coeffs"):
        X32.create(model_type="smplx", num_expression_coeffs=7)
    assert len(body._dev.forward_args) == 2
