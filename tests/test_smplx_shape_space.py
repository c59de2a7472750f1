"""num_betas and num_expression_coeffs beyond 10, on the CPU: the loader's column choice, the asset cache's keys and slices, and the
drop-in SMPLX over a float64 stand-in device model (the pattern of tests/test_smplx_expression_autograd.py) built on
oracle.smplify_oracle.smplx_forward of a widened model.  The HIP model's own forward / vjp at these widths are held to the same oracle
in tests/test_gpu_smplx_shape_space.py."""
import numpy as np
import pytest
import torch

from bodyfitting_amd import assets, model_files
from bodyfitting_amd import synthetic as S
from oracle import smplify_oracle as O

NV = 1200
INPUTS = ("betas", "global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose")
ALL = INPUTS + ("expression",)


@pytest.fixture(scope="module")
def small_model():
    return S.make_model("smplx", seed=0, nv=NV)


def test_widen_shape_space_keeps_what_is_there_and_scales_what_it_adds(small_model):
    before = small_model["shapedirs"].copy()
    wide = S.widen_shape_space(small_model, 16, 50, seed=3)
    assert wide["num_betas"] == 16 and wide["shapedirs"].shape == (NV, 3, 66) and wide["shapedirs"].dtype == np.float32
    np.testing.assert_array_equal(small_model["shapedirs"], before)
    assert "num_betas" not in small_model
    np.testing.assert_array_equal(wide["shapedirs"][:, :, :10], before[:, :, :10])
    np.testing.assert_array_equal(wide["shapedirs"][:, :, 16:26], before[:, :, 10:])
    again = S.widen_shape_space(small_model, 16, 50, seed=3)
    assert again["shapedirs"].tobytes() == wide["shapedirs"].tobytes()
    assert S.widen_shape_space(small_model, 16, 50, seed=4)["shapedirs"].tobytes() != wide["shapedirs"].tobytes()
    # later directions move the mesh less: 1 / (1 + index / 10)
    big = S.widen_shape_space(small_model, 300, 100, seed=3)["shapedirs"]
    rms = np.sqrt((big.astype(np.float64) ** 2).mean(axis=(0, 1)))
    assert rms[290:300].mean() < 0.1 * rms[:10].mean() and rms[390:400].mean() < 0.2 * rms[300:310].mean()
    # cutting, and a dict that already says num_betas
    cut = S.widen_shape_space(wide, 12, 3)
    np.testing.assert_array_equal(cut["shapedirs"], np.concatenate([wide["shapedirs"][:, :, :12], wide["shapedirs"][:, :, 16:19]], axis=2))
    with pytest.raises(ValueError, match="num_betas"):
        S.widen_shape_space(small_model, 9, 10)


@pytest.fixture(scope="module")
def files(small_model, tmp_path_factory):
    """a 400-column and a 20-column file of the small model; the 400-column file's shapedirs replaced by seeded columns"""
    folder = tmp_path_factory.mktemp("official400")
    path, vid = S.write_official_files(small_model, str(folder), shape_columns=400)
    z = dict(np.load(path, allow_pickle=True))
    z["shapedirs"] = np.random.default_rng(21).normal(0, 0.01, (NV, 3, 400))
    np.savez(path, **z)
    folder20 = tmp_path_factory.mktemp("official20")
    path20, _ = S.write_official_files(small_model, str(folder20), shape_columns=20)
    return path, path20, vid, z["shapedirs"].astype(np.float32)


@pytest.mark.parametrize("nb,ne", [(16, 50), (300, 100)])
def test_loader_picks_exactly_the_columns_asked_for(files, nb, ne):
    path, _, vid, cols = files
    m = model_files.load_smplx(path, vid, num_betas=nb, num_expression_coeffs=ne)
    assert m["num_betas"] == nb and m["shapedirs"].shape == (NV, 3, nb + ne) and m["shapedirs"].dtype == np.float32
    np.testing.assert_array_equal(m["shapedirs"][:, :, :nb], cols[:, :, :nb])
    np.testing.assert_array_equal(m["shapedirs"][:, :, nb:], cols[:, :, 300:300 + ne])


def test_loader_defaults_give_the_dict_of_before_and_missing_columns_raise(files):
    path, path20, vid, cols = files
    m = model_files.load_smplx(path, vid)
    assert "num_betas" not in m and m["shapedirs"].shape == (NV, 3, 20)
    np.testing.assert_array_equal(m["shapedirs"], np.concatenate([cols[:, :, :10], cols[:, :, 300:310]], axis=2))
    same = model_files.load_smplx(path, vid, num_betas=10, num_expression_coeffs=10)
    assert set(same) == set(m) and all(np.array_equal(np.asarray(same[k]), np.asarray(m[k])) for k in m)
    m20 = model_files.load_smplx(path20, vid)
    assert "num_betas" not in m20 and m20["shapedirs"].shape == (NV, 3, 20)
    np.testing.assert_array_equal(model_files.load_smplx(path20, vid, num_expression_coeffs=4)["shapedirs"], m20["shapedirs"][:, :, :14])
    with pytest.raises(ValueError, match="20 shapedirs columns"):
        model_files.load_smplx(path20, vid, num_betas=16)
    with pytest.raises(ValueError, match="10 expression"):
        model_files.load_smplx(path20, vid, num_expression_coeffs=11)
    with pytest.raises(ValueError, match="400 shapedirs columns"):
        model_files.load_smplx(path, vid, num_expression_coeffs=101)
    with pytest.raises(ValueError, match="300 shape"):
        model_files.load_smplx(path, vid, num_betas=301)
    with pytest.raises(ValueError, match="num_betas"):
        model_files.load_smplx(path, vid, num_betas=9)


def test_model_desc_keeps_ten_columns_and_attaches_the_rest(small_model):
    from bodyfitting_amd import native as N
    gmm = S.make_gmm(seed=0)
    d, info, keep = N.model_desc(small_model, gmm)
    assert (d.n_betas, info["n_betas"], info["num_betas"]) == (10, 10, 10) and keep["exprdirs"].shape == (NV, 3, 10)
    wide = S.widen_shape_space(small_model, 16, 50)
    d, info, keep = N.model_desc(wide, gmm)
    assert (d.n_betas, info["n_betas"], info["num_betas"]) == (10, 10, 16)
    np.testing.assert_array_equal(keep["shapedirs"], wide["shapedirs"][:, :, :10])
    np.testing.assert_array_equal(keep["exprdirs"], wide["shapedirs"][:, :, 10:])
    with pytest.raises(ValueError, match="num_betas"):
        N.model_desc(dict(small_model, num_betas=21), gmm)


class FakeDeviceModel:
    def __init__(self, model, gmm, device=0):
        self.model, self.device = model, device

    def close(self):
        pass


def test_get_device_model_keys_and_slices(small_model, monkeypatch):
    from bodyfitting_amd import native as N
    wide = S.widen_shape_space(small_model, 16, 50, seed=1)
    monkeypatch.setattr(N, "DeviceModel", FakeDeviceModel)
    monkeypatch.setattr(assets, "_GMM", {"gmm": S.make_gmm(seed=0)})
    monkeypatch.setattr(assets, "_MODELS", {("smplx", "neutral"): wide})
    planted = FakeDeviceModel(wide, None)
    monkeypatch.setattr(assets, "_DEVICE_MODELS", {("smplx", "neutral", 0): planted})
    # the defaults, and the registered model's own counts, are the key and the model of before
    assert assets.get_device_model("smplx", "neutral", 0) is planted
    assert assets.get_device_model("smplx", "neutral", 0, num_betas=16, num_expression_coeffs=50) is planted
    assert assets.get_device_model("smplx", "neutral", 0, num_expression_coeffs=50) is planted
    assert set(assets._DEVICE_MODELS) == {("smplx", "neutral", 0)}
    # other counts: a key of their own, the registered dict's columns sliced
    a = assets.get_device_model("smplx", "neutral", 0, num_betas=11, num_expression_coeffs=7)
    assert a is not planted and a is assets.get_device_model("smplx", "neutral", 0, num_betas=11, num_expression_coeffs=7)
    assert ("smplx", "neutral", 0, "space", 11, 7) in assets._DEVICE_MODELS and a.model["num_betas"] == 11
    np.testing.assert_array_equal(a.model["shapedirs"], np.concatenate([wide["shapedirs"][:, :, :11], wide["shapedirs"][:, :, 16:23]], axis=2))
    b = assets.get_device_model("smplx", "neutral", 0, num_betas=10)
    assert b.model["num_betas"] == 10 and b.model["shapedirs"].shape[2] == 60
    # more than the registered dict holds and no file: refused with what it holds
    with pytest.raises(ValueError, match="16 shape and 50 expression"):
        assets.get_device_model("smplx", "neutral", 0, num_betas=17)
    with pytest.raises(ValueError, match="SMPL-X only"):
        assets.get_device_model("smpl", "neutral", 0, num_betas=11)


class StandInDevice:
    """DeviceModel's forward_smplx / vjp_smplx interface over the fp64 torch oracle on a model with `nb` betas and `ne` expression
    coefficients; records how often it was called."""

    def __init__(self, model, nb, ne, dtype=np.float64):
        self.m = O.to_torch_model(model, torch.float64)
        assert model["shapedirs"].shape[2] == nb + ne
        self.dtype, self.n_betas, self.n_expression = dtype, nb, ne
        self.n_hand_pca, self.n_joints = model["left_hand_components"].shape[0], model["J_regressor"].shape[0]
        self.widths = (nb, 3, 63, 3, 3, 3, 6, 6, ne)
        self.calls = 0

    def _inputs(self, arrays, expression, grad=False):
        n = np.asarray(arrays[0]).reshape(-1, self.n_betas).shape[0]
        return [torch.tensor(np.zeros((n, w)) if a is None else np.asarray(a, np.float64).reshape(n, w), requires_grad=grad)
                for a, w in zip(tuple(arrays) + (expression,), self.widths)]

    def _forward(self, x):
        b, go, bp, jaw, le, re, lh, rh, ex = x
        out = O.smplx_forward(self.m, b, go, bp, le, re, lh, rh, jaw_pose=jaw, expression=ex, mapped=False)
        return {"vertices": out["vertices"], "joints_all": out["joints"], "joints": out["joints"][:, self.m["joint_map"]],
                "full_pose": out["full_pose"], "dyn_row": out["dyn_row"]}

    def forward_smplx(self, *arrays, **kw):
        self.calls += 1
        out = self._forward(self._inputs(arrays, kw.get("expression")))
        return {k: v.numpy().astype(np.int32) if k == "dyn_row" else v.numpy() for k, v in out.items()}

    def vjp_smplx(self, *arrays, dverts=None, djoints=None, djoints_all=None, dfull_pose=None, **kw):
        self.calls += 1
        with torch.enable_grad():
            x = self._inputs(arrays, kw.get("expression"), grad=True)
            out = self._forward(x)
            total = sum((out[k] * torch.as_tensor(np.asarray(d, np.float64))).sum()
                        for k, d in (("vertices", dverts), ("joints", djoints), ("joints_all", djoints_all), ("full_pose", dfull_pose))
                        if d is not None)
            g = torch.autograd.grad(total, x, allow_unused=True)
        g = tuple((gi if gi is not None else torch.zeros_like(xi)).numpy() for gi, xi in zip(g, x))
        return g if "expression" in kw else g[:8]


def _dropin(model, nb, ne, monkeypatch, dtype=np.float64):
    stand_in = StandInDevice(model, nb, ne, dtype)
    asked = []
    monkeypatch.setattr(assets, "_MODELS", {("smplx", "neutral"): model})
    monkeypatch.setattr(assets, "get_device_model", lambda *a, **k: (asked.append((a, k)), stand_in)[1])
    from bodyfitting_amd import smplx
    return smplx, stand_in, asked


def _params(n, widths, seed=0, dtype=torch.float64):
    rng = np.random.default_rng(seed)
    scale = dict(zip(ALL, (0.7, 0.8, 0.3, 0.2, 0.2, 0.2, 0.5, 0.5, 0.7)))
    return {k: torch.tensor(rng.normal(0, scale[k], (n, w)), dtype=dtype, requires_grad=dtype == torch.float64) for k, w in zip(ALL, widths)}


def test_create_16_50_takes_the_wide_blocks_and_passes_gradcheck(small_model, monkeypatch):
    wide = S.widen_shape_space(small_model, 16, 50)
    X, stand_in, asked = _dropin(wide, 16, 50, monkeypatch)
    body = X.create(model_type="smplx", use_face_contour=True, num_betas=16, num_expression_coeffs=50)
    assert asked == [(("smplx", "neutral", 0), {"num_betas": 16, "num_expression_coeffs": 50})]
    assert body.num_betas == 16 and body.num_expression_coeffs == 50
    p = _params(2, stand_in.widths)
    out = body(**p)
    assert out.vertices.shape == (2, NV, 3) and out.betas.shape == (2, 16) and out.expression.shape == (2, 50)
    # the betas beyond the tenth and the expression beyond the tenth both move the mesh
    q = {k: v.detach().clone() for k, v in p.items()}
    q["betas"][:, 10:] = 0
    assert float((body(**q).vertices - out.vertices).abs().max()) > 1e-3
    q = {k: v.detach().clone() for k, v in p.items()}
    q["expression"][:, 10:] = 0
    assert float((body(**q).vertices - out.vertices).abs().max()) > 1e-3

    def f(betas, expression):
        o = body(**dict(p, betas=betas, expression=expression), return_full_pose=True)
        return o.vertices, o.joints

    assert torch.autograd.gradcheck(f, (p["betas"], p["expression"]), eps=1e-6, atol=1e-6, rtol=1e-5, fast_mode=True)
    # betas alone (no other argument): the batch follows the wide betas
    assert body(betas=torch.zeros(3, 16, dtype=torch.float64)).vertices.shape == (3, NV, 3)
    assert body(betas=np.zeros((3, 16), np.float32)).vertices.shape == (3, NV, 3)


def test_wrong_widths_and_other_counts_are_refused(small_model, monkeypatch):
    wide = S.widen_shape_space(small_model, 16, 50)
    X, stand_in, asked = _dropin(wide, 16, 50, monkeypatch, np.float32)
    body = X.create(model_type="smplx", use_face_contour=True, num_betas=16, num_expression_coeffs=50)
    p = {k: v.detach().float() for k, v in _params(2, stand_in.widths, seed=1).items()}
    assert body(**p).joints.shape == (2, 144, 3)
    before = stand_in.calls
    for bad in (torch.zeros(2, 10), torch.zeros(2, 49), torch.zeros(2, 51), torch.zeros(1, 50)):
        with pytest.raises(ValueError, match="expression"):
            body(**dict(p, expression=bad))
    with pytest.raises(ValueError):
        body(**dict(p, betas=torch.zeros(2, 10)))                # ten betas on a sixteen-beta model: the batch does not come out
    assert stand_in.calls == before
    # a device model with other counts than the constructor's: the named ValueError
    with pytest.raises(ValueError, match="num_betas"):
        X.create(model_type="smplx", num_betas=11, num_expression_coeffs=50)
    with pytest.raises(ValueError, match="num_betas"):
        X.create(model_type="smplx", num_expression_coeffs=50)
    # (num_betas=10 on a model that has more: asked for again by name, so that a registered wide dict is cut to its first ten)
    assert asked[-1] == (("smplx", "neutral", 0), {"num_betas": 10, "num_expression_coeffs": 50})
    with pytest.raises(ValueError, match="num_expression_coeffs"):
        X.create(model_type="smplx", num_betas=16, num_expression_coeffs=7)
    with pytest.raises(ValueError, match="num_betas"):
        X.create(model_type="smplx", num_betas=9)


def test_default_construction_asks_get_device_model_for_nothing_new(small_model, monkeypatch):
    X, stand_in, asked = _dropin(small_model, 10, 10, monkeypatch)
    body = X.create(model_type="smplx", use_face_contour=True)
    assert asked == [(("smplx", "neutral", 0), {})]
    assert body.num_betas == 10 and body.num_expression_coeffs == 10
    X.create(model_type="smplx", num_betas=10, gender="neutral", device=0)
    assert asked[1] == (("smplx", "neutral", 0), {})
    X.create(model_type="smplx", num_expression_coeffs=10)
    assert asked[2] == (("smplx", "neutral", 0), {"num_expression_coeffs": 10})
