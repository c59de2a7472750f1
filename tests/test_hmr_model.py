"""The host side of the HMR initial estimate (bodyfitting_amd/hmr.py): the torch-free checkpoint reader, the key-matching rules of
HMR_forward (smplify/body_fitting.py:21-27), the BatchNorm fold, the resize and post-processing restatements - against torch here
and the reference's own module through tests/golden/hmr_synthetic.npz (tools/gen_hmr_golden.py).  No GPU."""
import collections
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden
from bodyfitting_amd import assets, hmr as H, synthetic as S
import hmr_oracle


@pytest.fixture(scope="module")
def weights():
    return S.make_hmr_weights(0)


@pytest.fixture(scope="module")
def golden():
    return load_golden("hmr_synthetic.npz")


def _torch_state(sd):
    return collections.OrderedDict((k, torch.from_numpy(np.asarray(v))) for k, v in sd.items())


@pytest.mark.parametrize("zipped", [True, False])
def test_reader_equals_torch_load(tmp_path, zipped):
    sd = collections.OrderedDict(
        w=torch.randn(4, 3, 2, 2), b=torch.arange(5, dtype=torch.float64)[1:], n=torch.tensor(7), t=torch.randn(3, 4).t(),
        i=torch.arange(6, dtype=torch.int32).view(2, 3), shared=None)
    sd["shared"] = sd["w"][1]                               # a view into another tensor's storage, with an offset
    obj = {"model": sd, "epoch": 3, "optimizer": {"lr": [0.1, 0.2]}}
    path = str(tmp_path / "ck.pt")
    torch.save(obj, path, _use_new_zipfile_serialization=zipped)
    got, want = H.load_checkpoint(path), torch.load(path, weights_only=False)
    assert got["epoch"] == 3 and got["optimizer"] == {"lr": [0.1, 0.2]}
    assert list(got["model"]) == list(want["model"])
    for k, v in want["model"].items():
        assert got["model"][k].dtype == v.numpy().dtype, k
        np.testing.assert_array_equal(got["model"][k], v.numpy(), err_msg=k)


class _Boom:
    def __reduce__(self):
        return (os.system, ("echo should-not-run > /dev/null",))


@pytest.mark.parametrize("zipped", [True, False])
def test_restricted_unpickler_refuses_foreign_globals(tmp_path, monkeypatch, zipped):
    path = str(tmp_path / "evil.pt")
    torch.save({"model": {"x": torch.ones(2)}, "payload": _Boom()}, path, _use_new_zipfile_serialization=zipped)
    calls = []
    monkeypatch.setattr(os, "system", lambda *a: calls.append(a))
    with pytest.raises(pickle.UnpicklingError, match="refusing"):
        H.load_checkpoint(path)
    assert calls == []


def test_key_matching_rules(weights):
    sd, mean = weights
    # model_checkpoint.pt: strict=False - unexpected keys ignored, missing buffers from the npz
    extra = dict(sd, **{"smpl.betas": np.zeros(3)})
    st = H.match_state(extra, "/x/model_checkpoint.pt", mean)
    assert "smpl.betas" not in st
    np.testing.assert_array_equal(st["init_pose"][0], mean["pose"])
    # buffers in the checkpoint win over the npz (the reference's load order)
    with_buf = dict(sd, init_cam=np.full((1, 3), 5.0, np.float32))
    np.testing.assert_array_equal(H.match_state(with_buf, "model_checkpoint.pt", mean)["init_cam"], with_buf["init_cam"])
    # a missing convolution / BatchNorm / linear entry is an error naming it (torch would keep the random init)
    for key in ("layer3.2.conv2.weight", "layer1.0.downsample.1.running_var", "decshape.bias"):
        bad = {k: v for k, v in sd.items() if k != key}
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            H.match_state(bad, "model_checkpoint.pt", mean)
    # any other name: `module.` stripped, strict
    full = dict(sd, init_pose=mean["pose"][None], init_shape=mean["shape"][None], init_cam=mean["cam"][None])
    prefixed = {"module." + k: v for k, v in full.items()}
    st2 = H.match_state(prefixed, "best.pt")
    np.testing.assert_array_equal(st2["fc1.weight"], sd["fc1.weight"])
    with pytest.raises(ValueError, match="unexpected"):
        H.match_state(dict(prefixed, **{"module.extra": np.zeros(1)}), "best.pt")
    with pytest.raises(ValueError, match="init_cam"):
        H.match_state({k: v for k, v in prefixed.items() if k != "module.init_cam"}, "best.pt", mean)
    with pytest.raises(ValueError, match="shape"):
        H.match_state(dict(sd, **{"fc2.bias": np.zeros(3, np.float32)}), "model_checkpoint.pt", mean)


def test_folded_and_unfolded_agree_in_fp64(weights, golden):
    sd, mean = weights
    st = H.match_state(sd, "model_checkpoint.pt", mean)
    _, x = hmr_oracle.network_input([golden["resized"][2]])
    a = hmr_oracle.backbone(st, x, torch.float64, folded=False)
    b = hmr_oracle.backbone(st, x, torch.float64, folded=True)
    assert float((a - b).abs().max()) <= 1e-10 * max(1.0, float(a.abs().max()))


def test_restatement_reproduces_the_golden(weights, golden):
    sd, mean = weights
    st = H.match_state(sd, "model_checkpoint.pt", mean)
    assert str(golden["weights_digest"]) == H.weights_digest(st)
    assert 0.2 <= float(golden["layer4_positive"]) <= 0.8
    images = S.make_hmr_images(0, ((512, 512), (480, 640), (224, 224)))      # (tools/gen_hmr_golden.py SIZES)
    resized, x = hmr_oracle.network_input(images)
    np.testing.assert_array_equal(resized, golden["resized"])
    xf = hmr_oracle.backbone(st, x, torch.float64)
    np.testing.assert_allclose(xf.numpy(), golden["xf_64"], rtol=0, atol=1e-10)
    pose6d, betas, cam = hmr_oracle.regressor(st, xf, torch.float64)
    for name, v in (("pose6d", pose6d), ("betas", betas), ("cam", cam)):
        np.testing.assert_allclose(v.numpy(), golden[name + "_64"], rtol=0, atol=1e-10, err_msg=name)
    np.testing.assert_allclose(hmr_oracle.rot6d_to_rotmat(pose6d).numpy().reshape(-1, 24, 3, 3), golden["rotmat_64"], atol=1e-12)
    # the numpy float32 post-processing on the reference's fp32 rotations
    rot = H.rot6d_to_rotmat(golden["pose6d_32"]).reshape(-1, 24, 3, 3)
    np.testing.assert_allclose(rot, golden["rotmat_32"], atol=2e-6)
    np.testing.assert_allclose(H.convert_hom_to_angle(H.apply_root(golden["rotmat_32"], golden["c2w"])), golden["pose_32"], atol=2e-5)


def test_resize_known_answers():
    const = np.full((333, 517, 3), 77, np.uint8)
    assert (H.resize_224(const) == 77).all()
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (448, 448, 3)).astype(np.uint8)
    blocks = img.astype(np.int64).reshape(224, 2, 224, 2, 3).sum((1, 3))
    np.testing.assert_array_equal(H.resize_224(img), ((blocks + 2) >> 2).astype(np.uint8))      # INTER_AREA's 2 x 2 mean
    ident = rng.integers(0, 256, (224, 224, 3)).astype(np.uint8)
    np.testing.assert_array_equal(H.resize_224(ident), ident)
    up = rng.integers(0, 256, (100, 150, 3)).astype(np.uint8)          # upscaling: rows clamp the index, columns the weight too
    r = H.resize_224(up)
    assert r.shape == (224, 224, 3) and r.min() >= up.min() and r.max() <= up.max()
    for bad in (np.zeros((10, 10, 3), np.float32), np.zeros((10, 10), np.uint8), np.zeros((10, 10, 4), np.uint8)):
        with pytest.raises(ValueError):
            H.resize_224(bad)
    x = H.normalize(ident)
    want = ((torch.from_numpy(ident).float() / 255. - torch.tensor(H.IMG_NORM_MEAN)) / torch.tensor(H.IMG_NORM_STD)).numpy()
    np.testing.assert_array_equal(x, want)


def _axis_angle_to_R(aa):
    th = np.linalg.norm(aa)
    if th == 0:
        return np.eye(3)
    k = aa / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def test_convert_hom_to_angle_branches(golden):
    """identity (NaN -> 0 path), 180-degree rotations about x, y, z (the mask_d2 branches) and generic rotations: the numpy
    restatement against torchgeometry's algorithm as the reference writes it (restated in torch here) and against the angle"""
    rots = [np.eye(3), _axis_angle_to_R(np.array([np.pi, 0, 0])), _axis_angle_to_R(np.array([0, np.pi, 0])),
            _axis_angle_to_R(np.array([0, 0, np.pi])), _axis_angle_to_R(np.array([0.3, -1.2, 0.5])),
            _axis_angle_to_R(np.array([2.9, 0.1, -0.4])), _axis_angle_to_R(np.array([-0.2, 2.8, 0.9]))]
    R = np.zeros((1, 24, 3, 3), np.float32)
    R[0, :] = np.eye(3)
    for i, r in enumerate(rots):
        R[0, i] = r
    pose = H.convert_hom_to_angle(R).reshape(24, 3)
    assert np.isfinite(pose).all()
    np.testing.assert_array_equal(pose[0], 0)
    for i in range(1, len(rots)):
        np.testing.assert_allclose(_axis_angle_to_R(pose[i].astype(np.float64)), rots[i], atol=2e-3)
    t = np.transpose(R.reshape(-1, 3, 3), (0, 2, 1))
    branches = set()
    for tt in t:
        d2 = tt[2, 2] < 1e-6
        branches.add((d2, bool(tt[0, 0] > tt[1, 1]) if d2 else bool(tt[0, 0] < -tt[1, 1])))
    assert len(branches) == 4
    np.testing.assert_allclose(H.convert_hom_to_angle(H.apply_root(golden["rotmat_64"], golden["c2w"])), golden["pose_64"], atol=1e-5)


def test_bodyfitting_without_weights_raises(tmp_path, monkeypatch):
    from bodyfitting_amd.body_fitting import BodyFitting
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(assets, "_HMR", {})
    bf = BodyFitting(SimpleNamespace(smpl_type="smpl"))
    img = np.zeros((64, 64, 3), np.uint8)
    with pytest.raises(ValueError, match=r"model_checkpoint\.pt.*smpl_mean_params\.npz"):
        bf([img] * 2, [np.eye(4)] * 2, [np.eye(3)] * 2, np.zeros((2, 25, 3)), keyframe=1, use_frames=[0, 1])


def test_get_hmr_reads_the_reference_files(tmp_path, monkeypatch, weights):
    """data/model_checkpoint.pt (legacy torch.save format, as the published checkpoint) + data/smpl_mean_params.npz"""
    sd, mean = weights
    os.makedirs(tmp_path / "data")
    torch.save({"model": _torch_state(sd)}, str(tmp_path / "data" / "model_checkpoint.pt"), _use_new_zipfile_serialization=False)
    np.savez(tmp_path / "data" / "smpl_mean_params.npz", **mean)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(assets, "_HMR", {})
    packed, m = assets.get_hmr()
    want_p, want_m = H.fold_and_pack(H.match_state(sd, "model_checkpoint.pt", mean))
    np.testing.assert_array_equal(packed, want_p)
    np.testing.assert_array_equal(m, want_m)
