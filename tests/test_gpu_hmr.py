"""HMR on the MI355X (csrc/hmr_kernels.hip): the convolution kernel on every ResNet-50 shape, the image pipeline bit for bit, the
whole network against the reference's own module (tests/golden/hmr_synthetic.npz, tools/gen_hmr_golden.py) and BodyFitting without
a caller-supplied net_output.

Bands follow the project's rule - set by the reference's own error, not guessed: for every compared array
    max|HIP - fp64| <= 4 * max|torch fp32 - fp64| + 1e-6 * max|fp64|."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from bodyfitting_amd import _lib, assets, hmr as H, synthetic as S

pytestmark = pytest.mark.gpu
SIZES = ((512, 512), (480, 640), (224, 224))


def band_check(name, got, f32, f64):
    got, f32, f64 = (np.asarray(a, np.float64) for a in (got, f32, f64))
    err, ref_err, scale = np.abs(got - f64).max(), np.abs(f32 - f64).max(), np.abs(f64).max()
    band = 4 * ref_err + 1e-6 * scale
    print(f"{name}: |HIP - fp64| {err:.3e}, |torch fp32 - fp64| {ref_err:.3e}, band {band:.3e} ({err / band:.2f} of it)")
    assert err <= band, (name, err, band)


@pytest.fixture(scope="module")
def weights():
    return S.make_hmr_weights(0)


@pytest.fixture(scope="module")
def golden():
    return load_golden("hmr_synthetic.npz")


@pytest.fixture(scope="module")
def net(weights):
    sd, mean = weights
    h = H.HMR(sd, mean, device=0, max_batch=32)
    yield h
    h.close()


def _conv(n, Hs, Ws, cin, cout, k, s, p, res, relu, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, Hs, Ws, cin)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (k * k * cin))).astype(np.float32)
    b = rng.normal(0, 0.1, cout).astype(np.float32)
    Ho, Wo = (Hs + 2 * p - k) // s + 1, (Ws + 2 * p - k) // s + 1
    r = rng.standard_normal((n, Ho, Wo, cout)).astype(np.float32) if res else None
    y = np.zeros((n, Ho, Wo, cout), np.float32)
    wp = np.ascontiguousarray(w.transpose(2, 3, 1, 0).reshape(-1, cout))
    _lib.check(_lib.load().bf_hmr_selftest_conv(0, n, Hs, Ws, cin, cout, k, s, p, _lib.fptr(x), _lib.fptr(wp), _lib.fptr(b), _lib.fptr(r),
                                                int(relu), _lib.fptr(y)), "bf_hmr_selftest_conv")

    def ref(dtype):
        t = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2).to(dtype), torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype),
                     stride=s, padding=p).permute(0, 2, 3, 1)
        if res:
            t = t + torch.from_numpy(r).to(dtype)
        return (F.relu(t) if relu else t).numpy()
    return y, ref(torch.float32), ref(torch.float64)


def resnet_shapes():
    """every distinct (input size, cin, cout, k, stride, pad) of ResNet-50 v1.5 as models/hmr.py builds it"""
    out, size = [], {}
    for conv, bn, cin, cout, k, s, p in H.conv_layers():
        block = ".".join(conv.split(".")[:2])          # layerX.Y
        if conv == "conv1":
            out.append((224, cin, cout, k, s, p))
            cur = 56
        elif conv.endswith("conv1") or conv.endswith("downsample.0"):
            out.append((size.setdefault(block, cur), cin, cout, k, s, p))
        elif conv.endswith("conv2"):
            out.append((size[block], cin, cout, k, s, p))
        else:                                         # conv3, after the stride of conv2
            cur = (size[block] - 1) // [l[5] for l in H.conv_layers() if l[0] == block + ".conv2"][0] + 1
            out.append((cur, cin, cout, k, s, p))
    return sorted(set(out), key=out.index)


@pytest.mark.parametrize("n", [1, 3])
def test_conv_kernel_on_every_resnet50_shape(n):
    shapes = resnet_shapes()
    assert len(shapes) >= 15
    for i, (Hs, cin, cout, k, s, p) in enumerate(shapes):
        got, f32, f64 = _conv(n, Hs, Hs, cin, cout, k, s, p, res=(k == 1 and s == 1), relu=(i % 2 == 0), seed=i)
        band_check(f"n={n} {Hs}x{Hs} {cin}->{cout} k{k}/s{s}", got, f32, f64)


def test_conv_kernel_ragged_shapes():
    for i, (n, Hs, Ws, cin, cout, k, s, p) in enumerate(
            [(3, 7, 7, 5, 157, 1, 1, 0), (2, 9, 13, 3, 70, 7, 2, 3), (1, 1, 1, 2205, 1024, 1, 1, 0), (5, 11, 6, 33, 65, 3, 2, 1),
             (3, 7, 7, 512, 2048, 1, 1, 0), (1, 3, 3, 1, 1, 3, 1, 1)]):
        for res in (False, True):
            got, f32, f64 = _conv(n, Hs, Ws, cin, cout, k, s, p, res=res, relu=res, seed=100 + i)
            band_check(f"ragged n={n} {Hs}x{Ws} {cin}->{cout} k{k}/s{s}", got, f32, f64)


def test_preprocessing_is_bit_exact(net):
    images = S.make_hmr_images(3, SIZES + ((1000, 750),))
    for im in images:
        resized, normalized = net.preprocess([im])
        np.testing.assert_array_equal(resized[0], H.resize_224(im))
        np.testing.assert_array_equal(normalized[0], H.normalize(H.resize_224(im)))
    resized, _ = net.preprocess(np.stack([images[0], images[0][::-1].copy()]))
    np.testing.assert_array_equal(resized[1], H.resize_224(images[0][::-1]))
    with pytest.raises(ValueError):
        net.preprocess([images[0].astype(np.float32)])


def test_network_against_the_reference(net, golden):
    images = S.make_hmr_images(0, SIZES)
    for i, im in enumerate(images):
        np.testing.assert_array_equal(net.preprocess([im])[0][0], golden["resized"][i])
    xf = net.features(images)
    band_check("xf n=3", xf, golden["xf_32"], golden["xf_64"])
    pose6d, betas, cam = net.regress(images)
    rotmat, _, _ = net.forward(images)
    for name, got in (("pose6d", pose6d), ("betas", betas), ("cam", cam), ("rotmat", rotmat)):
        band_check(name + " n=3", got, golden[name + "_32"], golden[name + "_64"])
    betas_p, pose = net.predict(images, golden["c2w"])
    np.testing.assert_array_equal(betas_p, betas)
    band_check("pose n=3", pose, golden["pose_32"], golden["pose_64"])
    # a batch equals its single images, and a re-run the first run, bit for bit
    for i, im in enumerate(images):
        p1, b1, c1 = net.regress([im])
        np.testing.assert_array_equal(p1[0], pose6d[i]); np.testing.assert_array_equal(b1[0], betas[i]); np.testing.assert_array_equal(c1[0], cam[i])
        np.testing.assert_array_equal(net.features([im])[0], xf[i])
    again = net.regress(images)
    for a, b in zip(again, (pose6d, betas, cam)):
        np.testing.assert_array_equal(a, b)
    big = [images[i % 3] for i in range(32)]
    p32, b32, c32 = net.regress(big)
    for i in range(32):
        np.testing.assert_array_equal(p32[i], pose6d[i % 3]); np.testing.assert_array_equal(b32[i], betas[i % 3])
        np.testing.assert_array_equal(c32[i], cam[i % 3])
    band_check("betas n=32", b32, golden["betas_32"][[i % 3 for i in range(32)]], golden["betas_64"][[i % 3 for i in range(32)]])


@pytest.fixture
def hmr_data(tmp_path, monkeypatch, weights):
    """a data folder with the synthetic weights as a legacy-format model_checkpoint.pt (as the published one) + smpl_mean_params.npz"""
    sd, mean = weights
    os.makedirs(tmp_path / "data")
    torch.save({"model": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}, str(tmp_path / "data" / "model_checkpoint.pt"),
               _use_new_zipfile_serialization=False)
    np.savez(tmp_path / "data" / "smpl_mean_params.npz", **mean)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(assets, "_HMR", {})
    monkeypatch.setattr(assets, "_DEVICE_MODELS", {})
    monkeypatch.setattr(assets, "_KID_TEMPLATE", {})
    monkeypatch.setattr(assets, "_GMM", {"gmm": S.make_gmm(seed=0)})
    yield tmp_path
    for d in list(assets._DEVICE_MODELS.values()):
        d.close()


@pytest.mark.parametrize("smpl_type,age", [("smpl", "adult"), ("smplx", "adult"), ("smpl", "kid")])
def test_bodyfitting_runs_hmr_without_net_output(hmr_data, monkeypatch, smpl_type, age):
    """BodyFitting(options)(images, Rts, Ks, keypoints, gender=..., keyframe=25, use_frames=list(range(48))) as
    apps/genebody_fitting.py calls it: HMR on images[25] / c2ws[25], then the fit; == the same call with HIP's own HMR.predict
    output passed as net_output, bit for bit"""
    from bodyfitting_amd.body_fitting import BodyFitting
    model = S.make_model(smpl_type, seed=0)
    monkeypatch.setattr(assets, "_MODELS", {(smpl_type, "male"): model, (smpl_type, "neutral"): model})
    if age == "kid":
        assets.register_kid_template(S.make_kid_template(model))
    prob = S.make_problem_smplx(model, frame=0, n_views=48) if smpl_type == "smplx" else S.make_problem(model, frame=0, n_views=48)
    base = S.make_hmr_images(5, ((512, 512), (512, 512)))
    images = [base[i % 2] for i in range(48)]
    opts = SimpleNamespace(smpl_type=smpl_type, age=age, num_iters=30)
    out1 = hmr_data / f"run_{smpl_type}_{age}"
    bf = BodyFitting(opts)
    res = bf(images, prob["c2ws"], prob["Ks"], prob["keypoints"], gender="male", keyframe=25, use_frames=list(range(48)),
             output_folder=str(out1))
    saved = np.load(out1 / f"{smpl_type}_parameter.npy", allow_pickle=True).item()
    est = H.HMR(device=0, max_batch=1)
    net_output = est.predict([images[25]], np.asarray(prob["c2ws"][25])[None])
    est.close()
    assert net_output[0].shape == (1, 10) and net_output[1].shape == (1, 72)
    want = BodyFitting(opts)(images, prob["c2ws"], prob["Ks"], prob["keypoints"], gender="male", keyframe=25, use_frames=list(range(48)),
                             net_output=net_output)
    for k in ("betas", "body_pose", "global_orient", "vertices"):
        if k in want:
            np.testing.assert_array_equal(np.asarray(res[k]), np.asarray(want[k]), err_msg=k)
            np.testing.assert_array_equal(np.asarray(saved[k]), np.asarray(want[k]), err_msg=k)
    if age == "kid":
        assert np.asarray(res["betas"]).size == 11
