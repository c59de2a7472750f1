"""The OpenPose body estimator on the MI355X (csrc/openpose_kernels.hip): the convolution kernel on every shape of the network, the
network against the reference's own module (tests/golden/openpose_synthetic.npz, tools/gen_openpose_golden.py), the image and map
pipeline bit for bit against the numpy restatements, the peaks and limb scores exactly, the drop-ins and BodyFitting without
keypoints.

Bands follow the project's rule - set by the reference's own error, not guessed: for every compared array
    max|HIP - fp64| <= 4 * max|torch fp32 - fp64| + 1e-6 * max|fp64|."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from openpose_cases import bodypose_forward, planted_outputs
from bodyfitting_amd import _lib, assets, openpose as O, synthetic as S

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def band_check(name, got, f32, f64):
    got, f32, f64 = (np.asarray(a, np.float64) for a in (got, f32, f64))
    err, ref_err, scale = np.abs(got - f64).max(), np.abs(f32 - f64).max(), np.abs(f64).max()
    band = 4 * ref_err + 1e-6 * scale
    print(f"{name}: |HIP - fp64| {err:.3e}, |torch fp32 - fp64| {ref_err:.3e}, band {band:.3e} ({err / band:.2f} of it)")
    assert err <= band, (name, err, band)


@pytest.fixture(scope="module")
def weights():
    return S.make_openpose_weights(0)


@pytest.fixture(scope="module")
def golden():
    return load_golden("openpose_synthetic.npz")


@pytest.fixture(scope="module")
def net(weights):
    op = O.OpenPose(weights, device=0, max_batch=3, max_h=256, max_w=256)
    yield op
    op.close()


# (cin, cout, k): every distinct convolution of bodypose_model, and the merged L1 | L2 layers
SHAPES = ((3, 64, 3), (64, 64, 3), (64, 128, 3), (128, 128, 3), (128, 256, 3), (256, 256, 3), (256, 512, 3), (512, 512, 3),
          (512, 256, 3), (256, 128, 3), (128, 512, 1), (512, 38, 1), (512, 19, 1), (185, 128, 7), (128, 128, 7), (128, 128, 1),
          (128, 38, 1), (128, 19, 1), (192, 256, 7))


def _conv(n, Hs, Ws, cin, cout, k, relu, seed):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (k * k * cin))).astype(np.float32)
    b = rng.normal(0, 0.1, cout).astype(np.float32)
    x = rng.standard_normal((n, Hs, Ws, cin)).astype(np.float32)          # (image 0 is the same for every n)
    y = np.zeros((n, Hs, Ws, cout), np.float32)
    wp = np.ascontiguousarray(w.transpose(2, 3, 1, 0).reshape(-1, cout))
    _lib.check(_lib.load().bf_openpose_selftest_conv(0, n, Hs, Ws, cin, cout, k, int(relu), _lib.fptr(x), _lib.fptr(wp), _lib.fptr(b),
                                                     _lib.fptr(y)), "bf_openpose_selftest_conv")

    def ref(dtype):
        t = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2).to(dtype), torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype),
                     padding=k // 2)
        if relu:
            t = torch.relu(t)
        return t.permute(0, 2, 3, 1).numpy()
    return y, ref(torch.float32), ref(torch.float64)


@pytest.mark.parametrize("cin,cout,k", SHAPES)
def test_conv_shapes(cin, cout, k):
    y3, f32, f64 = _conv(3, 13, 11, cin, cout, k, cout != 19, seed=cin * 1000 + cout + k)
    band_check(f"conv {cin}->{cout} k{k} n=3", y3, f32, f64)
    y1, _, _ = _conv(1, 13, 11, cin, cout, k, cout != 19, seed=cin * 1000 + cout + k)
    np.testing.assert_array_equal(y1[0], y3[0])                 # a batch equals its single images bit for bit


def test_network_against_reference(net, weights, golden):
    """every scale against tests/openpose_cases.bodypose_forward in fp32 / fp64 (pinned to the imported module on the CPU); the first
    scale also against the reference's own outputs"""
    img = golden["net_image"]
    outs, ins = net.network([img])
    for m, s in enumerate(O.scales(img.shape[0])):
        x = O.preprocess(img, s)
        np.testing.assert_array_equal(ins[m][0], x, err_msg=f"input scale {m}")
        x = x.transpose(2, 0, 1)[None]
        f32, f64 = bodypose_forward(weights, x, torch.float32), bodypose_forward(weights, x, torch.float64)
        assert outs[m][0].shape == f64.shape
        band_check(f"stage-6 outputs scale {m}", outs[m][0], f32, f64)
    band_check("stage-6 outputs scale 0 (reference)", outs[0][0], golden["net_out32_0"], golden["net_out64_0"])


@pytest.fixture(scope="module")
def net_outputs(net, golden):
    outs, _ = net.network([golden["net_image"]])
    return outs


def test_maps_and_gaussian_bit_for_bit(net, golden, net_outputs):
    """the resize / crop / resize / accumulation and the Gaussian equal numpy's, through maps() and through the injection hook"""
    img = golden["net_image"]
    H, W = img.shape[:2]
    want_h, want_p = O.accumulate([o[0] for o in net_outputs], H, W)
    heat, paf = net.maps([img])
    np.testing.assert_array_equal(heat[0], want_h)
    np.testing.assert_array_equal(paf[0], want_p)
    heat, paf = net.inject(net_outputs, H, W)
    np.testing.assert_array_equal(heat[0], want_h)
    np.testing.assert_array_equal(paf[0], want_p)
    peaks, blurred = net.peaks(1, blurred=True)
    np.testing.assert_array_equal(np.moveaxis(blurred[0], 2, 0), O.gaussian_filter(np.moveaxis(want_h[:, :, :18], 2, 0)))
    assert peaks[0] == O.find_peaks(want_h)


def test_planted_outputs_give_the_reference_answer(net, golden):
    H, W = (int(v) for v in golden["planted_hw"])
    net.inject([o[None] for o in planted_outputs(H, W)], H, W)
    cand, subset = net._detect_resident(1)[0]
    np.testing.assert_array_equal(cand, golden["planted_candidate"])
    np.testing.assert_array_equal(subset, golden["planted_subset"])


def test_pairs_equal_numpy(net, golden, net_outputs):
    H, W = golden["net_image"].shape[:2]
    _, paf = net.inject(net_outputs, H, W)
    rng = np.random.default_rng(1)
    jobs = [(int(rng.integers(19)), int(rng.integers(W)), int(rng.integers(H)), int(rng.integers(W)), int(rng.integers(H)))
            for _ in range(300)] + [(3, 10, 10, 10, 10), (0, 0, 0, W - 1, H - 1), (18, 5, 7, 5, 90)]
    score, cnt = net.pairs(0, jobs)
    for i, j in enumerate(jobs):
        s, c = O.score_pair(paf[0], *j, H)
        assert (score[i], cnt[i]) == (s, c), (j, score[i], s, cnt[i], c)


def test_batch_equals_single(net):
    imgs = S.make_hmr_images(11, ((96, 80),) * 3)
    heat, paf = net.maps(imgs)
    for i, im in enumerate(imgs):
        h1, p1 = net.maps([im])
        np.testing.assert_array_equal(h1[0], heat[i])
        np.testing.assert_array_equal(p1[0], paf[i])


def test_dropin_body_equals_numpy_postprocess(weights, tmp_path):
    path = str(tmp_path / "body_pose_model.pth")
    torch.save({k: torch.from_numpy(v) for k, v in weights.items()}, path)
    sys.path.insert(0, os.path.join(REPO, "bodyfitting_amd", "dropin"))
    try:
        from openpose.body import Body
        from openpose.infer_openpose import get_pose
    finally:
        sys.path.remove(os.path.join(REPO, "bodyfitting_amd", "dropin"))
    img = S.make_hmr_images(4, ((120, 100),))[0]
    body = Body(path)
    cand, subset = body(img)
    heat, paf = body._net.maps([img])
    want_c, want_s = O.postprocess(heat[0], paf[0])
    np.testing.assert_array_equal(cand, want_c)
    np.testing.assert_array_equal(subset, want_s)
    assert len(cand) > 0
    poses = get_pose(img, body)
    assert len(poses) == len(subset) and all(p.shape == (17, 3) for p in poses)
    body._net.close()


def test_bodyfitting_detects_keypoints(weights, monkeypatch):
    """BodyFitting(...)(images, c2ws, Ks, keypoints=None) == the same call with the detections passed explicitly, bit for bit"""
    from bodyfitting_amd.body_fitting import BodyFitting
    model = S.make_model("smpl", seed=0)
    monkeypatch.setattr(assets, "_MODELS", {("smpl", "male"): model, ("smpl", "neutral"): model})
    monkeypatch.setattr(assets, "_GMM", {"gmm": S.make_gmm(seed=0)})
    assets.register_openpose(weights)
    try:
        prob = S.make_problem(model, frame=0, n_views=4)
        images = S.make_hmr_images(6, ((128, 128),) * 4)
        opts = SimpleNamespace(smpl_type="smpl", num_iters=10)
        net_output = (np.zeros((1, 10), np.float32), np.zeros((1, 72), np.float32))
        kw = dict(gender="male", keyframe=0, use_frames=list(range(4)), net_output=net_output)
        bf = BodyFitting(opts)
        res = bf(images, prob["c2ws"], prob["Ks"], None, **kw)
        est = O.OpenPose(weights, device=0, max_batch=4, max_h=128, max_w=128)
        kps = [O.select_person(p) for p in est.pose25([im[:, :, ::-1] for im in images])]
        est.close()
        assert any(k is not None for k in kps)
        want = BodyFitting(opts)(images, prob["c2ws"], prob["Ks"], kps, **kw)
        assert set(res) == set(want) and "vertices" in want
        for k, v in want.items():
            if isinstance(v, np.ndarray):
                np.testing.assert_array_equal(np.asarray(res[k]), v, err_msg=k)
    finally:
        assets.register_openpose(None)


def test_refusals(net, weights):
    img = np.zeros((300, 64, 3), np.uint8)
    with pytest.raises(_lib.BodyfitError, match="max_h"):
        net.maps([img])
    with pytest.raises(ValueError, match="uint8"):
        net.maps([np.zeros((64, 64, 3), np.float32)])
    with pytest.raises(ValueError, match="one size"):
        net.maps([np.zeros((64, 64, 3), np.uint8), np.zeros((64, 32, 3), np.uint8)])
    assets.register_openpose(None)
    with pytest.raises(ValueError, match="body_pose_model.pth"):
        O.OpenPose(device=0)
    with pytest.raises(_lib.BodyfitError, match="view"):
        net.pairs(7, [(0, 1, 1, 2, 2)])
