"""The OpenPose hand estimator on the MI355X (csrc/openpose_hand_kernels.hip): the new convolution shapes, the network against the
reference's own module (tests/golden/openpose_hand_synthetic.npz, tools/gen_openpose_hand_golden.py), the crop and map pipeline and
the Gaussian bit for bit against the numpy restatements, the labelling against scipy, the component pick exactly, batches of mixed
crops equal to each crop alone, the drop-in, and BodyFitting with hands.

Bands follow tests/test_gpu_openpose.py: max|HIP - fp64| <= 4 * max|torch fp32 - fp64| + 1e-6 * max|fp64|."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from scipy import ndimage

from conftest import load_golden
from openpose_hand_cases import PLANT_SIDE, handpose_forward, planted_outputs
from test_gpu_openpose import _conv, band_check
from bodyfitting_amd import _lib, assets, openpose as O, openpose_hand as OH, synthetic as S

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def weights():
    return S.make_openpose_hand_weights(0)


@pytest.fixture(scope="module")
def golden():
    return load_golden("openpose_hand_synthetic.npz")


@pytest.fixture(scope="module")
def net(weights):
    h = OH.OpenPoseHand(weights, device=0, max_hands=2, max_h=256, max_w=256)
    yield h
    h.close()


# (cin, cout, k): the convolutions handpose_model adds to the body's
SHAPES = ((152, 128, 7), (512, 128, 3), (128, 512, 1), (512, 22, 1), (128, 22, 1))


@pytest.mark.parametrize("cin,cout,k", SHAPES)
def test_conv_shapes(cin, cout, k):
    y3, f32, f64 = _conv(3, 13, 11, cin, cout, k, cout != 22, seed=cin * 1000 + cout + k)
    band_check(f"conv {cin}->{cout} k{k} n=3", y3, f32, f64)
    y1, _, _ = _conv(1, 13, 11, cin, cout, k, cout != 22, seed=cin * 1000 + cout + k)
    np.testing.assert_array_equal(y1[0], y3[0])


@pytest.fixture(scope="module")
def crop_run(net, golden):
    crop = golden["net_crop"]
    h, w = crop.shape[:2]
    view = np.full((h + 20, w + 30, 3), 17, np.uint8)
    view[9:9 + h, 21:21 + w] = crop                                  # the crop inside a larger view: its own edges replicate
    box = (0, 21, 9, w, h)
    outs, ins = net.network([view], [box])
    heat = net.maps([view], [box])[0]
    return crop, box, view, outs, ins, heat


def test_network_against_reference(weights, golden, crop_run):
    crop, _, _, outs, ins, _ = crop_run
    for m, s in enumerate(OH.hand_scales(crop.shape[0])):
        x = OH.preprocess_crop(crop, s)
        np.testing.assert_array_equal(ins[m][0], x, err_msg=f"input scale {m}")
        x = x.transpose(2, 0, 1)[None]
        f32, f64 = handpose_forward(weights, x, torch.float32), handpose_forward(weights, x, torch.float64)
        assert outs[m][0].shape == f64.shape
        band_check(f"hand outputs scale {m}", outs[m][0], f32, f64)
    band_check("hand outputs scale 0 (reference)", outs[0][0], golden["net_out32_0"], golden["net_out64_0"])


def test_maps_and_gaussian_bit_for_bit(net, crop_run):
    crop, box, view, outs, _, heat = crop_run
    h, w = crop.shape[:2]
    want = OH.accumulate_hand([o[0] for o in outs], h, w)
    np.testing.assert_array_equal(heat, want)
    got = net.inject(outs, [box])[0]
    np.testing.assert_array_equal(got, want)
    res, blurred = net.peaks(blurred=True)
    np.testing.assert_array_equal(np.moveaxis(blurred[0], 2, 0), O.gaussian_filter(np.moveaxis(want[:, :, :21], 2, 0)))
    pk, sc, fd = OH.hand_postprocess(want)
    np.testing.assert_array_equal(res[0][0], pk)
    np.testing.assert_array_equal(res[0][1], sc)
    np.testing.assert_array_equal(res[0][2], fd)


def test_label_is_scipy():
    rng = np.random.default_rng(7)
    lib = _lib.load()
    for H, W in ((1, 1), (17, 23), (64, 64), (150, 203)):
        for density in (0.3, 0.5, 0.62, 0.95):
            b = (rng.random((3, H, W)) < density).astype(np.uint8)
            b[1] = ndimage.binary_dilation(b[1], iterations=2)               # large winding components
            labels = np.zeros((3, H, W), np.int32)
            counts = np.zeros(3, np.int32)
            _lib.check(lib.bf_openpose_hand_selftest_label(0, 3, H, W, O.OpenPose._u8(np.ascontiguousarray(b)), _lib.iptr(labels),
                                                           _lib.iptr(counts)), "bf_openpose_hand_selftest_label")
            for i in range(3):
                want, n = ndimage.label(b[i], np.ones((3, 3), int))
                assert counts[i] == n
                np.testing.assert_array_equal(labels[i], want)


def test_planted_outputs_give_the_reference_answer(net, golden):
    outs = [[o] for o in planted_outputs(PLANT_SIDE)]
    heat = net.inject(outs, [(0, 0, 0, PLANT_SIDE, PLANT_SIDE)])[0]
    pk, sc, fd = net.peaks()[0]
    np.testing.assert_array_equal(pk, golden["planted_peaks"])
    want = OH.hand_postprocess(heat)
    np.testing.assert_array_equal(sc, want[1])
    np.testing.assert_array_equal(fd, want[2])


def test_mixed_boxes_equal_each_box_alone(net):
    views = np.stack(S.make_hmr_images(12, ((96, 128),) * 3))
    boxes = [(0, 5, 7, 40, 40), (2, 60, 30, 40, 40), (1, 20, 10, 33, 50), (0, 50, 40, 30, 20), (1, 0, 0, 128, 96), (2, 88, 56, 40, 40)]
    heat = net.maps(views, boxes)
    res = net.peaks()
    for i, b in enumerate(boxes):
        one = net.maps(views, [b])[0]
        np.testing.assert_array_equal(one, heat[i], err_msg=str(b))
        r = net.peaks()[0]
        for a, c in zip(r, res[i]):
            np.testing.assert_array_equal(a, c)
        pk, sc, fd = OH.hand_postprocess(heat[i])
        np.testing.assert_array_equal(res[i][0], pk)
        np.testing.assert_array_equal(res[i][1], sc)


def test_dropin_hand_equals_postprocess_of_its_maps(weights, tmp_path):
    path = str(tmp_path / "hand_pose_model.pth")
    torch.save({k: torch.from_numpy(v) for k, v in weights.items()}, path)
    sys.path.insert(0, os.path.join(REPO, "bodyfitting_amd", "dropin"))
    try:
        from openpose.hand import Hand
        from openpose import util
    finally:
        sys.path.remove(os.path.join(REPO, "bodyfitting_amd", "dropin"))
    crop = S.make_hmr_images(3, ((70, 70),))[0][:, :, ::-1]
    hand = Hand(path)
    peaks = hand(crop)
    heat = hand._net.maps([np.ascontiguousarray(crop)], [(0, 0, 0, 70, 70)])[0]
    assert peaks.dtype == np.int64 and peaks.shape == (21, 2)
    np.testing.assert_array_equal(peaks, OH.hand_postprocess(heat)[0])
    assert util.npmax(np.array([[0, 3, 3], [3, 1, 0]])) == (0, 1)
    hand._net.close()


def test_bodyfitting_detects_hands(weights, monkeypatch):
    """BodyFitting(smplx, detect_hands=True)(..., keypoints=None) == the same call with the detected dicts passed explicitly"""
    from bodyfitting_amd.body_fitting import BodyFitting
    from bodyfitting_amd import openpose_hand
    model = S.make_model("smplx", seed=0)
    monkeypatch.setattr(assets, "_MODELS", {("smplx", "male"): model, ("smplx", "neutral"): model})
    monkeypatch.setattr(assets, "_GMM", {"gmm": S.make_gmm(seed=0)})
    body_w = S.make_openpose_weights(0)
    assets.register_openpose(body_w)
    assets.register_openpose_hand(weights)
    try:
        prob = S.make_problem_smplx(model, 0, 4)
        images = S.make_hmr_images(6, ((128, 128),) * 4)
        opts = SimpleNamespace(smpl_type="smplx", num_iters=10, detect_hands=True)
        net_output = (np.zeros((1, 10), np.float32), np.zeros((1, 72), np.float32))
        kw = dict(gender="male", keyframe=0, use_frames=list(range(4)), net_output=net_output)
        res = BodyFitting(opts)(images, prob["c2ws"], prob["Ks"], None, **kw)
        body = O.OpenPose(body_w, device=0, max_batch=4, max_h=128, max_w=128)
        hand = openpose_hand.OpenPoseHand(weights, device=0, max_hands=16, max_h=128, max_w=128)
        bgr = [np.ascontiguousarray(im[:, :, ::-1]) for im in images]
        kps = [openpose_hand.select_person_entry(p) for p in openpose_hand.detect_people(body, hand, bgr)]
        body.close()
        hand.close()
        assert any(k is not None and "hand_left" in k for k in kps)
        want = BodyFitting(opts)(images, prob["c2ws"], prob["Ks"], kps, **kw)
        assert set(res) == set(want) and "vertices" in want
        for k, v in want.items():
            if isinstance(v, np.ndarray):
                np.testing.assert_array_equal(np.asarray(res[k]), v, err_msg=k)
    finally:
        assets.register_openpose(None)
        assets.register_openpose_hand(None)


def test_refusals(net, tmp_path, monkeypatch):
    view = np.zeros((64, 64, 3), np.uint8)
    with pytest.raises(_lib.BodyfitError, match="outside its view"):
        net.maps([view], [(0, 40, 0, 30, 30)])
    with pytest.raises(_lib.BodyfitError, match="outside its view"):
        net.maps([view], [(1, 0, 0, 30, 30)])
    with pytest.raises(_lib.BodyfitError, match="max_h"):
        net.maps([np.zeros((300, 64, 3), np.uint8)], [(0, 0, 0, 20, 20)])
    assets.register_openpose_hand(None)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="hand_pose_model.pth"):
        OH.OpenPoseHand(device=0)
