"""The OpenPose hand estimator's host side, no GPU: the torch-free weight reader, the packing, the numpy restatements the kernels are
held to (skimage's 8-connected labelling, numpy's pairwise sum, Hand.__call__'s post-processing, util.handDetect) against the
reference's own answers (tests/golden/openpose_hand_synthetic.npz, tools/gen_openpose_hand_golden.py), and the JSON with hands."""
import json
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from conftest import load_golden
from openpose_hand_cases import DETECT_HW, PLANT_SIDE, detect_inputs, handpose_forward, planted_outputs
from bodyfitting_amd import assets, io, openpose as O, openpose_hand as OH, synthetic as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def weights():
    return S.make_openpose_hand_weights(0)


@pytest.fixture(scope="module")
def golden():
    return load_golden("openpose_hand_synthetic.npz")


def test_weight_reader_and_errors(weights, tmp_path):
    torch = pytest.importorskip("torch")
    path = str(tmp_path / "hand_pose_model.pth")
    torch.save({k: torch.from_numpy(v) for k, v in weights.items()}, path)
    got = OH.load_hand_weights(path)
    assert list(got) == list(OH.expected_hand_keys())
    for k, v in weights.items():
        assert got[k].dtype == np.float32
        np.testing.assert_array_equal(got[k], v, err_msg=k)
    torch.save({k: torch.from_numpy(v) for k, v in weights.items() if k != "Mconv7_stage6.bias"}, path)
    with pytest.raises(ValueError, match="Mconv7_stage6.bias"):
        OH.load_hand_weights(path)
    with pytest.raises(ValueError, match="conv5_3_CPM.weight"):
        assets.register_openpose_hand({k: v for k, v in weights.items() if k != "conv5_3_CPM.weight"})
    bad = dict(weights)
    bad["Mconv1_stage2.weight"] = bad["Mconv1_stage2.weight"][:, :149]
    with pytest.raises(ValueError, match="Mconv1_stage2.weight"):
        OH.match_hand_state(bad)


def test_missing_weights_name_the_file(tmp_path, monkeypatch):
    assets.register_openpose_hand(None)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="hand_pose_model.pth.*keypoints="):
        assets.get_openpose_hand()


def test_pack_layout(weights):
    from bodyfitting_amd import _lib
    p = OH.pack_hand(OH.match_hand_state(weights))
    assert p.size == _lib.load().bf_openpose_hand_n_weights()
    w0 = p[:9 * 4 * 64].reshape(3, 3, 4, 64)
    np.testing.assert_array_equal(w0[:, :, :3], weights["conv1_1.weight"].transpose(2, 3, 1, 0))
    assert not w0[:, :, 3].any()
    # the stage input: out_prev 0:22 | 0 0 | out1_0 24:152
    assert OH.HCAT_POS.tolist() == list(range(22)) + list(range(24, 152))
    assert set(range(OH.HCAT_C)) - set(OH.HCAT_POS.tolist()) == {22, 23}
    # Mconv1_stage2 sits after the VGG front and conv6_1 / conv6_2: rows 22, 23 of every tap are zero, the rest are torch's channels
    at = 0
    for v in OH.HAND_VGG + OH.HAND_STAGE1:
        if v != "pool":
            cin, cout, k = v[1], v[2], v[3]
            at += k * k * (-(-cin // 4) * 4) * (-(-cout // 4) * 4) + (-(-cout // 4) * 4)
    m1 = p[at:at + 49 * 152 * 128].reshape(7, 7, 152, 128)
    assert not m1[:, :, 22:24].any()
    w = weights["Mconv1_stage2.weight"].transpose(2, 3, 1, 0)
    np.testing.assert_array_equal(m1[:, :, OH.HCAT_POS], w)


def test_gaussian_weights_in_the_hand_kernel_source():
    src = open(os.path.join(REPO, "bodyfitting_amd", "csrc", "openpose_hand_kernels.hip")).read()
    body = re.search(r"oh_gauss_w\[OH_GR \+ 1\] = \{(.*?)\};", src, re.S).group(1)
    assert [float.fromhex(v.strip()) for v in body.split(",")] == O.gaussian_weights(3.0)[12:].tolist()


def test_label8_is_scipy():
    rng = np.random.default_rng(5)
    for shape in ((1, 1), (3, 9), (40, 33), (97, 120)):
        for density in (0.2, 0.45, 0.6, 0.9):
            b = rng.random(shape) < density
            got, n = OH.label8(b)
            want, m = ndimage.label(b, np.ones((3, 3), int))
            assert n == m
            np.testing.assert_array_equal(got, want)
    # a U whose first pixel (top of the left arm) is not where the arms meet; the right arm starts later on row 0
    u = np.zeros((6, 7), bool)
    u[0:5, 1] = u[0:5, 5] = u[4, 1:6] = True
    u[0, 3] = True                                        # a lone pixel between the arms, after the left arm's first pixel
    lab, n = OH.label8(u)
    assert n == 2 and lab[0, 1] == lab[0, 5] == lab[4, 3] == 1 and lab[0, 3] == 2
    # components touching only diagonally are one; the numbering follows the first pixel
    d = np.zeros((5, 5), bool)
    d[0, 4] = d[1, 3] = d[2, 2] = True
    d[4, 0] = True
    lab, n = OH.label8(d)
    assert n == 2 and lab[0, 4] == lab[2, 2] == 1 and lab[4, 0] == 2
    lab, n = OH.label8(np.zeros((4, 4), bool))
    assert n == 0 and not lab.any()


@pytest.mark.parametrize("n", [1, 7, 8, 127, 128, 129, 1000, 8191, 8192, 8193, 16384, 16391, 100000, 512 * 512])
def test_pairwise_sum_is_numpy(n):
    rng = np.random.default_rng(n)
    a = rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))
    assert OH.pairwise_sum(a) == np.sum(a)
    g = a[rng.random(n) < 0.7]                            # a gather, as np.sum(map_ori[label_img == i]) sees it
    assert OH.pairwise_sum(g) == np.sum(g)


def test_forward_restatement_is_the_reference(weights, golden):
    crop = golden["net_crop"]
    x = OH.preprocess_crop(crop, OH.hand_scales(crop.shape[0])[0]).transpose(2, 0, 1)[None]
    torch = pytest.importorskip("torch")
    f64 = handpose_forward(weights, x, torch.float64)
    want64, want32 = golden["net_out64_0"], golden["net_out32_0"]
    assert f64.shape == want64.shape == (23, 6, 22)
    assert np.abs(f64 - want64).max() <= 1e-12 * np.abs(want64).max()
    f32 = handpose_forward(weights, x, torch.float32)
    assert np.abs(f32 - want64).max() <= 4 * np.abs(want32 - want64).max() + 1e-6 * np.abs(want64).max()


def test_postprocess_equals_reference(golden):
    heat = OH.accumulate_hand(planted_outputs(PLANT_SIDE), PLANT_SIDE, PLANT_SIDE)
    peaks, scores, found = OH.hand_postprocess(heat)
    np.testing.assert_array_equal(peaks, golden["planted_peaks"])
    assert peaks.dtype == np.int64 and peaks.shape == (21, 2)
    assert not found[3] and tuple(peaks[3]) == (0, 0)                     # the empty part
    assert found[4] and scores[4] == 0 and tuple(peaks[4]) != (0, 0)      # an all-negative component: a zeroed pixel
    m1 = heat[:, :, 1]
    gy, gx = np.unravel_index(np.argmax(m1), m1.shape)
    assert (gx, gy) != tuple(peaks[1])                                    # the larger sum, not the global maximum
    assert tuple(peaks[2]) == (50, 50)                                    # the tie: the first label


def test_hand_detect_equals_reference(golden):
    cand, subset = detect_inputs()
    got = OH.hand_detect(cand, subset, *DETECT_HW)
    want = golden["detect"]
    assert [[x, y, w, int(left)] for x, y, w, left in got] == want.tolist()
    assert len(got) == 4 and [b[3] for b in got] == [True, False, True, False]


def test_json_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    people = []
    for i in range(3):
        p = {"pose": np.column_stack([rng.integers(0, 500, (25, 2)), rng.uniform(0, 1, 25)])}
        if i != 1:
            pk = rng.integers(0, 120, (21, 2))
            sc = rng.uniform(0.01, 0.9, 21)
            fd = rng.random(21) < 0.8
            p["hand_left"] = OH.hand_array((30, 40), pk, sc, fd)
        if i == 2:
            p["hand_right"] = np.zeros((21, 3))                           # no part found: dropped as the reader drops it
        people.append(p)
    path = str(tmp_path / "image_keypoints.json")
    OH.write_json(path, people)
    doc = json.load(open(path))
    assert "hand_left_keypoints_2d" in doc["people"][0] and "hand_left_keypoints_2d" not in doc["people"][1]
    got = io.load_openpose(path)
    want = OH.select_person_entry(people)
    assert set(got) == set(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k])
    every = io.load_openpose(path, only_one=False)
    assert "hand_right" not in every[2] and "hand_left" in every[2]
    a = OH.hand_array((30, 40), np.array([[5, 6]] * 21), np.full(21, 0.5), np.array([True] + [False] * 20))
    assert a[0].tolist() == [35, 46, 0.5] and not a[1:].any()
