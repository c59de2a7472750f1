"""The OpenPose body estimator's host side, no GPU: the torch-free weight reader, the packing, the numpy restatements the kernels are
held to (cv2 INTER_CUBIC, scipy's gaussian_filter, Body.__call__'s post-processing) and the BODY_25 JSON."""
import os
import re

import numpy as np
import pytest
from scipy.ndimage import gaussian_filter as scipy_gaussian

from conftest import load_golden
from openpose_cases import bodypose_forward, planted_outputs
from bodyfitting_amd import assets, io, openpose as O, synthetic as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def weights():
    return S.make_openpose_weights(0)


@pytest.fixture(scope="module")
def golden():
    return load_golden("openpose_synthetic.npz")


def test_weight_reader_and_missing_key(weights, tmp_path):
    torch = pytest.importorskip("torch")
    path = str(tmp_path / "body_pose_model.pth")
    torch.save({k: torch.from_numpy(v) for k, v in weights.items()}, path)
    got = O.load_weights(path)
    assert list(got) == list(O.expected_keys())
    for k, v in weights.items():
        assert got[k].dtype == np.float32
        np.testing.assert_array_equal(got[k], v, err_msg=k)
    assert sum(v.size for v in got.values()) == 52311446
    partial = {k: torch.from_numpy(v) for k, v in weights.items() if k != "Mconv7_stage6_L2.bias"}
    torch.save(partial, path)
    with pytest.raises(ValueError, match="Mconv7_stage6_L2.bias"):
        O.load_weights(path)
    with pytest.raises(ValueError, match="conv4_4_CPM.weight"):
        assets.register_openpose({k: v for k, v in weights.items() if k != "conv4_4_CPM.weight"})
    bad = dict(weights)
    bad["conv1_1.weight"] = bad["conv1_1.weight"][:, :2]
    with pytest.raises(ValueError, match="conv1_1.weight"):
        O.match_state(bad)


def test_pack_layout(weights):
    p = O.pack(O.match_state(weights))
    from bodyfitting_amd import _lib
    assert p.size == _lib.load().bf_openpose_n_weights()
    # the first layer: [3 * 3 * 4][64] with a zero row per tap for the padded input channel, then the bias
    w0 = p[:9 * 4 * 64].reshape(3, 3, 4, 64)
    np.testing.assert_array_equal(w0[:, :, :3], weights["conv1_1.weight"].transpose(2, 3, 1, 0))
    assert not w0[:, :, 3].any()
    np.testing.assert_array_equal(p[9 * 4 * 64:9 * 4 * 64 + 64], weights["conv1_1.bias"])
    # Mconv1's concat rows: torch channel c sits at CAT_POS[c]; the seven pad rows are zero
    assert sorted(O.CAT_POS.tolist()) == sorted(set(O.CAT_POS.tolist())) and len(O.CAT_POS) == 185
    assert set(range(O.CAT_C)) - set(O.CAT_POS.tolist()) == {166, 167, 187, 188, 189, 190, 191}


def test_gaussian_is_scipy_bit_for_bit():
    rng = np.random.default_rng(3)
    for shape in ((96, 128), (13, 40), (161, 97)):
        a = rng.standard_normal(shape) * rng.uniform(0.1, 5)
        np.testing.assert_array_equal(O.gaussian_filter(a), scipy_gaussian(a, sigma=3))
    y, x = np.mgrid[0:120, 0:90]
    blob = 3.75 * np.exp(-((x - 40.3) ** 2 + (y - 70.1) ** 2) / 50.0)
    np.testing.assert_array_equal(O.gaussian_filter(blob), scipy_gaussian(blob, sigma=3))


def test_gaussian_weights_in_the_kernel_source():
    src = open(os.path.join(REPO, "bodyfitting_amd", "csrc", "openpose_kernels.hip")).read()
    body = re.search(r"op_gauss_w\[OP_GR \+ 1\] = \{(.*?)\};", src, re.S).group(1)
    table = [float.fromhex(v.strip()) for v in body.split(",")]
    w = O.gaussian_weights(3.0)
    assert table == w[12:].tolist() == w[12::-1].tolist()


def test_cubic_known_answers():
    assert O.scaled_size(5, 0.5) == 2 and O.scaled_size(7, 0.5) == 4 and O.scaled_size(512, 368 / 512) == 368
    assert [d[:2] for d in O.scale_dims(512, 512)] == [(184, 184), (368, 368), (552, 552), (736, 736)]
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (37, 23, 3), dtype=np.uint8)
    np.testing.assert_array_equal(O.resize_cubic_u8(img, 1.0), img)
    for s in (0.5, 1.37, 2.875):
        c = np.full((31, 17, 3), 77, np.uint8)
        r = O.resize_cubic_u8(c, s)
        assert r.shape == (O.scaled_size(31, s), O.scaled_size(17, s), 3)
        assert (r == 77).all()
    f = rng.standard_normal((9, 11, 5)).astype(np.float32)
    np.testing.assert_array_equal(O.resize_cubic_f32(f, 9, 11, 1.0, 1.0), f)
    cf = np.full((6, 7, 2), 0.375, np.float32)
    np.testing.assert_allclose(O.resize_cubic_f32(cf, 48, 56, 8.0, 8.0), 0.375, rtol=0, atol=2e-7)
    # coefficients sum to one and interpolate at integer positions
    c = O.cubic_coeffs(np.float32([0, 0.25, 0.5]))
    np.testing.assert_array_equal(c[0], np.float32([0, 1, 0, 0]))
    np.testing.assert_allclose(c.sum(1), 1, atol=1e-7)


def test_postprocess_equals_reference(golden):
    """the numpy restatement of body.py:101-238 on the planted per-scale outputs the reference's Body produced its answer from"""
    H, W = (int(v) for v in golden["planted_hw"])
    heat, paf = O.accumulate(planted_outputs(H, W), H, W)
    cand, subset = O.postprocess(heat, paf)
    np.testing.assert_array_equal(cand, golden["planted_candidate"])
    np.testing.assert_array_equal(subset, golden["planted_subset"])
    assert len(subset) == 2 and sorted(subset[:, -1]) == [8, 18]


def test_forward_restatement_is_the_reference(weights, golden):
    """tests/openpose_cases.bodypose_forward (what the GPU tests compare every scale with) against the imported bodypose_model"""
    img = golden["net_image"]
    x = O.preprocess(img, O.scales(img.shape[0])[0]).transpose(2, 0, 1)[None]
    torch = pytest.importorskip("torch")
    f64 = bodypose_forward(weights, x, torch.float64)
    want64, want32 = golden["net_out64_0"], golden["net_out32_0"]
    assert f64.shape == want64.shape
    assert np.abs(f64 - want64).max() <= 1e-12 * np.abs(want64).max()
    f32 = bodypose_forward(weights, x, torch.float32)
    assert np.abs(f32 - want64).max() <= 4 * np.abs(want32 - want64).max() + 1e-6 * np.abs(want64).max()


def test_json_round_trip(golden, tmp_path):
    people = O.pose25(golden["planted_candidate"], golden["planted_subset"])
    assert len(people) == 2 and all(p.shape == (25, 3) for p in people)
    for p in people:
        assert not p[[1, 8, 19, 20, 21, 22, 23, 24]].any()                 # neck, mid-hip, feet
        np.testing.assert_array_equal(p, p.astype(np.float32))
    path = str(tmp_path / "image_keypoints.json")
    O.write_json(path, people)
    import json
    doc = json.load(open(path))
    assert doc["version"] == 1.3 and [q["person_id"] for q in doc["people"]] == [[-1], [-1]]
    got = io.load_openpose(path)
    np.testing.assert_array_equal(got["pose"], O.select_person(people)["pose"])
    every = io.load_openpose(path, only_one=False)
    for a, b in zip(every, people):
        np.testing.assert_array_equal(a["pose"], b)
    O.write_json(path, [])
    assert io.load_openpose(path) is None and O.select_person([]) is None
