"""The GeneBody runner's host side (bodyfitting_amd/genebody.py) against the reference's apps/genebody_fitting.py, through the golden
tools/gen_genebody_golden.py wrote (tests/golden/genebody_prep.npz), without a GPU: the view preparation object is replaced by a
numpy stand-in here; the kernels themselves are tests/test_gpu_genebody.py's."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import genebody_cases as G                                        # noqa: E402
from bodyfitting_amd import genebody as GB                        # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "genebody_prep.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    return G.write_capture(str(tmp_path_factory.mktemp("genebody") / "capture"))


class NumpyPrep:
    """ViewPrep's contract in numpy (the stand-in for the device object of the runner tests)"""

    def __init__(self, L):
        self.L = L

    def bbox(self, masks, names=None):
        out = []
        for i, m in enumerate(masks):
            ys, xs = np.nonzero(m)
            if ys.size == 0:
                raise ValueError(f"view {names[i] if names else i}: the mask is empty")
            out.append((ys.min(), xs.min(), ys.max(), xs.max()))
        self._masks = [np.asarray(m) for m in masks]
        return np.asarray(out, np.int32)

    def prepare(self, rects, images, mask_view=None):
        n, L = len(images), self.L
        out, msk, sums = np.zeros((n, L, L, 3), np.uint8), np.zeros((n, L, L), np.uint8), np.zeros(n, np.int64)
        for i, ((t, l, b, r), im, m) in enumerate(zip(rects, images, self._masks)):
            img = (np.asarray(im) * (m > 128)[..., None])[t:b, l:r]
            out[i] = GB.cv2_resize_linear(img, (L, L))
            sums[i] = int(out[i].astype(np.int64).sum())
            if mask_view is not None and mask_view[i]:
                msk[i] = GB.cv2_resize_linear(m[t:b, l:r], (L, L))
        return out, msk, sums


def args_for(root, out, subject="zhuna", **kw):
    a = GB.config_parser().parse_args(["--target_dir", root, "--output_dir", out, "--subject", subject])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def check_data(got, golden, k):
    images, masks, Ks, Rts, use_frames, mask_frames = got
    assert use_frames == golden[f"data_{k}_use_frames"].tolist()
    assert mask_frames == golden[f"data_{k}_mask_frames"].tolist()
    np.testing.assert_array_equal(np.stack(images), golden[f"data_{k}_images"])
    if mask_frames:
        np.testing.assert_array_equal(np.stack(masks), golden[f"data_{k}_masks"])
    else:
        assert masks == []
    for name, arr in (("Ks", Ks), ("Rts", Rts)):
        assert all(a.dtype == np.float32 for a in arr)
        np.testing.assert_array_equal(np.stack(arr), golden[f"data_{k}_{name}"])


def test_image_cropping_equals_the_reference(golden):
    masks = G.crop_masks()
    got = np.asarray([[int(x) for x in GB.image_cropping(m)] for m in masks])
    np.testing.assert_array_equal(got, golden["crop"])
    # the cases reach the negative start of size > w and of size > h, and crops past the right and bottom edges
    assert (got[:, 1] < 0).any() and (got[:, 0] < 0).any()
    assert any(r[3] > m.shape[1] for r, m in zip(got, masks)) and any(r[2] > m.shape[0] for r, m in zip(got, masks))


def test_image_cropping_of_an_empty_mask_raises():
    with pytest.raises(ValueError):
        GB.image_cropping(np.zeros((8, 8), np.uint8))


def test_slice_rect_is_numpy_slicing():
    a = np.zeros((20, 30))
    for crop in ((0, -12, 20, 30), (0, -5, 20, 30), (-3, 2, 25, 40), (2, 3, 9, 31)):
        t, l, b, r = GB.slice_rect(crop, 20, 30)
        assert a[crop[0]:crop[2], crop[1]:crop[3]].shape == (b - t, r - l)
    with pytest.raises(ValueError, match="empty"):
        GB.slice_rect((0, -10, 20, 5), 20, 30)


@pytest.mark.parametrize("k", range(len(G.DATA_CASES)))
def test_numpy_restatement_equals_reference_get_data(golden, capture, k):
    """cv2_resize_linear (and the rest of get_data's lines) bit for bit against the reference's get_data output"""
    subject, frame, use_mask, L = G.DATA_CASES[k]
    views = golden[f"views_{subject}"].tolist()
    imgs, msks = G.read_frame(capture, subject, views, frame)
    annots = np.load(os.path.join(capture, "annots.npy"), allow_pickle=True).item()
    check_data(G.prepare_frame_numpy(imgs, msks, annots, views, GB.MASK_FRAMES, use_mask, L), golden, k)


def test_resize_known_answers():
    rng = np.random.default_rng(3)
    for shape in ((17, 17, 3), (40, 40), (64, 64, 3)):
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        np.testing.assert_array_equal(GB.cv2_resize_linear(a, (shape[1], shape[0])), a)          # identity at n_src == L
        h = a.astype(np.int64)
        if shape[0] % 2 == 0:                                     # exact 2x: INTER_AREA's 2 x 2 mean, (sum + 2) >> 2
            s = h[0::2, 0::2] + h[0::2, 1::2] + h[1::2, 0::2] + h[1::2, 1::2]
            np.testing.assert_array_equal(GB.cv2_resize_linear(a, (shape[1] // 2, shape[0] // 2)), ((s + 2) >> 2).astype(np.uint8))
    for v in (0, 1, 77, 255):
        c = np.full((23, 31, 3), v, np.uint8)
        for L in (5, 31, 64, 100):
            np.testing.assert_array_equal(GB.cv2_resize_linear(c, (L, L)), np.full((L, L, 3), v, np.uint8))


def test_views_sequence_and_defaults(golden, capture):
    for subject in G.SUBJECTS:
        r = object.__new__(GB.runner)
        r.subject, r.target_dir = subject, os.path.join(capture, subject)
        assert r.get_views() == golden[f"views_{subject}"].tolist()
        assert r.get_sequence() == golden[f"seq_{subject}"].tolist()
    got = vars(GB.config_parser().parse_args([]))
    assert got.pop("device") == 0
    assert json.loads(json.dumps(got, sort_keys=True)) == json.loads(str(golden["defaults"]))
    j = object.__new__(GB.runner)
    j.subject = "joseph_matanda"
    assert j.get_views() == list(range(39)) + [41]


@pytest.mark.parametrize("k", range(len(G.DATA_CASES)))
def test_runner_get_data_with_a_stub_device(golden, capture, tmp_path, k):
    """the runner's get_data (decode, prepare_frame, PNG writes) with the device object injected: cameras by enumerate index (the
    wuwenyan case has views 34 and 36 excluded), the black and dim views dropped, the kept views written"""
    subject, frame, use_mask, L = G.DATA_CASES[k]
    r = GB.runner(args_for(capture, str(tmp_path), subject, use_mask=use_mask, load_size=L), prep=NumpyPrep(L))
    got = r.get_data(frame)
    check_data(got, golden, k)
    img_dir = tmp_path / subject / ("%06d" % frame) / "images"
    assert sorted(os.listdir(img_dir)) == ["%02d.png" % v for v in got[4]]
    np.testing.assert_array_equal(GB.read_image(img_dir / ("%02d.png" % got[4][-1])), got[0][-1])
    r.close()


def test_keyframe_choice():
    r = object.__new__(GB.runner)
    assert r.keyframe(list(range(48))) == 25
    assert r.keyframe([1, 7, 13, 19, 25, 31, 37, 43]) == 4                  # view 25, at its index in the kept list
    assert r.keyframe([3, 4, 30]) == 0                                     # view 25 dropped: the first kept view


def test_output_layout_and_openpose_skip(capture, tmp_path, monkeypatch):
    """run(): the openpose task skips detection when enough JSONs exist, read_openpose reads them in sorted order, the smplify task
    calls BodyFitting as :165-170 does and the output task copies what it wrote"""
    from bodyfitting_amd import openpose as O
    r = GB.runner(args_for(capture, str(tmp_path), use_mask=True, load_size=40), prep=NumpyPrep(40))
    r.seqs = [0]
    fdir = tmp_path / "zhuna" / "000000"
    (fdir / "openpose").mkdir(parents=True)
    people = {v: [np.full((25, 3), v + 1.0)] for v in range(48)}
    for v in range(48):
        O.write_json(str(fdir / "openpose" / ("%02d_keypoints.json" % v)), people[v])
    monkeypatch.setattr(O, "OpenPose", lambda *a, **k: pytest.fail("detection ran although the JSONs exist"))
    calls = []

    def fitter(images, Rts, Ks, keypoints, **kw):
        calls.append((images, Rts, Ks, keypoints, kw))
        out = kw["output_folder"]
        os.makedirs(out, exist_ok=True)
        np.save(os.path.join(out, "smpl_parameter.npy"), {"betas": np.zeros(10)})
        open(os.path.join(out, "smpl.obj"), "w").write("v 0 0 0\n")
        return {}

    r.bodyfitter = fitter
    r.run()
    (images, Rts, Ks, keypoints, kw) = calls[0]
    assert kw["use_frames"] == [v for v in range(48) if v not in (G.BLACK_VIEW, G.DIM_VIEW)]
    assert kw["keyframe"] == kw["use_frames"].index(25) and kw["gender"] == "neutral" and kw["use_mask"] is True
    assert kw["mask_frames"] == GB.MASK_FRAMES and len(kw["masks"]) == 8
    assert len(keypoints) == 48 and keypoints[3]["pose"][0, 0] == 4.0
    assert os.path.exists(tmp_path / "zhuna" / "smpl" / "0000.obj")
    assert np.load(tmp_path / "zhuna" / "param" / "0000.npy", allow_pickle=True).item()["betas"].shape == (10,)
    r.close()


def test_info_dir_gender(capture, tmp_path):
    info = tmp_path / "info.csv"
    info.write_text("zhuna,0\nwuwenyan,1\n")
    assert GB.runner(args_for(capture, str(tmp_path), info_dir=str(info)), prep=NumpyPrep(512)).gender == "female"
    assert GB.runner(args_for(capture, str(tmp_path), "wuwenyan", info_dir=str(info)), prep=NumpyPrep(512)).gender == "male"


def test_masks_must_be_single_channel():
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="single-channel"):
        GB.prepare_frame([img], [np.zeros((8, 8, 3), np.uint8)], {"K": np.eye(3)[None], "RT": np.eye(4)[None]}, [0], [], False, 4,
                         prep=NumpyPrep(4))


def test_io_threads(monkeypatch):
    monkeypatch.delenv("OMP_NUM_THREADS", raising=False)
    assert GB.io_threads() == 8
    monkeypatch.setenv("OMP_NUM_THREADS", "64")
    assert GB.io_threads() == 16
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    assert GB.io_threads() == 3
