"""The GeneBody view preparation on the MI355X (csrc/views_kernels.hip through genebody.ViewPrep) bit for bit against the numpy
restatement and the reference's get_data (tests/golden/genebody_prep.npz), and the runner end to end."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import genebody_cases as G                                        # noqa: E402
from bodyfitting_amd import assets, genebody as GB, synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "genebody_prep.npz")


def numpy_view(img, msk, L):
    """get_data's lines for one view (:122-131) -> (resized image, resized mask, sum)"""
    top, left, bottom, right = GB.image_cropping(msk)
    im = GB.cv2_resize_linear((img * (msk > 128)[..., None])[top:bottom, left:right].copy(), (L, L))
    return im, GB.cv2_resize_linear(msk[top:bottom, left:right].copy(), (L, L)), int(im.astype(np.int64).sum())


def device_views(prep, imgs, msks, mask_view=True):
    box = prep.bbox(msks)
    H, W = msks[0].shape
    rects = [GB.slice_rect(GB.crop_from_box(*b, H, W), H, W) for b in box]
    return prep.prepare(rects, imgs, [mask_view] * len(imgs))


def textured(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(xx * 3 + yy) % 256, (yy * 5 + 40) % 256, (xx * yy) % 256], -1)
    return (base ^ rng.integers(0, 64, (H, W, 3))).astype(np.uint8)


def test_bbox_equals_np_where():
    rng = np.random.default_rng(0)
    prep = GB.ViewPrep(device=0, L=64)
    for H, W, n in ((2448, 2048, 3), (37, 53, 5), (64, 96, 48), (1, 17, 2)):
        masks = []
        for k in range(n):
            m = np.zeros((H, W), np.uint8)
            t, l = rng.integers(0, H), rng.integers(0, W)
            b, r = rng.integers(t, H), rng.integers(l, W)
            m[t:b + 1, l:r + 1] = rng.integers(0, 256, (b + 1 - t, r + 1 - l)) * (rng.random((b + 1 - t, r + 1 - l)) < 0.3)
            m[t, l] = 200
            if k % 3 == 1:
                m[rng.integers(0, H), rng.integers(0, W)] = rng.integers(1, 129)        # counted by the box (!= 0), not by > 128
            if k % 3 == 2:
                m[:] = 0
                m[rng.integers(0, H), rng.integers(0, W)] = 1                          # a single pixel
            masks.append(m)
        got = prep.bbox(masks)
        for m, g in zip(masks, got):
            ys, xs = np.where(m != 0)
            assert tuple(g) == (ys.min(), xs.min(), ys.max(), xs.max())
    masks = [np.full((40, 40), 3, np.uint8), np.zeros((40, 40), np.uint8)]
    with pytest.raises(ValueError, match="view 1: the mask is empty"):
        prep.bbox(masks)
    with pytest.raises(ValueError, match="single-channel"):
        prep.bbox([np.zeros((4, 4, 3), np.uint8)])
    with pytest.raises(ValueError, match="call bbox"):
        prep.prepare([(0, 0, 4, 4)], [np.zeros((4, 4, 3), np.uint8)])
    prep.close()


def branch_cases(L):
    """(name, image, mask) reaching each image_cropping branch, the wrapped negative start, the clipped non-square crop, crop = 2L,
    crop < L and crop = L"""
    rng = np.random.default_rng(1)
    out = []

    def case(name, H, W, t, l, b, r, vals=255):
        m = np.zeros((H, W), np.uint8)
        m[t:b, l:r] = vals
        out.append((name, textured(rng, H, W), m))

    case("tall centred", 90, 120, 10, 50, 80, 70)
    case("tall left", 90, 120, 10, 0, 80, 12)
    case("tall right", 90, 120, 10, 110, 80, 120)
    case("wide centred", 120, 90, 50, 10, 70, 80)
    case("wide top", 120, 90, 0, 10, 12, 80)
    case("wide bottom", 120, 90, 108, 10, 120, 80)
    case("size > w: wrapped negative start", 80, 50, 2, 45, 78, 50)
    case("size > h: wrapped negative start", 50, 80, 35, 2, 50, 78)
    case("size > w: clipped non-square", 80, 50, 2, 35, 78, 50)
    case("crop = 2L", 2 * L, 2 * L + 10, 1, 20, 2 * L - 1, 30)
    case("crop < L", 20, 25, 2, 5, 18, 20, rng.integers(0, 256, (16, 15)))
    case("crop = L", L, L + 20, 0, 15, L, 25)
    return out


@pytest.mark.parametrize("L", [32, 64])
def test_prepare_equals_numpy_per_branch(L):
    prep = GB.ViewPrep(device=0, L=L, max_views=1)
    for name, img, msk in branch_cases(L):
        t, l, b, r = GB.image_cropping(msk)
        H, W = msk.shape
        if name == "size > w: wrapped negative start":
            assert l < 0 and GB.slice_rect((t, l, b, r), H, W)[1] == 2 * W - (r - l), name
        if name == "size > h: wrapped negative start":
            assert t < 0 and GB.slice_rect((t, l, b, r), H, W)[0] == 2 * H - (b - t), name
        if name == "size > w: clipped non-square":
            assert r > W and GB.slice_rect((t, l, b, r), H, W) == (0, 0, H, W), name
        want_i, want_m, want_s = numpy_view(img, msk, L)
        for mv in (True, False):
            o, om, s = device_views(prep, [img], [msk], mv)
            np.testing.assert_array_equal(o[0], want_i, err_msg=name)
            np.testing.assert_array_equal(om[0], want_m if mv else 0, err_msg=name)
            assert s[0] == want_s, name
    prep.close()


def test_black_frame_threshold():
    """identity resize (crop = L): sum == 10 * 3L^2 is dropped, one more is kept, as np.mean(img) > 10"""
    L = 24
    msk = np.full((L, L), 255, np.uint8)
    img = np.full((L, L, 3), 10, np.uint8)
    img2 = img.copy()
    img2[5, 7, 1] = 11
    annots = {"K": np.tile(np.eye(3, dtype=np.float32), (2, 1, 1)), "RT": np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))}
    prep = GB.ViewPrep(device=0, L=L)
    assert GB.image_cropping(msk) == (0, 0, L, L)
    _, _, s = device_views(prep, [img, img2], [msk, msk])
    assert s.tolist() == [30 * L * L, 30 * L * L + 1]
    out = GB.prepare_frame([img, img2], [msk, msk], annots, [0, 1], [], False, L, prep=prep)
    assert out[4] == [1] and np.mean(out[0][0]) > 10 and np.mean(img) == 10
    prep.close()


def test_batch_of_48_equals_one_at_a_time():
    rng = np.random.default_rng(2)
    L, H, W = 48, 70, 90
    imgs, msks = [], []
    for k in range(48):
        m = np.zeros((H, W), np.uint8)
        t, l = rng.integers(0, H - 4), rng.integers(0, W - 4)
        m[t:rng.integers(t + 2, H), l:rng.integers(l + 2, W)] = rng.integers(100, 256)
        imgs.append(textured(rng, H, W))
        msks.append(m)
    prep = GB.ViewPrep(device=0, L=L)
    o, om, s = device_views(prep, imgs, msks)
    for k in range(48):
        o1, om1, s1 = device_views(prep, [imgs[k]], [msks[k]])
        np.testing.assert_array_equal(o[k], o1[0])
        np.testing.assert_array_equal(om[k], om1[0])
        assert s[k] == s1[0]
        wi, wm, ws = numpy_view(imgs[k], msks[k], L)
        np.testing.assert_array_equal(o[k], wi)
        np.testing.assert_array_equal(om[k], wm)
    prep.close()


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    return G.write_capture(str(tmp_path_factory.mktemp("genebody") / "capture"))


@pytest.mark.parametrize("k", range(len(G.DATA_CASES)))
def test_prepare_frame_equals_reference_get_data(capture, k):
    golden = np.load(GOLDEN)
    subject, frame, use_mask, L = G.DATA_CASES[k]
    views = golden[f"views_{subject}"].tolist()
    imgs, msks = G.read_frame(capture, subject, views, frame)
    annots = np.load(os.path.join(capture, "annots.npy"), allow_pickle=True).item()
    images, masks, Ks, Rts, use_frames, mask_frames = GB.prepare_frame(imgs, msks, annots, views, GB.MASK_FRAMES, use_mask, L)
    assert use_frames == golden[f"data_{k}_use_frames"].tolist()
    assert mask_frames == golden[f"data_{k}_mask_frames"].tolist()
    np.testing.assert_array_equal(np.stack(images), golden[f"data_{k}_images"])
    if mask_frames:
        np.testing.assert_array_equal(np.stack(masks), golden[f"data_{k}_masks"])
    np.testing.assert_array_equal(np.stack(Ks), golden[f"data_{k}_Ks"])
    np.testing.assert_array_equal(np.stack(Rts), golden[f"data_{k}_Rts"])


@pytest.fixture
def registered(monkeypatch):
    models = {t: S.make_model(t, seed=0) for t in ("smpl", "smplx")}
    monkeypatch.setattr(assets, "_MODELS", {(t, g): m for t, m in models.items() for g in ("neutral", "male", "female")})
    monkeypatch.setattr(assets, "_GMM", {"gmm": S.make_gmm(seed=0)})
    monkeypatch.setattr(assets, "_DEVICE_MODELS", {})
    sd, mean = S.make_hmr_weights(0)
    assets.register_hmr(sd, mean)
    assets.register_openpose(S.make_openpose_weights(0))
    assets.register_openpose_hand(S.make_openpose_hand_weights(0))
    yield
    assets.register_hmr(None)
    assets.register_openpose(None)
    assets.register_openpose_hand(None)


@pytest.mark.parametrize("smpl_type,use_mask", [("smpl", True), ("smplx", False)])
def test_runner_end_to_end(tmp_path, registered, smpl_type, use_mask):
    """a 48-view capture whose views are black except the eight mask views: the black-frame test keeps those eight, OpenPose (and, for
    SMPL-X, the hand estimator) runs on them, the JSONs read back are the detected people, and the fit equals BodyFitting called
    directly on the numpy-prepared views; a second run finds the JSONs and skips detection"""
    from bodyfitting_amd import openpose as O, openpose_hand as OH
    from bodyfitting_amd.body_fitting import BodyFitting
    from bodyfitting_amd.io import load_openpose
    L = 64
    root = G.write_capture(str(tmp_path / "capture"), subjects=("zhuna",), frames=1, mask_views_only=True)
    argv = ["--target_dir", root, "--output_dir", str(tmp_path / "out"), "--load_size", str(L), "--smpl_type", smpl_type]
    args = GB.config_parser().parse_args(argv + (["--use_mask"] if use_mask else []))
    args.num_iters = 20
    r = GB.runner(args)
    r.run()
    fdir = tmp_path / "out" / "zhuna" / "000000"
    assert sorted(os.listdir(fdir / "images")) == ["%02d.png" % v for v in GB.MASK_FRAMES]
    assert sorted(os.listdir(fdir / "openpose")) == ["%02d_keypoints.json" % v for v in GB.MASK_FRAMES]
    assert os.path.exists(tmp_path / "out" / "zhuna" / "smpl" / "0000.obj")
    got = np.load(tmp_path / "out" / "zhuna" / "param" / "0000.npy", allow_pickle=True).item()

    views = list(range(48))
    imgs, msks = G.read_frame(root, "zhuna", views, 0)
    annots = np.load(os.path.join(root, "annots.npy"), allow_pickle=True).item()
    images, masks, Ks, Rts, use_frames, mask_frames = G.prepare_frame_numpy(imgs, msks, annots, views, GB.MASK_FRAMES, use_mask, L)
    assert use_frames == GB.MASK_FRAMES
    bgr = np.stack([im[:, :, ::-1] for im in images])
    body = O.OpenPose(device=0, max_batch=4, max_h=1024, max_w=1024)
    if smpl_type == "smplx":
        hand = OH.OpenPoseHand(device=0, max_hands=16, max_h=1024, max_w=1024)
        people = OH.detect_people(body, hand, bgr)
        want_kp = [OH.select_person_entry(p) for p in people]
        hand.close()
    else:
        want_kp = [O.select_person(p) for p in body.pose25(bgr)]
    body.close()
    read = [load_openpose(str(fdir / "openpose" / ("%02d_keypoints.json" % v))) for v in GB.MASK_FRAMES]
    assert any(k is not None for k in want_kp)
    for a, b in zip(read, want_kp):
        assert (a is None) == (b is None)
        if a is not None:
            assert set(a) == set(b)
            for key in a:
                np.testing.assert_array_equal(a[key], b[key])
    opts = SimpleNamespace(**vars(args))
    want = BodyFitting(opts)(images, Rts, Ks, read, gender="neutral", keyframe=use_frames.index(25), use_frames=use_frames,
                             use_mask=use_mask, masks=masks, mask_frames=mask_frames, output_folder=str(tmp_path / "direct"))
    assert set(got) == set(want)
    for key, v in want.items():
        if isinstance(v, np.ndarray):
            np.testing.assert_array_equal(np.asarray(got[key]), v, err_msg=key)

    stamp = {p: os.path.getmtime(fdir / "openpose" / p) for p in os.listdir(fdir / "openpose")}
    r.tasks = ["openpose"]
    r._openpose = SimpleNamespace(pose25=lambda *_: pytest.fail("detection ran although the JSONs exist"))
    r._openpose_hand = None
    OH_detect = OH.detect_people
    OH.detect_people = lambda *_: pytest.fail("detection ran although the JSONs exist")
    try:
        r.run()
    finally:
        OH.detect_people = OH_detect
        r._openpose = None
        r.close()
    assert {p: os.path.getmtime(fdir / "openpose" / p) for p in os.listdir(fdir / "openpose")} == stamp
