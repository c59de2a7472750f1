"""The LBAM texture inpainter on the CPU: the weights (keys, loading, packing, clamps), the torch restatement of the network against
the reference's own module (tests/golden/inpaint_synthetic.npz, tools/gen_inpaint_golden.py), the face test against the golden, the
filled-contour rule by known answers (cv2 is absent, as oracle/contour_oracle.py pins findContours), the morphology against scipy,
the input checks, the drop-in imports and TextureFitting(inpaint=True)'s construction."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

from conftest import load_golden
import inpaint_cases as IC
from bodyfitting_amd import assets, hmr, inpaint as I, synthetic as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def weights():
    return S.make_lbam_weights(0)


@pytest.fixture(scope="module")
def golden():
    return load_golden("inpaint_synthetic.npz")


# ---------------------------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_and_shapes(weights):
    keys = I.expected_keys()
    assert len(keys) == 79
    assert sum(int(np.prod(s)) for s in keys.values()) == 68304948          # LBAMModel(4, 3): 68.3 M parameters, no biases
    assert set(weights) == set(keys)
    for k, v in weights.items():
        assert np.shape(v) == keys[k], k


def test_match_state_is_strict(weights):
    assert set(I.match_state(weights)) == set(weights)
    missing = dict(weights)
    del missing["dc3.conv.weight"]
    with pytest.raises(ValueError, match="missing key 'dc3.conv.weight'"):
        I.match_state(missing)
    extra = dict(weights, **{"vgg.enc_1.0.weight": np.zeros(1, np.float32)})
    with pytest.raises(ValueError, match="unexpected key 'vgg.enc_1.0.weight'"):
        I.match_state(extra)
    bad = dict(weights, **{"ec2.conv.maskConv.weight": np.zeros((128, 64, 3, 3), np.float32)})
    with pytest.raises(ValueError, match="ec2.conv.maskConv.weight"):
        I.match_state(bad)


@pytest.mark.parametrize("legacy", [False, True])
def test_load_checkpoint_round_trips_torch_save(weights, tmp_path, legacy):
    path = str(tmp_path / "lbam.pth")
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()}
    torch.save(sd, path, _use_new_zipfile_serialization=not legacy)
    got = I.load_weights(path)
    assert set(got) == set(weights)
    for k, v in weights.items():
        np.testing.assert_array_equal(got[k], np.asarray(v, np.float32))
    assert hmr.load_checkpoint(path).keys() == sd.keys()


def test_pack_applies_the_gauss_clamps(weights):
    raw = np.array([[weights[f"ec{l}.conv.activationFuncG_A.{g}"] for g in I.GAUSS_NAMES] for l in range(1, 8)], np.float32)
    lo, hi = I.GAUSS_LO_64.astype(np.float32), I.GAUSS_HI_64.astype(np.float32)
    assert ((raw < lo) | (raw > hi)).any(), "the synthetic parameters should reach outside the clamp ranges"
    packed = I.pack(I.match_state(weights))
    assert packed.dtype == np.float32
    g = packed[-13 * 4:].reshape(13, 4)
    np.testing.assert_array_equal(g[6:], np.minimum(np.maximum(raw, lo), hi))
    assert (g >= lo).all() and (g <= hi).all()


def test_pack_size_and_layout(weights):
    """the packed array: conv weights [16 cin_pad][cout_pad] in (ky, kx, ci) order, ConvTranspose2d per phase, the Gauss parameters
    last - the sizes inpaint_api.hip's IpLayout walks"""
    packed = I.pack(I.match_state(weights))
    n = 16 * 4 * 64                                                    # reverseConv1 (3 -> 4 input channels)
    n += sum(16 * I.REV[l - 1] * I.REV[l] for l in range(2, 7))
    n += 2 * sum(16 * I.ENC[l - 1] * I.ENC[l] for l in range(1, 8))  # ec1's maskConv padded 3 -> 4
    n += sum(16 * cin * ((cout + 3) // 4 * 4) for cin, cout in I.DEC)
    assert packed.size == n + 13 * 4
    # ec2's conv at (ky, kx, ci, co) = (1, 2, 5, 7)
    at = 16 * 4 * 64 + sum(16 * I.REV[l - 1] * I.REV[l] for l in range(2, 7)) + 2 * 16 * 4 * 64
    assert packed[at + ((1 * 4 + 2) * 64 + 5) * 128 + 7] == weights["ec2.conv.conv.weight"][7, 5, 1, 2]
    # dc7 phase (py, px) = (1, 0), tap (ty, tx) = (0, 1): kernel (KY[1][0], KY[0][1]) = (0, 3)
    at7 = n - 16 * 128 * 4
    assert packed[at7 + (2 * 4 * 128 + (1 * 128 + 9)) * 4 + 2] == weights["dc7.weight"][9, 2, 0, 3]


# ---------------------------------------------------------------------------------------------------------------------------------
# the network restatement against the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def test_lbam_forward_equals_the_reference(weights, golden):
    out64 = IC.golden_out64(golden)
    for i, name in enumerate(golden["mask_names"]):
        f64 = IC.inpaint_forward(weights, golden["image"], golden["masks"][i], torch.float64)
        f32 = IC.inpaint_forward(weights, golden["image"], golden["masks"][i], torch.float32)
        scale = max(np.abs(out64[i]).max(), 1e-30)
        assert np.abs(f64 - out64[i]).max() <= 1e-12 * scale, name
        band = 4 * np.abs(golden["out32"][i].astype(np.float64) - out64[i]).max() + 1e-6 * scale
        assert np.abs(f32 - out64[i]).max() <= band, name


def test_synthetic_network_is_not_degenerate(weights, golden):
    i = list(golden["mask_names"]).index("large")
    x, m = IC.prepare(golden["image"], golden["masks"][i])
    with torch.no_grad():
        _, d7 = IC.lbam_forward(weights, x, m, torch.float32, pre_tanh=True)
    d7 = d7.numpy()
    assert (np.abs(d7) < 2).mean() >= 0.25
    assert d7.std() > 0.05
    hole = golden["masks"][i][:, :, 0] >= 128
    spread = golden["out32"][i][hole]
    assert spread.std() > 0.02 and spread.min() < spread.max()


def test_known_pixels_are_the_input(golden):
    for i in range(len(golden["mask_names"])):
        known = golden["masks"][i] < 128
        np.testing.assert_array_equal(golden["out32"][i][known], (golden["image"].astype(np.float32) / np.float32(255))[known])


# ---------------------------------------------------------------------------------------------------------------------------------
# the hole mask
# ---------------------------------------------------------------------------------------------------------------------------------
def test_face_selection_equals_the_golden(golden):
    sel = I.select_faces(golden["tex_img"], golden["tex_uv"])
    np.testing.assert_array_equal(np.flatnonzero(sel), golden["tex_sel"])
    mask, sel2 = I.hole_mask(golden["tex_img"], golden["tex_uv"])
    np.testing.assert_array_equal(sel2, sel)
    np.testing.assert_array_equal(mask, golden["tex_mask"])


def test_face_samples_kernel_rule_matches_numpy(golden):
    """the kernel computes each sample as fma(d2, u2, fma(d1, u1, d0 u0)); numpy's `dims @ face` goes through BLAS.  Every sample of
    the golden's faces truncates the same way under both (a mismatch is listed, not hidden)."""
    uv = golden["tex_uv"][:300]
    dims = I.sample_dims()
    want = np.stack([(dims @ f).astype(np.int32) for f in uv]).astype(np.int64)
    got = I.sample_points_fma(uv)
    bad = np.argwhere(want != got)
    assert len(bad) == 0, f"{len(bad)} samples truncate differently: (face, sample, axis) {bad[:10].tolist()}"


def _filled(tri, H=40, W=40):
    m = np.zeros((H, W), np.uint8)
    I.fill_triangle(m, np.array(tri, np.int32))
    return m > 0


def _bresenham8(p, q):
    m = np.zeros((40, 40), np.uint8)
    I.line8(m, p, q)
    return m > 0


def test_fill_contains_vertices_and_edges():
    rng = np.random.default_rng(1)
    for _ in range(50):
        tri = rng.integers(0, 40, (3, 2))
        f = _filled(tri)
        for x, y in tri:
            assert f[y, x]
        for a, b in ((0, 1), (1, 2), (2, 0)):
            e = _bresenham8(tuple(tri[a]), tuple(tri[b]))
            assert (f | ~e).all()


def test_line8_is_8_connected_from_end_to_end():
    for p, q in (((2, 3), (30, 11)), ((30, 11), (2, 3)), ((5, 30), (9, 1)), ((0, 0), (0, 0)), ((7, 7), (20, 7))):
        e = _bresenham8(p, q)
        ys, xs = np.nonzero(e)
        assert e[p[1], p[0]] and e[q[1], q[0]]
        assert len(xs) == max(abs(p[0] - q[0]), abs(p[1] - q[1])) + 1


def test_fill_of_a_rectangle_is_the_rectangle():
    m = np.zeros((30, 30), np.uint8)
    for tri in (((3, 4), (17, 4), (17, 21)), ((3, 4), (17, 21), (3, 21))):
        I.fill_triangle(m, np.array(tri, np.int32))
    want = np.zeros((30, 30), bool)
    want[4:22, 3:18] = True
    np.testing.assert_array_equal(m > 0, want)


def test_degenerate_triangle_fills_a_line():
    f = _filled(((2, 2), (10, 10), (20, 20)))
    want = np.zeros((40, 40), bool)
    want[np.arange(2, 21), np.arange(2, 21)] = True
    np.testing.assert_array_equal(f, want)
    f = _filled(((2, 5), (30, 5), (11, 5)))                      # horizontal: no edges to fill, the lines alone
    want = np.zeros((40, 40), bool)
    want[5, 2:31] = True
    np.testing.assert_array_equal(f, want)


def test_fill_covers_the_interior_and_nothing_far_from_it():
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[0:40, 0:40]
    for _ in range(60):
        tri = rng.integers(0, 40, (3, 2)).astype(np.float64)
        f = _filled(tri.astype(np.int32))
        (x0, y0), (x1, y1), (x2, y2) = tri
        area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
        if area == 0:
            continue
        s = np.sign(area)
        d = []
        for (ax, ay), (bx, by) in (((x0, y0), (x1, y1)), ((x1, y1), (x2, y2)), ((x2, y2), (x0, y0))):
            d.append(s * ((bx - ax) * (yy - ay) - (by - ay) * (xx - ax)) / np.hypot(bx - ax, by - ay))
        d = np.stack(d)
        inside = (d > 0).all(0)
        assert f[inside].all(), tri
        assert (d[:, f] > -1.0 - 1e-9).all(), tri                 # every filled pixel within 1 px of each edge's inner side


def test_fill_clips_at_the_image_border():
    m = np.zeros((20, 20), np.uint8)
    I.fill_triangle(m, np.array(((-10, -4), (30, 5), (8, 40)), np.int32))
    assert m[10, 10] and m.sum() > 0
    m2 = np.zeros((20, 20), np.uint8)
    I.fill_triangle(m2, np.array(((-10, -10), (-5, -3), (-8, -1)), np.int32))
    assert m2.sum() == 0


def test_face_test_raises_on_an_index_past_the_end():
    img = np.full((128, 128, 3), 128, np.uint8)
    with pytest.raises(IndexError):
        I.select_faces(img, np.array([[[10, 10], [128, 10], [10, 20]]], np.float32))
    sel = I.select_faces(img, np.array([[[-10, 10], [-20, 10], [-10, 20]]], np.float32))    # negative indices wrap
    assert sel[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# morphology and post-processing
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("shape", [(13, 29), (21, 10, 3), (7, 9, 1)])
def test_morphology_equals_scipy(k, shape):
    a = np.random.default_rng(k).integers(0, 256, shape).astype(np.uint8)
    size = (k, k) + (1,) * (len(shape) - 2)
    np.testing.assert_array_equal(I.erode(a, k), ndimage.grey_erosion(a, size=size, mode="nearest"))
    np.testing.assert_array_equal(I.dilate(a, k), ndimage.grey_dilation(a, size=size, mode="nearest"))


def test_postprocess_equals_the_golden(golden):
    want = golden["tex_out"]
    got = I.postprocess(I.quantize(golden["tex_net32"]))
    np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------------------
# input checks, imports, construction
# ---------------------------------------------------------------------------------------------------------------------------------
def test_sizes_not_multiple_of_128_raise_before_the_gpu(weights, monkeypatch):
    from bodyfitting_amd import _lib

    def no_gpu():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_gpu)
    inp = I.Inpainter(weights)
    for H, W in ((128, 200), (100, 128), (0, 128)):
        img = np.zeros((H, W, 3), np.uint8)
        with pytest.raises(ValueError, match="multiples of 128"):
            inp(img, img)
    with pytest.raises(ValueError):
        inp(np.zeros((128, 128, 3), np.uint8), np.zeros((128, 256, 3), np.uint8))


def test_dropin_imports_resolve():
    d = os.path.join(REPO, "bodyfitting_amd", "dropin")
    sys.path.insert(0, d)
    try:
        for m in ("models", "models.inpaint", "models.smpl", "smplify", "smplify.texture_fitting"):
            sys.modules.pop(m, None)
        from models import Inpainter
        from models.inpaint import Inpainter as Inpainter2
        from smplify.texture_fitting import TextureFitting
    finally:
        sys.path.remove(d)
        for m in ("models", "models.inpaint", "models.smpl", "smplify", "smplify.texture_fitting"):
            sys.modules.pop(m, None)
    from bodyfitting_amd import texture_dropin as TD
    assert Inpainter is I.Inpainter and Inpainter2 is I.Inpainter
    assert TextureFitting is TD.TextureFitting


def test_texture_fitting_with_inpaint_constructs(weights, tmp_path, monkeypatch):
    from bodyfitting_amd import texture_dropin as TD
    monkeypatch.chdir(tmp_path)
    assets.register_inpainter(weights)
    try:
        tf = TD.TextureFitting("smpl_uv.obj", inpaint=True)
        assert tf.is_inpaint and tf.inpainter is None                  # the GPU network opens on the first inpaint
        assert tf._inpaint_weights.size == I.pack(I.match_state(weights)).size
    finally:
        assets.register_inpainter(None)


def test_texture_fitting_reads_the_weights_file(weights, tmp_path, monkeypatch):
    from bodyfitting_amd import texture_dropin as TD
    monkeypatch.chdir(tmp_path)
    os.makedirs("external")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()}, os.path.join("external", "LBAM_NoBN_ParisStreetView.pth"))
    assets.register_inpainter(None)
    try:
        tf = TD.TextureFitting("smpl_uv.obj", inpaint=True)
        np.testing.assert_array_equal(tf._inpaint_weights, I.pack(I.match_state(weights)))
    finally:
        assets.register_inpainter(None)


def test_missing_weights_error_is_both_kinds(tmp_path, monkeypatch):
    from bodyfitting_amd import texture_dropin as TD
    monkeypatch.chdir(tmp_path)
    assets.register_inpainter(None)
    with pytest.raises(FileNotFoundError, match="register_inpainter"):
        TD.TextureFitting("smpl_uv.obj", inpaint=True)
    with pytest.raises(NotImplementedError, match="DESIGN.md"):
        TD.TextureFitting("smpl_uv.obj", inpaint=True)
    with pytest.raises(assets.InpainterWeightsMissing, match="LBAM_NoBN_ParisStreetView.pth"):
        I.Inpainter()
