"""The LBAM texture inpainter on the MI355X (csrc/inpaint_kernels.hip): every convolution shape against torch fp32 / fp64, the split-K
tail included; the network against the reference's own module (tests/golden/inpaint_synthetic.npz) and against the torch restatement
at a non-square size; known pixels, batches and repeated runs bit for bit; the uint8 bytes; the hole mask, the morphology and
render_texture_map(morph=True) bit for bit against the numpy restatements; TextureFitting.inpaint against the golden; and a short
TextureFitting(inpaint=True) run end to end.

Bands follow tests/test_gpu_openpose.py: max|HIP - fp64| <= 4 * max|torch fp32 - fp64| + 1e-6 * max|fp64|."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
import inpaint_cases as IC
from test_gpu_openpose import band_check
from bodyfitting_amd import _lib, assets, inpaint as I, synthetic as S, texture_dropin as TD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def weights():
    return S.make_lbam_weights(0)


@pytest.fixture(scope="module")
def golden():
    return load_golden("inpaint_synthetic.npz")


@pytest.fixture(scope="module")
def net(weights):
    h = I.Inpainter(weights, device=0, max_batch=4)
    yield h
    h.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# single convolutions
# ---------------------------------------------------------------------------------------------------------------------------------
def _selftest(deconv, x, w_packed, cout, xm=None, wm_packed=None):
    n, H, W, cin = x.shape
    Ho, Wo = (2 * H, 2 * W) if deconv else (H // 2, W // 2)
    y = np.empty((n, Ho, Wo, cout), np.float32)
    ym = np.empty_like(y) if xm is not None else None
    lib = _lib.load()
    _lib.check(lib.bf_inpaint_selftest_conv(0, deconv, n, H, W, cin, cout, _lib.fptr(x), _lib.fptr(xm), _lib.fptr(w_packed),
                                            _lib.fptr(wm_packed), _lib.fptr(y), _lib.fptr(ym)), "bf_inpaint_selftest_conv")
    return y, ym


def _torch(deconv, x, w, dtype):
    t = torch.from_numpy(x).permute(0, 3, 1, 2).to(dtype)
    wt = torch.from_numpy(w).to(dtype)
    with torch.no_grad():
        y = F.conv_transpose2d(t, wt, stride=2, padding=1) if deconv else F.conv2d(t, wt, stride=2, padding=1)
    return y.permute(0, 2, 3, 1).numpy()


def _pad_c(x, c):
    return np.ascontiguousarray(np.concatenate([x, np.zeros(x.shape[:3] + (c - x.shape[3],), x.dtype)], 3)) if x.shape[3] < c else x


# encoder level l: input side 512 >> (l - 1) at a 512^2 texture, capped at 128 (the CPU's fp64 reference); (H, W) not square
ENC_CASES = [(l, I.ENC[l - 1], I.ENC[l], min(512 >> (l - 1), 128)) for l in range(1, 8)]
REV_CASES = [(l, I.REV[l - 1], I.REV[l], min(512 >> (l - 1), 128)) for l in range(1, 7)]
DEC_CASES = [(t, cin, cout, min(4 << (t - 1), 64)) for t, (cin, cout) in enumerate(I.DEC, 1)]


@pytest.mark.parametrize("l,cin,cout,side", ENC_CASES)
def test_encoder_attention_conv(l, cin, cout, side):
    rng = np.random.default_rng(100 + l)
    H, W = side, max(side // 2, 2)
    cm = 3 if l == 1 else cin
    x = rng.standard_normal((3, H, W, cin)).astype(np.float32)
    xm = rng.standard_normal((3, H, W, cm)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 4, 4)) / np.sqrt(16 * cin)).astype(np.float32)
    wm = (rng.standard_normal((cout, cm, 4, 4)) / np.sqrt(16 * cm)).astype(np.float32)
    y3, ym3 = _selftest(0, x, I._pack_conv(w), cout, _pad_c(xm, cin), I._pack_conv(wm, cin))
    band_check(f"ec{l} conv {cin}->{cout} {H}x{W} n=3", y3, _torch(0, x, w, torch.float32), _torch(0, x, w, torch.float64))
    band_check(f"ec{l} maskConv {cm}->{cout}", ym3, _torch(0, xm, wm, torch.float32), _torch(0, xm, wm, torch.float64))
    y1, ym1 = _selftest(0, x[:1].copy(), I._pack_conv(w), cout, _pad_c(xm[:1].copy(), cin), I._pack_conv(wm, cin))
    np.testing.assert_array_equal(y1[0], y3[0])
    np.testing.assert_array_equal(ym1[0], ym3[0])


@pytest.mark.parametrize("l,cin,cout,side", REV_CASES)
def test_reverse_conv(l, cin, cout, side):
    rng = np.random.default_rng(200 + l)
    H, W = max(side // 2, 2), side
    x = rng.random((3, H, W, cin)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 4, 4)) / np.sqrt(16 * cin)).astype(np.float32)
    xp = _pad_c(x, (cin + 3) // 4 * 4)
    y3, _ = _selftest(0, xp, I._pack_conv(w), cout)
    band_check(f"reverseConv{l} {cin}->{cout} {H}x{W} n=3", y3, _torch(0, x, w, torch.float32), _torch(0, x, w, torch.float64))
    y1, _ = _selftest(0, xp[:1].copy(), I._pack_conv(w), cout)
    np.testing.assert_array_equal(y1[0], y3[0])


@pytest.mark.parametrize("t,cin,cout,side", DEC_CASES)
def test_transposed_conv(t, cin, cout, side):
    rng = np.random.default_rng(300 + t)
    H, W = side, max(side // 2, 1)
    x = rng.standard_normal((3, H, W, cin)).astype(np.float32)
    w = (rng.standard_normal((cin, cout, 4, 4)) / np.sqrt(4 * cin)).astype(np.float32)
    y3, _ = _selftest(1, x, I._pack_deconv(w), cout)
    band_check(f"dc{t} {cin}->{cout} {H}x{W} n=3", y3, _torch(1, x, w, torch.float32), _torch(1, x, w, torch.float64))
    y1, _ = _selftest(1, x[:1].copy(), I._pack_deconv(w), cout)
    np.testing.assert_array_equal(y1[0], y3[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# the network
# ---------------------------------------------------------------------------------------------------------------------------------
def _known_exact(image, mask, got):
    known = mask < 128
    np.testing.assert_array_equal(got[known], (image.astype(np.float32) / np.float32(255))[known])


def test_network_against_the_reference_golden(net, golden):
    out64 = IC.golden_out64(golden)
    for i, name in enumerate(golden["mask_names"]):
        got = net(golden["image"], golden["masks"][i])
        band_check(f"LBAM 128^2 {name}", got, golden["out32"][i], out64[i])
        _known_exact(golden["image"], golden["masks"][i], got)


@pytest.fixture(scope="module")
def wide(weights):
    """256 x 512 (not square: an H / W swap shows): image, masks and the torch fp32 / fp64 results of scattered and large"""
    H, W = 256, 512
    image = IC.golden_image(H, W, seed=8)
    masks = IC.masks(H, W, seed=9)
    want = {}
    xs, ms = zip(*(IC.prepare(image, masks[k]) for k in ("scattered", "large")))
    x, m = torch.cat(xs), torch.cat(ms)
    with torch.no_grad():
        for dtype in (torch.float32, torch.float64):
            o = IC.lbam_forward(weights, x.to(dtype), m.to(dtype), dtype)
            o = o * (1 - m.to(dtype)) + x[:, :3].to(dtype) * m.to(dtype)
            want[dtype] = o.permute(0, 2, 3, 1).numpy()
    return image, masks, want


def test_network_against_the_restatement_at_256x512(net, wide):
    image, masks, want = wide
    for j, k in enumerate(("scattered", "large")):
        got = net(image, masks[k])
        band_check(f"LBAM 256x512 {k}", got, want[torch.float32][j], want[torch.float64][j])
        _known_exact(image, masks[k], got)
    np.testing.assert_array_equal(net(image, masks["empty"]), image.astype(np.float32) / np.float32(255))
    np.testing.assert_array_equal(net(image, masks["full"]), np.full(image.shape, 0.5, np.float32))


def test_batch_equals_single_and_runs_repeat(net, wide):
    image, masks, _ = wide
    names = ("scattered", "large", "empty")
    images = np.stack([image, image[::-1].copy(), image[:, ::-1].copy()])
    ms = np.stack([masks[k] for k in names])
    got = net.batch(images, ms)
    for i in range(3):
        np.testing.assert_array_equal(got[i], net(images[i], ms[i]))
    np.testing.assert_array_equal(net.batch(images, ms), got)


def test_bytes_follow_the_fp64_truncation(net, wide):
    image, masks, want = wide
    f32, f64 = want[torch.float32][1], want[torch.float64][1]
    got = net(image, masks["large"])
    band = 4 * np.abs(f32.astype(np.float64) - f64).max() + 1e-6 * np.abs(f64).max()
    q = I.quantize(got).astype(int)
    v = f64 * 255
    q64 = np.trunc(v).astype(int)
    assert np.abs(q - q64).max() <= 1
    far = np.abs(v - np.round(v)) > 255 * band
    np.testing.assert_array_equal(q[far], q64[far])
    print(f"bytes: {int((q != q64).sum())} of {q.size} off by one, all within {255 * band:.2e} of an integer")


# ---------------------------------------------------------------------------------------------------------------------------------
# hole mask, morphology, post-processing
# ---------------------------------------------------------------------------------------------------------------------------------
def _uv_of(text, tmp_path, size):
    p = tmp_path / "uv.obj"
    p.write_text(text)
    return TD.load_obj_uv(str(p)) * size, str(p)


def test_hole_mask_kernels_at_512(net, tmp_path):
    size = 512
    text, _ = IC.uv_obj_text(n=40, seed=13)
    uv, _ = _uv_of(text, tmp_path, size)
    extra = np.array([[[-5.5, 10.2], [40.7, 30.1], [10.3, -3.9]],           # wraps in the sample test, clipped by the fill
                      [[500.2, 3.3], [511.9, 0.4], [505.1, 20.7]],
                      [[100.0, 100.0], [140.0, 100.0], [120.0, 100.0]],        # degenerate: a horizontal line
                      [[300.5, 200.5], [300.5, 200.5], [300.5, 260.5]]], np.float32)
    uv = np.ascontiguousarray(np.concatenate([uv, extra]), np.float32)
    img = IC.texture_image(size, size, seed=17)
    img[0:60, 480:512] = 128
    img[:, 0:20] = 125
    img[190:270, 280:320] = 127
    sel = net.select_faces(img, uv)
    want_sel = I.select_faces(img, uv)
    if (sel != want_sel).any():
        faces = np.flatnonzero(sel != want_sel)
        dims = I.sample_dims()
        numpy_pts = np.stack([(dims @ f).astype(np.int32) for f in uv[faces]])
        kernel_pts = I.sample_points_fma(uv[faces])
        pytest.fail(f"faces {faces.tolist()[:20]} differ; samples where numpy's BLAS and the kernel's fma chain truncate apart: "
                    f"{np.argwhere(numpy_pts != kernel_pts).tolist()[:20]}")
    assert 0 < sel.sum() < len(sel)
    want_mask, _ = I.hole_mask(img, uv)
    np.testing.assert_array_equal(net.hole_mask(img, uv), want_mask)
    bad = np.array([[[10, 10], [512, 10], [10, 20]]], np.float32)
    with pytest.raises(_lib.BodyfitError, match="outside the image"):
        net.hole_mask(img, bad)


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("C", [1, 3])
def test_morphology_kernels(k, C):
    a = np.random.default_rng(k * 10 + C).integers(0, 256, (2, 37, 53, C)).astype(np.uint8)
    a[0, 5:9, 7:30] = 255
    a[1, 20:, :3] = 0
    for op, fn in ((I.MORPH_ERODE, I.erode), (I.MORPH_DILATE, I.dilate)):
        got = I.morph_u8(op, k, a)
        for i in range(2):
            np.testing.assert_array_equal(got[i], fn(a[i], k))
    np.testing.assert_array_equal(I.morph_u8(I.MORPH_DILATE, k, a[0, :, :, 0]), I.dilate(a[0, :, :, 0], k))


def test_render_texture_map_morph(tmp_path):
    text, _ = IC.uv_obj_text(n=6, seed=3)
    _, obj = _uv_of(text, tmp_path, 1)
    rng = np.random.default_rng(4)
    rgb = rng.random((3, 96, 96)).astype(np.float32)
    depth = np.where(rng.random((96, 96)) < 0.3, 100.0, 1.0).astype(np.float32)
    depth[40:60, 10:50] = 100.0

    class FakeRenderer:
        device = 0

        def render_texture(self, uv, uv_faces, textures):
            return rgb, depth
    got = TD.render_texture_map(FakeRenderer(), obj, morph=True)
    tex = TD.to8b(rgb.transpose((1, 2, 0))[:, :, ::-1])
    np.testing.assert_array_equal(got, I.morph_texture(tex, depth))
    np.testing.assert_array_equal(TD.render_texture_map(FakeRenderer(), obj, morph=False), tex)


def test_texture_inpaint_against_the_golden(weights, golden, tmp_path, monkeypatch):
    text, _ = IC.uv_obj_text()
    uv, obj = _uv_of(text, tmp_path, 128)
    np.testing.assert_array_equal(uv, golden["tex_uv"])
    assets.register_inpainter(weights)
    try:
        tf = TD.TextureFitting(obj, inpaint=True)
        img = golden["tex_img"]
        got = tf.inpaint(img.copy())
    finally:
        assets.register_inpainter(None)
    inp = tf.inpainter
    out, mask = inp.texture(img, uv, return_mask=True)
    np.testing.assert_array_equal(out, got)
    np.testing.assert_array_equal(mask, golden["tex_mask"])
    net = inp(img, mask)
    np.testing.assert_array_equal(got, I.postprocess(I.quantize(net)))
    # the network's bytes follow the fp64 truncation; outside the holes' reach (15 x 15 around them) the result is the golden's
    f64 = IC.golden_out64(golden, "tex_net")
    band = 4 * np.abs(golden["tex_net32"].astype(np.float64) - f64).max() + 1e-6 * np.abs(f64).max()
    band_check("TextureFitting.inpaint network", net, golden["tex_net32"], f64)
    q, q64 = I.quantize(net).astype(int), np.trunc(f64 * 255).astype(int)
    assert np.abs(q - q64).max() <= 1
    far = np.abs(f64 * 255 - np.round(f64 * 255)) > 255 * band
    np.testing.assert_array_equal(q[far], q64[far])
    reach = I.dilate(golden["tex_mask"], 15) > 0
    np.testing.assert_array_equal(got[~reach], golden["tex_out"][~reach])
    print(f"TextureFitting.inpaint: {int((got != golden['tex_out']).sum())} bytes differ from the reference's, all within the holes' reach")


def test_texture_fitting_inpaint_end_to_end(weights, tmp_path):
    from PIL import Image
    from test_gpu_obj_textures import _write_texfit_inputs
    scan_path, smpld, uv_obj, _, _ = _write_texfit_inputs(str(tmp_path))
    size, iters = 128, 4
    outs = {}
    assets.register_inpainter(weights)
    try:
        for inpaint in (False, True):
            out = str(tmp_path / f"texfit_{int(inpaint)}")
            np.random.seed(5)
            tf = TD.TextureFitting(uv_obj, tex_img_size=64, render_img_size=size, iter_num=iters, render=False, inpaint=inpaint)
            tf(out, smpld, scan_path)
            outs[inpaint] = np.asarray(Image.open(os.path.join(out, "smpl.png")))
    finally:
        assets.register_inpainter(None)
    want = tf.inpainter.texture(outs[False], TD.load_obj_uv(uv_obj) * size)
    np.testing.assert_array_equal(outs[True], want)
    mask = I.hole_mask(outs[False], TD.load_obj_uv(uv_obj) * size)[0]
    assert mask.any() and (outs[True] != outs[False]).any()
