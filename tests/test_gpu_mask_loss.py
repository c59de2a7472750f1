"""bf_silhouette_* (native.Silhouette) and the drop-in `smplify.loss.extract_countours` / `multview_mask_loss` on the MI355X.

Oracle: torch autograd of oracle.smplify_oracle.multview_mask_loss with respect to the vertices (mask_loss_cases.references): float64
with exact distances is the truth, the same function in float32 (pairwise "exact" / "torch") sets the band - DESIGN.md 2.3's rule,
scan_loss_cases.Band: value max(3e-6, 8 rel32), gradient block max(5e-6 M, 8 err32).  Every case is built well posed on the CPU
(tests/test_mask_loss_autograd.py asserts and prints the margins); nothing is skipped, filtered or compared by share, except against
the golden of the imported reference, whose inputs are what they are.  Every check prints its position inside its band; the last
test prints the worst.
"""
import numpy as np
import pytest
import torch

import mask_loss_cases as MC
from conftest import load_golden
from bodyfitting_amd import _lib, assets
from bodyfitting_amd import loss as L
from bodyfitting_amd import native as N
from oracle import contour_oracle as CO

pytestmark = pytest.mark.gpu
BAND = MC.Band()
FORMS = (("exact", False), ("cdist", True))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def silhouettes():
    """name -> native.Silhouette with the case's contours handed over (the oracle's)"""
    made = {}

    def get(name):
        if name not in made:
            b = MC.build(name)
            made[name] = N.Silhouette(b["masks"], b["contours"], device=0)
        return made[name]

    yield get
    for s in made.values():
        s.close()


def _loss(sil, name, cdist, **kw):
    b = MC.build(name)
    c = b["case"]
    return sil.loss(b["verts"], b["w2c"], b["K"], imsize=c.imsize, epsilon=c.eps, stride=MC.STRIDE, cdist_form=cdist, **kw)


@pytest.mark.parametrize("name", MC.CASE_NAMES)
def test_case_against_the_oracle_in_both_distance_forms(silhouettes, name):
    b, ref = MC.build(name), MC.references(name)
    c, sil = b["case"], silhouettes(name)
    v64, g64 = ref["f64"]
    for form, cdist in FORMS:
        value, terms, grad = _loss(sil, name, cdist)
        BAND.value(f"{name} {form} value", value, v64, ref[form][0])
        BAND.block(f"{name} {form} dverts", grad, g64, ref[form][1])
        # the value is the view terms added in memory order, in float32
        tot = np.float32(0)
        for t in terms.reshape(-1):
            tot = np.float32(tot + t)
        assert _bits(tot) == _bits(value)
        assert not _bits(grad[np.arange(c.n_verts) % MC.STRIDE != 0]).any()           # unsampled vertices: bit-zero
        for i in c.away:
            assert _bits(terms[i, 0]) == 0                                              # no inside vertex: the binary term only
        if c.mask == "full":
            assert not _bits(terms[:, 1]).any()                                         # all foreground: no binary term
        # the drop-in function on tensors: the native call's bits, and .backward()
        v = torch.tensor(b["verts"][None], requires_grad=True)
        out = L.multview_mask_loss([torch.tensor(k).reshape(-1, 1, 2) for k in b["contours"]], torch.tensor(b["masks"]), v, None,
                                   torch.tensor(b["w2c"]), torch.tensor(b["K"]), list(range(c.M)), epsilon=c.eps, imsize=c.imsize,
                                   pairwise=None if cdist else "exact")
        assert out.shape == () and out.dtype == torch.float32 and _bits(out.detach().numpy()) == _bits(value)
        out.backward()
        np.testing.assert_array_equal(_bits(v.grad.numpy()[0]), _bits(grad))


@pytest.mark.parametrize("name", ["ns17", "ns257", "views8", "view_without_inside_vertex", "contour1100", "all_foreground"])
def test_bits(silhouettes, name):
    """two calls give equal bits; want_grad=False returns the same value bits; every view's row of view_terms and its share of the
    gradient are those of the view alone; cotangents 1, -2.5 and 0 scale the gradient, a zero cotangent gives a bit-zero one"""
    b = MC.build(name)
    c, sil = b["case"], silhouettes(name)
    for form, cdist in FORMS:
        value, terms, grad = _loss(sil, name, cdist)
        again = _loss(sil, name, cdist)
        assert _bits(again[0]) == _bits(value)
        np.testing.assert_array_equal(_bits(again[1]), _bits(terms))
        np.testing.assert_array_equal(_bits(again[2]), _bits(grad))
        value_only = _loss(sil, name, cdist, want_grad=False)
        assert value_only[2] is None and _bits(value_only[0]) == _bits(value)
        np.testing.assert_array_equal(_bits(value_only[1]), _bits(terms))
        total = np.zeros_like(grad)
        for i in range(c.M):
            one = N.Silhouette(b["masks"][i:i + 1], b["contours"][i:i + 1], device=0)
            v1, t1, g1 = one.loss(b["verts"], b["w2c"][i:i + 1], b["K"][i:i + 1], imsize=c.imsize, epsilon=c.eps, cdist_form=cdist)
            one.close()
            np.testing.assert_array_equal(_bits(t1[0]), _bits(terms[i]), err_msg=f"{name} {form} view {i}")
            total = total + g1                                                         # (float32, in view order)
        np.testing.assert_array_equal(_bits(total), _bits(grad), err_msg=f"{name} {form}: the views' shares in view order")
    contours = [torch.tensor(k).reshape(-1, 1, 2) for k in b["contours"]]
    for cot in (1.0, -2.5, 0.0):
        v = torch.tensor(b["verts"][None], requires_grad=True)
        out = L.multview_mask_loss(contours, torch.tensor(b["masks"]), v, None, torch.tensor(b["w2c"]), torch.tensor(b["K"]), list(range(c.M)),
                                   epsilon=c.eps, imsize=c.imsize)
        (out * cot).backward()
        np.testing.assert_array_equal(_bits(v.grad.numpy()[0]), _bits(grad * np.float32(cot) + np.float32(0)), err_msg=f"{name} x {cot}")
        if cot == 0.0:
            assert not _bits(v.grad.numpy()).any()
        assert not _bits(v.grad.numpy()[0][np.arange(c.n_verts) % MC.STRIDE != 0]).any()


@pytest.mark.parametrize("name", ["two_components", "contour17", "h48_w80", "all_foreground", "contour1"])
def test_contours_followed_on_the_device_equal_the_oracle(name):
    """contour_count == NULL: bf_contour_kernel's borders, read back by bf_silhouette_contours, are oracle/contour_oracle.py's point
    for point - and the loss on them is the loss on the oracle's contours handed over, bit for bit; the same through
    extract_countours and the multview_mask_loss that follows it (one upload)"""
    b = MC.build(name)
    c = b["case"]
    want = [CO.extract_contour(m, "opencv_first") for m in b["masks"]]
    sil = N.Silhouette(b["masks"], None, device=0)
    got = sil.contours()
    assert len(got) == c.M
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    given = N.Silhouette(b["masks"], want, device=0)
    for g, w in zip(given.contours(), want):
        np.testing.assert_array_equal(g, w)
    args = (b["verts"], b["w2c"], b["K"])
    kw = dict(imsize=c.imsize, epsilon=c.eps)
    for x, y in zip(sil.loss(*args, **kw), given.loss(*args, **kw)):
        np.testing.assert_array_equal(_bits(x), _bits(y))
    for select, key in ((_lib.CONTOUR_RASTER_FIRST, "raster_first"), (_lib.CONTOUR_LONGEST, "longest")):
        other = N.Silhouette(b["masks"], None, device=0, contour_select=select)
        for g, m in zip(other.contours(), b["masks"]):
            np.testing.assert_array_equal(g, CO.extract_contour(m, key))
        other.close()
    # the drop-in pair
    masks = torch.tensor(b["masks"].astype(np.float32))
    L._SILHOUETTES.clear()
    contours = L.extract_countours(masks)
    for g, w in zip(contours, want):
        assert g.dtype == torch.float32 and tuple(g.shape) == (len(w), 1, 2)
        np.testing.assert_array_equal(g.numpy()[:, 0], w)
    v = torch.tensor(b["verts"][None], requires_grad=True)
    out = L.multview_mask_loss(contours, masks, v, None, torch.tensor(b["w2c"]), torch.tensor(b["K"]), list(range(c.M)), c.eps, c.imsize)
    assert len(L._SILHOUETTES) == 1 and _bits(out.detach().numpy()) == _bits(sil.loss(*args, **kw)[0])
    sil.close(); given.close()


def test_refusals_before_any_launch(silhouettes):
    """the C ABI's refusals, and the fixed-point bound at its derived boundary: max(|epsilon|, 1) x the longest contour <= 2^20"""
    b = MC.build("contour17")
    c, sil = b["case"], silhouettes("contour17")
    args = (b["verts"], b["w2c"], b["K"])
    with pytest.raises(_lib.BodyfitError, match="stride"):
        sil.loss(*args, stride=0)
    for bad in (dict(imsize=float("nan")), dict(imsize=0.0), dict(imsize=-4.0), dict(imsize=float("inf")), dict(epsilon=float("nan")),
                dict(epsilon=float("inf"))):
        with pytest.raises(_lib.BodyfitError, match="imsize"):
            sil.loss(*args, **dict(dict(imsize=c.imsize), **bad))
    lib = _lib.load()
    one = np.zeros(1, np.float32)
    assert lib.bf_silhouette_loss(sil._h, 0, 4, _lib.fptr(b["verts"]), _lib.fptr(b["w2c"]), _lib.fptr(b["K"]), 16.0, 10.0, 1, _lib.fptr(one), None, None) == -1
    # the boundary, computed here from epsilon and the contour's length as a count: 17 points
    longest, limit = 17, 2 ** 20
    assert max(len(k) for k in b["contours"]) == longest
    fits = np.float32(limit / longest)                         # 61680.94, rounded to float32 - downwards:
    if float(fits) * longest > limit:
        fits = np.nextafter(fits, np.float32(0))
    assert float(fits) * longest <= limit < float(np.nextafter(fits, np.float32(np.inf))) * longest
    value, _, grad = sil.loss(*args, imsize=c.imsize, epsilon=float(fits))
    assert np.isfinite(value) and np.isfinite(grad).all()
    for eps in (float(np.nextafter(fits, np.float32(np.inf))), -float(np.nextafter(fits, np.float32(np.inf))), 1e9):
        with pytest.raises(_lib.BodyfitError, match="fixed-point") as e:
            sil.loss(*args, imsize=c.imsize, epsilon=eps)
        assert "(-3)" in str(e.value)                          # BF_ERR_UNSUPPORTED
    sil.loss(*args, imsize=c.imsize, epsilon=-float(fits))
    # sizes the kernels do not take
    h = _lib.C.c_void_p()
    tiny = np.ones((1, 2, 2), np.uint8)
    p8 = lambda a: a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint8))
    assert lib.bf_silhouette_create(0, 65536, 2, 2, p8(tiny), None, None, 0, _lib.C.byref(h)) == -3 and not h.value
    assert lib.bf_silhouette_create(0, 1, 16385, 2, p8(tiny), None, None, 0, _lib.C.byref(h)) == -3
    assert lib.bf_silhouette_create(0, 1, 2, 16385, p8(tiny), None, None, 0, _lib.C.byref(h)) == -3
    assert lib.bf_silhouette_create(0, 0, 2, 2, p8(tiny), None, None, 0, _lib.C.byref(h)) == -1
    assert lib.bf_silhouette_create(0, 1, 2, 2, p8(tiny), None, None, 3, _lib.C.byref(h)) == -1
    count = np.array([(1 << 22) + 1], np.int32)
    assert lib.bf_silhouette_create(0, 1, 2, 2, p8(tiny), _lib.iptr(count), _lib.fptr(np.zeros(2, np.float32)), 0, _lib.C.byref(h)) == -3
    count[0] = -1
    assert lib.bf_silhouette_create(0, 1, 2, 2, p8(tiny), _lib.iptr(count), _lib.fptr(np.zeros(2, np.float32)), 0, _lib.C.byref(h)) == -1
    # a view without contour points is taken: its binary term only
    empty = N.Silhouette(b["masks"], [b["contours"][0], np.zeros((0, 2), np.float32)], device=0)
    _, terms, _ = empty.loss(*args, imsize=c.imsize, epsilon=c.eps)
    assert terms[0, 0] > 0 and _bits(terms[1, 0]) == 0 and terms[1, 1] > 0
    empty.close()


def test_golden_of_the_imported_reference(smpl_model):
    """tests/golden/mask_loss_f0.npz: the imported reference's value and sampled gradient for 6,890 vertices, 8 views' 4 masks and
    512 px.  The stand-alone function in cdist form at the oracle's float32 vertices for the golden's parameters, held to the
    golden with the thresholds of tests/test_gpu_mask.py::test_mask_loss_value_and_gradient (the one place a share is allowed: the
    golden's inputs are not margin-selected)."""
    from test_mask_oracle import MASK_FRAMES, golden_vertices, mask_inputs
    g = load_golden("mask_loss_f0.npz")
    prob, contours, masks, w2cs, Ks = mask_inputs(smpl_model, torch.float32)
    verts = golden_vertices(smpl_model, prob, g, torch.float32)[None].requires_grad_(True)
    loss = L.multview_mask_loss([k.reshape(-1, 1, 2) for k in contours], masks, verts, None, w2cs, Ks, MASK_FRAMES, imsize=512)
    loss.backward()
    grad = verts.grad.numpy()[0]
    print(f"    value {float(loss):.6f} against the golden's {float(g['loss']):.6f}: {abs(float(loss) - float(g['loss'])) / float(g['loss']):.2e} relative")
    assert float(loss) == pytest.approx(float(g["loss"]), rel=2e-4)
    assert not _bits(grad[np.arange(6890) % 4 != 0]).any()
    share = float(np.mean(np.abs(grad[::4] - g["grad_sampled"]) < 1e-4 * np.abs(g["grad_sampled"]).max()))
    print(f"    share of the sampled gradient within 1e-4 max|g|: {share:.4f}")
    assert share > 0.985


@pytest.fixture
def smpl690(gmm, monkeypatch):
    model, _, _ = MC.loop_problem()
    monkeypatch.setattr(assets, "_MODELS", {("smpl", "neutral"): model})
    monkeypatch.setattr(assets, "_GMM", {"gmm": gmm})
    monkeypatch.setattr(assets, "_DEVICE_MODELS", {})
    from bodyfitting_amd.prior import MaxMixturePrior
    from bodyfitting_amd.smpl import SMPL
    smpl = SMPL(gender="neutral").to(torch.device("cpu"))                       # smplify.py:51-56
    prior = MaxMixturePrior(prior_folder="prior", num_gaussians=8, dtype=torch.float32).to(torch.device("cpu"))      # smplify.py:46
    yield smpl, prior
    for d in list(assets._DEVICE_MODELS.values()):
        d.close()
    for d in prior._on_device.values():
        d.close()


def test_one_step_of_a_users_loop(smpl690):
    """smplify.py:177-213 with use_mask=True, line for line on the drop-ins - the model's forward, the two similarity lines,
    multiview_keypoint_loss, multview_mask_loss, loss = body + 5 * mask, backward() - on the 690-vertex model at imsize 64 with two
    mask views: the total and every parameter block's gradient against float64 autograd of the oracle's same expression"""
    from bodyfitting_amd.loss import extract_countours, multiview_keypoint_loss, multview_mask_loss
    smpl, prior = smpl690
    model, prob, mk = MC.loop_problem()
    _, params, _ = MC.loop_case()
    t64, g64, _ = MC.loop_evaluate(params, torch.float64)
    t32, g32, _ = MC.loop_evaluate(params, torch.float32)
    P = {k: torch.tensor(np.asarray(params[k], np.float32).reshape(1, -1), requires_grad=True) for k in MC.LOOP_BLOCKS}
    global_transl, body_scale, body_pose, betas, global_orient = (P[k] for k in MC.LOOP_BLOCKS)
    w2cs = torch.inverse(torch.tensor(np.asarray(prob["c2ws"], np.float32)))    # smplify.py:131-135
    Ks = torch.tensor(np.asarray(prob["Ks"], np.float32))
    masks = torch.tensor((np.array(prob["masks"]) > 128).astype(np.float32))    # smplify.py:139
    mask_ids = [prob["use_frames"].index(f) for f in prob["mask_frames"]]
    contours = extract_countours(masks)                                         # smplify.py:144
    constant_scale = prob.get("constant_scale", 0.3)
    faces = np.asarray(model["faces"], np.int64)[None]

    smpl_output = smpl(betas=betas, global_orient=global_orient, body_pose=body_pose)
    model_joints = (smpl_output.joints + global_transl) * body_scale * constant_scale
    body_vertices = (smpl_output.vertices + global_transl) * body_scale * constant_scale
    body_loss, _ = multiview_keypoint_loss(w2cs, Ks, prob["keypoints"], model_joints, body_pose, betas, prob["use_frames"], prior,
                                           imsize=prob["imsize"])
    mask_loss = multview_mask_loss(contours, masks, body_vertices, faces, w2cs[mask_ids], Ks[mask_ids], prob["mask_frames"],
                                   imsize=prob["imsize"], pairwise="exact")
    loss = body_loss + 5 * mask_loss
    loss.backward()
    BAND.value("one step: total", float(loss), t64, t32)
    for k in MC.LOOP_BLOCKS:
        BAND.block(f"one step: d{k}", P[k].grad.numpy()[0], g64[k], g32[k])


def test_worst_position_inside_the_band():
    """(last: what the checks of this file printed, at its worst)"""
    worst = BAND.worst()
    assert worst is not None
    print(f"\n    worst position inside the band over this file: {worst[0]} at {worst[3]:.3f} (error {worst[1]:.3e} of {worst[2]:.3e} allowed), "
          f"{len(BAND.rows)} checks")
    assert worst[3] <= 1.0
