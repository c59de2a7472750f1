"""bodyfitting_amd.loss.extract_countours / multview_mask_loss on the CPU: the argument handling, the autograd plumbing and the
Silhouette cache, with the native calls replaced by float64 stand-ins over the oracle (mask_loss_cases.install_stand_ins), and the
well-posedness of every case the GPU module compares (tests/test_gpu_mask_loss.py)."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mask_loss_cases as MC
from oracle import contour_oracle as CO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def L(monkeypatch):
    MC.install_stand_ins(monkeypatch)
    from bodyfitting_amd import loss
    return loss


def _tensors(name, dtype=torch.float32, grad=True):
    b = MC.build(name)
    c = b["case"]
    return dict(contours=[torch.tensor(k, dtype=dtype).reshape(-1, 1, 2) for k in b["contours"]], masks=torch.tensor(b["masks"], dtype=dtype),
                smpl_verts=torch.tensor(b["verts"], dtype=dtype)[None].requires_grad_(grad), smpl_faces=None,
                w2cs=torch.tensor(b["w2c"], dtype=dtype), Ks=torch.tensor(b["K"], dtype=dtype), mask_frames=list(range(c.M)),
                epsilon=c.eps, imsize=c.imsize)


def test_parameter_lists():
    from bodyfitting_amd import loss
    sig = inspect.signature(loss.multview_mask_loss)
    assert list(sig.parameters) == ["contours", "masks", "smpl_verts", "smpl_faces", "w2cs", "Ks", "mask_frames", "epsilon", "imsize", "device",
                                    "pairwise"]
    defaults = {k: p.default for k, p in sig.parameters.items()}
    assert defaults["contours"] is inspect.Parameter.empty and defaults["masks"] is inspect.Parameter.empty
    assert all(defaults[k] is None for k in ("smpl_verts", "smpl_faces", "w2cs", "Ks", "mask_frames", "device", "pairwise"))
    assert defaults["epsilon"] == 10 and defaults["imsize"] == 512
    sig = inspect.signature(loss.extract_countours)
    assert list(sig.parameters) == ["masks", "device"] and sig.parameters["device"].default is None
    with pytest.raises(NotImplementedError, match="SMPLify"):                     # still the stub: nothing in the reference calls it
        loss.point_cloud_loss_chamfer_naive(np.zeros((3, 3)), np.zeros((3, 3)))


def test_drop_in_import_lines_without_torch():
    """smplify.py:14's import, from the drop-in package, in a child process: the names exist and torch is not imported for them"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from smplify.loss import multiview_keypoint_loss, multview_mask_loss, extract_countours, point_cloud_loss_mesh_grid\n"
            "assert callable(multview_mask_loss) and callable(extract_countours)\n"
            "assert 'torch' not in sys.modules\nprint('ok')\n") % (REPO, os.path.join(REPO, "bodyfitting_amd", "dropin"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


@pytest.mark.parametrize("name", MC.GRADCHECK_CASES)
def test_value_and_gradcheck_in_float64(L, name):
    kw = _tensors(name, torch.float64)
    got = L.multview_mask_loss(**kw)
    want, grad = MC.references(name)["f64"]
    assert got.dtype == torch.float64 and got.shape == () and float(got) == pytest.approx(want, rel=1e-12)
    got.backward()
    np.testing.assert_allclose(kw["smpl_verts"].grad.numpy()[0], grad, rtol=1e-12, atol=1e-12)
    rest = {k: v for k, v in kw.items() if k != "smpl_verts"}
    v = kw["smpl_verts"].detach().clone().requires_grad_(True)
    # (the steps stay far inside the case's margins: the pieces do not change under them)
    assert torch.autograd.gradcheck(lambda x: L.multview_mask_loss(smpl_verts=x, **rest), (v,), eps=1e-7, atol=1e-5, rtol=1e-4, nondet_tol=0.0)


def test_accepted_shapes_device_and_dtype(L):
    name = "ns33"
    kw = _tensors(name)
    want = MC.references(name)["f64"][0]
    a = L.multview_mask_loss(**kw)
    assert a.dtype == torch.float32 and a.shape == () and a.device == kw["smpl_verts"].device and a.requires_grad
    assert float(a) == pytest.approx(want, rel=1e-6)
    flat = dict(kw, smpl_verts=kw["smpl_verts"].detach()[0], contours=[k[:, 0] for k in kw["contours"]], w2cs=list(kw["w2cs"]), Ks=list(kw["Ks"]))
    b = L.multview_mask_loss(**flat)
    assert float(b) == float(a) and not b.requires_grad
    # positional, as smplify.py:198 calls it
    c = L.multview_mask_loss(kw["contours"], kw["masks"], kw["smpl_verts"], np.zeros((1, 4, 3), np.int64), kw["w2cs"], kw["Ks"], kw["mask_frames"],
                             kw["epsilon"], kw["imsize"])
    assert float(c) == float(a)
    with torch.no_grad():
        assert not L.multview_mask_loss(**kw).requires_grad
    # cotangents: the backward only scales the gradient that came with the value; zeros are +0
    grad = MC.references(name)["f64"][1]
    for cot in (1.0, -2.5, 0.0):
        v = kw["smpl_verts"].detach().clone().requires_grad_(True)
        (L.multview_mask_loss(**dict(kw, smpl_verts=v)) * cot).backward()
        np.testing.assert_allclose(v.grad.numpy()[0], grad * cot, rtol=1e-6, atol=1e-6 * np.abs(grad).max())
        zero = v.grad.numpy()[0][np.arange(len(grad)) % 4 != 0]
        assert not np.ascontiguousarray(zero).view(np.uint32).any()
        if cot == 0.0:
            assert not v.grad.numpy().view(np.uint32).any()


def test_numpy_in_float_out(L):
    name = "h48_w80"
    b = MC.build(name)
    c = b["case"]
    got = L.multview_mask_loss([k.reshape(-1, 1, 2) for k in b["contours"]], b["masks"].astype(np.float32), b["verts"][None], None, b["w2c"], b["K"],
                               list(range(c.M)), c.eps, c.imsize)
    assert isinstance(got, float) and got == pytest.approx(MC.references(name)["f64"][0], rel=1e-6)
    got = L.multview_mask_loss(b["contours"], b["masks"] != 0, b["verts"], None, list(b["w2c"]), list(b["K"]), range(c.M), c.eps, c.imsize,
                               pairwise="exact")
    assert isinstance(got, float)


def test_refusals(L):
    kw = _tensors("ns33")
    call = L.multview_mask_loss
    for name in ("contours", "masks", "smpl_verts", "w2cs", "Ks"):
        for bad in (None, "scan.obj", 3.0, object()):
            with pytest.raises(NotImplementedError, match="SMPLify"):
                call(**dict(kw, **{name: bad}))
    with pytest.raises(NotImplementedError, match="SMPLify"):
        call(None, None)
    with pytest.raises(NotImplementedError, match="SMPLify"):
        call(**dict(kw, contours=[kw["contours"][0], "x"]))
    with pytest.raises(NotImplementedError, match="SMPLify"):
        L.extract_countours(None, None)
    with pytest.raises(NotImplementedError, match="SMPLify"):
        L.extract_countours([[0, 1], [1, 1]])

    def refused(match, **change):
        with pytest.raises(ValueError, match=match):
            call(**dict(kw, **change))

    refused("mix", w2cs=kw["w2cs"].numpy())
    refused("mix", contours=[k.numpy() for k in kw["contours"]])
    refused("mix", masks=kw["masks"].numpy())
    refused(r"\[1,N,3\]", smpl_verts=torch.zeros(1, 8, 2))
    refused(r"\[1,N,3\]", smpl_verts=torch.zeros(2, 8, 3))
    refused(r"\[1,N,3\]", smpl_verts=torch.zeros(1, 0, 3))
    refused("mask_frames", mask_frames=[0])
    refused("mask_frames", mask_frames=[0, 1, 2])
    refused("mask_frames", mask_frames=None)
    refused("mask_frames", contours=kw["contours"][:1])
    refused("mask_frames", w2cs=kw["w2cs"][:1])
    refused("mask_frames", Ks=list(kw["Ks"]) + [kw["Ks"][0]])
    refused("no points", contours=[kw["contours"][0], torch.zeros(0, 1, 2)])
    refused(r"\[C,1,2\]", contours=[kw["contours"][0], torch.zeros(5, 3)])
    refused("0 / 1", masks=kw["masks"] * 255)
    refused("0 / 1", masks=kw["masks"] * 0.5)
    refused("larger than the masks", imsize=33)
    refused("imsize", imsize=float("nan"))
    refused("imsize", imsize=0)
    refused("epsilon", epsilon=float("inf"))
    refused("epsilon", epsilon=float("nan"))
    refused("requires grad", masks=kw["masks"].clone().requires_grad_(True))
    refused("requires grad", contours=[k.clone().requires_grad_(True) for k in kw["contours"]])
    refused("requires grad", w2cs=kw["w2cs"].clone().requires_grad_(True))
    refused("requires grad", Ks=[k.clone().requires_grad_(True) for k in kw["Ks"]])
    refused("pairwise", pairwise="torch")
    refused(r"\[M,4,4\]", w2cs=kw["w2cs"][:, :3])


def test_float32_is_required_without_the_stand_ins():
    from bodyfitting_amd import loss
    kw = _tensors("ns33", torch.float64)
    with pytest.raises(ValueError, match="float32"):
        loss.multview_mask_loss(**kw)


def test_extract_countours_against_the_oracle(L):
    b = MC.build("two_components")
    masks = b["masks"]
    want = [CO.extract_contour(m, "opencv_first") for m in masks]
    for given in (masks, masks != 0, masks.astype(np.float32), masks.astype(np.int64)):
        got = L.extract_countours(given)
        assert isinstance(got, list) and len(got) == len(masks)
        for g, w in zip(got, want):
            assert isinstance(g, np.ndarray) and g.dtype == np.float32 and g.shape == (len(w), 1, 2)
            np.testing.assert_array_equal(g[:, 0], w)
    for dtype in (torch.float32, torch.bool, torch.uint8):
        t = torch.tensor(masks).to(dtype)
        got = L.extract_countours(t)
        for g, w in zip(got, want):
            assert torch.is_tensor(g) and g.dtype == torch.float32 and g.device == t.device and tuple(g.shape) == (len(w), 1, 2)
            np.testing.assert_array_equal(g.numpy()[:, 0], w)
    one = L.extract_countours(masks[0])                                       # [H,W]
    assert len(one) == 1 and one[0].shape == (len(want[0]), 1, 2)
    assert len(want[0]) == 2 * (4 + 2) - 4                                    # the small component, met last: what loss.py:80 keeps
    with pytest.raises(ValueError, match="no foreground"):
        L.extract_countours(np.stack([masks[0], np.zeros_like(masks[0])]))
    with pytest.raises(ValueError, match="0 / 1"):
        L.extract_countours(masks * 255)
    with pytest.raises(ValueError, match="requires grad"):
        L.extract_countours(torch.tensor(masks, dtype=torch.float32).requires_grad_(True))


def test_silhouette_cache(L):
    S = MC.StandInSilhouette
    kw = _tensors("ns33", grad=False)
    masks = kw["masks"]
    contours = L.extract_countours(masks)
    assert (S.created, S.followed) == (1, 1)
    L.extract_countours(masks)
    for _ in range(3):                                                        # the loop: the same tensors every iteration
        L.multview_mask_loss(**dict(kw, contours=contours))
    assert (S.created, S.followed) == (1, 1)
    # equal contours held elsewhere ([C,2] copies): compared by value, still the same object
    L.multview_mask_loss(**dict(kw, contours=[k[:, 0].clone() for k in contours]))
    assert S.created == 1
    # other contours for the same masks: uploaded with them, once
    other = [k[: len(k) // 2] for k in contours]
    a = L.multview_mask_loss(**dict(kw, contours=other))
    b = L.multview_mask_loss(**dict(kw, contours=other))
    assert (S.created, S.followed) == (2, 1) and float(a) == float(b) != float(L.multview_mask_loss(**dict(kw, contours=contours)))
    # an in-place edit of the masks is seen
    masks[0, 0, 0] = 1 - masks[0, 0, 0]
    L.extract_countours(masks)
    assert (S.created, S.followed) == (3, 2)
    # arrays: told apart by their bytes
    arr = MC.build("ns33")["masks"]
    L.extract_countours(arr)
    L.extract_countours(arr.copy())
    assert (S.created, S.followed) == (4, 3)
    # the slot limit: the oldest goes first
    for k in range(2 * L._SILHOUETTE_SLOTS):
        m = arr.copy()
        m[0, 0, k] = 1
        L.extract_countours(m)
        assert len(L._SILHOUETTES) <= L._SILHOUETTE_SLOTS
    created = S.created
    L.extract_countours(arr)                                                  # long gone: built again
    assert S.created == created + 1


@pytest.mark.parametrize("name", MC.CASE_NAMES)
def test_case_is_well_posed(name):
    """the three float64 margins of every case exceed its margin; the case has the sizes it is named for"""
    b = MC.build(name)
    c, m = b["case"], b["margins"]
    print(f"  {name}: n_verts {c.n_verts} ({c.ns} sampled), {c.M} views {c.H} x {c.W}, imsize {c.imsize:g}, contours {[len(k) for k in b['contours']]}: "
          f"margin {m['margin']:.3e} (8 x uv_err32 {m['uv_err32']:.2e}, 16 x cdist_err32 {m['cdist_err32']:.2e}); gap {m['gap']:.3e}, "
          f"pixel {m['pixel']:.3e}, border {m['border']:.3e}; nearest vertex-contour pair {m['near']:.2f} px")
    again, _ = MC.margins(c, b["verts"], b["w2c"], b["K"], b["contours"])
    assert again == m
    assert m["margin"] > 0 and min(m["gap"], m["pixel"], m["border"]) > m["margin"]
    assert len(b["verts"]) == c.n_verts and -(-c.n_verts // MC.STRIDE) == c.ns and b["masks"].shape == (c.M, c.H, c.W)
    want = {"contour1": 1, "contour15": 15, "contour16": 16, "contour17": 17}.get(name)
    if want:
        assert all(len(k) == want for k in b["contours"])
    if name == "contour200":
        assert all(150 <= len(k) <= 250 for k in b["contours"])
    if name == "contour1100":
        assert all(len(k) * 16 > 64 * 256 for k in b["contours"])              # more than 64 block sums per view
    if name == "all_foreground":
        assert b["masks"].all()
    # the float32 references agree with the truth far inside the decisions: the band never degenerates
    ref = MC.references(name)
    M = np.abs(ref["f64"][1]).max()
    for form in ("exact", "cdist"):
        assert np.abs(ref[form][1] - ref["f64"][1]).max() <= 1e-3 * M, form


def test_loop_case_is_well_posed():
    """the parameter point of tests/test_gpu_mask_loss.py's one step of a user's loop: chosen by seed, margins as above (exact form)"""
    seed, params, m = MC.loop_case()
    model, prob, masks = MC.loop_problem()
    print(f"  seed {seed}: contours {[len(k) for k in masks['contours']]}, margin {m['margin']:.3e} (8 x uv_err32 {m['uv_err32']:.2e}); gap {m['gap']:.3e}, "
          f"pixel {m['pixel']:.3e}, border {m['border']:.3e}")
    assert prob["imsize"] == MC.LOOP_IMSIZE and len(np.asarray(model["v_template"])) == 690 and len(masks["contours"]) == 2
    assert m["margin"] > 0 and min(m["gap"], m["pixel"], m["border"]) > m["margin"]
    t64, g64, _ = MC.loop_evaluate(params, torch.float64)
    t32, g32, _ = MC.loop_evaluate(params, torch.float32)
    assert abs(t32 - t64) <= 1e-5 * abs(t64)
    for k in MC.LOOP_BLOCKS:
        assert np.abs(g32[k] - g64[k]).max() <= 1e-3 * np.abs(g64[k]).max(), k
