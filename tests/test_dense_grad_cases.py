"""CPU side of tests/test_gpu_dense_grad.py: the oracle of the dense iterations' objective (oracle.smplify_oracle.dense_loss_and_grad)
is right - its autograd gradient against central differences in float64 - and every case of tests/dense_grad_cases.py is well posed:
torch's own float32 evaluation of the same oracle is within 1e-5 of the block's maximum of the float64 one, and the silhouette case
keeps its three margins."""
import numpy as np
import pytest
import torch

import dense_grad_cases as DC
from oracle import smplify_oracle as O


def _objective(terms, bv, cot):
    return sum(terms.values()) + (0.0 if cot is None else float((cot * bv).sum()))


def _directional(fn, p, names, seed, h=1e-6):
    """(autograd directional derivative, central difference) of fn(params) -> (terms, grads, bv, cot) along a seeded direction"""
    rng = np.random.default_rng(seed)
    d = {k: rng.normal(size=np.shape(p[k])) for k in names}
    terms, grads, bv, cot = fn(p)
    an = sum(float((grads[k] * d[k]).sum()) for k in names)
    vals = []
    for sgn in (1.0, -1.0):
        q = {k: p[k] + sgn * h * d[k] if k in d else p[k] for k in p}
        t, _, v, c = fn(q)
        vals.append(_objective(t, v, c))
    return an, (vals[0] - vals[1]) / (2 * h)


@pytest.mark.parametrize("name", ["smpl690", "kid690"])
def test_oracle_gradient_against_central_differences(name):
    """keypoints + scan term (constant closest points) + cotangent on a 690-vertex model, five random directions over all blocks:
    autograd and (L(p + h d) - L(p - h d)) / 2h agree to 1e-6 of the gradient's size along d in float64"""
    frame, sc = 0, 1.0
    m = DC.model(name)
    if name == "smpl690":
        prob, sv, sf = DC.scan_problem(name, frame, sc)
        p = DC.scan_params(name, frame, sc)
        cot = DC.scan_cotangent(name, frame, sc)
        _, _, bv = O.dense_loss_and_grad(m, DC.LC.gmm_bufs(), prob, p, dtype=torch.float32)
        _, closest = DC.closest_points(sv, sf, bv)
        kw = {"closest": closest, "scan_height": DC.scan_height(sv)}
    else:
        prob, p, cot, kw = DC.problem(name, frame), DC.params(name, frame), DC.cotangent(name, frame), {}

    def fn(q):
        return O.dense_loss_and_grad(m, DC.LC.gmm_bufs(), prob, q, cot=cot, **kw) + (cot,)
    for seed in range(5):
        an, fd = _directional(fn, p, DC.blocks(name), seed)
        print(f"{name} direction {seed}: autograd {an:.10g} central difference {fd:.10g}")
        assert an == pytest.approx(fd, rel=1e-6)
    terms, _, _, _ = fn(p)
    assert (terms["scan_loss"] > 0) == (name == "smpl690") and terms["mask_loss"] == 0


def test_oracle_silhouette_gradient_against_central_differences():
    """the silhouette term of the well-posed case: inside its margins the objective is smooth, so central differences apply"""
    p = DC.mask_params()
    mi = DC.mask_inputs()
    masks = {k: mi[k] for k in ("contours", "masks", "views")}

    def fn(q):
        return O.dense_loss_and_grad(DC.model(DC.MASK_MODEL), DC.LC.gmm_bufs(), DC.mask_problem(), q, masks=masks) + (None,)
    for seed in range(3):
        an, fd = _directional(fn, p, DC.blocks(DC.MASK_MODEL), seed, h=1e-8)
        print(f"silhouette direction {seed}: autograd {an:.10g} central difference {fd:.10g}")
        assert an == pytest.approx(fd, rel=1e-5)
    assert fn(p)[0]["mask_loss"] > 0


def _well_posed(what, names, r64, r32):
    for k in names:
        _, M, err = DC.band(r64[1][k], r32[1][k])
        assert err <= DC.WELL_POSED * M, (what, k, err, M)
    for k in O.DENSE_TERMS:
        if r64[0][k] != 0:
            assert abs(r32[0][k] - r64[0][k]) <= DC.WELL_POSED * abs(r64[0][k]), (what, k)


@pytest.mark.parametrize("name", list(DC.MODELS))
def test_every_reverse_case_is_well_posed(name):
    """full model and sub-model cotangents, every frame the GPU file uses"""
    todo = [(f, None) for f in DC.frames(name, max(DC.REVERSE_F[name]))]
    todo += [(f, w) for w in DC.sub_models(name) for f in DC.frames(name, max(DC.SUB_F))]
    for f, w in todo:
        r = DC.reverse_reference(name, f, w)
        _well_posed((name, f, w), DC.blocks(name), (r["terms64"], r["grads64"]), (r["terms32"], r["grads32"]))
        p = DC.params(name, f)
        assert np.abs(p["global_transl"]).min() > 0 and abs(p["scale"][0] - 1) > 1e-4 and np.abs(p["betas"]).min() > 0
        cot = DC.cotangent(name, f, w)
        assert np.isfinite(cot).all() and np.abs(cot).max() > 0
        if w is not None:
            off = np.ones(len(cot), bool)
            off[DC.sub_vertices(name, w)] = False
            assert not cot[off].any() and off.any()


def test_sub_model_sizes():
    """the sub-models the cases assume: SMPL kinds have the sampled-first one, SMPL-X both; 3,285 and 899 vertices at full size"""
    assert DC.sub_models("smpl690") == (DC.SUB_SAMPLED,) and DC.sub_models("smplx1200") == (DC.SUB_SAMPLED, DC.SUB_KP)
    assert len(DC.sub_vertices("smplx10475", DC.SUB_SAMPLED)) == 3285 and len(DC.sub_vertices("smplx10475", DC.SUB_KP)) == 899
    for name in DC.MODELS:
        assert DC.sub_models(name)


@pytest.mark.parametrize("name", DC.SCAN_MODELS)
def test_every_scan_case_is_well_posed(name):
    """closest points from the reference's search at torch's float32 vertices; with and without the cotangent"""
    for frame, sc in DC.SCAN_FRAMES:
        prob, sv, sf = DC.scan_problem(name, frame, sc)
        _, _, bv32 = DC.scan_evaluate(name, frame, sc, None, dtype=torch.float32)
        _, closest = DC.closest_points(sv, sf, bv32)
        for cot in (None, DC.scan_cotangent(name, frame, sc)):
            r64 = DC.scan_evaluate(name, frame, sc, closest, cot)
            r32 = DC.scan_evaluate(name, frame, sc, closest, cot, dtype=torch.float32)
            _well_posed((name, frame, cot is not None), DC.blocks(name), r64, r32)
            assert r64[0]["scan_loss"] > 0
    assert DC.scan_height(DC.scan_problem(name, 0, 1.0)[1]) > 1.5 * DC.scan_height(DC.scan_problem(name, 1, 0.5)[1])


def test_silhouette_case_margins():
    """gap between the nearest and the second-nearest projected vertex of every contour point, distance of the chosen vertices' pixel
    coordinates from an integer, distance of every projected vertex from the image border: all above 8 x the float32 projection's
    largest error, which is what dense_grad_cases.MASK_UV_ERR32 records"""
    assert DC.MASK_MARGIN == 8 * DC.MASK_UV_ERR32
    for what, cscale in (("alone", None), ("with the scan attached", DC.scan_cscale(DC.mask_scan()[0]))):
        m = DC.mask_margins(cscale=cscale)
        print("silhouette case", what, m, "margin", DC.MASK_MARGIN)
        assert m["uv_err32"] <= DC.MASK_UV_ERR32
        assert m["gap"] > DC.MASK_MARGIN and m["pixel"] > DC.MASK_MARGIN and m["border"] > DC.MASK_MARGIN
    mi = DC.mask_inputs()
    assert len(mi["contours"]) == 2 and min(len(c) for c in mi["contours"]) > 50


def test_silhouette_case_is_well_posed():
    """alone, and together with a scan term (closest points at torch's float32 vertices)"""
    r64, r32 = DC.mask_evaluate(), DC.mask_evaluate(torch.float32)
    _well_posed("silhouette", DC.blocks(DC.MASK_MODEL), r64, r32)
    assert r64[0]["mask_loss"] > 0
    sv, sf = DC.mask_scan()
    h, c = DC.scan_height(sv), DC.scan_cscale(sv)
    _, closest = DC.closest_points(sv, sf, DC.mask_evaluate(torch.float32, cscale=c)[2])
    r64, r32 = DC.mask_evaluate(closest=closest, height=h, cscale=c), DC.mask_evaluate(torch.float32, closest=closest, height=h, cscale=c)
    _well_posed("silhouette + scan", DC.blocks(DC.MASK_MODEL), r64, r32)
    assert r64[0]["mask_loss"] > 0 and r64[0]["scan_loss"] > 0
