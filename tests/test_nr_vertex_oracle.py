"""tests/nr_vertex_oracle.py against what the reference itself records and computes (tests/golden/nr_vertex_grad.npz, written by
tools/gen_nr_vertex_golden.py): its four recorded gradient cases, and torch autograd in float64 through its lighting.py and
projection.py.  CPU only."""
import os

import numpy as np
import pytest

import nr_vertex_oracle as VO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nr_vertex_grad.npz")
AMBIENT_ONLY = dict(ambient=1.0, directional=0.0, color_ambient=(1, 1, 1), color_directional=(1, 1, 1), direction=(0, 1, 0))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("case", range(4))
def test_the_references_recorded_gradient_cases(golden, case):
    """test_rasterize_silhouettes.py / test_rasterize.py, test_backward_case1 / 2, through the ndc path: look_at with
    perspective=False and the default eye leaves x and y and adds 2.732 to z.  Image size 64, no anti-aliasing; the colour cases
    with ambient 1, directional 0, textures of ones and the cotangent of a channel mean.  Held to the reference's own
    allclose(rtol=1e-2)."""
    v = golden["case_vertices"][case] + np.array([0, 0, 2.732], np.float32)
    f, (py, px), ref = golden["case_faces"][case], golden["case_pixel"][case], golden["case_grad_ref"][case]
    colour, minus_one = bool(golden["case_colour"][case]), bool(golden["case_minus_one"][case])
    tex = np.ones((1, 4, 4, 4, 3), np.float32) if colour else None
    want = ("rgb", "depth", "alpha") if colour else ("alpha",)
    rgb, _, alpha, keep = VO.render(v, f, tex, image_size=64, anti_aliasing=False, ndc=True, light=AMBIENT_ONLY, lightoff=not colour, want=want)
    value = rgb[:, py, px].mean() if colour else alpha[py, px]
    sign = np.sign(value - 1.0) if minus_one else np.sign(value)      # d |image - 1| or d |image|
    if colour:
        g = np.zeros((3, 64, 64), np.float32)
        g[:, py, px] = np.float32(sign) / np.float32(3)
        out = VO.vertex_vjp(keep, g_rgb=g)
    else:
        g = np.zeros((64, 64), np.float32)
        g[py, px] = sign
        out = VO.vertex_vjp(keep, g_alpha=g)
    got = out["verts"][0]
    rel = np.abs(got - ref)[ref != 0] / np.abs(ref[ref != 0])
    print(f"case {case}: largest relative difference {rel.max():.3g}")
    assert np.allclose(got, ref, rtol=1e-2)
    assert not got[ref == 0].any()
    assert out["R"] is None and out["t"] is None


def test_light_vjp_follows_autograd_through_the_references_lighting(golden):
    """Largest difference measured here (printed): 7.11e-15 against gradients of magnitude up to ~20 - both
    sides are float64.  Asserted: 4 x that."""
    worst = 0.0
    for row, cot, want in zip(golden["lights"], golden["light_cotangent"], golden["light_corner_grad"]):
        M = VO.light_corner_jacobian(golden["light_face_world"], directional=row[1], color_directional=row[5:8], direction=row[8:11])
        got = np.einsum("kcij,kc->kij", M, cot)
        worst = max(worst, float(np.abs(got - want).max()))
        if row[1] == 0:
            assert not got.any()
    print(f"largest difference: light corner gradient {worst:.3g} (largest magnitude {np.abs(golden['light_corner_grad']).max():.3g})")
    assert worst <= 4 * 7.11e-15


def test_projection_vjp_follows_autograd_through_the_references_projection(golden):
    """Largest differences measured here (printed): vertices 4.44e-16, R 1.78e-15, t 5.33e-15 - float64 on both
    sides.  Asserted: 4 x that."""
    worst = np.zeros(3)
    for cam, cot, gv, gR, gt in zip(golden["proj_cams"], golden["proj_cotangent"], golden["proj_grad_verts"], golden["proj_grad_R"], golden["proj_grad_t"]):
        (v, _), (R, _), (t, _) = VO.projection_vjp(golden["proj_verts"], cam[:9], cam[9:18], cam[18:21], cam[21], cot)
        worst = np.maximum(worst, [np.abs(v - gv).max(), np.abs(R - gR).max(), np.abs(t - gt).max()])
    print(f"largest difference: vertices {worst[0]:.3g}, R {worst[1]:.3g}, t {worst[2]:.3g}")
    assert worst[0] <= 4 * 4.44e-16 and worst[1] <= 4 * 1.78e-15 and worst[2] <= 4 * 5.33e-15


def test_a_degenerate_face_and_a_back_record_take_no_gradient():
    """corners 0 and 1 on one point: |n| = 0, the light's reverse is zero (relu at 0), and a record that shows its back is skipped"""
    face = np.array([[[0.3, 0.2, 1.0], [0.3, 0.2, 1.0], [0.5, 0.1, 2.0]]], np.float32)
    assert not VO.light_corner_jacobian(face, 0.8, (0.6, 1.0, 0.8), (0.3, 0.8, -0.5)).any()
    v = np.array([[-0.6, -0.5, 2.0], [0.7, -0.4, 2.2], [0.1, 0.8, 1.9]], np.float32)
    _, _, _, keep = VO.render(v, np.array([[0, 1, 2]]), None, image_size=8, anti_aliasing=False, ndc=True, want=("alpha",))
    g = np.random.default_rng(0).standard_normal((8, 8)).astype(np.float32)
    grad, n, _ = VO.frec_grad(keep, g_alpha=g)
    front = int(n[0].sum() == 0)                                      # the record that is drawn
    assert n[front].sum() > 0 and not n[1 - front].any() and not grad[1 - front].any()
