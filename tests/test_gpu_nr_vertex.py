"""The geometry gradient of the stand-alone neural_renderer.Renderer on the GPU (bf_nr_render_taped, bf_nr_tape_vertex_grad,
bf_nr_mesh_set_vertices through native.Nr*) against tests/nr_vertex_oracle.py.

The bound.  The oracle returns per gradient value the number of terms n and the sum of their magnitudes S; a float32 sum of n terms
in any order is within (n - 1) 2^-23 S of the exact sum of those terms, and each term carries k roundings of its own, so
|got - want| <= (n + k) 2^-23 S elementwise.  k, counted from the kernels:
  * a soft-edge term is diff_grad / dist.  Both operands are the oracle's own float32 values, operation for operation (they decide
    `diff_grad <= 0`, so they have to be): the term adds the division's rounding, 1;
  * a depth term is g w depth^2 / z_k^2 (5: depth^2, z^2, two products, the division) or g tmp w depth^2 is / 2 with tmp a sum of
    three quotients (8 against the magnitudes of tmp's terms);
  so K_FREC = 8 for the rows per record (dL/d projected corners), checked for EVERY shape on a triangle soup in ndc, where every
  vertex has one drawn record and the fold adds nothing.  A lit soup's grad_verts is rows + the light's reverse (in ndc the light
  sees the vertices as given); the two are bounded separately, (n + K_FREC) 2^-23 S of the rows plus (n + K_LIGHT) 2^-23 S of the
  light's part, so the rows keep K_FREC also where the colour map is lit;
  * the projection's reverse: p = R v + t (5 roundings, into the coefficients), 2 / orig (2), K's rows (3), the divisions by z and
    z^2 (6), R^T (5), the light's part (1): 22, rounded up to K_PROJ = 24;
  * the light's reverse per record: a, b (2), n (3), |n| and n^ (6), n^ . d (5), dL/dcos (6), the projection off n^ (7), / |n| (1),
    two cross products (6), the corner sums (2): 38, rounded up to K_LIGHT = 40.  Its S is the oracle's magnitude Jacobian
    (light_corner_magnitude), which covers the two places where that chain cancels.
  K_FINAL = K_FREC + K_PROJ + K_LIGHT = 72 for grad_verts, grad_R and grad_t.
Where the oracle has no term the result is exactly zero.  The worst fraction of the bound seen is printed per case (DESIGN.md
section 22 records it).

Shapes reuse tests/test_gpu_nr.py's builders: one tile (output 8), partial tiles (20 and 32 with anti-aliasing), occlusion (sphere,
fans), back records only (the open shell from inside), a box above BF_TEX_GATHER_MAX with more than 64 lines per edge (the big face
at output 40), a walk longer than 64 lanes (output 64 with anti-aliasing: 128 pixels a side), a vertex of valence 70, a degenerate
face."""
import re

import numpy as np
import pytest

from bodyfitting_amd import _lib, native
from oracle import texfit_oracle as TO
from texfit_cases import icosphere
from test_gpu_nr import AMBIENT_ONLY, EYE, LIGHT, _K, _big_face, _distinct, _fan, _hemisphere, _sphere, _triangle, _views
import nr_oracle as NO
import nr_vertex_oracle as VO

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
K_FREC, K_PROJ, K_LIGHT = 8, 24, 40
K_FINAL = K_FREC + K_PROJ + K_LIGHT
BOTH = native.TAPE_TEXTURES | native.TAPE_GEOMETRY
ALL = ("rgb", "depth", "alpha")
BF_ERR_INVALID = -1               # include/bodyfit.h
GOLDEN = __file__.replace("test_gpu_nr_vertex.py", "golden/nr_vertex_grad.npz")


class Scene:
    """a native renderer + mesh, one taped render of it and the oracle's render of the same"""

    def __init__(self, mesh, size, aa, cam=None, near=0.1, far=100.0, fill_back=True, lightoff=False, want=ALL, light=LIGHT, flags=None,
                 background=(0.1, 0.2, 0.3)):
        self.v, self.f, self.tex = mesh
        self.size, self.want, self.ndc = size, want, cam is None
        self.r = native.NrRenderer(size, aa, near, far, background)
        self.r.set_light(**light)
        ts = 0 if self.tex is None else self.tex.shape[1]
        self.m = native.NrMesh(self.r, self.v, self.f, ts, self.tex)
        self.cam = dict(ndc=True) if cam is None else dict(K=_K(size), R=cam[0], t=cam[1], orig_size=size)
        self.args = dict(fill_back=fill_back, lightoff=lightoff, want=want, **self.cam)
        flags = flags if flags is not None else (BOTH if self.tex is not None else native.TAPE_GEOMETRY)
        *self.got, self.tape = self.r.render_taped(self.m, flags=flags, **self.args)
        *self.ref, self.keep = VO.render(self.v, self.f, self.tex, image_size=size, anti_aliasing=aa, near=np.float32(near), far=np.float32(far),
                                         background=background, light=light, **self.args)
        for name, g, w in zip(ALL, self.got, self.ref):
            assert (g is None) == (w is None) == (name not in want)
            if g is not None:
                np.testing.assert_array_equal(g, w, err_msg=name)

    def cotangents(self, which=ALL, seed=0):
        rng = np.random.default_rng(seed)
        n = self.size
        g = dict(rgb=rng.standard_normal((3, n, n)), depth=rng.standard_normal((n, n)), alpha=rng.standard_normal((n, n)))
        return [g[nm].astype(np.float32) if nm in which and nm in self.want else None for nm in ALL]

    def close(self):
        self.tape.close(); self.m.close(); self.r.close()


def _within(got, want, k, what):
    grad, n, S = want
    assert got.shape == grad.shape, what
    bound = (n + k) * EPS32 * S
    err = np.abs(got.astype(np.float64) - grad)
    hit = S > 0
    frac = float((err[hit] / bound[hit]).max()) if hit.any() else 0.0
    print(f"{what}: {int(hit.sum())} values with terms, largest n {int(np.max(n))}, largest err / bound {frac:.3f}")
    assert (err <= bound).all(), (what, float((err - bound).max()))
    assert not got[~hit].any(), what                                  # exact zeros where the oracle has no term
    return frac


def _check(s, which=ALL, seed=0, need_terms=True):
    """grad_verts, grad_R, grad_t of scene `s` for random cotangents on `which` outputs, twice (equal bits), against the oracle"""
    g = s.cotangents(which, seed)
    gv, gR, gt = s.tape.vertex_grad(*g, camera=not s.ndc)
    again = s.tape.vertex_grad(*g, camera=not s.ndc)
    for a, b in zip((gv, gR, gt), again):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()
    want = VO.vertex_vjp(s.keep, *g)
    if need_terms:
        assert (want["verts"][2] > 0).any()
    _within(gv, want["verts"], K_FINAL, "grad_verts")
    if not s.ndc:
        _within(gR, want["R"], K_FINAL, "grad_R")
        _within(gt, want["t"], K_FINAL, "grad_t")
    return gv, gR, gt, want


def _soup(mesh, cam, size):
    """the projected mesh as independent triangles in ndc: vertex 3 i + c is corner c of face i, so grad_verts of a render of it IS
    the per-record rows (a face's front and back record share its vertices, and only one of them is drawn)"""
    v, f, tex = mesh
    pv = v if cam is None else TO.project(v, _K(size), cam[0], cam[1], size)
    return np.ascontiguousarray(pv[f].reshape(-1, 3)), np.arange(3 * len(f), dtype=np.int32).reshape(-1, 3), tex


def _check_rows(mesh, size, aa, cam, near=0.1, far=100.0, which=ALL, seed=1, lightoff=True, want=ALL, need_terms=True):
    """the per-record rows of `mesh` seen through `cam`, at K_FREC (module docstring); lit: plus the light's part at K_LIGHT"""
    v, f, tex = _soup(mesh, cam, size)
    s = Scene((v, f, tex if "rgb" in want else None), size, aa, None, near, far, lightoff=lightoff, want=want)
    g = s.cotangents(which, seed)
    gv, _, _ = s.tape.vertex_grad(*g, camera=False)
    again, _, _ = s.tape.vertex_grad(*g, camera=False)
    assert gv.tobytes() == again.tobytes()
    out = VO.vertex_vjp(s.keep, *g)
    rows, n, S = out["frec"]
    nf = len(s.f)
    drawn_twice = (S[:nf].reshape(nf, -1).sum(1) > 0) & (S[nf:].reshape(nf, -1).sum(1) > 0)
    assert not drawn_twice.any()                                      # (one record per face has terms: the fold adds nothing)
    (_, nn, Sn), (_, nw, Sw) = out["parts"]
    assert Sn.any() or not need_terms
    bound = (nn + K_FREC) * EPS32 * Sn + (nw + K_LIGHT) * EPS32 * Sw
    err = np.abs(gv.astype(np.float64) - out["verts"][0])
    hit = bound > 0
    print(f"rows per record{' (+ light: ' + str(int((Sw > 0).sum())) + ' values)' if Sw.any() else ''}: {int(hit.sum())} values with terms, "
          f"largest n {int(nn.max())}, largest err / bound {float((err[hit] / bound[hit]).max()) if hit.any() else 0:.3f}")
    assert (err <= bound).all(), float((err - bound).max())
    assert not gv[~hit].any()
    s.close()


def _view(v, i):
    views, far = _views(v)
    return (views[i][:3, :3], views[i][:3, 3]), far


# ---- shapes --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", [0.0, 0.9])
def test_one_triangle_in_one_tile_and_partly_outside_the_image(shift):
    cam = (EYE[0], np.array([shift, 0.3 * shift, 0], np.float32))
    s = Scene(_triangle(), 8, False, cam)
    _check(s)
    s.close()
    for lightoff in (True, False):
        _check_rows(_triangle(), 8, False, cam, lightoff=lightoff)


@pytest.mark.parametrize("case", range(4))
def test_the_references_recorded_cases(case):
    """tests/test_nr_vertex_oracle.py's four cases on the device: within the bound of the oracle AND within the reference's own
    allclose(rtol=1e-2) of its recorded grad_ref"""
    g = np.load(GOLDEN)
    v = g["case_vertices"][case] + np.array([0, 0, 2.732], np.float32)
    (py, px), ref, colour = g["case_pixel"][case], g["case_grad_ref"][case], bool(g["case_colour"][case])
    tex = np.ones((1, 4, 4, 4, 3), np.float32) if colour else None
    s = Scene((v, g["case_faces"][case], tex), 64, False, None, want=ALL if colour else ("alpha",), lightoff=not colour, light=AMBIENT_ONLY,
              background=(0, 0, 0))
    value = s.got[0][:, py, px].mean() if colour else s.got[2][py, px]
    sign = np.sign(value - 1.0) if g["case_minus_one"][case] else np.sign(value)
    cot = [None, None, None]
    if colour:
        cot[0] = np.zeros((3, 64, 64), np.float32); cot[0][:, py, px] = np.float32(sign) / np.float32(3)
    else:
        cot[2] = np.zeros((64, 64), np.float32); cot[2][py, px] = sign
    gv, _, _ = s.tape.vertex_grad(*cot, camera=False)
    _within(gv, VO.vertex_vjp(s.keep, *cot)["verts"], K_FREC, "grad_verts (ndc)")
    assert np.allclose(gv, ref, rtol=1e-2)
    assert not gv[ref == 0].any()
    s.close()


@pytest.mark.parametrize("size,aa,lightoff", [(20, True, True), (32, True, False)])
@pytest.mark.parametrize("name", ["sphere", "fan33", "fan70"])
def test_occlusion_and_partial_tiles(name, size, aa, lightoff):
    mesh = _sphere() if name == "sphere" else _fan(int(name[3:]))
    cam, far = _view(mesh[0], 7) if name == "sphere" else (EYE, 100.0)
    s = Scene(mesh, size, aa, cam, 0.0 if name == "sphere" else 0.1, far, lightoff=lightoff)
    _check(s)
    s.close()
    _check_rows(mesh, size, aa, cam, 0.0 if name == "sphere" else 0.1, far, lightoff=lightoff)


def test_open_shell_from_inside_back_records_carry_the_gradient():
    v, f, tex, views, far = _hemisphere()
    cam = (views[0][:3, :3], views[0][:3, 3])
    s = Scene((v, f, tex), 20, True, cam, 0.0, far)
    assert (s.keep["face_index"] >= len(f)).any() and not ((s.keep["face_index"] >= 0) & (s.keep["face_index"] < len(f))).any()
    _, _, _, want = _check(s)
    rows, n, S = want["frec"]
    assert S[len(f):].any() and not S[:len(f)].any()                   # only back records have terms: corner c of one is the face's corner 2 - c
    s.close()
    s = Scene((v, f, tex), 20, True, cam, 0.0, far, fill_back=False)    # nothing is drawn: every gradient is exactly zero
    _check(s, need_terms=False)
    s.close()
    for lightoff in (True, False):
        _check_rows((v, f, tex), 20, True, cam, 0.0, far, lightoff=lightoff)


def test_big_face_long_walks_many_lines_and_a_large_box():
    """output 40 with anti-aliasing: 80-pixel walks, more than 64 lines per edge, a pixel box above BF_TEX_GATHER_MAX = 4096"""
    s = Scene(_big_face(), 40, True, EYE)
    fv = s.keep["fv"][0]
    px = 0.5 * (fv[:, :2] * 80 + 79)
    assert np.ptp(px[:, 0]) > 64 and np.ptp(px[:, 1]) > 64 and np.ptp(px[:, 0]) * np.ptp(px[:, 1]) > 4096
    _check(s)
    s.close()
    for lightoff in (True, False):
        _check_rows(_big_face(), 40, True, EYE, lightoff=lightoff)


def test_a_walk_longer_than_a_wave():
    """output 64 with anti-aliasing (128 pixels a side): a small triangle at the left border, whose "out" walks run ~110 pixels to
    the right border - two strides of the 64 lanes"""
    v = np.array([[-0.95, -0.2, 2.0], [-0.8, -0.15, 2.1], [-0.9, 0.1, 1.9]], np.float32)
    mesh = (v, np.array([[0, 1, 2]], np.int32), _distinct(1, 2, seed=5))
    s = Scene(mesh, 64, True, None)
    _, _, _, want = _check(s, which=("rgb", "alpha"))
    assert want["frec"][1].max() > 64
    s.close()
    for lightoff in (True, False):
        _check_rows(mesh, 64, True, None, which=("rgb", "alpha"), lightoff=lightoff)


def test_a_vertex_of_valence_70():
    ang = np.linspace(0, 2 * np.pi, 71)[:-1]
    ring = np.stack([0.7 * np.cos(ang), 0.7 * np.sin(ang), 2.0 + 0.2 * np.sin(3 * ang)], 1)
    v = np.concatenate([[[0.03, -0.02, 1.7]], ring]).astype(np.float32)
    f = np.array([[0, 1 + i, 1 + (i + 1) % 70] for i in range(70)], np.int32)
    mesh = (v, f, _distinct(70, 2, seed=6))
    s = Scene(mesh, 20, True, EYE)
    _, _, _, want = _check(s)
    assert want["verts"][2][0].all()                                  # the apex has terms in x, y and z
    s.close()
    for lightoff in (True, False):
        _check_rows(mesh, 20, True, EYE, lightoff=lightoff)


def test_a_degenerate_face():
    mesh = _sphere(degenerate=True)
    cam, far = _view(mesh[0], 3)
    s = Scene(mesh, 20, True, cam, 0.0, far)
    gv, _, _, _ = _check(s)
    assert np.isfinite(gv).all()
    s.close()
    for lightoff in (True, False):
        _check_rows(mesh, 20, True, cam, 0.0, far, lightoff=lightoff)


@pytest.mark.parametrize("which", [("rgb",), ("depth",), ("alpha",), ALL])
@pytest.mark.parametrize("lightoff", [False, True])
def test_each_cotangent_alone_and_together_lit_and_unlit(which, lightoff):
    mesh = _sphere()
    cam, far = _view(mesh[0], 0)
    s = Scene(mesh, 20, True, cam, 0.0, far, lightoff=lightoff)
    _check(s, which=which, seed=2)
    s.close()
    _check_rows(mesh, 20, True, cam, 0.0, far, which=which, seed=2, lightoff=lightoff)


@pytest.mark.parametrize("want", [("alpha",), ("depth",), ("rgb",)])
def test_single_output_renders(want):
    """render_silhouettes / render_depth need no textures; render_rgb has no alpha term in diff_grad"""
    v, f, tex = _sphere()
    cam, far = _view(v, 5)
    s = Scene((v, f, tex if "rgb" in want else None), 20, True, cam, 0.0, far, want=want)
    _check(s, which=want)
    s.close()
    _check_rows((v, f, tex), 20, True, cam, 0.0, far, which=want, want=want, lightoff="rgb" not in want)


# ---- tapes ---------------------------------------------------------------------------------------------------------------------------

def test_a_tape_outlives_set_vertices_set_textures_and_its_mesh_and_keeps_the_old_texture_bits():
    mesh = _sphere()
    cam, far = _view(mesh[0], 0)
    s = Scene(mesh, 20, True, cam, 0.0, far)
    g = s.cotangents()
    first = s.tape.vertex_grad(*g)
    _, _, _, old = s.r.render(s.m, tape=True, **s.args)                 # bf_nr_render's tape: the texture gradient's old path
    tex_old = old.texture_grad(g[0])
    assert s.tape.texture_grad(g[0]).tobytes() == tex_old.tobytes()
    old.close()
    s.m.set_vertices(s.v + np.float32(0.05))
    moved = s.r.render_taped(s.m, flags=native.TAPE_GEOMETRY, **s.args)
    assert not np.array_equal(moved[2], s.got[2])                      # (the new positions are drawn)
    moved[3].close()
    s.m.set_textures(np.zeros_like(s.tex))
    for stage in ("after set_vertices and set_textures", "after the mesh is destroyed"):
        again = s.tape.vertex_grad(*g)
        for a, b in zip(first, again):
            assert a.tobytes() == b.tobytes(), stage
        assert s.tape.texture_grad(g[0]).tobytes() == tex_old.tobytes(), stage
        s.m.close()
    s.close()


def test_refusals():
    mesh = _sphere()
    cam, far = _view(mesh[0], 0)
    s = Scene(mesh, 8, False, cam, 0.0, far, want=("alpha",))
    g = s.cotangents(ALL)
    n = s.size

    def code(fn):
        with pytest.raises(_lib.BodyfitError) as e:
            fn()
        return int(re.search(r"failed \((-?\d+)\)", str(e.value)).group(1))

    assert code(lambda: s.tape.vertex_grad(np.zeros((3, n, n), np.float32), None, None)) == BF_ERR_INVALID        # no rgb was rendered
    assert code(lambda: s.tape.vertex_grad(None, np.zeros((n, n), np.float32), None)) == BF_ERR_INVALID
    _, _, _, tex_tape = s.r.render(s.m, tape=True, **{**s.args, "want": ALL})
    assert code(lambda: tex_tape.vertex_grad()) == BF_ERR_INVALID                                                        # a tape without GEOMETRY
    tex_tape.close()
    geo = s.r.render_taped(s.m, flags=native.TAPE_GEOMETRY, **s.args)[3]
    assert code(lambda: geo.texture_grad(np.zeros((3, n, n), np.float32))) == BF_ERR_INVALID                       # a tape without TEXTURES
    geo.close()
    assert code(lambda: s.r.render_taped(s.m, flags=0, **s.args)) == BF_ERR_INVALID
    assert code(lambda: s.r.render_taped(s.m, flags=4, **s.args)) == BF_ERR_INVALID
    bare = native.NrMesh(s.r, s.v, s.f)
    assert code(lambda: s.r.render_taped(bare, flags=BOTH, **s.args)) == BF_ERR_INVALID                            # a texture tape of a mesh without textures
    bare.close()
    ndc = s.r.render_taped(s.m, flags=native.TAPE_GEOMETRY, ndc=True, want=("alpha",))[3]
    assert code(lambda: ndc.vertex_grad(None, None, g[2], camera=True)) == BF_ERR_INVALID                           # an ndc render has no R, t
    ndc.close()
    s.r.close()
    assert code(lambda: s.tape.vertex_grad(None, None, g[2])) == BF_ERR_INVALID                                     # the renderer is gone
    s.tape.close(); s.m.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------

def _adam(step, v0, steps=20, lr=np.float32(5e-3)):
    """torch.optim.Adam's update (betas 0.9 / 0.999, eps 1e-8) in float32 numpy; step(v) -> (loss, gradient).  -> the losses before
    each step and after the last"""
    F = np.float32
    v, m, s, b1, b2, eps = v0.copy(), np.zeros_like(v0), np.zeros_like(v0), F(0.9), F(0.999), F(1e-8)
    losses = []
    for i in range(1, steps + 1):
        loss, g = step(v)
        losses.append(loss)
        m = (b1 * m + (F(1) - b1) * g).astype(F); s = (b2 * s + (F(1) - b2) * g * g).astype(F)
        v = (v - lr * (m / (F(1) - b1 ** i)) / (np.sqrt(s / (F(1) - b2 ** i)) + eps)).astype(F)
    losses.append(step(v)[0])
    return np.array(losses)


def test_twenty_adam_steps_move_a_sphere_onto_a_shifted_silhouette():
    """A sphere's 42 vertices, output 16 with anti-aliasing, loss = sum (alpha - target)^2 against the silhouette of the sphere
    shifted by (0.25, 0.15): the loss goes from 22.06 to 8.56 in the oracle loop.  The device loop gets the same Adam arithmetic
    and differs only through its gradient, which is held to (n + K_FINAL) 2^-23 S of the oracle's.  Drift, measured on the CPU:
    the oracle loop with every gradient value moved by that whole bound, random signs, three seeds, ended at 8.875, 8.5625 and
    8.5625 - at most 0.3125 (five quarter-pixels) from the undisturbed 8.5625; the loss is a sum of squares of multiples of 1/4, so
    it moves in such steps when a pixel changes hands.  Allowed here: 2 x 0.3125."""
    F = np.float32
    size = 16
    v, f = icosphere(1)
    v = (v * 0.6 + np.array([0, 0, 2.5], F)).astype(F)
    cam = dict(K=_K(size), R=EYE[0], t=EYE[1], orig_size=size)
    cfg = dict(image_size=size, anti_aliasing=True, near=F(0.1), far=F(10.0))
    target = VO.render(v + np.array([0.25, 0.15, 0], F), f, None, want=("alpha",), lightoff=True, **cam, **cfg)[2]
    r = native.NrRenderer(size, True, 0.1, 10.0)
    m = native.NrMesh(r, v, f)
    uploads = []

    def device(vv):
        m.set_vertices(vv)
        uploads.append(1)
        _, _, alpha, tape = r.render_taped(m, want=("alpha",), lightoff=True, flags=native.TAPE_GEOMETRY, **cam)
        d = (alpha - target).astype(F)
        g = tape.vertex_grad(None, None, (F(2) * d).astype(F))[0]
        tape.close()
        return float((d.astype(np.float64) ** 2).sum()), g

    def oracle(vv):
        _, _, alpha, keep = VO.render(vv, f, None, want=("alpha",), lightoff=True, **cam, **cfg)
        d = (alpha - target).astype(F)
        return float((d.astype(np.float64) ** 2).sum()), VO.vertex_vjp(keep, g_alpha=(F(2) * d).astype(F))["verts"][0].astype(F)

    got, want = _adam(device, v), _adam(oracle, v)
    print("device losses", got, "\noracle losses", want)
    assert got[0] == want[0] and got[-1] < 0.5 * got[0]
    assert abs(got[-1] - want[-1]) <= 2 * 0.3125
    m.close(); r.close()
