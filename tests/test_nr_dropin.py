"""The drop-in `neural_renderer` (bodyfitting_amd/neural_renderer.py, bodyfitting_amd/dropin_nr) on a machine without a GPU:
`native.NrRenderer` / `NrMesh` / `NrTape` are replaced by tests/nr_oracle.py's stand-ins, so everything above the C ABI runs -
argument handling, the batch loop, autograd, the mesh cache, the refusals.  The oracle's own light and projection are held to what
the reference's lighting.py and projection.py returned (tests/golden/nr_lighting.npz, tools/gen_nr_golden.py)."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bodyfitting_amd import native
from bodyfitting_amd import neural_renderer as nr
from bodyfitting_amd import obj_textures as OT
from oracle import texfit_oracle as TO
from texfit_cases import icosphere
import nr_oracle as NO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "nr_lighting.npz")
# renderer.py:12-19, recorded
REFERENCE_INIT = [("image_size", 256), ("anti_aliasing", True), ("background_color", [0, 0, 0]), ("fill_back", True),
                  ("camera_mode", 'projection'), ("K", None), ("R", None), ("t", None), ("dist_coeffs", None), ("orig_size", 1024),
                  ("perspective", True), ("viewing_angle", 30), ("camera_direction", [0, 0, 1]), ("near", 0.1), ("far", 100),
                  ("light_intensity_ambient", 0.5), ("light_intensity_directional", 0.5), ("light_color_ambient", [1, 1, 1]),
                  ("light_color_directional", [1, 1, 1]), ("light_direction", [0, 1, 0])]
IS = 8
K = np.array([[[IS, 0, IS // 2], [0, IS, IS // 2], [0, 0, 1]]], np.float32)
R = np.eye(3, dtype=np.float32)[None]
T = np.zeros((1, 1, 3), np.float32)


@pytest.fixture(autouse=True)
def oracle_backend(monkeypatch):
    monkeypatch.setattr(native, "NrRenderer", NO.OracleRenderer)
    monkeypatch.setattr(native, "NrMesh", NO.OracleMesh)
    monkeypatch.setattr(native, "NrTape", NO.OracleTape)
    for k in NO.OracleRenderer.LOG:
        NO.OracleRenderer.LOG[k] = 0
    return NO.OracleRenderer.LOG


def _mesh(ts=2, seed=0):
    v, f = icosphere(1)
    v = (v * 0.6 + np.array([0, 0, 2.5], np.float32)).astype(np.float32)
    tex = np.random.default_rng(seed).uniform(0, 1, (len(f), ts, ts, ts, 3)).astype(np.float32)
    return v, f, tex


def _renderer(**kw):
    cfg = dict(image_size=IS, K=K, R=R, t=T, orig_size=IS, near=0.1, far=10.0)
    cfg.update(kw)
    return nr.Renderer(**cfg)


def _tensors(v, f, tex):
    return torch.from_numpy(v)[None], torch.from_numpy(f)[None], torch.from_numpy(tex.copy())[None]


# ---- the oracle against the reference's own lighting and projection ----------------------------------------------------------------

def test_oracle_light_and_projection_follow_the_reference_golden():
    """Largest differences measured here (printed below): light and lit textures 1.19e-07 (one unit in the last
    place of values in [1, 2)), projection 2.38e-07 - torch sums three products in another order than the fixed left-to-right one.
    Asserted: 4 x that."""
    g = np.load(GOLDEN)
    worst_light = worst_lit = 0.0
    for row, want_light, want_lit in zip(g["lights"], g["light"], g["lit"]):
        rows = NO.light_rows(g["face_world"], row[0], row[1], row[2:5], row[5:8], row[8:11])
        worst_light = max(worst_light, float(np.abs(rows - want_light).max()))
        worst_lit = max(worst_lit, float(np.abs((g["textures"] * rows[:, None, None, None, :]).astype(np.float32) - want_lit).max()))
    worst_proj = 0.0
    for cam, want in zip(g["cams"], g["projected"]):
        got = TO.project(g["verts"], cam[:9].reshape(3, 3), cam[9:18].reshape(3, 3), cam[18:21], float(cam[21]))
        worst_proj = max(worst_proj, float(np.abs(got - want).max()))
    print(f"largest difference: light {worst_light:.3g}, lit textures {worst_lit:.3g}, projection {worst_proj:.3g}")
    assert worst_light <= 4 * 1.19e-07 and worst_lit <= 4 * 1.19e-07
    assert worst_proj <= 4 * 2.38e-07


def test_a_degenerate_face_gets_the_ambient_term_exactly():
    face = np.array([[[0.3, 0.2, 1.0], [0.3, 0.2, 1.0], [0.5, 0.1, 2.0]], [[1, 1, 1], [1, 1, 1], [1, 1, 1]]], np.float32)
    rows = NO.light_rows(face, 0.3, 0.8, (1.0, 0.9, 0.7), (0.6, 1.0, 0.8), (0.3, 0.8, -0.5))
    np.testing.assert_array_equal(rows, np.tile(np.float32(0.3) * np.array([1.0, 0.9, 0.7], np.float32), (2, 1)))
    np.testing.assert_array_equal(NO.light_rows(face, 0.0, 0.0), np.zeros((2, 3), np.float32))


# ---- names ---------------------------------------------------------------------------------------------------------------------------

def test_import_names_resolve_in_a_child_process():
    code = ("import os, sys, bodyfitting_amd\n"
            "root = os.path.dirname(bodyfitting_amd.__file__)\n"
            "sys.path.insert(0, os.path.join(root, 'dropin_nr'))\n"
            "import neural_renderer as nr\n"
            "assert nr.__file__.startswith(os.path.join(root, 'dropin_nr')), nr.__file__\n"
            "from neural_renderer import Renderer, load_obj, save_obj\n"
            "assert nr.__version__ == '1.1.3' and callable(nr.Renderer)\n"
            "for name in ('lighting', 'look_at', 'Mesh', 'rasterize', 'vertices_to_faces', 'projection'):\n"
            "    try:\n"
            "        getattr(nr, name)\n"
            "    except NotImplementedError:\n"
            "        continue\n"
            "    raise SystemExit(name + ' did not raise')\n"
            "try:\n"
            "    nr.no_such_name\n"
            "except AttributeError:\n"
            "    print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=REPO)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr[-800:]


def test_constructor_list_is_the_reference_list():
    params = list(inspect.signature(nr.Renderer.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == REFERENCE_INIT
    r = nr.Renderer()
    assert r.to("cuda") is r and r.cuda() is r and r.rasterizer_eps == 1e-3


# ---- shapes, modes, arrays ----------------------------------------------------------------------------------------------------------

def test_shapes_dtypes_modes_and_the_numpy_path():
    v, f, tex = _mesh()
    r = _renderer()
    tv, tf, tt = _tensors(v, f, tex)
    out = r.render(tv, tf, tt)
    assert isinstance(out, tuple) and len(out) == 3
    rgb, depth, alpha = out
    assert rgb.shape == (1, 3, IS, IS) and depth.shape == alpha.shape == (1, IS, IS)
    assert all(o.dtype == torch.float32 and o.device == tv.device and not o.requires_grad for o in out)
    want = NO.render(v, f, tex, K[0], R[0], T[0, 0], IS, image_size=IS, near=np.float32(0.1), far=np.float32(10.0))
    for got, ref in zip(out, want):
        np.testing.assert_array_equal(got[0].numpy(), ref)
    assert 0 < float(alpha.mean()) < 1
    for got, ref in zip(r(tv, tf, tt), out):                          # forward / __call__, mode=None
        assert torch.equal(got, ref)
    assert torch.equal(r(tv, tf, tt, mode='rgb'), rgb) and torch.equal(r.render_rgb(tv, tf, tt), rgb)
    assert torch.equal(r(tv, tf, mode='silhouettes'), alpha) and torch.equal(r.render_silhouettes(tv, tf), alpha)
    assert torch.equal(r(tv, tf, mode='depth'), depth) and torch.equal(r.render_depth(tv, tf), depth)
    with pytest.raises(ValueError):
        r(tv, tf, tt, mode='normals')
    assert not torch.equal(r.render_rgb(tv, tf, tt, lightoff=True), rgb)
    # arrays in, arrays out; cameras per call override the constructor's
    a_rgb, a_depth, a_alpha = r.render(v[None], f[None], tex[None], K=K, R=R, t=T, orig_size=IS)
    assert isinstance(a_rgb, np.ndarray) and a_rgb.dtype == np.float32
    np.testing.assert_array_equal(a_rgb, rgb.numpy())
    np.testing.assert_array_equal(a_alpha, alpha.numpy())
    # a batch of two is a host loop: two cameras for one K
    v2, f2, t2 = np.stack([v, v]), np.stack([f, f]), np.stack([tex, tex[::-1]])
    R2 = np.stack([R[0], np.diag([-1.0, 1.0, 1.0]).astype(np.float32)])
    b_rgb = r.render_rgb(v2, f2, t2, R=R2)
    assert b_rgb.shape == (2, 3, IS, IS)
    np.testing.assert_array_equal(b_rgb[0], a_rgb[0])
    np.testing.assert_array_equal(b_rgb[1], NO.render(v, f, tex[::-1], K[0], R2[1], T[0, 0], IS, image_size=IS, near=np.float32(0.1), far=np.float32(10.0))[0])
    # the light is read at every render, like the reference reads its attributes
    r.light_intensity_directional = 0.0
    r.light_intensity_ambient = 1.0
    np.testing.assert_array_equal(r.render_rgb(v[None], f[None], tex[None]), r.render_rgb(v[None], f[None], tex[None], lightoff=True))


# ---- autograd --------------------------------------------------------------------------------------------------------------------------

def test_adjoint_identity_once_differentiable_and_gradients_only_where_asked(oracle_backend):
    v, f, tex = _mesh(ts=3)
    r = _renderer(light_color_directional=[0.6, 1.0, 0.8], light_direction=[0.3, 0.8, -0.5])
    tv, tf, tt = _tensors(v, f, tex)
    tt.requires_grad_(True)
    rgb = r.render_rgb(tv, tf, tt)
    assert rgb.requires_grad and oracle_backend["tapes_open"] == 1
    g = torch.randn(rgb.shape, generator=torch.Generator().manual_seed(0))
    (grad,) = torch.autograd.grad((rgb * g).sum(), tt)
    assert oracle_backend["tapes_open"] == 0                          # freed by the backward pass
    assert grad.shape == tt.shape and grad.dtype == torch.float32 and not grad.requires_grad          # once differentiable
    with torch.no_grad():
        zero = r.render_rgb(tv, tf, torch.zeros_like(tt))
    # rgb is linear in the textures: <g, render(T) - render(0)> = <vjp(g), T>
    lhs = float(((rgb.detach() - zero).double() * g.double()).sum())
    rhs = float((grad.double() * tt.detach().double()).sum())
    assert lhs == pytest.approx(rhs, rel=1e-5, abs=1e-5) and float(grad.abs().sum()) > 1
    with pytest.raises(RuntimeError):                                 # the graph is spent: a second backward has no tape
        torch.autograd.grad((rgb * g).sum(), tt)
    # no tape without requires_grad, or under no_grad
    assert not r.render_rgb(tv, tf, tt.detach()).requires_grad and oracle_backend["tapes_open"] == 0
    with torch.no_grad():
        assert not r.render_rgb(tv, tf, tt).requires_grad and oracle_backend["tapes_open"] == 0
    # depth and alpha cotangents: bit-zero
    out = r.render(tv, tf, tt)
    (gz,) = torch.autograd.grad(out[1].sum() + out[2].sum(), tt)
    assert not gz.any() and oracle_backend["tapes_open"] == 0
    # a graph that is dropped frees its tape
    out = r.render(tv, tf, tt)
    assert oracle_backend["tapes_open"] == 1
    del out
    assert oracle_backend["tapes_open"] == 0


def test_two_renders_of_one_mesh_in_one_graph_sum(oracle_backend):
    v, f, tex = _mesh()
    r = _renderer()
    tv, tf, tt = _tensors(v, f, tex)
    tt.requires_grad_(True)
    Rb = torch.from_numpy(np.diag([-1.0, 1.0, 1.0]).astype(np.float32))[None]
    g = torch.randn(1, 3, IS, IS, generator=torch.Generator().manual_seed(1))
    a, b = r.render_rgb(tv, tf, tt), r.render_rgb(tv, tf, tt, R=Rb)
    assert oracle_backend["tapes_open"] == 2 and oracle_backend["uploads"] == 1 and oracle_backend["meshes"] == 1
    ((a * g).sum() + (b * g).sum()).backward()
    (ga,) = torch.autograd.grad((r.render_rgb(tv, tf, tt) * g).sum(), tt)
    (gb,) = torch.autograd.grad((r.render_rgb(tv, tf, tt, R=Rb) * g).sum(), tt)
    np.testing.assert_allclose(tt.grad.numpy(), (ga + gb).numpy(), rtol=0, atol=1e-6)
    assert ga.any() and gb.any() and not torch.equal(ga, gb) and oracle_backend["tapes_open"] == 0


def test_textures_go_up_again_only_on_a_version_change(oracle_backend):
    v, f, tex = _mesh()
    r = _renderer()
    tv, tf, tt = _tensors(v, f, tex)
    scan_t = tt.clone()
    tt.requires_grad_(True)
    opt = torch.optim.Adam([tt], lr=1e-2)
    v2 = tv.clone()                                                   # a second (vertices, faces) pair: the loop's two meshes
    for i in range(3):
        opt.zero_grad()
        loss = torch.sum(torch.abs(r.render_rgb(v2, tf, scan_t, lightoff=True) - r.render_rgb(tv, tf, tt)))
        loss.backward()
        opt.step()
    assert oracle_backend["meshes"] == 2 and len(r._meshes) == 2
    assert oracle_backend["uploads"] == 1 + 3                         # the scan's once, the fitted ones once per iteration
    r.render_rgb(tv, tf, tt)
    assert oracle_backend["uploads"] == 1 + 3 + 1                     # (the last step bumped the version)
    r.render_rgb(tv, tf, tt)
    assert oracle_backend["uploads"] == 1 + 3 + 1
    v2.add_(0.0)                                                      # an in-place change of the vertices: the mesh is rebuilt
    r.render_silhouettes(v2, tf)
    assert oracle_backend["meshes"] == 3
    # arrays are remembered by their bytes; four meshes are kept, the oldest goes first
    for k in range(5):
        r.render_silhouettes(v[None] + np.float32(k), f[None])
    assert oracle_backend["meshes"] == 3 + 5 and len(r._meshes) == 4
    r.render_silhouettes(v[None] + np.float32(4), f[None])
    assert oracle_backend["meshes"] == 3 + 5


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------

def test_every_refusal():
    v, f, tex = _mesh()
    tv, tf, tt = _tensors(v, f, tex)
    for mode in ('look', 'look_at', 'orthogonal'):
        with pytest.raises(NotImplementedError, match="camera_mode"):
            nr.Renderer(camera_mode=mode)
    with pytest.raises(ValueError):
        nr.Renderer(camera_mode='fisheye')
    with pytest.raises(NotImplementedError, match="dist_coeffs"):
        nr.Renderer(dist_coeffs=np.array([[0.1, 0, 0, 0, 0]], np.float32))
    nr.Renderer(dist_coeffs=torch.zeros(1, 5))
    r = _renderer()
    with pytest.raises(NotImplementedError, match="dist_coeffs"):
        r.render_rgb(tv, tf, tt, dist_coeffs=torch.tensor([[0.0, 0.01, 0, 0, 0]]))
    for name in ("vertices", "K", "R", "t"):
        args = dict(vertices=tv, K=torch.from_numpy(K), R=torch.from_numpy(R), t=torch.from_numpy(T))
        args[name] = args[name].clone().requires_grad_(True)
        verts = args.pop("vertices")
        with pytest.raises(NotImplementedError, match="soft-edge vertex gradient"):
            r.render(verts, tf, tt, **args)
        with pytest.raises(NotImplementedError, match="backward_depth_map"):
            r.render_depth(verts, tf, **args)
        with pytest.raises(NotImplementedError, match="backward_pixel_map"):
            r.render_silhouettes(verts, tf, **args)
    with torch.no_grad():                                             # nothing is asked to be differentiated here
        r.render_silhouettes(tv.clone().requires_grad_(True), tf)
    with pytest.raises(ValueError):
        r.render_rgb(tv[0], tf, tt)
    with pytest.raises(ValueError):
        r.render_rgb(tv, tf, tt[0])
    with pytest.raises(ValueError):
        r.render_rgb(tv, tf, None)
    with pytest.raises(ValueError):
        nr.Renderer(image_size=IS).render_silhouettes(tv, tf)        # no K, R, t anywhere
    with pytest.raises(NotImplementedError, match="textured form"):
        nr.save_obj("x.obj", tv[0], tf[0], textures=tt[0])
    with pytest.raises(NotImplementedError):
        nr.get_points_from_angles
    with pytest.raises(AttributeError):
        nr.not_a_name_of_the_reference


# ---- files -----------------------------------------------------------------------------------------------------------------------------

def test_save_obj_then_load_obj_round_trips_and_load_obj_is_obj_textures(tmp_path):
    v, f, _ = _mesh()
    path = str(tmp_path / "mesh.obj")
    nr.save_obj(path, torch.from_numpy(v), torch.from_numpy(f))
    lines = open(path).read().splitlines()
    assert lines[0] == "# mesh.obj" and lines[3].startswith("v ") and lines[-1] == "f %d %d %d" % tuple(f[-1] + 1)
    lv, lf = nr.load_obj(path)
    assert isinstance(lv, torch.Tensor) and lv.dtype == torch.float32 and lf.dtype == torch.int32
    np.testing.assert_array_equal(lf.cpu().numpy(), f)
    np.testing.assert_allclose(lv.cpu().numpy(), v, rtol=0, atol=5e-9 + 1e-7 * np.abs(v).max())          # '%.8f'
    for kw in (dict(), dict(normalization=True)):
        want = OT.load_obj(path, **{"normalization": False, **kw})
        got = nr.load_obj(path, **kw)
        assert len(got) == len(want) == 2
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a.cpu().numpy(), b)
    assert list(inspect.signature(nr.load_obj).parameters) == ["filename_obj", "normalization", "texture_size", "load_texture", "texture_wrapping",
                                                               "use_bilinear"]
    nr.save_obj(path, v, f)                                           # arrays as well
    np.testing.assert_array_equal(nr.load_obj(path)[1].cpu().numpy(), f)


def test_render_texture_reads_the_obj_and_draws_both_sides(tmp_path):
    from texfit_cases import uv_atlas
    nf, ts = 6, 2
    uv, uvf = uv_atlas(nf)
    path = str(tmp_path / "uv.obj")
    with open(path, "w") as fh:
        for i in range(3 * nf):
            fh.write(f"v {i} 0 0\n")
        for u, w in uv:
            fh.write(f"vt {float(u)!r} {float(w)!r}\n")
        for a, b, c in uvf + 1:
            fh.write(f"f {a}/{a} {b}/{b} {c}/{c}\n")
    tex = np.random.default_rng(3).uniform(0, 1, (nf, ts, ts, ts, 3)).astype(np.float32)
    r = nr.Renderer(image_size=12, background_color=[1, 1, 1], near=0.0, far=4.0)
    rgb, depth = r.render_texture(path, torch.from_numpy(tex)[None])
    want_rgb, want_depth = TO.render_texture(uv, uvf, tex, 12, 0.0, 4.0)
    assert rgb.shape == (1, 3, 12, 12) and depth.shape == (1, 12, 12) and isinstance(rgb, torch.Tensor)
    np.testing.assert_array_equal(rgb[0].numpy(), want_rgb)
    np.testing.assert_array_equal(depth[0].numpy(), want_depth)
