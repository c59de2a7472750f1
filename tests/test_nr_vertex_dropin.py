"""`neural_renderer.Renderer` with `geometry_grad` on, on a machine without a GPU: native.NrRenderer / NrMesh / NrTape are replaced
by tests/nr_vertex_oracle.py's stand-ins, so everything above the C ABI runs - the switch, which inputs join the autograd node,
how gradients of shared cameras are summed, the mesh cache's vertex uploads, tape lifetime, the refusals.  The numbers behind the
stand-ins are held to the reference by tests/test_nr_vertex_oracle.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bodyfitting_amd import native
from bodyfitting_amd import neural_renderer as nr
from texfit_cases import icosphere
import nr_vertex_oracle as VO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IS = 8
K = np.array([[[IS, 0, IS // 2], [0, IS, IS // 2], [0, 0, 1]]], np.float32)
R = np.eye(3, dtype=np.float32)[None]
T = np.zeros((1, 1, 3), np.float32)
CFG = dict(image_size=IS, near=np.float32(0.1), far=np.float32(10.0))


@pytest.fixture(autouse=True)
def oracle_backend(monkeypatch):
    monkeypatch.setattr(native, "NrRenderer", VO.OracleRenderer)
    monkeypatch.setattr(native, "NrMesh", VO.OracleMesh)
    monkeypatch.setattr(native, "NrTape", VO.OracleTape)
    log = VO.OracleRenderer.LOG
    log["vertex_uploads"] = 0
    for k in log:
        log[k] = 0
    return log


def _mesh(ts=2, seed=0):
    v, f = icosphere(1)
    v = (v * 0.6 + np.array([0.05, -0.03, 2.5], np.float32)).astype(np.float32)
    tex = np.random.default_rng(seed).uniform(0, 1, (len(f), ts, ts, ts, 3)).astype(np.float32)
    return v, f, tex


def _renderer(**kw):
    cfg = dict(image_size=IS, K=K, R=R, t=T, orig_size=IS, near=0.1, far=10.0)
    cfg.update(kw)
    r = nr.Renderer(**cfg)
    r.geometry_grad = True                                            # (whatever BF_NR_GEOMETRY_GRAD was at import)
    return r


def _tensors(v, f, tex):
    return torch.from_numpy(v.copy())[None], torch.from_numpy(f)[None], torch.from_numpy(tex.copy())[None]


def _cot(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def test_the_switch_is_a_module_attribute_and_an_instance_attribute_not_a_parameter(monkeypatch):
    import inspect
    assert nr.GEOMETRY_GRAD is (os.environ.get("BF_NR_GEOMETRY_GRAD", "") == "1")          # read once, at import
    assert "geometry_grad" not in inspect.signature(nr.Renderer.__init__).parameters
    for value in (False, True):
        monkeypatch.setattr(nr, "GEOMETRY_GRAD", value)
        assert nr.Renderer(image_size=IS).geometry_grad is value


def test_gradients_of_vertices_R_t_and_textures_from_one_node_only_where_asked(oracle_backend):
    v, f, tex = _mesh()
    r = _renderer(light_direction=[0.3, 0.8, -0.5])
    tv, tf, tt = _tensors(v, f, tex)
    tR, tT = torch.from_numpy(R.copy()), torch.from_numpy(T.copy())
    for x in (tv, tt, tR, tT):
        x.requires_grad_(True)
    rgb, depth, alpha = r.render(tv, tf, tt, R=tR, t=tT)
    assert oracle_backend["tapes_open"] == 1 and rgb.grad_fn is depth.grad_fn is alpha.grad_fn        # one node per render
    g = [_cot(o.shape, i) for i, o in enumerate((rgb, depth, alpha))]
    gv, gt, gR, gT = torch.autograd.grad((rgb * g[0]).sum() + (depth * g[1]).sum() + (alpha * g[2]).sum(), (tv, tt, tR, tT))
    assert oracle_backend["tapes_open"] == 0
    for grad, x in ((gv, tv), (gt, tt), (gR, tR), (gT, tT)):
        assert grad.shape == x.shape and grad.dtype == torch.float32 and not grad.requires_grad
    light = dict(ambient=0.5, directional=0.5, color_ambient=(1, 1, 1), color_directional=(1, 1, 1),
                 direction=np.array([0.3, 0.8, -0.5], np.float32))       # (float32, as the Renderer hands it down)
    *_, keep = VO.render(v, f, tex, K[0], R[0], T[0, 0], IS, light=light, **CFG)
    want = VO.vertex_vjp(keep, *[x[0].numpy() for x in g])
    np.testing.assert_array_equal(gv[0].numpy(), want["verts"][0].astype(np.float32))
    np.testing.assert_array_equal(gR[0].numpy(), want["R"][0].astype(np.float32))
    np.testing.assert_array_equal(gT[0, 0].numpy(), want["t"][0].astype(np.float32))
    assert gv.abs().sum() > 0 and gR.abs().sum() > 0 and gT.abs().sum() > 0 and gt.abs().sum() > 0
    # the textures' gradient still sees the rgb cotangent only: bit-zero for depth and alpha
    out = r.render(tv, tf, tt)
    gv2, gt2 = torch.autograd.grad(out[1].sum() + out[2].sum(), (tv, tt))
    assert not gt2.any() and gv2.any()
    # only what requires grad joins the node; nothing does under no_grad or when nothing asks
    out = r.render_silhouettes(tv.detach(), tf, R=tR)
    (gR3,) = torch.autograd.grad(out.sum(), tR)
    assert gR3.shape == tR.shape and out.requires_grad
    assert not r.render_silhouettes(tv.detach(), tf).requires_grad and oracle_backend["tapes_open"] == 0
    with torch.no_grad():
        assert not r.render_silhouettes(tv, tf).requires_grad and oracle_backend["tapes_open"] == 0
    with pytest.raises(RuntimeError):                                 # once differentiable, and the tape is spent
        torch.autograd.grad(rgb.sum(), tv)


@pytest.mark.parametrize("mode", ["silhouettes", "depth", "rgb", None])
def test_every_mode_differentiates_the_vertices(mode, oracle_backend):
    v, f, tex = _mesh()
    r = _renderer()
    tv, tf, tt = _tensors(v, f, tex)
    tv.requires_grad_(True)
    args = (tv, tf) if mode in ("silhouettes", "depth") else (tv, tf, tt)
    out = r(*args, mode=mode)
    direct = dict(silhouettes=lambda: r.render_silhouettes(tv, tf), depth=lambda: r.render_depth(tv, tf), rgb=lambda: r.render_rgb(tv, tf, tt),
                  none=lambda: r.render(tv, tf, tt))[mode or "none"]()
    outs = out if isinstance(out, tuple) else (out,)
    for a, b in zip(outs, direct if isinstance(direct, tuple) else (direct,)):
        assert torch.equal(a, b) and a.requires_grad
    g = [_cot(o.shape, i) for i, o in enumerate(outs)]
    (gv,) = torch.autograd.grad(sum((o * c).sum() for o, c in zip(outs, g)), tv)
    want_names = dict(silhouettes=("alpha",), depth=("depth",), rgb=("rgb",)).get(mode, ("rgb", "depth", "alpha"))
    *_, keep = VO.render(v, f, tex if "rgb" in want_names else None, K[0], R[0], T[0, 0], IS, want=want_names, lightoff="rgb" not in want_names, **CFG)
    cots = dict(zip(want_names, (c[0].numpy() for c in g)))
    want = VO.vertex_vjp(keep, cots.get("rgb"), cots.get("depth"), cots.get("alpha"))
    np.testing.assert_array_equal(gv[0].numpy(), want["verts"][0].astype(np.float32))
    assert gv.any()
    del direct, a, b
    assert oracle_backend["tapes_open"] == 0                          # the other graph was dropped: its tape went with it


def test_a_camera_shared_by_a_batch_of_two_takes_the_sum(oracle_backend):
    v, f, _ = _mesh()
    r = _renderer()
    v2 = torch.from_numpy(np.stack([v, v + np.float32(0.07)]))
    f2 = torch.from_numpy(np.stack([f, f]))
    tR, tT = torch.from_numpy(R.copy()).requires_grad_(True), torch.from_numpy(T.copy()).requires_grad_(True)
    assert tR.shape == (1, 3, 3) and tT.shape == (1, 1, 3)
    alpha = r.render_silhouettes(v2, f2, R=tR, t=tT)
    assert alpha.shape == (2, IS, IS) and oracle_backend["tapes_open"] == 2
    g = _cot(alpha.shape, 3)
    gR, gT = torch.autograd.grad((alpha * g).sum(), (tR, tT))
    assert gR.shape == (1, 3, 3) and gT.shape == (1, 1, 3) and oracle_backend["tapes_open"] == 0
    each = []
    for b in range(2):
        *_, keep = VO.render(v2[b].numpy(), f, None, K[0], R[0], T[0, 0], IS, want=("alpha",), lightoff=True, **CFG)
        each.append(VO.vertex_vjp(keep, g_alpha=g[b].numpy()))
    np.testing.assert_array_equal(gR[0].numpy(), each[0]["R"][0].astype(np.float32) + each[1]["R"][0].astype(np.float32))
    np.testing.assert_array_equal(gT[0, 0].numpy(), each[0]["t"][0].astype(np.float32) + each[1]["t"][0].astype(np.float32))
    # per-item cameras get per-item gradients
    R2 = torch.from_numpy(np.concatenate([R, R])).requires_grad_(True)
    (gR2,) = torch.autograd.grad((r.render_silhouettes(v2, f2, R=R2, t=tT.detach()) * g).sum(), R2)
    for b in range(2):
        np.testing.assert_array_equal(gR2[b].numpy(), each[b]["R"][0].astype(np.float32))


def test_two_renders_in_one_graph_and_tape_lifetime(oracle_backend):
    v, f, _ = _mesh()
    r = _renderer()
    tv, tf, _ = _tensors(v, f, _mesh()[2])
    tv.requires_grad_(True)
    Rb = torch.from_numpy(np.array([[[0.96, 0, 0.28], [0, 1, 0], [-0.28, 0, 0.96]]], np.float32))
    tb = torch.from_numpy(np.array([[[-0.7, 0, 0.1]]], np.float32))
    g = _cot((1, IS, IS), 4)
    a, b = r.render_silhouettes(tv, tf), r.render_depth(tv, tf, R=Rb, t=tb)
    assert oracle_backend["tapes_open"] == 2 and oracle_backend["meshes"] == 1
    ((a * g).sum() + (b * g).sum()).backward()
    assert oracle_backend["tapes_open"] == 0
    (ga,) = torch.autograd.grad((r.render_silhouettes(tv, tf) * g).sum(), tv)
    (gb,) = torch.autograd.grad((r.render_depth(tv, tf, R=Rb, t=tb) * g).sum(), tv)
    np.testing.assert_array_equal(tv.grad.numpy(), (ga + gb).numpy())
    assert ga.any() and gb.any()
    out = r.render_silhouettes(tv, tf)                                # a graph that is dropped frees its tape
    assert oracle_backend["tapes_open"] == 1
    del out
    assert oracle_backend["tapes_open"] == 0


def test_K_is_still_refused_with_a_message_of_its_own():
    v, f, tex = _mesh()
    r = _renderer()
    tv, tf, tt = _tensors(v, f, tex)
    tK = torch.from_numpy(K.copy()).requires_grad_(True)
    for call in (lambda: r.render(tv, tf, tt, K=tK), lambda: r.render_silhouettes(tv, tf, K=tK), lambda: r.render_depth(tv, tf, K=tK)):
        with pytest.raises(NotImplementedError, match="K is not differentiated"):
            call()
    with torch.no_grad():
        r.render_silhouettes(tv, tf, K=tK)
    r.geometry_grad = False                                           # set back: today's refusal, today's message
    with pytest.raises(NotImplementedError, match="soft-edge vertex gradient"):
        r.render_silhouettes(tv.clone().requires_grad_(True), tf)
    with pytest.raises(NotImplementedError, match="soft-edge vertex gradient"):
        r.render_silhouettes(tv, tf, K=tK)


def test_three_adam_steps_on_the_vertices_one_mesh_three_vertex_uploads(oracle_backend):
    v, f, _ = _mesh()
    r = _renderer()
    tv, tf, _ = _tensors(v, f, _mesh()[2])
    with torch.no_grad():
        target = r.render_silhouettes(tv + torch.tensor([0.15, 0.1, 0.0]), tf)
    meshes_before = oracle_backend["meshes"]
    tv.requires_grad_(True)
    opt = torch.optim.Adam([tv], lr=1e-2)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = torch.sum((r.render_silhouettes(tv, tf) - target) ** 2)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert tv.grad.any()
    r.render_silhouettes(tv, tf)                                      # (the last step's positions go up at the next render)
    r.render_silhouettes(tv, tf)
    assert oracle_backend["meshes"] == meshes_before + 1 and oracle_backend["vertex_uploads"] == 3
    assert oracle_backend["tapes_open"] == 0
    r.geometry_grad = False                                           # off: a changed _version rebuilds the mesh, as before
    with torch.no_grad():
        tv.add_(0.0)
        r.render_silhouettes(tv, tf)
    assert oracle_backend["meshes"] == meshes_before + 2 and oracle_backend["vertex_uploads"] == 3


def test_with_the_switch_off_only_todays_calls_reach_the_backend(monkeypatch):
    """off, the Renderer calls nothing newer than tests/nr_oracle.py's stand-ins know (the existing drop-in tests run on those)"""
    import nr_oracle as NO
    monkeypatch.setattr(native, "NrRenderer", NO.OracleRenderer)
    monkeypatch.setattr(native, "NrMesh", NO.OracleMesh)
    monkeypatch.setattr(native, "NrTape", NO.OracleTape)
    monkeypatch.setattr(nr, "GEOMETRY_GRAD", False)                   # (the default, whatever this process's environment says)
    v, f, tex = _mesh()
    r = nr.Renderer(image_size=IS, K=K, R=R, t=T, orig_size=IS, near=0.1, far=10.0)
    tv, tf, tt = _tensors(v, f, tex)
    tt.requires_grad_(True)
    r.render(tv, tf, tt)[0].sum().backward()
    tv.add_(0.0)
    r.render_silhouettes(tv, tf)
    assert tt.grad.any()


def test_the_module_imported_in_a_child_process_reads_the_variable_once():
    code = ("import torch, numpy as np\n"
            "from bodyfitting_amd import neural_renderer as nr\n"
            "print(nr.GEOMETRY_GRAD, nr.Renderer(image_size=8).geometry_grad)\n"
            "r = nr.Renderer(image_size=8, K=np.eye(3, dtype=np.float32)[None], R=np.eye(3, dtype=np.float32)[None], t=np.zeros((1, 1, 3), np.float32), orig_size=8)\n"
            "v = torch.zeros(1, 3, 3, requires_grad=True); f = torch.zeros(1, 1, 3, dtype=torch.int32)\n"
            "try:\n"
            "    r.render_silhouettes(v, f)\n"
            "except NotImplementedError as e:\n"
            "    print('refused:', 'soft-edge vertex gradient' in str(e) and 'backward_pixel_map' in str(e) and 'backward_depth_map' in str(e))\n")
    for value, want in ((None, "False False"), ("0", "False False"), ("1", "True True")):
        env = {k: v for k, v in os.environ.items() if k != "BF_NR_GEOMETRY_GRAD"}
        if value is not None:
            env["BF_NR_GEOMETRY_GRAD"] = value
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=REPO, env=env)
        lines = out.stdout.splitlines()
        assert out.returncode == 0 or value == "1", out.stderr[-800:]
        assert lines[0] == want, (value, out.stdout, out.stderr[-400:])
        if value != "1":
            assert lines[1] == "refused: True"                        # unset or off: refused exactly as before
