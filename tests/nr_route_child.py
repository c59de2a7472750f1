"""The device route of neural_renderer.Renderer in FRESH processes (tests/test_gpu_nr_device_route.py): bf_nr_render_dev,
bf_nr_tape_texture_grad_dev, bf_nr_tape_vertex_grad_dev and the drop-in on tensors of cuda:0.  Like tests/mask_route_child.py, torch
is imported before the library, so that both share one HIP runtime, and every function asserts the route it means to measure before
it measures anything.  Every address handed to a *_dev entry is that of a live torch tensor of the stated size.

The yardstick of the equality tests is the host route of the same build - native.NrRenderer.render_taped / NrTape.*_grad on numpy
arrays and the drop-in on CPU tensors, which tests/test_gpu_nr.py and tests/test_gpu_nr_vertex.py hold to the oracles: the device
route issues the same kernels on the same inputs and must give the same BITS (compared as uint32, so that -0.0 is not +0.0)."""
import itertools
import os

import numpy as np
import torch                    # (first: see above)

from device_route_child import GPU, GUARD, _guard_kept, _guarded, _repo, _took
from lanes_child import _run
from scan_route_child import _bits, _same, _stats

ALL = ("rgb", "depth", "alpha")
INVALID = -1


def _start(switch="1"):
    """before the library and the drop-in are imported: the switches as this child means them"""
    os.environ["BF_NR_DEVICE_ROUTE"] = "1"
    os.environ["BF_TORCH_DEVICE_ROUTE"] = switch
    os.environ["BF_NR_GEOMETRY_GRAD"] = "0"
    _repo()
    from bodyfitting_amd import native as N, neural_renderer as nr
    assert nr.DEVICE_ROUTE
    _took("device" if switch != "0" else "host")
    return N, nr


def _gpu(a, grad=False):
    return torch.tensor(np.ascontiguousarray(a), device=GPU, requires_grad=grad)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nr_stats():
    from bodyfitting_amd import native as N
    return N.nr_route_stats()


def _shapes(size):
    return {"rgb": (3, size, size), "depth": (size, size), "alpha": (size, size)}


def _cotangents(size, which, seed):
    rng = np.random.default_rng(seed)
    g = {nm: rng.standard_normal(s).astype(np.float32) for nm, s in _shapes(size).items()}
    return [g[nm] if nm in which else None for nm in ALL]


class Case:
    """one renderer and mesh, and a render + its gradients through either route"""

    def __init__(self, N, mesh, size, aa, cam, near=0.1, far=100.0, light=None, background=(0.1, 0.2, 0.3)):
        from test_gpu_nr import LIGHT, _K
        self.N, self.size, self.cam = N, size, cam
        self.v, self.f, self.tex = mesh
        self.r = N.NrRenderer(size, aa, near, far, background)
        self.r.set_light(**(light or LIGHT))
        self.ts = 0 if self.tex is None else self.tex.shape[1]
        self.m = N.NrMesh(self.r, self.v, self.f, self.ts, self.tex)
        self.K = _K(size)
        self.light = light or LIGHT
        self.cfg = dict(image_size=size, anti_aliasing=aa, near=np.float32(near), far=np.float32(far), background=background)
        self.d_v, self.d_tex = _gpu(self.v), (None if self.tex is None else _gpu(self.tex))

    def args(self):
        return dict(ndc=True) if self.cam is None else dict(K=self.K, R=self.cam[0], t=self.cam[1], orig_size=self.size)

    def host(self, fill_back, lightoff, want, flags):
        return self.r.render_taped(self.m, fill_back=fill_back, lightoff=lightoff, want=want, flags=flags, **self.args())

    def dev(self, fill_back, lightoff, want, flags, by_address=(False, False, False), stream=None, misalign=0, workspace_check=None):
        """-> ({name: guarded tensor}, tape, what must stay alive).  by_address: K, R, t read from GPU tensors; misalign: the tape's
        storage starts that many floats into its tensor"""
        N, n = self.N, self.size
        out = {nm: _guarded(int(np.prod(_shapes(n)[nm]))) for nm in ALL if nm in want}
        lit = not lightoff and ("rgb" in want or bool(flags & N.TAPE_TEXTURES))
        floats = self.r.tape_floats(self.m, fill_back, lit, flags, "rgb" in want)
        storage = torch.empty((floats + misalign,), dtype=torch.float32, device=GPU) if flags else None
        args, held = self.args(), []
        if self.cam is not None:
            for nm, addr in zip(("K", "R", "t"), by_address):
                if addr:
                    held.append(_gpu(np.asarray(args[nm], np.float32)))
                    args[nm] = held[-1].data_ptr()
        tape = self.r.render_dev(self.m, _stream() if stream is None else stream, self.d_v.data_ptr(), 0 if self.d_tex is None else self.d_tex.data_ptr(),
                                 fill_back=fill_back, lightoff=lightoff, rgb=out["rgb"][1] if "rgb" in out else 0,
                                 depth=out["depth"][1] if "depth" in out else 0, alpha=out["alpha"][1] if "alpha" in out else 0, flags=flags,
                                 storage=0 if storage is None else storage.data_ptr() + 4 * misalign, storage_floats=floats, **args)
        return {nm: t for nm, (t, _) in out.items()}, tape, (storage, held)

    def close(self):
        self.m.close(); self.r.close()


def _holds(t, want, what):
    want = np.ascontiguousarray(want, np.float32).reshape(-1)
    got = t[:want.size].cpu().numpy().view(np.uint32)
    w = want.view(np.uint32)
    assert np.array_equal(got, w), f"{what}: {int((got != w).sum())} of {w.size} words differ from the host route"
    _guard_kept(t, want.size, what)


def _dev_grads(c, tape, g, camera, textures):
    """the device tape's gradients for host cotangents g -> guarded tensors (grad_verts, grad_R, grad_t, grad_textures)"""
    d_g = [None if x is None else _gpu(x) for x in g]
    gv, gR, gt = _guarded(c.v.size), (_guarded(9) if camera else (None, 0)), (_guarded(3) if camera else (None, 0))
    tape.vertex_grad_dev(_stream(), gv[1], *[0 if x is None else x.data_ptr() for x in d_g], gR[1], gt[1])
    gtex = (None, 0)
    if textures and g[0] is not None:
        gtex = _guarded(c.tex.size)
        tape.texture_grad_dev(_stream(), d_g[0].data_ptr(), gtex[1])
    torch.cuda.synchronize()
    return gv[0], gR[0], gt[0], gtex[0]


ATOMIC = {"words": 0, "host_against_itself": 0, "device_against_host": 0, "worst": 0.0}


def _atomic_cubes(c, what, gtex, host, host_again, g_rgb, fill_back, lightoff, faces):
    """grad_textures where a face's pixel box exceeds BF_TEX_GATHER_MAX: bf_nr_backward_large_kernel adds those pixels with float
    atomics on global memory, in no fixed order, so the host route has no single value there - two calls of it differ
    in their last bits - and "the host route's bytes" is not defined for the cubes of `faces`.  Every other cube is held to the host
    route byte for byte, the guard stays whole, and the cubes of `faces` are held - both routes - to the oracle within the texture
    VJP's own bound, (n + 3) 2^-23 S"""
    import nr_oracle as NO
    got = gtex[:c.tex.size].cpu().numpy().view(np.float32).reshape(c.tex.shape)
    rest = np.ones(len(c.f), bool)
    rest[list(faces)] = False
    assert np.array_equal(_bits(got[rest]), _bits(host[rest])), f"{what}: a cube outside the atomic kernel's faces differs from the host route"
    _guard_kept(gtex, c.tex.size, what)
    keep = {}
    NO.render(c.v, c.f, c.tex, c.K, c.cam[0], c.cam[1], c.size, fill_back=fill_back, lightoff=lightoff, light=c.light, keep=keep, **c.cfg)
    ref, n, S = NO.texture_vjp(g_rgb, keep)
    bound = (n + 3) * 2.0 ** -23 * S
    for name, x in (("device", got), ("host", host), ("host again", host_again)):
        err = np.abs(x.astype(np.float64) - ref)
        assert (n[~rest] > 0).any() and (err[~rest] <= bound[~rest]).all(), (what, name, float((err - bound)[~rest].max()))
        assert not x[n == 0].any(), (what, name)
        hit = n[~rest] > 0
        ATOMIC["worst"] = max(ATOMIC["worst"], float((err[~rest][hit] / bound[~rest][hit]).max()))
    ATOMIC["words"] += int(got[~rest].size)
    ATOMIC["host_against_itself"] += int((_bits(host[~rest]) != _bits(host_again[~rest])).sum())
    ATOMIC["device_against_host"] += int((_bits(got[~rest]) != _bits(host[~rest])).sum())


def _compare(c, what, fill_back=True, lightoff=False, want=ALL, which=(ALL,), by_address=(False, False, False), seed=0, misalign=0, atomic_faces=()):
    """one render through both routes with a geometry (+ texture) tape, and the gradients for every cotangent choice of `which`.
    atomic_faces: see _atomic_cubes"""
    N = c.N
    textures = c.tex is not None and "rgb" in want
    flags = N.TAPE_GEOMETRY | (N.TAPE_TEXTURES if textures else 0)
    *h_out, h_tape = c.host(fill_back, lightoff, want, flags)
    before, nr_before = _stats(), _nr_stats()
    d_out, d_tape, keep = c.dev(fill_back, lightoff, want, flags, by_address, misalign=misalign)
    torch.cuda.synchronize()
    after, nr_after = _stats(), _nr_stats()
    assert after["dev_calls"] == before["dev_calls"] + 1 and after["host_calls"] == before["host_calls"], (what, before, after)
    assert nr_after["renders"] == nr_before["renders"] + 1 and nr_after["bytes_back"] == nr_before["bytes_back"] + 4, (what, nr_before, nr_after)
    for nm, h in zip(ALL, h_out):
        assert (h is None) == (nm not in d_out), (what, nm)
        if h is not None:
            _holds(d_out[nm], h, f"{what}: {nm}")
    camera = c.cam is not None
    for k, names in enumerate(which):
        g = _cotangents(c.size, [nm for nm in names if nm in want], seed + k)
        h_gv, h_gR, h_gt = h_tape.vertex_grad(*g, camera=camera)
        gv, gR, gt, gtex = _dev_grads(c, d_tape, g, camera, textures)
        tag = f"{what} cotangents {'+'.join(names)}"
        _holds(gv, h_gv, tag + ": grad_verts")
        if camera:
            _holds(gR, h_gR, tag + ": grad_R")
            _holds(gt, h_gt, tag + ": grad_t")
        if gtex is not None and atomic_faces:
            _atomic_cubes(c, tag + ": grad_textures", gtex, h_tape.texture_grad(g[0]), h_tape.texture_grad(g[0]), g[0], fill_back, lightoff, atomic_faces)
        elif gtex is not None:
            _holds(gtex, h_tape.texture_grad(g[0]), tag + ": grad_textures")
    h_tape.close(); d_tape.close()
    del keep


def _valence70(ts=2):
    from test_gpu_nr import _distinct
    ang = np.linspace(0, 2 * np.pi, 71)[:-1]
    ring = np.stack([0.7 * np.cos(ang), 0.7 * np.sin(ang), 2.0 + 0.2 * np.sin(3 * ang)], 1)
    v = np.concatenate([[[0.03, -0.02, 1.7]], ring]).astype(np.float32)
    f = np.array([[0, 1 + i, 1 + (i + 1) % 70] for i in range(70)], np.int32)
    return v, f, _distinct(70, ts, seed=6)


def same_bits(out_path):
    """rgb, depth, alpha, grad_textures, grad_verts, grad_R, grad_t of the *_dev entries against the host entries, byte for byte"""
    def body():
        N, _ = _start()
        from test_gpu_nr import AMBIENT_ONLY, EYE, _big_face, _fan, _hemisphere, _sphere, _triangle, _views
        each = (("rgb",), ("depth",), ("alpha",), ALL)
        n = 0
        for shift in (0.0, 0.9):                                     # one triangle at 8 without anti-aliasing, also partly outside
            c = Case(N, _triangle(4), 8, False, (EYE[0], np.array([shift, 0.3 * shift, 0], np.float32)))
            for fill_back, lightoff in itertools.product((True, False), (False, True)):
                _compare(c, f"triangle shift {shift} fill_back {fill_back} lightoff {lightoff}", fill_back, lightoff, which=each); n += 1
            c.close()
        for nf in (33, 70):                                          # the fans at 20 (70: across the 64-record LDS stage), ts 2
            c = Case(N, _fan(nf, ts=2), 20, True, EYE)
            _compare(c, f"fan{nf} lit", True, False); n += 1
            _compare(c, f"fan{nf} lightoff front", False, True); n += 1
            c.close()
        v, f, tex, views, far = _hemisphere(4)                       # the open shell seen from inside
        c = Case(N, (v, f, tex), 20, True, (views[0][:3, :3].astype(np.float32), views[0][:3, 3].astype(np.float32)), 0.0, far)
        _compare(c, "open shell from inside", True, False); n += 1
        _compare(c, "open shell from inside, nothing drawn", False, False); n += 1
        c.close()
        c = Case(N, _big_face(3), 40, True, EYE)                     # a box above 4,096 pixels: the large backward kernel, the multi-stride gather
        _compare(c, "big face lit", True, False, which=each, atomic_faces=(0,)); n += 1
        _compare(c, "big face lightoff", True, True, atomic_faces=(0,)); n += 1
        c.close()
        c = Case(N, _valence70(2), 20, True, EYE)
        _compare(c, "valence 70", True, False); n += 1
        c.close()
        mesh = _sphere(4, degenerate=True)
        vw, far = _views(mesh[0])
        cam = (vw[3][:3, :3].astype(np.float32), vw[3][:3, 3].astype(np.float32))
        c = Case(N, mesh, 20, True, cam, 0.0, far)
        _compare(c, "degenerate face", True, False); n += 1
        for want in (("alpha",), ("depth",), ("rgb",)):              # single-output renders
            _compare(c, f"only {want[0]}", True, "rgb" not in want, want=want, which=(want,)); n += 1
        for by in itertools.product((False, True), repeat=3):        # K, R, t each by value or by address: the same bits
            _compare(c, f"camera by address {by}", True, False, by_address=by); n += 1
        c.close()
        c = Case(N, _sphere(2), 20, True, cam, 0.0, far, light=AMBIENT_ONLY)      # ts 2, no directional term: no unlit samples kept
        _compare(c, "sphere ts 2 ambient only", True, False); n += 1
        c.close()
        tri = _triangle(2)
        c = Case(N, (tri[0], tri[1], None), 20, True, None)          # ndc, a mesh without textures
        _compare(c, "ndc silhouette and depth", True, True, want=("depth", "alpha"), which=(("depth", "alpha"), ("alpha",))); n += 1
        c.close()
        print(f"cubes of the atomic kernel: {ATOMIC}")
        return {"cases": np.int64(n), **{"atomic_" + k: np.float64(v) for k, v in ATOMIC.items()}}
    _run(out_path, body)


def _batch_scene(nr, where, grad, shared_camera, seed=0):
    from test_gpu_nr import LIGHT, _K, _sphere, _views
    v, f, tex = _sphere(2)
    vw, far = _views(v)
    r = nr.Renderer(image_size=20, K=_K(20)[None], orig_size=20, near=0.0, far=float(far), background_color=[0.1, 0.2, 0.3],
                    light_intensity_ambient=LIGHT["ambient"], light_intensity_directional=LIGHT["directional"],
                    light_color_ambient=LIGHT["color_ambient"], light_color_directional=LIGHT["color_directional"],
                    light_direction=LIGHT["direction"])
    r.geometry_grad = True
    t_ = lambda a, g=False: torch.tensor(np.ascontiguousarray(a), device=where, requires_grad=g)      # noqa: E731
    rng = np.random.default_rng(seed)
    vv = np.stack([v, v + rng.normal(0, 0.01, v.shape).astype(np.float32)])
    ids = (3,) if shared_camera else (3, 8)
    R = np.stack([vw[i][:3, :3] for i in ids]).astype(np.float32)
    t = np.stack([vw[i][:3, 3] for i in ids]).astype(np.float32)
    x = dict(v=t_(vv, grad), f=t_(np.stack([f, f])), tex=t_(np.stack([tex, tex[::-1].copy()]), grad), R=t_(R, grad), t=t_(t, grad))
    return r, x


def batches_and_graphs(out_path):
    """the drop-in with geometry_grad on: a [1,3,3] camera shared by B = 2 and a [2,3,3] one; two taped renders of one mesh from two
    views kept in one graph and one backward.  GPU tensors against CPU tensors (the host route), bit for bit"""
    def body():
        N, nr = _start()
        res = {}
        for shared in (True, False):
            got = {}
            for where in ("cpu", GPU):
                r, x = _batch_scene(nr, where, True, shared)
                before = _stats()
                out = r.render(x["v"], x["f"], x["tex"], R=x["R"], t=x["t"])
                g = [torch.tensor(c, device=where) for c in (np.random.default_rng(5).standard_normal(o.shape).astype(np.float32) for o in out)]
                sum((o * c).sum() for o, c in zip(out, g)).backward()
                after = _stats()
                if where == GPU:
                    assert after["host_calls"] == before["host_calls"] and after["dev_calls"] == before["dev_calls"] + 6, (before, after)
                    assert all(o.device.type == "cuda" for o in out)
                else:
                    assert after["dev_calls"] == before["dev_calls"]
                got[where] = [o.detach().cpu().numpy() for o in out] + [x[k].grad.cpu().numpy() for k in ("v", "tex", "R", "t")]
                r.close()
            for k, (a, b) in enumerate(zip(got[GPU], got["cpu"])):
                _same(a, b, f"shared camera {shared}: result {k}")
            assert got[GPU][5].shape == ((1, 3, 3) if shared else (2, 3, 3))
            res[f"gR_{int(shared)}"] = got[GPU][5]
        # two renders of one mesh from two views in one graph, one backward
        got = {}
        for where in ("cpu", GPU):
            r, x = _batch_scene(nr, where, False, False)
            v = x["v"][:1].clone().requires_grad_(True)
            tex = x["tex"][:1].clone().requires_grad_(True)
            a = r.render(v, x["f"][:1], tex, R=x["R"][:1], t=x["t"][:1])
            b = r.render(v, x["f"][:1], tex, R=x["R"][1:], t=x["t"][1:])
            loss = sum((o * o).sum() for o in a) + sum((o * 0.5).sum() for o in b)
            loss.backward()
            got[where] = [v.grad.cpu().numpy(), tex.grad.cpu().numpy()]
            try:
                loss.backward()
            except RuntimeError:
                pass
            else:
                raise AssertionError("a second backward went through")
            r.close()
        _same(got[GPU][0], got["cpu"][0], "two tapes, one graph: grad_verts")
        _same(got[GPU][1], got["cpu"][1], "two tapes, one graph: grad_textures")
        return res
    _run(out_path, body)


def _padded(mesh, nv):
    """`mesh` with unreferenced vertices behind it up to nv"""
    v, f, tex = mesh
    extra = np.random.default_rng(nv).uniform(-1, 1, (nv - len(v), 3)).astype(np.float32) + np.array([0, 0, 3], np.float32)
    return np.concatenate([v, extra]).astype(np.float32), f, tex


def view_kernels_alone(out_path):
    """bf_tex_project_view_kernel and bf_nr_fold_view_kernel against their by-value forms at 1, 255, 256 and 257 vertices, valence 1
    (a triangle soup) and 70, with the TexView at a 4-byte-aligned address that is not 16-byte-aligned inside a larger tensor: every
    output of the render and of the fold downstream of them, byte for byte"""
    def body():
        N, _ = _start()
        from test_gpu_nr import EYE, _distinct
        n = 0
        cam = (EYE[0], np.array([0.05, -0.02, 0.1], np.float32))
        one = (np.array([[0.1, 0.2, 2.0]], np.float32), np.array([[0, 0, 0]], np.int32), _distinct(1, 2, seed=1))
        c = Case(N, one, 8, False, cam)
        for misalign in (1, 3):
            _compare(c, f"one vertex, view at +{4 * misalign} bytes", True, False, misalign=misalign, by_address=(False, True, True)); n += 1
        c.close()
        for nv in (255, 256, 257):
            rng = np.random.default_rng(nv)
            k = nv // 3
            base = np.array([[-0.5, -0.5, 0.0], [0.5, -0.5, 0.0], [0.0, 0.5, 0.0]]) * 0.3
            soup_v = (base[None] + np.c_[rng.uniform(-0.6, 0.6, (k, 2)), 2.0 + 0.4 * rng.uniform(size=k)][:, None, :]).reshape(-1, 3)
            soup = (soup_v.astype(np.float32), np.arange(3 * k, dtype=np.int32).reshape(-1, 3), _distinct(k, 2, seed=nv))
            for name, mesh in (("valence 1", _padded(soup, nv)), ("valence 70", _padded(_valence70(2), nv))):
                assert len(mesh[0]) == nv
                c = Case(N, mesh, 20, True, cam)
                for misalign in (1, 2):
                    assert (4 * misalign) % 16 != 0
                    _compare(c, f"{name}, {nv} vertices, view at +{4 * misalign} bytes", True, False, misalign=misalign,
                             by_address=(bool(misalign & 1), True, True)); n += 1
                c.close()
        return {"cases": np.int64(n)}
    _run(out_path, body)


def oracle_independent(out_path):
    """independent of the host route: a lit fill-back case and a lightoff front-only case against tests/nr_oracle.py (renders bit for
    bit, the texture VJP within (n + 3) 2^-23 S with zeros where the oracle has no term) and tests/nr_vertex_oracle.py (grad_verts
    within (n + 72) 2^-23 S): the bounds of tests/test_gpu_nr.py and tests/test_gpu_nr_vertex.py"""
    def body():
        N, _ = _start()
        import nr_oracle as NO
        import nr_vertex_oracle as VO
        from test_gpu_nr import LIGHT, _sphere, _views
        EPS32 = 2.0 ** -23
        mesh = _sphere(4)
        vw, far = _views(mesh[0])
        cam = (vw[7][:3, :3].astype(np.float32), vw[7][:3, 3].astype(np.float32))
        worst = {}
        for name, fill_back, lightoff in (("lit_fill_back", True, False), ("lightoff_front", False, True)):
            c = Case(N, mesh, 20, True, cam, 0.0, far)
            out, tape, keep_alive = c.dev(fill_back, lightoff, ALL, N.TAPE_GEOMETRY | N.TAPE_TEXTURES, by_address=(False, True, True))
            cfg = dict(image_size=20, anti_aliasing=True, near=np.float32(0.0), far=np.float32(far), background=(0.1, 0.2, 0.3))
            keep = {}
            want = NO.render(c.v, c.f, c.tex, c.K, cam[0], cam[1], 20, fill_back=fill_back, lightoff=lightoff, light=LIGHT, keep=keep, **cfg)
            torch.cuda.synchronize()
            for nm, w in zip(ALL, want):
                _holds(out[nm], w, f"{name}: {nm} against the oracle")
            g = _cotangents(20, ALL, 11)
            gv, gR, gt, gtex = _dev_grads(c, tape, g, True, True)
            got = gtex[:c.tex.size].cpu().numpy().view(np.float32).reshape(c.tex.shape)
            ref, n, S = NO.texture_vjp(g[0], keep)
            err = np.abs(got.astype(np.float64) - ref)
            bound = (n + 3) * EPS32 * S
            print(f"{name}: texture VJP, largest err / bound {float((err[n > 0] / bound[n > 0]).max()):.3f}")
            assert (n > 0).any() and (err <= bound).all(), (name, float((err - bound).max()))
            assert not got[n == 0].any(), name
            *_, vkeep = VO.render(c.v, c.f, c.tex, K=c.K, R=cam[0], t=cam[1], orig_size=20, fill_back=fill_back, lightoff=lightoff, light=LIGHT, **cfg)
            vref = VO.vertex_vjp(vkeep, *g)
            for what, t_, (grad, nn, SS) in (("verts", gv, vref["verts"]), ("R", gR, vref["R"]), ("t", gt, vref["t"])):
                x = t_[:grad.size].cpu().numpy().view(np.float32).reshape(grad.shape)
                bound = (nn + 72) * EPS32 * SS
                err = np.abs(x.astype(np.float64) - grad)
                hit = SS > 0
                worst[f"{name}_{what}"] = float((err[hit] / bound[hit]).max())
                print(f"{name}: grad_{what}, largest err / bound {worst[f'{name}_{what}']:.3f}")
                assert hit.any() and (err <= bound).all(), (name, what, float((err - bound).max()))
                assert not x[~hit].any(), (name, what)
            tape.close(); c.close()
            del keep_alive
        return {k: np.float64(v) for k, v in worst.items()}
    _run(out_path, body)


def _quads():
    """tests/test_gpu_nr.py's overflowing render: 24 faces over all 64 tiles of a 64 x 64 image, 1,536 entries against 1,184"""
    from test_gpu_nr import _distinct
    quads_v, quads_f = [], []
    for q in range(12):
        z = 2.0 + 0.25 * q
        s = 1.5 * z
        quads_v.append(np.array([[-s, -s, z], [s, -s, z], [s, s, z], [-s, s, z]], np.float32))
        quads_f += [[4 * q, 4 * q + 1, 4 * q + 2], [4 * q, 4 * q + 2, 4 * q + 3]]
    v, f = np.concatenate(quads_v), np.asarray(quads_f, np.int32)
    return v, f, _distinct(len(f), 2, seed=8)


def tile_lists(out_path):
    """the render that overflows its first tile lists: one growth, no repeated render, the host route's bits; a smaller render behind
    it on the same renderer gives a fresh renderer's bits; 4 bytes read back per render and nothing else"""
    def body():
        N, _ = _start()
        from test_gpu_nr import EYE, _triangle
        flags = N.TAPE_GEOMETRY | N.TAPE_TEXTURES
        yard = Case(N, _quads(), 64, False, EYE, 0.0, 10.0)
        *want, h_tape = yard.host(True, False, ALL, flags)
        c = Case(N, _quads(), 64, False, EYE, 0.0, 10.0)             # a renderer and mesh whose lists have their first size
        s0, n0 = _stats(), _nr_stats()
        out, tape, keep = c.dev(True, False, ALL, flags)
        torch.cuda.synchronize()
        s1, n1 = _stats(), _nr_stats()
        assert n1["growths"] == n0["growths"] + 1 and n1["renders"] == n0["renders"] + 1 and n1["bytes_back"] == n0["bytes_back"] + 4, (n0, n1)
        assert s1["dev_calls"] == s0["dev_calls"] + 1 and s1["host_calls"] == s0["host_calls"]
        for nm, w in zip(ALL, want):
            _holds(out[nm], w, f"overflowing render: {nm}")
        g = _cotangents(64, ALL, 3)
        gv, gR, gt, gtex = _dev_grads(c, tape, g, True, True)
        h = h_tape.vertex_grad(*g)
        _holds(gv, h[0], "overflowing render: grad_verts"); _holds(gR, h[1], "overflowing render: grad_R"); _holds(gt, h[2], "overflowing render: grad_t")
        _holds(gtex, h_tape.texture_grad(g[0]), "overflowing render: grad_textures")
        out2, _, _ = c.dev(True, False, ALL, 0)                      # again with the grown lists: no growth
        torch.cuda.synchronize()
        n2 = _nr_stats()
        assert n2["growths"] == n1["growths"] and n2["bytes_back"] == n1["bytes_back"] + 4
        for nm, w in zip(ALL, want):
            _holds(out2[nm], w, f"overflowing render again: {nm}")
        # a smaller render behind it on the same renderer (another mesh) against a fresh renderer
        small = _triangle(2)
        m = N.NrMesh(c.r, *small[:2], 2, small[2])
        c.m, c.v, c.f, c.tex, c.d_v, c.d_tex, old = m, small[0], small[1], small[2], _gpu(small[0]), _gpu(small[2]), c.m
        out3, _, _ = c.dev(True, False, ALL, 0)
        fresh = Case(N, small, 64, False, EYE, 0.0, 10.0)
        ref, _, _ = fresh.dev(True, False, ALL, 0)
        torch.cuda.synchronize()
        for nm in ALL:
            _same(out3[nm], ref[nm], f"a small render behind the large one: {nm}")
        old.close(); tape.close(); h_tape.close(); fresh.close(); c.close(); yard.close()
        del keep
        return {"growths": np.int64(n2["growths"] - n0["growths"])}
    _run(out_path, body)


def outputs_workspace_streams(out_path):
    """guards (every _holds checks 64 words behind its output), a second identical call that allocates nothing and switches no
    stream, the same call under torch.cuda.stream(s), host / device / host on one renderer, and the new refusals' codes - all but
    "a workspace on another device", which one GPU cannot show (bf_ml_dev_check's comparison, shared with every other *_dev entry)"""
    def body():
        N, _ = _start()
        import ctypes as C
        from bodyfitting_amd import _lib
        from test_gpu_nr import _sphere, _views
        assert GUARD == 64
        mesh = _sphere(2)
        vw, far = _views(mesh[0])
        cam = (vw[5][:3, :3].astype(np.float32), vw[5][:3, 3].astype(np.float32))
        c = Case(N, mesh, 20, True, cam, 0.0, far)
        flags = N.TAPE_GEOMETRY | N.TAPE_TEXTURES
        g = _cotangents(20, ALL, 4)

        def host():
            *out, tape = c.host(True, False, ALL, flags)
            res = list(out) + list(tape.vertex_grad(*g)) + [tape.texture_grad(g[0])]
            tape.close()
            return res

        def dev(stream=None):
            out, tape, keep = c.dev(True, False, ALL, flags, by_address=(False, True, True), stream=stream)
            res = [out[nm] for nm in ALL] + list(_dev_grads(c, tape, g, True, True))
            tape.close()
            return res

        def check(res, want, what):
            for k, (a, b) in enumerate(zip(res, want)):
                _holds(a, b, f"{what}: result {k}")

        want = host()
        check(dev(), want, "first call")
        start = _stats()
        check(dev(), want, "second call")
        mid = _stats()
        check(dev(), want, "third call")
        end = _stats()
        assert end["allocations"] == mid["allocations"] == start["allocations"], (start, mid, end)
        assert end["stream_switches"] == start["stream_switches"] and end["host_calls"] == start["host_calls"], (start, end)
        assert end["dev_calls"] == start["dev_calls"] + 6
        # host, device, host on one renderer: each its route's usual bits
        for k in range(2):
            again = host()
            for a, b in zip(again, want):
                _same(a, b, f"host route behind the device route, round {k}")
            check(dev(), want, f"device route behind the host route, round {k}")
        # another stream: ordered behind the workspace's previous call, the same bits
        s = torch.cuda.Stream()
        before = _stats()
        with torch.cuda.stream(s):
            res = dev(stream=s.cuda_stream)
        s.synchronize()
        check(res, want, "under torch.cuda.stream(s)")
        assert _stats()["stream_switches"] > before["stream_switches"]
        check(dev(), want, "back on the current stream")
        # refusals: before anything is queued or counted
        lib = _lib.load()
        ws, stream = c.r.workspace(), _stream()
        out = torch.empty((3 * 20 * 20,), device=GPU)
        storage = torch.empty((c.r.tape_floats(c.m, True, True, flags, True),), device=GPU)
        K, R, t = (np.ascontiguousarray(a, np.float32) for a in (c.K, cam[0], cam[1]))
        h = C.c_void_p()

        def render(verts=c.d_v.data_ptr(), wsh=ws._h, store=storage.data_ptr(), floats=storage.numel(), tape=True, cam_dev=None, Kp=K):
            return lib.bf_nr_render_dev(c.r._h, c.m._h, _lib.fptr(Kp), _lib.fptr(R), _lib.fptr(t), 20.0, 1, 0, 0, out.data_ptr(), None, None, flags if tape else 0,
                                        C.byref(h) if tape else None, verts, c.d_tex.data_ptr(), C.byref(cam_dev) if cam_dev is not None else None,
                                        store, floats, wsh, stream)

        before, nr_before = _stats(), _nr_stats()
        assert render(wsh=None) == INVALID                            # no workspace
        assert render(verts=None) == INVALID                          # a null vertex pointer
        assert render(store=None) == INVALID                          # a tape without storage
        assert render(floats=storage.numel() - 1) == INVALID          # ... or with too little
        assert render(Kp=None) == INVALID                             # the host twin's: no K at all
        assert render(cam_dev=_lib.NrCameraDev(c.d_v.data_ptr(), None, None)) == INVALID       # K both ways
        assert lib.bf_nr_tape_texture_grad_dev(None, out.data_ptr(), out.data_ptr(), ws._h, stream) == INVALID
        assert lib.bf_nr_tape_vertex_grad_dev(None, None, None, None, out.data_ptr(), None, None, ws._h, stream) == INVALID
        assert render() == 0                                          # (and the call itself goes through)
        tape = N.NrTape(h, c.m.textures_shape, c.m.n_verts, 20, workspace=ws)
        assert lib.bf_nr_tape_texture_grad_dev(tape._h, out.data_ptr(), c.d_tex.data_ptr(), None, stream) == INVALID
        assert lib.bf_nr_tape_vertex_grad_dev(tape._h, None, None, None, None, None, None, ws._h, stream) == INVALID
        gh = np.zeros((3, 20, 20), np.float32)
        assert lib.bf_nr_tape_texture_grad(tape._h, _lib.fptr(gh), _lib.fptr(np.zeros(c.tex.shape, np.float32))) == INVALID    # a device tape on the host entry
        *_, h_tape = c.host(True, False, ALL, flags)
        assert lib.bf_nr_tape_texture_grad_dev(h_tape._h, out.data_ptr(), c.d_tex.data_ptr(), ws._h, stream) == INVALID        # ... and the reverse
        torch.cuda.synchronize()
        after, nr_after = _stats(), _nr_stats()
        assert after["dev_calls"] == before["dev_calls"] + 1 and nr_after["renders"] == nr_before["renders"] + 1, (before, after)
        assert torch.cuda.current_device() == 0
        tape.close(); h_tape.close(); c.close()
        return {"ok": np.int64(1)}
    _run(out_path, body)


def texture_loop(out_path, switched_off):
    """eight iterations of texture_fitting.py:257-276 as written on the small sphere pair of tests/test_gpu_nr.py's loop test,
    everything on cuda:0: K numpy in the constructor, fresh cuda R / t each step"""
    def body():
        N, nr = _start("0" if switched_off else "1")
        from bodyfitting_amd import texture_fitting as TF
        from test_gpu_nr import _K
        from texfit_cases import blob_pair
        IS = 32
        scan, fit = blob_pair(level=2, ts=4)
        center, dist = TF.scene_bound(scan[0])
        views = TF.gen_cam_views(center, 18, dist, gl=True)
        K = _K(IS).reshape(1, 3, 3)
        renderer = nr.Renderer(image_size=IS, fill_back=False, camera_mode='projection', orig_size=IS, light_intensity_ambient=1.0,
                               light_intensity_directional=0, near=0, far=2 * dist, background_color=[1, 1, 1], K=K)
        to = lambda a: torch.from_numpy(np.array(a)).to(GPU)[None]      # noqa: E731
        scan_v, scan_f, scan_t = to(scan[0]), to(scan[1]), to(scan[2])
        smpl_v, smpl_f, smpl_t = to(fit[0]), to(fit[1]), to(fit[2])
        smpl_t.requires_grad = True
        optimizer = torch.optim.Adam([smpl_t], lr=1e-2)
        losses, per_step = [], []
        for i in range(8):
            pose = views[(i * 5) % len(views)]
            t = pose[:3, 3].reshape([1, 1, 3])
            R = pose[:3, :3].reshape([1, 3, 3])
            R, t = torch.cuda.FloatTensor(R), torch.cuda.FloatTensor(t)
            s0, n0 = _stats(), _nr_stats()
            scan_img = renderer.render_rgb(scan_v, scan_f, scan_t, R=R, t=t)
            smpl_img = renderer.render_rgb(smpl_v, smpl_f, smpl_t, R=R, t=t)
            loss = torch.sum(torch.abs(scan_img - smpl_img))
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            s1, n1 = _stats(), _nr_stats()
            losses.append(loss.detach())
            per_step.append(({k: s1[k] - s0[k] for k in s0}, {k: n1[k] - n0[k] for k in n0}))
        for i, (s, n) in enumerate(per_step):
            if switched_off:
                assert s["dev_calls"] == 0 and s["host_calls"] == 3 and n["renders"] == 0, (i, s, n)
                continue
            assert s["host_calls"] == 0 and s["dev_calls"] == 3, (i, s)
            assert n["renders"] == 2 and n["bytes_back"] == 8, (i, n)
            assert s["stream_switches"] == 0, (i, s)
            if i > 0:
                assert s["allocations"] == 0 and n["growths"] == 0, (i, s, n)
        assert len(renderer._meshes) == 2
        out = {"losses": torch.stack(losses).cpu().numpy(), "texels": smpl_t.detach().cpu().numpy()}
        assert out["losses"][-1] < out["losses"][0]
        renderer.close()
        return out
    _run(out_path, body)


def vertex_loop(out_path, switched_off):
    """geometry_grad on: five Adam steps of a sphere toward a shifted silhouette, vertices, R and t on the GPU"""
    def body():
        N, nr = _start("0" if switched_off else "1")
        from test_gpu_nr import _K, _sphere, _views
        v, f, _ = _sphere(2)
        vw, far = _views(v)
        size = 32
        r = nr.Renderer(image_size=size, K=_K(size)[None], orig_size=size, near=0.0, far=float(far))
        r.geometry_grad = True
        R = torch.tensor(vw[4][:3, :3].astype(np.float32), device=GPU)[None]
        t = torch.tensor(vw[4][:3, 3].astype(np.float32), device=GPU)[None]
        faces = torch.tensor(f, device=GPU)[None]
        with torch.no_grad():
            target = r.render_silhouettes(torch.tensor(v + np.array([0.08, -0.05, 0.0], np.float32), device=GPU)[None], faces, R=R, t=t)
        sets = {"n": 0}
        real = N.NrMesh.set_vertices
        N.NrMesh.set_vertices = lambda self, verts: (sets.__setitem__("n", sets["n"] + 1), real(self, verts))[1]
        vv = torch.tensor(v, device=GPU)[None].requires_grad_(True)
        opt = torch.optim.Adam([vv], lr=5e-3)
        losses = []
        s0 = _stats()
        for i in range(5):
            opt.zero_grad()
            loss = ((r.render_silhouettes(vv, faces, R=R, t=t) - target) ** 2).sum()
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        s1 = _stats()
        if not switched_off:
            assert s1["host_calls"] == s0["host_calls"] and s1["dev_calls"] == s0["dev_calls"] + 10 and sets["n"] == 0, (s0, s1, sets)
        else:
            assert s1["dev_calls"] == s0["dev_calls"] and s1["host_calls"] == s0["host_calls"] + 10
        out = {"losses": torch.stack(losses).cpu().numpy(), "verts": vv.detach().cpu().numpy()}
        assert np.abs(out["verts"][0] - v).max() > 1e-3
        r.close()
        return out
    _run(out_path, body)
