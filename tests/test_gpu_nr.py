"""The stand-alone neural_renderer.Renderer on the GPU (bf_nr_*, native.Nr*, bodyfitting_amd/neural_renderer.py) against
tests/nr_oracle.py - oracle/texfit_oracle.py's rasteriser plus lighting, the concatenated fill-back form, alpha and a float64
texture VJP.  Renders are compared bit for bit (the kernels keep the reference's float32 operation order); the texture gradient is
a float32 sum in any order and is held elementwise to (n + 3) * 2^-23 * S: n terms of magnitudes summing to S, three roundings
per term.

Sizes: output 8 without anti-aliasing (one 8 x 8 tile), 20 and 32 with (40 and 64 super-sampled pixels: partial and whole tiles).
Two cases need more than these sizes can give and say so where they are built: a record's pixel box exceeds
BF_TEX_GATHER_MAX = 4096 pixels only above 64 super-sampled pixels a side (output 40 with anti-aliasing), and back-face culling
drops one record of every face before the tile lists, so the 33-face fan lists 33 records with fill-back, not 66 - a 70-face fan
beside it is what crosses the 64-record LDS stage."""
import os

import numpy as np
import pytest

from bodyfitting_amd import _lib, native
from bodyfitting_amd import texture_fitting as TF
from oracle import texfit_oracle as TO
from texfit_cases import blob_pair, icosphere, uv_atlas
import nr_oracle as NO

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
LIGHT = dict(ambient=0.3, directional=0.8, color_ambient=(1.0, 0.9, 0.7), color_directional=(0.6, 1.0, 0.8), direction=(0.3, 0.8, -0.5))
AMBIENT_ONLY = dict(ambient=1.0, directional=0.0, color_ambient=(1, 1, 1), color_directional=(1, 1, 1), direction=(0, 1, 0))
SIZES = [(8, False), (20, True), (32, True)]


def _K(n):
    return np.array([[n, 0, n // 2], [0, n, n // 2], [0, 0, 1]], np.float32)


def _distinct(nf, ts, seed=0):
    """every texel of every cube distinct (an axis exchange that is left out, or done twice, shows)"""
    rng = np.random.default_rng(seed)
    n = nf * ts ** 3 * 3
    return (rng.permutation(n).astype(np.float32) / np.float32(n)).reshape(nf, ts, ts, ts, 3)


def _sphere(ts=4, degenerate=False):
    scan, _ = blob_pair(level=2, ts=ts)
    v, f = scan[0], scan[1]
    if degenerate:                                                    # two corners on one vertex: |n| = 0, never drawn
        f = np.concatenate([f, np.array([[5, 5, 40]], np.int32)])
    return v, f, _distinct(len(f), ts)


def _views(v):
    center, dist = TF.scene_bound(v)
    return TF.gen_cam_views(center, 18, dist, gl=True), np.float32(2 * dist)


def _hemisphere(ts=4):
    """the half of the blob that lies AWAY from view 0: view 0 looks into the open shell (only back records can be drawn), view 9
    sees the same faces from outside"""
    v, f, _ = _sphere(ts)
    views, far = _views(v)
    p = views[0]
    zc = (v[f].mean(1) @ p[:3, :3].T + p[:3, 3])[:, 2]
    f = np.ascontiguousarray(f[zc > np.median(zc)])
    return v, f, _distinct(len(f), ts, seed=3), views, far


def _triangle(ts=4):
    v = np.array([[-0.6, -0.5, 2.0], [0.7, -0.4, 2.2], [0.1, 0.8, 1.9]], np.float32)
    return v, np.array([[0, 1, 2]], np.int32), _distinct(1, ts, seed=1)


def _fan(n, ts=2):
    """n triangles over (nearly) the same pixel box, alternately wound, their corners at random depths so that they cut through one
    another and many of them own pixels"""
    rng = np.random.default_rng(n)
    v, f = [], []
    for i in range(n):
        tri = np.array([[-0.5, -0.5, 2.0], [0.5, -0.5, 2.0], [0.0, 0.5, 2.0]]) + np.c_[0.01 * rng.standard_normal((3, 2)), 0.4 * rng.uniform(size=3)]
        f.append([3 * i, 3 * i + 1, 3 * i + 2] if i % 2 else [3 * i, 3 * i + 2, 3 * i + 1])
        v.append(tri)
    return np.concatenate(v).astype(np.float32), np.asarray(f, np.int32), _distinct(n, ts, seed=2)


def _big_face(ts=3):
    """one face over most of the image in front of a small sphere"""
    sv, sf = icosphere(1)
    v = np.concatenate([np.array([[-0.95, -0.9, 2.0], [0.95, -0.9, 2.0], [0.0, 0.95, 2.0]], np.float32),
                        sv * 0.3 + np.array([0, 0, 1.5], np.float32)]).astype(np.float32)
    f = np.concatenate([np.array([[0, 1, 2]], np.int32), sf + 3])
    return v, f, _distinct(len(f), ts, seed=4)


EYE = (np.eye(3, dtype=np.float32), np.zeros(3, np.float32))


class Scene:
    """a native renderer + mesh and the matching oracle call"""

    def __init__(self, mesh, size, aa, near, far, background=(0.1, 0.2, 0.3), light=None):
        self.v, self.f, self.tex = mesh
        self.cfg = dict(image_size=size, anti_aliasing=aa, near=np.float32(near), far=np.float32(far), background=background)
        self.light = light or NO.DEFAULT_LIGHT
        self.r = native.NrRenderer(size, aa, near, far, background)
        self.r.set_light(**self.light)
        self.m = native.NrMesh(self.r, self.v, self.f, self.tex.shape[1], self.tex)
        self.K = _K(size)

    def both(self, R, t, fill_back, lightoff=False, tape=False):
        size = self.cfg["image_size"]
        got = self.r.render(self.m, self.K, R, t, size, fill_back=fill_back, lightoff=lightoff, tape=tape)
        keep = {}
        want = NO.render(self.v, self.f, self.tex, self.K, R, t, size, fill_back=fill_back, lightoff=lightoff, light=self.light, keep=keep, **self.cfg)
        return got, want, keep

    def close(self):
        self.m.close(); self.r.close()


def _assert_same(got, want, what=""):
    for name, g, w in zip(("rgb", "depth", "alpha"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {name}")


def _check_vjp(tape, keep, seed=0):
    size = keep["image_size"]
    g = np.random.default_rng(seed).standard_normal((3, size, size)).astype(np.float32)          # normally distributed, not a sign image
    got = tape.texture_grad(g)
    want, n, S = NO.texture_vjp(g, keep)
    bound = (n + 3) * EPS32 * S
    err = np.abs(got.astype(np.float64) - want)
    print(f"vjp: {int((n > 0).sum())} texel values hit, largest n {int(n.max())}, largest err / bound {float((err[n > 0] / bound[n > 0]).max()) if (n > 0).any() else 0:.3f}")
    assert (n > 0).any()
    assert (err <= bound).all(), float((err - bound).max())
    assert not got[n == 0].any()                                      # zeros exactly where the oracle has no contribution
    return got, n


# ---- 1: the unlit, front-only render is the fused path's and the texfit oracle's ---------------------------------------------------

@pytest.mark.parametrize("size,aa", SIZES)
def test_ambient_front_only_render_is_the_texfit_render(size, aa):
    v, f, tex = _sphere()
    views, far = _views(v)
    s = Scene((v, f, tex), size, aa, 0.0, far, background=(1.0, 1.0, 1.0), light=AMBIENT_ONLY)
    old = TF.Renderer(size, 4, near=0.0, far=far, anti_aliasing=aa)
    old.set_mesh(old.TARGET, (v, f, tex))
    for vi in (0, 7):
        p = views[vi]
        rgb, depth, _, _ = s.r.render(s.m, s.K, p[:3, :3], p[:3, 3], size, fill_back=False)
        o_rgb, o_depth = old.render_rgbd(old.TARGET, p)
        np.testing.assert_array_equal(rgb, o_rgb)
        np.testing.assert_array_equal(depth, o_depth)
        np.testing.assert_array_equal(rgb, old.render_rgb(old.TARGET, p))
        np.testing.assert_array_equal(rgb, TO.render(v, f, tex, s.K, p[:3, :3], p[:3, 3], size, size, 0.0, far, anti_aliasing=aa))
        assert (rgb < 1).any()
    old.close(); s.close()


# ---- 2: directional light ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size,aa", SIZES)
def test_lit_render_is_the_oracle_bit_for_bit(size, aa):
    v, f, tex = _sphere(degenerate=True)
    views, far = _views(v)
    s = Scene((v, f, tex), size, aa, 0.0, far, light=LIGHT)
    rows = NO.light_rows(v[f.astype(np.int64)], **LIGHT)
    cos_zero = np.all(rows == rows[-1], 1)                             # the ambient term alone: cos clamped at 0 (or the degenerate face)
    assert 10 < cos_zero.sum() < len(f) - 10
    np.testing.assert_array_equal(rows[-1], (np.float32(0.3) * np.asarray(LIGHT["color_ambient"], np.float32)))
    drawn = set()
    for vi, lightoff in ((0, False), (0, True), (7, False), (13, False)):
        p = views[vi]
        got, want, keep = s.both(p[:3, :3], p[:3, 3], fill_back=False, lightoff=lightoff)
        _assert_same(got, want, f"view {vi} lightoff {lightoff}")
        drawn |= set(np.unique(keep["face_index"][keep["face_index"] >= 0]).tolist())
    drawn = np.array(sorted(drawn))
    assert cos_zero[drawn].any() and (~cos_zero[drawn]).any()               # faces with and without directional light are in the pictures
    a = s.r.render(s.m, s.K, views[0][:3, :3], views[0][:3, 3], size, fill_back=False)[0]
    b = s.r.render(s.m, s.K, views[0][:3, :3], views[0][:3, 3], size, fill_back=False, lightoff=True)[0]
    assert (a != b).any()
    s.close()


# ---- 3: fill-back ------------------------------------------------------------------------------------------------------------------

def _fill_back_case(name):
    if name == "sphere":
        v, f, tex = _sphere()
        views, far = _views(v)
        return (v, f, tex), [(views[3][:3, :3], views[3][:3, 3])], far, None
    if name == "hemisphere":
        v, f, tex, views, far = _hemisphere()
        return (v, f, tex), [(views[0][:3, :3], views[0][:3, 3]), (views[9][:3, :3], views[9][:3, 3])], far, "inside"
    if name == "triangle":
        v, f, tex = _triangle()
        flip = (np.diag([-1.0, 1.0, 1.0]).astype(np.float32), np.zeros(3, np.float32))      # a mirrored camera sees the other side
        return (v, f, tex), [EYE, flip], 10.0, None
    v, f, tex = _fan(33 if name == "fan33" else 70)
    return (v, f, tex), [EYE], 10.0, None


@pytest.mark.parametrize("size,aa", SIZES)
@pytest.mark.parametrize("name", ["sphere", "hemisphere", "triangle", "fan33", "fan70"])
def test_fill_back_is_the_concatenated_form(name, size, aa):
    mesh, cams, far, inside = _fill_back_case(name)
    nf = len(mesh[1])
    s = Scene(mesh, size, aa, 0.0, far, light=LIGHT)
    fronts = backs = 0
    for i, (R, t) in enumerate(cams):
        got, want, keep = s.both(R, t, fill_back=True)
        _assert_same(got, want, f"{name} camera {i}")
        fi = keep["face_index"]
        fronts += int(((fi >= 0) & (fi < nf)).sum()); backs += int((fi >= nf).sum())
        if inside and i == 0:
            assert (fi >= nf).any() and not ((fi >= 0) & (fi < nf)).any()          # only back records can win inside the shell
            off = s.r.render(s.m, s.K, R, t, size, fill_back=False, want=("alpha",))[2]
            assert not off.any() and got[2].any()
    assert fronts > 0 and (backs > 0 or name == "sphere"), (fronts, backs)          # (a closed surface hides its back records)
    s.close()


# ---- 4: render_texture ----------------------------------------------------------------------------------------------------------------

def _write_uv_obj(path, uv, uvf):
    with open(path, "w") as fh:
        for i in range(int(uvf.max()) + 1):
            fh.write(f"v {i} 0 0\n")
        for u, w in uv:
            fh.write(f"vt {float(u)!r} {float(w)!r}\n")
        for a, b, c in uvf + 1:
            fh.write(f"f {a}/{a} {b}/{b} {c}/{c}\n")


@pytest.mark.parametrize("size,aa", [(20, True), (32, False)])
def test_render_texture_is_the_oracle(tmp_path, size, aa):
    from bodyfitting_amd import neural_renderer as nr
    nf, ts = 20, 4
    uv, uvf = uv_atlas(nf)
    tex = _distinct(nf, ts, seed=6)
    path = os.path.join(tmp_path, "uv.obj")
    _write_uv_obj(path, uv, uvf)
    r = nr.Renderer(image_size=size, anti_aliasing=aa, background_color=[1, 1, 1], near=0.0, far=4.0)
    rgb, depth = r.render_texture(path, tex[None])
    want_rgb, want_depth = TO.render_texture(uv, uvf, tex, size, 0.0, 4.0, anti_aliasing=aa)
    np.testing.assert_array_equal(rgb[0], want_rgb)
    np.testing.assert_array_equal(depth[0], want_depth)
    assert (depth < 4.0).mean() > 0.2 and (depth == 4.0).any()
    r.close()


# ---- 5: the texture VJP ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ts", [2, 4, 6])
def test_texture_vjp_lit_with_fill_back_front_and_back_of_one_face_from_two_tapes(ts):
    v, f, tex, views, far = _hemisphere(ts)
    s = Scene((v, f, tex), 20, True, 0.0, far, light=LIGHT)
    hit = []
    tapes = []
    for vi in (0, 9):                                                 # inside (back records), outside (front records)
        got, want, keep = s.both(views[vi][:3, :3], views[vi][:3, 3], fill_back=True, tape=True)
        _assert_same(got[:3], want)
        tapes.append((got[3], keep))
    s.m.set_textures(0 * tex)                                         # the tapes do not read the textures
    for i, (tape, keep) in enumerate(tapes):
        g, n = _check_vjp(tape, keep, seed=i)
        hit.append((n > 0).reshape(len(f), -1).any(1))
        tape.close()
    assert (hit[0] & hit[1]).sum() > 10                               # faces whose cube took both a back and a front contribution
    s.close()


@pytest.mark.parametrize("size,aa,fill_back", [(8, False, True), (32, True, False)])
def test_texture_vjp_on_the_sphere(size, aa, fill_back):
    v, f, tex = _sphere(ts=4, degenerate=True)
    views, far = _views(v)
    s = Scene((v, f, tex), size, aa, 0.0, far, light=LIGHT)
    for lightoff in (False, True):
        got, want, keep = s.both(views[5][:3, :3], views[5][:3, 3], fill_back=fill_back, lightoff=lightoff, tape=True)
        _check_vjp(got[3], keep)
        got[3].close()
    s.close()


def test_texture_vjp_of_a_face_with_a_large_pixel_box_takes_the_per_pixel_kernel():
    """output 40 x 40 with anti-aliasing = 80 x 80 super-sampled: the big face's box (> 4096 pixels) goes through
    bf_nr_backward_large_kernel - front in one view, back record in the mirrored one - the small sphere's through the gather"""
    v, f, tex = _big_face()
    s = Scene((v, f, tex), 40, True, 0.0, 10.0, light=LIGHT)
    for cam in (EYE, (np.diag([-1.0, 1.0, 1.0]).astype(np.float32), np.zeros(3, np.float32))):
        got, want, keep = s.both(*cam, fill_back=True, tape=True)
        _assert_same(got[:3], want)
        fi = keep["face_index"]
        big = (fi % len(f) == 0) & (fi >= 0)
        ys, xs = np.nonzero(big)
        assert (np.ptp(ys) + 1) * (np.ptp(xs) + 1) > 4096 and ((fi >= 0) & ~big).any()
        g, n = _check_vjp(got[3], keep)
        assert n[0].max() > 100 and np.abs(g[0]).max() > 0
        got[3].close()
    s.close()


# ---- 6, 7: through torch --------------------------------------------------------------------------------------------------------------------

def _torch_scene(size=20):
    import torch
    from bodyfitting_amd import neural_renderer as nr
    scan, fit = blob_pair(level=2, ts=4)
    center, dist = TF.scene_bound(scan[0])
    views = TF.gen_cam_views(center, 18, dist, gl=True)
    views.append(np.linalg.inv(TF.sphere2rot(dist, 0.7, 2.1, t=center)))
    views.append(np.linalg.inv(TF.sphere2rot(dist, 2.6, 5.0, t=center)))
    dev = torch.device("cpu")                                         # host tensors, as the other drop-ins' GPU tests pass them: the renders run on GPU 0
    r = nr.Renderer(image_size=size, K=_K(size)[None], orig_size=size, near=0.0, far=2 * dist, background_color=[1, 1, 1], fill_back=False,
                    light_intensity_ambient=1.0, light_intensity_directional=0.0)
    to = lambda a: torch.from_numpy(np.array(a)).to(dev)[None]      # noqa: E731  (a copy: Adam steps its tensor in place)
    return torch, r, scan, fit, views, dist, to


def test_depth_and_alpha_cotangents_give_bit_zero():
    torch, r, scan, fit, views, dist, to = _torch_scene()
    v, f = to(fit[0]), to(fit[1])
    R, t = to(views[2][:3, :3].astype(np.float32)), to(views[2][:3, 3].astype(np.float32))[None]
    for which in (1, 2):
        tex = to(scan[2]).requires_grad_(True)
        out = r.render(v, f, tex, R=R, t=t)
        assert out[0].shape == (1, 3, 20, 20) and out[1].shape == out[2].shape == (1, 20, 20) and out[0].device == tex.device
        (out[which] * torch.randn_like(out[which])).sum().backward()
        assert tex.grad is not None and tex.grad.shape == tex.shape and not tex.grad.any()
    tex = to(scan[2]).requires_grad_(True)
    r.render(v, f, tex, R=R, t=t)[0].sum().backward()
    assert tex.grad.any()
    with pytest.raises(NotImplementedError, match="soft-edge vertex gradient"):
        r.render(v.clone().requires_grad_(True), f, tex, R=R, t=t)
    r.close()


def test_torch_adam_loop_on_the_dropin_follows_bf_texfit_step_and_the_oracle_loop():
    """the loop of texture_fitting.py:262-275 with torch.optim.Adam on the drop-in, on test_adam_steps_follow_the_oracle_loop's
    views (tests/test_gpu_texfit.py), under that test's criteria"""
    IS = 32
    torch, r, scan, fit, views, dist, to = _torch_scene(IS)
    fused = TF.Renderer(IS, 4, near=0.0, far=2 * dist)
    fused.set_mesh(fused.TARGET, scan); fused.set_mesh(fused.FITTED, fit)
    o = TO.TextureFit(scan, fit, IS, 0.0, np.float32(2 * dist), lr=1e-2)
    scan_v, scan_f, scan_t = to(scan[0]), to(scan[1]), to(scan[2])
    smpl_v, smpl_f = to(fit[0]), to(fit[1])
    smpl_t = to(fit[2]).requires_grad_(True)
    optimizer = torch.optim.Adam([smpl_t], lr=1e-2)
    n = 8
    for i in range(n):
        pose = views[(i * 5) % len(views)]
        R, t = to(pose[:3, :3].astype(np.float32)), to(pose[:3, 3].astype(np.float32))[None]
        optimizer.zero_grad()
        scan_img = r.render_rgb(scan_v, scan_f, scan_t, R=R, t=t)
        smpl_img = r.render_rgb(smpl_v, smpl_f, smpl_t, R=R, t=t)
        loss = torch.sum(torch.abs(scan_img - smpl_img))
        loss.backward()
        optimizer.step()
        step_loss = fused.step(pose, 1e-2)
        want, _, _ = o.step(_K(IS), pose[:3, :3], pose[:3, 3], IS)
        print(f"iteration {i}: drop-in {float(loss):.6f} fused {step_loss:.6f} oracle {want:.6f}")
        assert float(loss) == pytest.approx(want, rel=1e-5), f"iteration {i}"
        assert float(loss) == pytest.approx(step_loss, rel=1e-5), f"iteration {i}"
    tex = smpl_t.detach().cpu().numpy()[0]
    for name, ref in (("oracle", o.mesh[2]), ("bf_texfit_step", fused.textures())):
        close = np.abs(tex - ref) < 1e-5
        print(f"{name}: {close.mean():.6f} of the texels within 1e-5, largest difference {np.abs(tex - ref).max():.3g}")
        assert close.mean() > 0.999, (name, close.mean())
        assert np.abs(tex - ref).max() <= n * 1e-2 * 1.01
    assert np.abs(tex - fit[2]).max() > 0.02                          # and the textures did move
    assert len(r._meshes) == 2                                        # one device mesh per (vertices, faces) pair, kept over the loop
    fused.close(); r.close()


# ---- 8: tile lists ----------------------------------------------------------------------------------------------------------------------------

def test_a_render_that_overflows_the_first_tile_list_guess_repeats_and_matches():
    """24 faces (twelve stacked quads) over all 64 tiles of a 64 x 64 render: 1,536 list entries against a first capacity of
    24 * 4 + 64 + 1024 = 1,184"""
    quads_v, quads_f = [], []
    for q in range(12):
        z = 2.0 + 0.25 * q
        s = 1.5 * z
        quads_v.append(np.array([[-s, -s, z], [s, -s, z], [s, s, z], [-s, s, z]], np.float32))
        quads_f += [[4 * q, 4 * q + 1, 4 * q + 2], [4 * q, 4 * q + 2, 4 * q + 3]]
    v, f = np.concatenate(quads_v), np.asarray(quads_f, np.int32)
    s = Scene((v, f, _distinct(len(f), 2, seed=8)), 64, False, 0.0, 10.0, light=LIGHT)
    got, want, keep = s.both(*EYE, fill_back=True, tape=True)
    _assert_same(got[:3], want)
    assert (keep["face_index"] >= 0).all()
    _assert_same(s.r.render(s.m, s.K, *EYE, 64, fill_back=True)[:3], want)           # and again, with the grown lists
    _check_vjp(got[3], keep)                                          # the tape is the repeated render's
    got[3].close()
    s.close()


# ---- 9: limits and refusals --------------------------------------------------------------------------------------------------------------------

def test_limits_and_refusals_return_their_codes():
    import ctypes as C
    lib = _lib.load()
    INVALID, UNSUPPORTED, NO_DEVICE = -1, -3, -4
    h = C.c_void_p()
    bg = np.zeros(3, np.float32)
    assert lib.bf_nr_create(0, 0, 1, 0.1, 100.0, _lib.fptr(bg), C.byref(h)) == INVALID
    assert lib.bf_nr_create(0, 16, 1, 5.0, 1.0, _lib.fptr(bg), C.byref(h)) == INVALID
    assert lib.bf_nr_create(0, 4097, 1, 0.1, 100.0, _lib.fptr(bg), C.byref(h)) == UNSUPPORTED
    assert lib.bf_nr_create(99, 16, 1, 0.1, 100.0, _lib.fptr(bg), C.byref(h)) == NO_DEVICE
    assert lib.bf_nr_create(0, 16, 1, 0.1, 100.0, None, None) == INVALID
    r = native.NrRenderer(16, True, 0.1, 100.0)
    other = native.NrRenderer(16, True, 0.1, 100.0)
    v, f, tex = _triangle()
    m = C.c_void_p()
    args = (len(v), _lib.fptr(v), 1, _lib.iptr(f))
    assert lib.bf_nr_mesh_create(r._h, *args, 17, None, C.byref(m)) == UNSUPPORTED
    assert lib.bf_nr_mesh_create(r._h, *args, 1, None, C.byref(m)) == INVALID
    assert lib.bf_nr_mesh_create(r._h, *args, 0, _lib.fptr(tex), C.byref(m)) == INVALID
    assert lib.bf_nr_mesh_create(r._h, 2, _lib.fptr(v), 1, _lib.iptr(f), 4, None, C.byref(m)) == INVALID          # face index out of range
    assert lib.bf_nr_mesh_create(None, *args, 4, None, C.byref(m)) == INVALID
    assert lib.bf_nr_mesh_create(r._h, len(v), _lib.fptr(v), (1 << 30) + 1, _lib.iptr(f), 4, None, C.byref(m)) == UNSUPPORTED      # 2 NF past an int
    assert b"2 x n_faces" in lib.bf_last_error()
    bare = native.NrMesh(r, v, f, 4)                                  # textures not set yet
    plain = native.NrMesh(r, v, f)                                    # no texture size at all
    full = native.NrMesh(r, v, f, 4, tex)
    K, (R, t) = _K(16), EYE
    cam = (_lib.fptr(K), _lib.fptr(R), _lib.fptr(t), 16.0, 1, 0, 0)
    rgb = np.empty((3, 16, 16), np.float32)
    tp = C.c_void_p()
    assert lib.bf_nr_render(r._h, bare._h, *cam, _lib.fptr(rgb), None, None, None) == INVALID             # rgb of a mesh without textures
    assert lib.bf_nr_render(r._h, plain._h, *cam, None, None, None, C.byref(tp)) == INVALID             # a tape of one
    assert lib.bf_nr_render(other._h, full._h, *cam, _lib.fptr(rgb), None, None, None) == INVALID         # another renderer's mesh
    assert lib.bf_nr_render(r._h, full._h, None, None, None, 16.0, 1, 0, 0, _lib.fptr(rgb), None, None, None) == INVALID
    assert lib.bf_nr_render(r._h, full._h, _lib.fptr(K), _lib.fptr(R), _lib.fptr(t), 0.0, 1, 0, 0, _lib.fptr(rgb), None, None, None) == INVALID
    assert lib.bf_nr_render(r._h, None, *cam, _lib.fptr(rgb), None, None, None) == INVALID
    assert lib.bf_nr_mesh_set_textures(plain._h, _lib.fptr(tex)) == INVALID
    assert lib.bf_nr_render(r._h, plain._h, *cam, None, None, _lib.fptr(rgb[0]), None) == 0               # silhouettes need no textures
    assert rgb[0].any()
    assert lib.bf_nr_render(r._h, full._h, *cam, _lib.fptr(rgb), None, None, C.byref(tp)) == 0
    g = np.ones((3, 16, 16), np.float32)
    out = np.empty(tex.shape, np.float32)
    assert lib.bf_nr_tape_texture_grad(tp, None, _lib.fptr(out)) == INVALID
    assert lib.bf_nr_tape_texture_grad(tp, _lib.fptr(g), _lib.fptr(out)) == 0 and out.any()
    for mesh in (bare, plain, full):
        mesh.close()
    r.close()
    assert lib.bf_nr_tape_texture_grad(tp, _lib.fptr(g), _lib.fptr(out)) == INVALID                        # the tape outlived its renderer
    assert b"outlived" in lib.bf_last_error()
    lib.bf_nr_tape_destroy(tp)
    other.close()
