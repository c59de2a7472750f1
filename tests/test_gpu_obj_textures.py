"""Textured OBJ scans on the GPU: bf_texfit_load_textures against tests/texload_oracle.py (the numpy restatement of
load_textures_cuda_kernel.cu) and the reference's own load_obj (tests/golden/nr_load_obj_textures.npz), bf_texfit_render_depth and
render_texture_mesh against oracle/texfit_oracle.py, and the drop-in TextureFitting end to end.  Everything is compared bit for bit:
the texture kernel and the rasteriser keep the reference's float32 operation order (-ffp-contract=off)."""
import os

import numpy as np
import pytest

from bodyfitting_amd import obj_textures as OT
from bodyfitting_amd import texture_dropin as TD
from bodyfitting_amd import texture_fitting as TF
from oracle import texfit_oracle as TXO
import texload_oracle as TO
from test_obj_textures import golden, modes, write_fixture
from texfit_cases import icosphere, uv_atlas

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.mark.parametrize("name", ["mixed", "scan"])
def test_kernel_equals_the_restatement_in_every_mode(name, tmp_path):
    g = golden()
    path = write_fixture(g, name, str(tmp_path))
    job = OT.parse_textures(path, OT.mtllib_files(path, OT._read_lines(path))[-1])
    for ts in (2, 4, 6):
        for wrap in OT.TEXTURE_WRAPPING:
            for bil in (True, False):
                got = OT.run_load_textures(job, ts, wrap, bil)
                want = TO.load_job(job, ts, OT.TEXTURE_WRAPPING[wrap], bil)
                np.testing.assert_array_equal(got, want, err_msg=f"{name} ts={ts} {wrap} bilinear={bil}")


@pytest.mark.parametrize("name", ["mixed", "scan"])
def test_load_obj_equals_the_reference_golden(name, tmp_path):
    g = golden()
    path = write_fixture(g, name, str(tmp_path))
    for key, ts, wrap, bil in modes(g, name):
        v, f, t = OT.load_obj(path, normalization=False, texture_size=ts, load_texture=True, texture_wrapping=wrap, use_bilinear=bil)
        np.testing.assert_array_equal(v, g[f'{name}__vertices_raw'])
        np.testing.assert_array_equal(f, g[f'{name}__faces'])
        np.testing.assert_array_equal(t, g[key], err_msg=key)
    v, f, _ = OT.load_obj(path, load_texture=True)
    np.testing.assert_array_equal(v, g[f'{name}__vertices_norm'])


def test_kernel_on_a_scan_sized_mesh():
    """250k faces, a 4096^2 image, UVs inside and outside [0, 1] and on exact integers"""
    rng = np.random.default_rng(5)
    nf, H, W = 250_000, 4096, 4096
    uv = rng.uniform(-0.5, 1.5, (nf, 3, 2)).astype(F32)
    uv[:1000] = np.round(uv[:1000])
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    face_image = np.where(rng.uniform(size=nf) < 0.95, 0, -1).astype(np.int32)
    job = dict(face_uv=uv, face_image=face_image, face_fill=rng.uniform(0, 1, (nf, 3)).astype(F32), images=[img])
    for wrap, bil in (('REPEAT', True), ('MIRRORED_REPEAT', False)):
        timing = {}
        got = OT.run_load_textures(job, 4, wrap, bil, timing=timing)
        want = TO.load_job(job, 4, OT.TEXTURE_WRAPPING[wrap], bil)
        np.testing.assert_array_equal(got, want, err_msg=wrap)
        assert timing['kernel_ms'] > 0


def test_texture_size_below_two_is_refused_by_the_entry_point():
    job = dict(face_uv=np.zeros((1, 3, 2), F32), face_image=np.zeros(1, np.int32), face_fill=np.zeros((1, 3), F32),
               images=[np.zeros((2, 2, 3), np.uint8)])
    with pytest.raises(ValueError):
        OT.run_load_textures(job, 1)
    from bodyfitting_amd import _lib
    job['face_image'][0] = 3                                  # (no such image: refused before anything reaches the device)
    with pytest.raises(_lib.BodyfitError):
        OT.run_load_textures(job, 2)


def _scan(tmp_path):
    g = golden()
    path = write_fixture(g, "scan", str(tmp_path))
    return path, OT.load_obj(path, normalization=False, load_texture=True)


def _oracle_rgbd(mesh, pose, K, size, far, background):
    """Renderer.render (rasterize_rgbad) from oracle/texfit_oracle.py's pieces: project, rasterize, sample, background, flip, pool"""
    v, f, t = mesh
    pv = TXO.project(v, K, pose[:3, :3], pose[:3, 3], size)
    fv = pv[np.asarray(f, np.int64)]
    fi, w, d = TXO.rasterize(fv, 2 * size, 0.0, F32(far))
    rgb, _, _ = TXO.sample_textures(fv, np.asarray(t, F32), fi, w, d)
    mask = (fi >= 0).astype(F32)[:, :, None]
    rgb = (rgb * mask + (F32(1) - mask) * np.asarray(background, F32)[None, None, :]).astype(F32)
    img = rgb.transpose(2, 0, 1)[:, ::-1, :].reshape(3, size, 2, size, 2)
    img = ((img[:, :, 0, :, 0] + img[:, :, 0, :, 1] + img[:, :, 1, :, 0] + img[:, :, 1, :, 1]) * F32(0.25)).astype(F32)
    dep = d[::-1, :].reshape(size, 2, size, 2)
    dep = ((dep[:, 0, :, 0] + dep[:, 0, :, 1] + dep[:, 1, :, 0] + dep[:, 1, :, 1]) * F32(0.25)).astype(F32)
    return img, dep


def test_render_depth_is_render_plus_the_pooled_depth(tmp_path):
    _, mesh = _scan(tmp_path)
    size = 32
    center, dist = TD.scene_bound(mesh[0])
    K = np.array([[size, 0, size / 2], [0, size, size / 2], [0, 0, 1]], F32)
    r = TF.Renderer(size, 4, near=0.0, far=2 * dist, background=(0.0, 0.0, 0.0), K=K, orig_size=size)
    try:
        r.set_mesh(r.TARGET, mesh)
        for pose in TD.gen_cam_views(center, 5, dist, gl=True)[:3]:
            rgb, depth = r.render_rgbd(r.TARGET, pose)
            np.testing.assert_array_equal(rgb, r.render_rgb(r.TARGET, pose))
            want_rgb, want_depth = _oracle_rgbd(mesh, pose, K, size, F32(2 * dist), (0, 0, 0))
            np.testing.assert_array_equal(rgb, want_rgb)
            np.testing.assert_array_equal(depth, want_depth)
            assert (depth < F32(2 * dist)).any() and (depth == F32(2 * dist)).any()
    finally:
        r.close()


@pytest.mark.parametrize("white_bkgd", [False, True])
def test_render_texture_mesh_equals_the_oracle(white_bkgd, tmp_path):
    path, mesh = _scan(tmp_path)
    size = 32
    imgs, masks, poses, Ks = TD.render_texture_mesh(path, imgsize=size, white_bkgd=white_bkgd)
    p2, k2 = TD.render_texture_mesh(path, imgsize=size, pose_only=True)
    np.testing.assert_array_equal(np.stack(poses), np.stack(p2))
    center, dist = TD.scene_bound(mesh[0])
    far = 2 * dist
    assert len(imgs) == 8 and len(masks) == 8
    for img, mask, pose, K in zip(imgs, masks, poses, Ks):
        rgb, dep = _oracle_rgbd(mesh, pose, K, size, F32(far), (0, 0, 0))
        want_img = (np.clip(rgb.transpose(1, 2, 0), 0, 1) * 255).astype(np.uint8)
        want_mask = ((dep < F32(far)) * 255).astype(np.uint8)
        if white_bkgd:
            want_img = want_img + (255 - want_mask[..., None])
        assert img.dtype == np.uint8 and mask.dtype == np.uint8
        np.testing.assert_array_equal(mask, want_mask)
        np.testing.assert_array_equal(img, want_img)
        assert 0 < (mask == 255).mean() < 1


def _write_texfit_inputs(d):
    """a textured scan (the golden's fixture), an SMPL+D OBJ on the same topology and the SMPL UV OBJ + MTL it takes its vt / f from"""
    from PIL import Image
    scan_path = write_fixture(golden(), "scan", d)
    v, f = icosphere(1)
    v = v * np.array([0.45, 0.8, 0.4], np.float32) + np.array([0.1, 0.9, -0.05], np.float32)
    v = v + 0.01 * np.random.default_rng(2).standard_normal(v.shape).astype(np.float32)
    uv, uvf = uv_atlas(len(f), seed=9)
    uvdir = os.path.join(d, "smpl_uv")
    os.makedirs(uvdir)
    with open(os.path.join(uvdir, "smpl_uv.mtl"), "w") as fh:
        fh.write("newmtl material_0\nKd 1 1 1\nmap_Kd smpl_uv.png\n")
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(os.path.join(uvdir, "smpl_uv.png"))
    lines = ["mtllib smpl_uv.mtl"] + ["v %.6f %.6f %.6f" % tuple(p) for p in v] + ["vt %.6f %.6f" % tuple(p) for p in uv]
    lines += ["usemtl material_0"] + [f"f {a + 1}/{ta + 1} {b + 1}/{tb + 1} {c + 1}/{tc + 1}" for (a, b, c), (ta, tb, tc) in zip(f, uvf)]
    with open(os.path.join(uvdir, "smpl_uv.obj"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    smpld = os.path.join(d, "smpl+d.obj")
    with open(smpld, "w") as fh:
        fh.write("".join("v %.6f %.6f %.6f\n" % tuple(p) for p in v) + "".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f))
    return scan_path, smpld, os.path.join(uvdir, "smpl_uv.obj"), uv, uvf


def test_texture_fitting_drop_in_end_to_end(tmp_path, capfd):
    from PIL import Image
    scan_path, smpld, uv_obj, uv, uvf = _write_texfit_inputs(str(tmp_path))
    size, iters, out = 32, 93, str(tmp_path / "texfit")
    np.random.seed(21)
    tf = TD.TextureFitting(uv_obj, tex_img_size=64, render_img_size=size, iter_num=iters, debug=print, render=True)
    textures, losses = tf(out, smpld, scan_path)
    assert "video.mp4" in capfd.readouterr().err
    # the loop is texture_fitting.TextureFitting.fit on the arrays nr.load_obj gives, with the reference's view sequence
    smpl = OT.load_obj(os.path.join(out, "smpl+d.obj"), normalization=False, load_texture=True)
    scan = OT.load_obj(scan_path, normalization=False, load_texture=True)
    np.testing.assert_allclose(smpl[2], 128 / 255, rtol=4e-7)
    center, dist = TD.scene_bound(scan[0])
    np.random.seed(21)
    poses = [np.linalg.inv(TXO.sphere2rot(dist, np.random.uniform(0, np.pi), np.random.uniform(0, np.pi * 2), t=center))
             for _ in range(iters - 90)]
    np.random.seed(21)
    views = tf.views(center, dist)
    for a, b in zip(views[90:], poses):
        np.testing.assert_array_equal(a, b)
    want_t, want_l = TF.TextureFitting(size, 1e-2, iters).fit(smpl, scan, poses=views, far=2 * dist)
    np.testing.assert_array_equal(textures, want_t)
    np.testing.assert_array_equal(losses, want_l)
    # smpl.png: the UV-space render of the fitted textures through the reference's to8b (RGB)
    rgb, _ = TXO.render_texture(uv, uvf, want_t, size, 0.0, F32(2 * dist))
    want_png = (np.clip(rgb.transpose(1, 2, 0), 0, 1) * 255).astype(np.uint8)
    np.testing.assert_array_equal(np.asarray(Image.open(os.path.join(out, "smpl.png"))), want_png)
    # render/: 36 views, scan | fitted; debug/: one image per iteration, the fitted mesh before that iteration's step
    K = np.array([[size, 0, size // 2], [0, size, size // 2], [0, 0, 1]], F32)
    rend = sorted(os.listdir(os.path.join(out, "render")))
    assert rend == [f"{i:04d}.png" for i in range(36)]
    pose = TD.gen_cam_views(center, 36, dist, gl=True)[7]
    img = np.asarray(Image.open(os.path.join(out, "render", "0007.png")))
    for half, mesh in ((img[:, :size], scan), (img[:, size:], (smpl[0], smpl[1], want_t))):
        want = TXO.render(*mesh, K, pose[:3, :3], pose[:3, 3], size, size, 0.0, F32(2 * dist))
        np.testing.assert_array_equal(half, (np.clip(want.transpose(1, 2, 0), 0, 1) * 255).astype(np.uint8))
    assert len(os.listdir(os.path.join(out, "debug"))) == iters
    want0 = TXO.render(*smpl, K, views[0][:3, :3], views[0][:3, 3], size, size, 0.0, F32(2 * dist))
    np.testing.assert_array_equal(np.asarray(Image.open(os.path.join(out, "debug", "0.png"))),
                                  (np.clip(want0.transpose(1, 2, 0), 0, 1) * 255).astype(np.uint8))
    assert not np.array_equal(np.asarray(Image.open(os.path.join(out, "debug", f"{iters - 1}.png"))),
                              np.asarray(Image.open(os.path.join(out, "debug", "0.png"))))
