"""Reading textured OBJ scans (bodyfitting_amd/obj_textures.py, nr.load_obj) and the drop-ins of apps/rp_fitting.py's texture steps
(bodyfitting_amd/texture_dropin.py), without a GPU: the host reader against tests/golden/nr_load_obj_textures.npz (the reference's own
load_obj.py and utils/renderer.py, tools/gen_texload_golden.py), known answers for tests/texload_oracle.py (the restatement of
load_textures_cuda_kernel.cu the GPU kernel is compared with), the refusals and the file-level helpers."""
import os
import sys

import numpy as np
import pytest

from bodyfitting_amd import obj_textures as OT
from bodyfitting_amd import texture_dropin as TD
import texload_oracle as TO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "nr_load_obj_textures.npz")
F32 = np.float32


def golden():
    return np.load(GOLDEN)


def write_fixture(g, name, d):
    """the fixture's files into directory d -> path of its OBJ"""
    for n in g[f'{name}__files']:
        with open(os.path.join(d, str(n)), 'wb') as fh:
            fh.write(g[f'{name}__file__{n}'].tobytes())
    return os.path.join(d, str(g[f'{name}__obj']))


def modes(g, name):
    for k in g.files:
        if k.startswith(f'{name}__tex__'):
            ts, rest = k.split('__')[2].split('_', 1)
            wrap, bil = rest.rsplit('_', 1)
            yield k, int(ts), wrap, bil == '1'


@pytest.mark.parametrize("name", ["mixed", "scan"])
def test_reader_equals_the_reference_load_obj(name, tmp_path):
    g = golden()
    path = write_fixture(g, name, str(tmp_path))
    lines = OT._read_lines(path)
    v, f = OT.load_vertices(path), OT.load_faces(path)
    np.testing.assert_array_equal(v, g[f'{name}__vertices_raw'])
    np.testing.assert_array_equal(OT.normalize_vertices(v), g[f'{name}__vertices_norm'])
    np.testing.assert_array_equal(f, g[f'{name}__faces'])
    mtls = OT.mtllib_files(path, lines)
    job = OT.parse_textures(path, mtls[-1])
    n = 0
    for key, ts, wrap, bil in modes(g, name):
        got = TO.load_job(job, ts, OT.TEXTURE_WRAPPING[wrap], bil)
        assert got.dtype == np.float32 and got.shape == g[key].shape
        np.testing.assert_array_equal(got, g[key], err_msg=key)
        n += 1
    assert n == 12
    if name == "mixed":
        assert len(mtls) == 2 and mtls[-1].endswith("second.mtl")
        assert sorted(os.path.basename(p) for p in job['image_files']) == ['grey.png', 'pal.png', 'rgb.png', 'rgba.png']
        # faces before any usemtl take the Kd written before any newmtl (material ''), `bare` and an unknown material keep 0.5
        np.testing.assert_array_equal(job['face_fill'][0], np.array([0.1, 0.2, 0.3], np.float32))
        assert (job['face_fill'] == F32(0.5)).all(1).sum() >= 2


@pytest.mark.parametrize("name", ["mixed", "scan"])
def test_pose_only_cameras_equal_the_reference(name, tmp_path):
    g = golden()
    path = write_fixture(g, name, str(tmp_path))
    for size in (512, 37):
        poses, Ks = TD.render_texture_mesh(path, imgsize=size, pose_only=True)
        np.testing.assert_array_equal(np.stack(poses), g[f'{name}__poses_{size}'])
        np.testing.assert_array_equal(np.stack(Ks), g[f'{name}__Ks_{size}'])
        assert Ks[0][0, 2] == size / 2                                  # `/`, not the texture loop's `//`


def test_dist_divides_the_float32_height_in_float64():
    """numpy 1 (the reference's environment) promotes float32 scalar / Python float to float64; numpy 2 would stay in float32"""
    v = np.array([[0, 0, 0], [0.3, 1.7123457, 0.2]], np.float32)
    _, dist = TD.scene_bound(v)
    h = np.float32(1.7123457)
    assert dist == np.float64(h) / 0.8
    assert dist != np.float64(h / np.float32(0.8))                       # (what numpy 2 gives for `height / 0.8`)
    assert isinstance(dist, np.float64)


def test_pose_only_reads_only_the_vertices(tmp_path):
    p = tmp_path / "plain.obj"
    p.write_text("v 0 0 0\nv 1 2 0\nv 0 1 1\nf 1 2 3\n")
    poses, Ks = TD.render_texture_mesh(str(p), imgsize=64, pose_only=True)
    assert len(poses) == 8 and len(Ks) == 8
    with pytest.raises(Exception, match="Failed to load textures."):
        OT.load_obj(str(p), load_texture=True)


# ---- known answers for the restatement of load_textures_cuda_kernel ------------------------------------------------------------------

def one_face(corners, image, ts=4, wrapping=TO.REPEAT, bilinear=True):
    faces = np.asarray(corners, np.float32).reshape(1, 3, 2)
    tex = np.full((1, ts, ts, ts, 3), 0.5, np.float32)
    return TO.load_textures(np.asarray(image, np.float32), faces, tex, np.ones(1, np.int32), wrapping, bilinear)[0]


def test_constant_image_gives_constant_texels():
    img = np.broadcast_to(np.array([0.2, 0.6, 0.9], np.float32), (9, 13, 3))
    for ts in (2, 4, 6):
        t = one_face([[0.1, 0.2], [0.8, 0.3], [0.4, 0.9]], img, ts=ts)
        np.testing.assert_allclose(t.reshape(-1, 3), np.broadcast_to([0.2, 0.6, 0.9], (ts ** 3, 3)), rtol=4e-7, atol=0)


def test_linear_ramp_gives_the_interpolated_value():
    W, H = 65, 33
    ramp = np.broadcast_to((np.arange(W, dtype=np.float32) / (W - 1))[None, :, None], (H, W, 3)).astype(np.float32)
    corners = np.array([[0.125, 0.25], [0.875, 0.5], [0.5, 0.75]], np.float32)
    ts = 4
    t = one_face(corners, ramp, ts=ts).reshape(-1, 3)
    d = TO.texel_dims(ts).astype(np.float64)
    want = d @ corners[:, 0].astype(np.float64)                          # the barycentric u of every texel
    np.testing.assert_allclose(t[:, 0], want, atol=1e-6)


def test_corner_texels_sample_the_vertex_uv():
    rng = np.random.default_rng(0)
    img = rng.uniform(0, 1, (17, 23, 3)).astype(np.float32)
    corners = np.array([[0.25, 0.5], [0.75, 0.125], [0.5, 1.0 - 1 / 16]], np.float32)
    for ts in (2, 4, 6):
        t = one_face(corners, img, ts=ts, bilinear=False)
        # texel (ts-1, 0, 0) is corner 0, (0, ts-1, 0) corner 1, (0, 0, ts-1) corner 2; (0, 0, 0) has no weights: corner uv x 0 -> (0, 0)
        for idx, c in (((ts - 1, 0, 0), 0), ((0, ts - 1, 0), 1), ((0, 0, ts - 1), 2)):
            u, v = corners[c]
            np.testing.assert_array_equal(t[idx], img[int(np.floor(v * 16 + 0.5)), int(np.floor(u * 22 + 0.5))])
        np.testing.assert_array_equal(t[0, 0, 0], img[0, 0])


def test_wrapping_by_hand():
    """texel (ts-1, 0, 0) samples corner 0 exactly; a 5-wide image, nearest: column = round(u' x 4)"""
    img = np.zeros((1, 5, 3), np.float32)
    img[0, :, 0] = np.arange(5)
    cases = [  # (u, wrapping, column)
        (0.0, TO.REPEAT, 4), (1.0, TO.REPEAT, 0), (-0.25, TO.REPEAT, 3), (1.25, TO.REPEAT, 1), (2.0, TO.REPEAT, 0),
        (-1.0, TO.REPEAT, 4),
        (0.25, TO.MIRRORED_REPEAT, 1), (1.25, TO.MIRRORED_REPEAT, 3), (-0.25, TO.MIRRORED_REPEAT, 1), (1.0, TO.MIRRORED_REPEAT, 4),
        (2.0, TO.MIRRORED_REPEAT, 0), (0.0, TO.MIRRORED_REPEAT, 0),          # mod(0, 2) = 2: 1 - mod(0, 1) = 0
        (-0.5, TO.CLAMP_TO_EDGE, 0), (1.5, TO.CLAMP_TO_EDGE, 4), (0.5, TO.CLAMP_TO_EDGE, 2),
    ]
    for u, w, col in cases:
        t = one_face([[u, 0.0], [0.5, 0.0], [0.5, 0.0]], img, ts=2, wrapping=w, bilinear=False)
        assert t[1, 0, 0, 0] == col, (u, w, t[1, 0, 0, 0], col)
    t = one_face([[0.3, 0.0], [0.5, 0.0], [0.5, 0.0]], img, ts=2, wrapping=TO.CLAMP_TO_BORDER)
    assert (t == 0).all()


def test_nearest_rounds_half_away_from_zero():
    img = np.zeros((1, 9, 3), np.float32)
    img[0, :, 0] = np.arange(9)
    # u = 2.5 / 8, 4.5 / 8 land exactly half-way between columns: half-to-even would give 2 and 4
    for u, col in ((2.5 / 8, 3), (4.5 / 8, 5), (0.5 / 8, 1)):
        t = one_face([[u, 0.0], [0.5, 0.0], [0.5, 0.0]], img, ts=2, wrapping=TO.CLAMP_TO_EDGE, bilinear=False)
        assert t[1, 0, 0, 0] == col
    np.testing.assert_array_equal(TO.round_half_away(np.array([0.5, 1.5, 2.5, -0.5, 0.49999997], np.float32)), [1, 2, 3, -1, 0])


def test_bilinear_upper_neighbour_rounds_in_float():
    """y1 = int(pos_y + 1) with the + 1 in float32: pos_y just below 1 gives y1 = 2 while y0 = 0"""
    py = np.float32(0.99999994)
    assert int(np.float32(py + np.float32(1))) == 2 and int(py) == 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def textured_obj(tmp_path, image=None, mtllib=True):
    from PIL import Image
    (tmp_path / "m.mtl").write_text("newmtl a\nKd 0.5 0.5 0.5\nmap_Kd t.png\n")
    img = image if image is not None else Image.fromarray(np.zeros((4, 4, 3), np.uint8))
    img.save(tmp_path / "t.png")
    text = ("mtllib m.mtl\n" if mtllib else "") + "v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nusemtl a\nf 1/1 2/2 3/3\n"
    (tmp_path / "m.obj").write_text(text)
    return str(tmp_path / "m.obj")


def test_texture_size_below_two_is_refused(tmp_path):
    path = textured_obj(tmp_path)
    for ts in (0, 1):
        with pytest.raises(ValueError, match="texture_size"):
            OT.load_obj(path, texture_size=ts, load_texture=True)


def test_sixteen_bit_and_two_channel_images_are_refused(tmp_path):
    from PIL import Image
    path = textured_obj(tmp_path, Image.fromarray(np.full((4, 4), 40000, np.uint16)))
    with pytest.raises(ValueError, match="t.png"):
        OT.parse_textures(path, str(tmp_path / "m.mtl"))
    Image.fromarray(np.zeros((4, 4, 2), np.uint8), mode="LA").save(tmp_path / "t.png")
    with pytest.raises(ValueError, match="t.png"):
        OT.parse_textures(path, str(tmp_path / "m.mtl"))


def test_palette_grey_and_rgba_images_become_rgb(tmp_path):
    from PIL import Image
    rgba = np.random.default_rng(1).integers(0, 256, (3, 5, 4), dtype=np.uint8)
    Image.fromarray(rgba).save(tmp_path / "a.png")
    np.testing.assert_array_equal(OT.read_image(str(tmp_path / "a.png")), rgba[:, :, :3])
    grey = rgba[:, :, 0].copy()
    Image.fromarray(grey).save(tmp_path / "g.png")
    np.testing.assert_array_equal(OT.read_image(str(tmp_path / "g.png")), np.stack([grey] * 3, -1))
    pal = Image.fromarray(rgba[:, :, :3]).convert("P", palette=Image.ADAPTIVE, colors=8)
    pal.save(tmp_path / "p.png")
    np.testing.assert_array_equal(OT.read_image(str(tmp_path / "p.png")), np.asarray(pal.convert("RGB")))


def test_negative_vertex_index_is_refused(tmp_path):
    p = tmp_path / "neg.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf -1 -2 -3\n")
    with pytest.raises(ValueError, match="vertex index"):
        OT.load_obj(str(p))


def test_missing_mtllib_fails_like_the_reference(tmp_path):
    path = textured_obj(tmp_path, mtllib=False)
    with pytest.raises(Exception, match="Failed to load textures."):
        OT.load_obj(path, load_texture=True)
    v, f = OT.load_obj(path)
    assert v.shape == (3, 3) and f.tolist() == [[0, 1, 2]]


def test_missing_vt_lines_fail_like_np_vstack(tmp_path):
    (tmp_path / "m.mtl").write_text("newmtl a\n")
    (tmp_path / "m.obj").write_text("mtllib m.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    with pytest.raises(ValueError):
        OT.parse_textures(str(tmp_path / "m.obj"), str(tmp_path / "m.mtl"))


# ---- the drop-in's file-level helpers ---------------------------------------------------------------------------------------------

def test_create_smpld_uv_writes_the_reference_file(tmp_path):
    from PIL import Image
    uvdir = tmp_path / "smpl_uv"
    uvdir.mkdir()
    (uvdir / "smpl_uv.mtl").write_text("newmtl material_0\nKd 1 1 1\nmap_Kd smpl_uv.png\n")
    (uvdir / "smpl_uv.obj").write_text("mtllib smpl_uv.mtl\nv 9 9 9\nv 8 8 8\nv 7 7 7\nvt 0.1 0.2\nvt 0.3 0.4\nvt 0.5 0.6\n"
                                       "usemtl material_0\nf 1/1 2/2 3/3\nf 3/3 2/2 1/1\n")
    (tmp_path / "smpl+d.obj").write_text("v 1.0 2.0 3.0\nv 4 5 6\nv 7 8 9\nf 1 2 3\n")
    out = tmp_path / "texfit"
    out.mkdir()
    TD.create_smpld_uv(str(out / "smpl+d.obj"), str(tmp_path / "smpl+d.obj"), str(uvdir / "smpl_uv.obj"), 16)
    assert (out / "smpl+d.obj").read_text() == ("v 1.0 2.0 3.0\nv 4 5 6\nv 7 8 9\nmtllib smpl_uv.mtl\nusemtl material_0\n"
                                                "vt 0.1 0.2\nvt 0.3 0.4\nvt 0.5 0.6\nf 1/1 2/2 3/3\nf 3/3 2/2 1/1\n")
    assert (out / "smpl_uv.mtl").read_text() == (uvdir / "smpl_uv.mtl").read_text()
    tex = np.asarray(Image.open(out / "smpl_uv.png"))
    assert tex.shape == (16, 16, 3) and (tex == 128).all()


def test_to8b_is_the_references_rgb_order():
    x = np.zeros((2, 2, 3), np.float32)
    x[..., 0], x[..., 2] = 1.0, 0.25
    y = TD.to8b(x[:, :, ::-1])                               # the caller's [:, :, ::-1], flipped back
    assert y[0, 0].tolist() == [255, 0, 63]


def test_load_obj_uv_follows_the_reference(tmp_path):
    p = tmp_path / "uv.obj"
    p.write_text("vt 0.25 0.75\nvt 0.5 0.5\nvt 1 0\nf 1/1 2/2 3/3 1/2\nf 1//1 2//2 3//3\n")
    uv = TD.load_obj_uv(str(p))
    assert uv.shape == (3, 3, 2) and uv.dtype == np.float32
    np.testing.assert_array_equal(uv[0], [[0.25, 0.25], [0.5, 0.5], [1, 1]])
    np.testing.assert_array_equal(uv[2], [[1, 1]] * 3)                 # v//vn -> vt index 0 -> the last vt


def test_inpaint_is_out_of_scope():
    with pytest.raises(NotImplementedError, match="DESIGN.md"):
        TD.TextureFitting("smpl_uv.obj", inpaint=True)


def test_view_schedule_uses_the_global_generator():
    tf = TD.TextureFitting("unused.obj", iter_num=93)
    c, d = np.array([0.1, 0.9, -0.05], np.float32), np.float64(2.2)
    np.random.seed(4)
    poses = tf.views(c, d)
    ring = TD.gen_cam_views(c, 18, d, gl=True)
    for i in range(90):
        np.testing.assert_array_equal(poses[i], ring[i % 18])
    np.random.seed(4)
    for i in range(90, 93):
        want = np.linalg.inv(TD.sphere2rot(d, np.random.uniform(0, np.pi), np.random.uniform(0, np.pi * 2), t=c))
        np.testing.assert_array_equal(poses[i], want)


def test_rp_fitting_import_lines_resolve_to_the_drop_in():
    """apps/rp_fitting.py:11,17 and smplify/texture_fitting.py:12 under the INTEGRATION.md sys.path line"""
    sys.path.insert(0, os.path.join(REPO, "bodyfitting_amd", "dropin"))
    try:
        for mod in [m for m in sys.modules if m.split(".")[0] in ("smplify", "utils")]:
            sys.modules.pop(mod)
        from smplify.texture_fitting import TextureFitting
        from utils.renderer import render_texture_mesh, gen_cam_views
        from smplify.texture_fitting import create_smpld_uv, load_obj_uv, sphere2rot, to8b, render_texture_map  # noqa: F401
        assert TextureFitting is TD.TextureFitting
        assert render_texture_mesh is TD.render_texture_mesh and gen_cam_views is TD.gen_cam_views
    finally:
        sys.path.pop(0)
        for mod in [m for m in sys.modules if m.split(".")[0] in ("smplify", "utils")]:
            sys.modules.pop(mod)
