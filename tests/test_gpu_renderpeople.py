"""The fit-check overlay kernel (csrc/overlay_kernels.hip through overlay.fit_overlays) bit for bit against the numpy restatement, and
the RenderPeople runner end to end on the MI355X against its stages called directly."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rp_cases as RC                                               # noqa: E402
from bodyfitting_amd import assets, overlay as OV, renderpeople as RP, synthetic as S   # noqa: E402

pytestmark = pytest.mark.gpu


def random_views(rng, n, H, W, nv):
    """n cameras looking at a body-sized cloud of nv points from 2.5-4 units, some of it off the image; plus points placed on the
    image's edges and corners (through the first camera)"""
    verts = rng.normal(0, 0.5, (nv, 3)).astype(np.float32)
    verts[:, 1] *= 2.0
    c2ws, Ks, images = [], [], []
    for _ in range(n):
        P = np.eye(4)
        P[:3, :3] = RC._rotation(rng)
        P[:3, 3] = rng.normal(0, 0.2, 3)
        P[2, 3] += rng.uniform(2.5, 4.0)
        c2ws.append(np.linalg.inv(P).astype(np.float32))
        f = W * rng.uniform(0.6, 1.4)
        Ks.append(np.array([[f, 0, W / 2 + rng.uniform(-5, 5)], [0, f * rng.uniform(0.98, 1.02), H / 2], [0, 0, 1]], np.float32))
        images.append(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    return images, verts, c2ws, Ks


def test_kernel_equals_numpy_on_random_bodies_and_cameras():
    rng = np.random.default_rng(0)
    for H, W, n, nv in ((64, 64, 3, 6890), (96, 128, 5, 10475), (480, 640, 2, 6890), (17, 23, 4, 300)):
        images, verts, c2ws, Ks = random_views(rng, n, H, W, nv)
        got = OV.fit_overlays(images, verts, c2ws, Ks, list(range(n)), list(range(n)))
        want = OV.fit_overlays_numpy(images, verts, c2ws, Ks, list(range(n)), list(range(n)))
        for k in range(n):
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{H}x{W} view {k}")
        # several views in one call equal one view at a time, in any frame order
        for k in range(n):
            np.testing.assert_array_equal(OV.check_smpl_fitting(images[k], verts, c2ws[k], Ks[k]), got[k])
        sel = OV.fit_overlays(images, verts, c2ws, Ks, [n - 1, 0], list(range(n)))
        np.testing.assert_array_equal(sel[0], got[n - 1])
        np.testing.assert_array_equal(sel[1], got[0])
        changed = [(g != im).any(axis=-1).mean() for g, im in zip(got, images)]
        assert all(0 < c < 1 for c in changed)


def test_kernel_on_edges_corners_and_the_camera_plane():
    for img, verts, c2w, K in RC.overlay_cases():
        np.testing.assert_array_equal(OV.check_smpl_fitting(img, verts, c2w, K), OV.check_smpl_fitting_numpy(img, verts, c2w, K))
    # points at exact pixels, just inside and just outside each edge, through the identity camera and K = I
    H, W = 31, 47
    xs = np.array([0, 0.0001, -0.0001, 1, W - 1, W - 0.001, W, W + 0.5, 17.5, -1e-30, np.nan, np.inf], np.float32)
    ys = np.array([0, H - 1, H - 0.001, H, -0.2, 5, 30.999, np.nan], np.float32)
    verts = np.array([(x, y, 1.0) for x in xs for y in ys], np.float32)
    img = np.full((H, W, 3), 7, np.uint8)
    got = OV.check_smpl_fitting(img, verts, np.eye(4, dtype=np.float32), np.eye(3, dtype=np.float32))
    np.testing.assert_array_equal(got, OV.check_smpl_fitting_numpy(img, verts, np.eye(4, dtype=np.float32), np.eye(3, dtype=np.float32)))
    assert (got[0, 0] == (0, 255, 0)).all() and (got[H - 1, W - 1] == (0, 255, 0)).all()
    # no vertices: the views come back as they were
    np.testing.assert_array_equal(OV.check_smpl_fitting(img, np.zeros((0, 3), np.float32), np.eye(4), np.eye(3)), img)
    with pytest.raises(ValueError):
        OV.check_smpl_fitting(img[:, :, :2], verts, np.eye(4), np.eye(3))


# ---------------------------------------------------------------------------------------------------------------------------------
# the runner end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def write_textured_obj(path, verts, faces, tex_seed):
    """an OBJ with a UV atlas and a PNG texture (mtllib beside it)"""
    from PIL import Image
    from texfit_cases import uv_atlas
    d, stem = os.path.dirname(path), os.path.splitext(os.path.basename(path))[0]
    uv, uvf = uv_atlas(len(faces), seed=tex_seed)
    yy, xx = np.mgrid[0:64, 0:64]
    tex = np.stack([(xx * 4 + tex_seed * 30) % 256, (yy * 4) % 256, ((xx + yy) * 2) % 256], -1).astype(np.uint8)
    Image.fromarray(tex).save(os.path.join(d, stem + ".png"))
    with open(os.path.join(d, stem + ".mtl"), "w") as fh:
        fh.write(f"newmtl material_0\nKd 1 1 1\nmap_Kd {stem}.png\n")
    lines = [f"mtllib {stem}.mtl"] + ["v %.6f %.6f %.6f" % tuple(p) for p in verts] + ["vt %.6f %.6f" % tuple(p) for p in uv]
    lines += ["usemtl material_0"] + [f"f {a + 1}/{ta + 1} {b + 1}/{tb + 1} {c + 1}/{tc + 1}" for (a, b, c), (ta, tb, tc) in zip(faces, uvf)]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


@pytest.fixture
def registered(monkeypatch):
    models = {t: S.make_model(t, seed=0) for t in ("smpl", "smplx")}
    monkeypatch.setattr(assets, "_MODELS", {(t, g): m for t, m in models.items() for g in ("neutral", "male", "female")})
    monkeypatch.setattr(assets, "_GMM", {"gmm": S.make_gmm(seed=0)})
    monkeypatch.setattr(assets, "_DEVICE_MODELS", {})
    sd, mean = S.make_hmr_weights(0)
    assets.register_hmr(sd, mean)
    assets.register_openpose(S.make_openpose_weights(0))
    assets.register_openpose_hand(S.make_openpose_hand_weights(0))
    yield models
    assets.register_hmr(None)
    assets.register_openpose(None)
    assets.register_openpose_hand(None)


def write_scans(root, model):
    """two textured scans of the synthetic body (the second moved and scaled) and a _30k decoy beside the first"""
    v = np.asarray(model["v_template"], np.float64)
    f = np.asarray(model["faces"], np.int64)
    for k, (subject, name) in enumerate((("s1", "s1.obj"), ("s2", "rp_s2_posed.obj"))):
        os.makedirs(os.path.join(root, subject), exist_ok=True)
        write_textured_obj(os.path.join(root, subject, name), v * (1 + 0.05 * k) + np.array([0.1 * k, 0, -0.05 * k]), f, k)
    write_textured_obj(os.path.join(root, "s1", "s1_30k.obj"), v[:, ::-1].copy(), f[:100], 7)


def write_smpl_uv(path, model):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    write_textured_obj(path, np.asarray(model["v_template"]), np.asarray(model["faces"], np.int64), 3)


@pytest.mark.parametrize("smpl_type,use_mask,tasks", [("smpl", True, ["openpose", "smplify", "output"]),
                                                      ("smplx", False, ["openpose", "smplify", "smpld", "texfit", "output"])])
def test_runner_end_to_end(tmp_path, registered, smpl_type, use_mask, tasks):
    from PIL import Image
    from bodyfitting_amd import openpose as O, openpose_hand as OH, texture_dropin as TD
    from bodyfitting_amd.body_fitting import BodyFitting
    from bodyfitting_amd.io import load_openpose
    model = registered[smpl_type]
    L = 64
    root, out = str(tmp_path / "scans"), str(tmp_path / "out")
    write_scans(root, model)
    uv = str(tmp_path / "uv" / "smpl_uv.obj")
    write_smpl_uv(uv, model)
    argv = ["--target_dir", root, "--output_dir", out, "--load_size", str(L), "--smpl_type", smpl_type, "--smpl_uv_dir", uv,
            "--tasks"] + tasks + (["--use_mask"] if use_mask else [])
    args = RP.config_parser().parse_args(argv)
    args.num_iters = 20
    args.texfit_iters, args.texfit_size = 12, 64
    r = RP.runner(args)
    assert sorted(r.subjects) == ["s1", "s2"] and not any("_30k" in m for m in r.meshfiles)
    r.run()

    # the file tree
    views = ["%02d.png" % i for i in range(8)]
    for s in ("s1", "s2"):
        sd = os.path.join(out, s)
        assert sorted(os.listdir(os.path.join(sd, "images"))) == views
        if use_mask:
            assert sorted(os.listdir(os.path.join(sd, "masks"))) == views
        else:
            assert not os.path.exists(os.path.join(sd, "masks"))
        assert sorted(os.listdir(os.path.join(sd, "openpose"))) == ["%02d_keypoints.json" % i for i in range(8)]
        want_smplify = {f"{smpl_type}.obj", f"{smpl_type}_parameter.npy", "smpl_fitting"} | ({f"{smpl_type}+d.obj"} if "smpld" in tasks else set())
        assert set(os.listdir(os.path.join(sd, "smplify"))) == want_smplify
        assert os.listdir(os.path.join(sd, "smplify", "smpl_fitting")) == ["00.png"]
        assert os.path.exists(os.path.join(sd, "texfit", "smpl.png")) == ("texfit" in tasks)
    assert sorted(os.listdir(os.path.join(out, "SMPL"))) == ["s1.npy", "s1.obj", "s2.npy", "s2.obj"]

    # the stages called directly on the first subject
    s, mesh = r.subjects[0], r.meshfiles[0]
    sd = os.path.join(out, s)
    images, masks, glRts, Ks = TD.render_texture_mesh(mesh, L, white_bkgd=True)
    for i in range(8):
        np.testing.assert_array_equal(np.asarray(Image.open(os.path.join(sd, "images", views[i]))), images[i])
        if use_mask:
            np.testing.assert_array_equal(np.asarray(Image.open(os.path.join(sd, "masks", views[i]))), masks[i])
    bgr = np.stack([im[:, :, ::-1] for im in images])
    body = O.OpenPose(device=0, max_batch=4, max_h=1024, max_w=1024)
    if smpl_type == "smplx":
        hand = OH.OpenPoseHand(device=0, max_hands=16, max_h=1024, max_w=1024)
        want_kp = [OH.select_person_entry(p) for p in OH.detect_people(body, hand, bgr)]
        hand.close()
    else:
        want_kp = [O.select_person(p) for p in body.pose25(bgr)]
    body.close()
    read = [load_openpose(os.path.join(sd, "openpose", "%02d_keypoints.json" % i)) for i in range(8)]
    for a, b in zip(read, want_kp):
        assert (a is None) == (b is None)
        if a is not None:
            assert set(a) == set(b)
            for key in a:
                np.testing.assert_array_equal(a[key], b[key])
    Rts = [np.linalg.inv(Rt).astype(np.float32) for Rt in glRts]
    Ks = [K.astype(np.float32) for K in Ks]
    fitter = BodyFitting(SimpleNamespace(**vars(args)))
    want = fitter(images, Rts, Ks, read, gender="neutral", keyframe=0, use_frames=list(range(8)), use_mask=use_mask,
                  masks=masks, mask_frames=list(range(8)), output_folder=str(tmp_path / "direct"), use_mesh=True, meshfile=mesh,
                  disp="smpld" in tasks)
    got = np.load(os.path.join(sd, "smplify", f"{smpl_type}_parameter.npy"), allow_pickle=True).item()
    assert set(got) == set(want)
    for key, v in want.items():
        if isinstance(v, np.ndarray):
            np.testing.assert_array_equal(np.asarray(got[key]), v, err_msg=key)
    np.testing.assert_array_equal(np.asarray(Image.open(os.path.join(sd, "smplify", "smpl_fitting", "00.png"))),
                                  OV.check_smpl_fitting_numpy(images[0], want["vertices"], Rts[0], Ks[0]))
    if "texfit" in tasks:
        tf = TD.TextureFitting(uv, render=True, debug=True, iter_num=12, render_img_size=64)
        tf(str(tmp_path / "direct_tex"), os.path.join(sd, "smplify", f"{smpl_type}+d.obj"), mesh)
        np.testing.assert_array_equal(np.asarray(Image.open(os.path.join(sd, "texfit", "smpl.png"))),
                                      np.asarray(Image.open(str(tmp_path / "direct_tex" / "smpl.png"))))

    # a second run: the images are read back (the renderer is asked for the cameras only) and detection is skipped
    calls = []
    r.render = lambda *a, **k: calls.append(k) or TD.render_texture_mesh(*a, **k)
    r.tasks = ["openpose"]
    r._openpose = SimpleNamespace(pose25=lambda *_: pytest.fail("detection ran although the JSONs exist"))
    OH_detect = OH.detect_people
    OH.detect_people = lambda *_: pytest.fail("detection ran although the JSONs exist")
    stamp = {p: os.path.getmtime(os.path.join(sd, "images", p)) for p in views}
    try:
        r.run()
    finally:
        OH.detect_people = OH_detect
        r._openpose = None
        r.close()
    assert calls == [{"pose_only": True}] * 2
    assert {p: os.path.getmtime(os.path.join(sd, "images", p)) for p in views} == stamp
