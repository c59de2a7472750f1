"""The RenderPeople runner's host side (bodyfitting_amd/renderpeople.py) and the overlay's numpy restatement (bodyfitting_amd/overlay.py)
against the reference's apps/rp_fitting.py and check_smpl_fitting, through the golden tools/gen_rp_golden.py wrote
(tests/golden/rp_runner.npz), without a GPU: the renderer, the detector, BodyFitting, TextureFitting and the overlay kernel are
replaced by stand-ins here; the device paths are tests/test_gpu_renderpeople.py's."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rp_cases as RC                                               # noqa: E402
from bodyfitting_amd import overlay as OV, renderpeople as RP       # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rp_runner.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


class Stubs:
    """the device objects of the runner, recording their calls"""

    def __init__(self):
        self.render_calls, self.fit_calls, self.tex_calls, self.overlay_calls, self.detected = [], [], [], [], []

    def render(self, file, imgsize=512, viewnum=8, white_bkgd=False, pose_only=False):
        self.render_calls.append(dict(file=file, imgsize=imgsize, viewnum=viewnum, white_bkgd=white_bkgd, pose_only=pose_only))
        return RC.fake_render(file, imgsize, viewnum, white_bkgd, pose_only)

    def make_fitter(self, smpl_type):
        stubs = self

        class Fitter:
            def __call__(self, images, c2ws, Ks, keypoints, **kw):
                stubs.fit_calls.append(dict(images=images, c2ws=c2ws, Ks=Ks, keypoints=keypoints, **kw))
                out = kw["output_folder"]
                os.makedirs(out, exist_ok=True)
                for name in (f"{smpl_type}.obj", f"{smpl_type}_parameter.npy"):
                    with open(os.path.join(out, name), "w") as f:
                        f.write(name)
                if kw.get("disp") and os.path.basename(os.path.dirname(out)) != "bob":
                    open(os.path.join(out, f"{smpl_type}+d.obj"), "w").close()
                rng = np.random.default_rng(len(stubs.fit_calls))
                return {"vertices": rng.normal(0, 1, (300, 3)).astype(np.float32)}
        return Fitter()

    def texfit(self, output_dir, smpld_dir, scan_dir):
        self.tex_calls.append(dict(output_dir=output_dir, smpld_dir=smpld_dir, scan_dir=scan_dir))

    def overlay(self, images, verts, c2ws, Ks, frames, use_frames):
        self.overlay_calls.append((frames, use_frames))
        return OV.fit_overlays_numpy(images, verts, c2ws, Ks, frames, use_frames)

    def pose25(self, bgr):
        self.detected.append(len(bgr))
        return [RC.people(np.asarray(im)[:, :, ::-1]) for im in bgr]


def make_runner(argv, stubs, smpl_type="smpl"):
    args = RP.config_parser().parse_args(argv)
    r = RP.runner(args, render=stubs.render, bodyfitter=stubs.make_fitter(smpl_type), texturefitter=stubs.texfit, overlay=stubs.overlay)
    r._openpose = stubs
    r._openpose_hand = object()
    return r


def files_under(d):
    return sorted(os.path.relpath(os.path.join(p, f), d) for p, _, fs in os.walk(d) for f in fs)


def test_defaults_and_subjects(golden, tmp_path):
    got = vars(RP.config_parser().parse_args([]))
    assert got.pop("device") == 0
    assert got == json.loads(str(golden["defaults"]))
    root = RC.write_tree(str(tmp_path / "scans"))
    r = make_runner(["--target_dir", root, "--output_dir", str(tmp_path / "out")], Stubs())
    assert sorted([s, os.path.relpath(m, root)] for s, m in zip(r.subjects, r.meshfiles)) == json.loads(str(golden["subjects"]))
    assert not any(m.endswith("_30k.obj") for m in r.meshfiles) and os.path.exists(os.path.join(root, *RC.DECOY))
    assert r.genders == ["neutral"] * 3
    r.close()


@pytest.mark.parametrize("use_mask", [0, 1])
def test_render_data_both_branches(golden, tmp_path, use_mask):
    root = RC.write_tree(str(tmp_path / "scans"))
    od = str(tmp_path / "out")
    s = Stubs()
    r = make_runner(["--target_dir", root, "--output_dir", od, "--load_size", str(RC.L)] + (["--use_mask"] if use_mask else []), s)
    mesh = os.path.join(root, "alice", "alice.obj")
    for branch in ("render", "reuse"):
        k = f"rd_{use_mask}_{branch}"
        s.render_calls.clear()
        images, masks, Ks, Rts, use_frames, mask_frames = r.render_data("alice", mesh)
        call = dict(s.render_calls[0])
        call["file"] = os.path.relpath(call["file"], root)
        assert call == json.loads(str(golden[k + "_call"]))
        assert call["pose_only"] == (branch == "reuse")
        np.testing.assert_array_equal(np.stack(images), golden[k + "_images"])
        if len(golden[k + "_masks"]):
            np.testing.assert_array_equal(np.stack(masks), golden[k + "_masks"])
        else:
            assert masks == []
        for name, arr in (("Ks", Ks), ("Rts", Rts)):
            assert all(a.dtype == np.float32 for a in arr)
            np.testing.assert_array_equal(np.stack(arr), golden[f"{k}_{name}"])
        assert [use_frames, mask_frames] == golden[k + "_frames"].tolist()
        assert files_under(od) == json.loads(str(golden[k + "_files"]))
    r.close()


def kp_array(kps):
    out = np.full((len(kps), 25, 3), np.nan)
    for i, k in enumerate(kps):
        if k is not None:
            out[i] = k["pose"]
    return out


@pytest.mark.parametrize("case", ["smpl", "smplx"])
def test_runner_against_the_reference(golden, tmp_path, case, monkeypatch, capfd):
    """whole runs: the JSON skip test (alice has 8 JSONs, bob 3), BodyFitting's arguments and keypoints, texfit only where +d.obj
    exists, the output copies under the subjects' names, one overlay per subject"""
    from bodyfitting_amd import openpose_hand as OH
    root = RC.write_tree(str(tmp_path / "scans"))
    od = str(tmp_path / "out")
    want = json.loads(str(golden[f"calls_{case}"]))
    if case == "smpl":
        extra, pre = ["--use_mask"], {"alice": 8, "bob": 3}
    else:
        extra, pre = ["--smpl_type", "smplx", "--tasks", "openpose", "smplify", "texfit", "output"], {}
    for subject, n in pre.items():
        d = os.path.join(od, subject, "openpose")
        os.makedirs(d, exist_ok=True)
        imgs = RC.fake_render(os.path.join(root, subject, dict(RC.SCANS)[subject]), RC.L, white_bkgd=True)[0]
        for i in range(n):
            RC.write_people_json(os.path.join(d, "%02d_keypoints.json" % i), RC.people(imgs[i]))
    s = Stubs()
    hands = []
    monkeypatch.setattr(OH, "detect_people", lambda body, hand, bgr: hands.append(len(bgr)) or
                        [[{"pose": p} for p in RC.people(np.asarray(im)[:, :, ::-1])] for im in bgr])
    r = make_runner(["--target_dir", root, "--output_dir", od, "--load_size", str(RC.L),
                     "--smpl_uv_dir", "uv/smpl_uv.obj"] + extra, s, smpl_type="smplx" if case == "smplx" else "smpl")
    r.run()
    assert "not produced" in capfd.readouterr().err
    # detection ran exactly where the reference ran openpose.bin, with --hand for SMPL-X
    detected_subjects = sorted(c.split("--image_dir <out>/")[1].split("/")[0] for c in want["_system"] if "openpose.bin" in c)
    assert (s.detected if case == "smpl" else hands) == [RC.VIEWS] * len(detected_subjects)
    assert all(("--hand" in c) == (case == "smplx") for c in want["_system"] if "openpose.bin" in c)
    assert len(s.fit_calls) == 3
    for call in s.fit_calls:
        subject = os.path.basename(os.path.dirname(call["output_folder"]))
        got = {k: os.path.relpath(v, od) if k == "output_folder" else os.path.relpath(v, root) if k == "meshfile" else v
               for k, v in call.items() if k not in ("images", "c2ws", "Ks", "keypoints", "masks")}
        assert got == want[subject]["fit"], subject
        assert len(call["images"]) == want[subject]["n_images"] and len(call["masks"] or []) == want[subject]["n_masks"]
        np.testing.assert_array_equal(kp_array(call["keypoints"]), golden[f"calls_{case}_keypoints_{subject}"])
        np.testing.assert_array_equal(np.stack(call["c2ws"]), golden[f"calls_{case}_Rts_{subject}"])
    # texfit: the reference's calls (bob's fit wrote no +d.obj; SMPL-X ran without smpld)
    want_tex = [c for c in want["_tex"] if "init" not in c]
    assert sorted([os.path.relpath(c["output_dir"], od), os.path.relpath(c["scan_dir"], root), os.path.relpath(c["smpld_dir"], od)]
                  for c in s.tex_calls) == sorted([c["output_dir"], c["scan_dir"], c["smpld_dir"]] for c in want_tex)
    # files: the reference's, and the runner's own: the copies under the subjects' names and smplify/smpl_fitting/00.png
    t = "smplx" if case == "smplx" else "smpl"
    ours = set(want["_files"]) | {f"SMPL/{s_}.{e}" for s_ in ("alice", "bob", "carol") for e in ("obj", "npy")}
    ours |= {f"{s_}/smplify/smpl_fitting/00.png" for s_ in ("alice", "bob", "carol")}
    assert set(files_under(od)) == ours
    for s_ in ("alice", "bob", "carol"):
        with open(os.path.join(od, "SMPL", f"{s_}.obj")) as f:
            assert f.read() == f"{t}.obj"
    assert [c[0] for c in s.overlay_calls] == [[0]] * 3
    r.close()


def test_genders_zip_stops_at_the_shorter_list(golden, tmp_path):
    root = RC.write_tree(str(tmp_path / "scans"))
    info = tmp_path / "info.csv"
    info.write_text("x,0\ny,1\n")
    s = Stubs()
    od = str(tmp_path / "out")
    r = make_runner(["--target_dir", root, "--output_dir", od, "--load_size", str(RC.L), "--info_dir", str(info), "--tasks", "smplify"],
                    s)
    for subject in r.subjects:
        os.makedirs(os.path.join(od, subject, "openpose"), exist_ok=True)
    r.run()
    want = json.loads(str(golden["genders"]))
    assert r.genders == want["genders"]
    assert [c["gender"] for c in s.fit_calls] == want["fits"]
    assert [os.path.basename(os.path.dirname(c["output_folder"])) for c in s.fit_calls] == r.subjects[:2]
    r.close()


def test_output_copies_and_reports_missing_sources(tmp_path, capfd):
    root = RC.write_tree(str(tmp_path / "scans"))
    od = tmp_path / "out"
    r = make_runner(["--target_dir", root, "--output_dir", str(od)], Stubs())
    (od / "alice" / "smplify").mkdir(parents=True)
    (od / "alice" / "smplify" / "smpl.obj").write_text("mesh")
    r.run_output("alice")
    assert (od / "SMPL" / "alice.obj").read_text() == "mesh"
    assert not (od / "SMPL" / "alice.npy").exists()
    err = capfd.readouterr().err
    assert err.count("not copied") == 1 and "smpl_parameter.npy" in err
    r.close()


def test_texfit_needs_the_smpld_mesh(tmp_path):
    root = RC.write_tree(str(tmp_path / "scans"))
    od = tmp_path / "out"
    s = Stubs()
    r = make_runner(["--target_dir", root, "--output_dir", str(od)], s)
    mesh = os.path.join(root, "alice", "alice.obj")
    r.run_texfit("alice", mesh)
    assert s.tex_calls == []
    (od / "alice" / "smplify").mkdir(parents=True)
    (od / "alice" / "smplify" / "smpl+d.obj").write_text("")
    r.run_texfit("alice", mesh)
    assert s.tex_calls == [dict(output_dir=str(od / "alice" / "texfit"), smpld_dir=str(od / "alice" / "smplify" / "smpl+d.obj"),
                                scan_dir=mesh)]
    r.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the overlay's numpy restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def test_overlay_numpy_equals_the_reference(golden):
    for k, (img, verts, c2w, K) in enumerate(RC.overlay_cases()):
        got = OV.check_smpl_fitting_numpy(img, verts, c2w, K)
        np.testing.assert_array_equal(got, golden[f"overlay_{k}"], err_msg=str(k))
        assert (got != img).any()


def identity_overlay(points, H=20, W=30):
    """the overlay of vertices (x, y, 1) through an identity camera and K = I: the projections are the float32 points themselves"""
    verts = np.asarray([(x, y, 1.0) for x, y in points], np.float32)
    return OV.check_smpl_fitting_numpy(np.zeros((H, W, 3), np.uint8), verts, np.eye(4, dtype=np.float32), np.eye(3, dtype=np.float32))


def green(img):
    return {(int(x), int(y)) for y, x in zip(*np.nonzero(img[:, :, 1] == 255))}


def test_overlay_known_answers():
    plus = lambda x, y: {(x, y), (x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)}
    img = identity_overlay([(5, 7)])
    assert green(img) == plus(5, 7)
    assert (img[:, :, 0] == 0).all() and (img[:, :, 2] == 0).all()
    assert green(identity_overlay([(5.99, 7.5)])) == plus(5, 7)                      # int() truncates
    assert green(identity_overlay([(-0.3, 4)])) == set()                             # dropped, although int(-0.3) == 0
    assert green(identity_overlay([(4, -0.3)])) == set()
    assert green(identity_overlay([(29.99, 3)])) == {(29, 3), (28, 3), (29, 2), (29, 4)}       # W - 0.01: kept, clipped
    assert green(identity_overlay([(30, 3), (3, 20)])) == set()                      # p == W, p == H: dropped
    assert green(identity_overlay([(0, 0)])) == {(0, 0), (1, 0), (0, 1)}             # corners
    assert green(identity_overlay([(29, 19)])) == {(29, 19), (28, 19), (29, 18)}
    assert green(identity_overlay([(0, 19)])) == {(0, 19), (1, 19), (0, 18)}
    assert green(identity_overlay([(29, 0)])) == {(29, 0), (28, 0), (29, 1)}
    # behind the camera (z < 0) still projects, as cv2.projectPoints does; z == 0 takes 1 / z = 1
    v = np.asarray([(-12.0, -9.0, -1.0), (0.5, 0.5, -1.0), (3.2, 4.7, 0.0)], np.float32)
    img = OV.check_smpl_fitting_numpy(np.zeros((20, 30, 3), np.uint8), v, np.eye(4, dtype=np.float32), np.eye(3, dtype=np.float32))
    assert green(img) == plus(12, 9) | plus(3, 4)


def test_rodrigues_round_trip_and_branches():
    rng = np.random.default_rng(4)
    for _ in range(20):
        R = RC._rotation(rng)
        for dt in (np.float32, np.float64):
            rv = OV.rodrigues_to_vector(R.astype(dt))
            assert rv.dtype == dt and rv.shape == (3, 1)
            np.testing.assert_allclose(OV.rodrigues_to_matrix(rv), R, atol=1e-6 if dt == np.float32 else 1e-12)
    assert not OV.rodrigues_to_vector(np.eye(3)).any()                                # s < 1e-5, c > 0
    for axis in np.eye(3):                                                              # s < 1e-5, c < 0: the half turns
        R = 2 * np.outer(axis, axis) - np.eye(3)
        np.testing.assert_allclose(np.abs(OV.rodrigues_to_vector(R).ravel()), np.pi * axis, atol=1e-12)
        np.testing.assert_allclose(OV.rodrigues_to_matrix(OV.rodrigues_to_vector(R)), R, atol=1e-12)
    assert not OV.rodrigues_to_vector(np.full((3, 3), 200.0)).any()                    # checkRange fails: zeros
    np.testing.assert_array_equal(OV.rodrigues_to_matrix(np.zeros(3)), np.eye(3))


def test_fit_overlays_numpy_picks_views_by_frame():
    cases = RC.overlay_cases()[:3]
    images, c2ws, Ks = [c[0] for c in cases[:1]] * 3, [c[2] for c in cases], [c[3] for c in cases]
    verts = cases[0][1]
    got = OV.fit_overlays_numpy(images, verts, c2ws, Ks, [7, 3], [3, 5, 7])
    np.testing.assert_array_equal(got[0], OV.check_smpl_fitting_numpy(images[2], verts, c2ws[2], Ks[2]))
    np.testing.assert_array_equal(got[1], OV.check_smpl_fitting_numpy(images[0], verts, c2ws[0], Ks[0]))
