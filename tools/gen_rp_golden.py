"""Write tests/golden/rp_runner.npz: the reference's own apps/rp_fitting.py and smplify/body_fitting.py's check_smpl_fitting (both
imported unmodified) on the seeded synthetic tree and overlay cases of tests/rp_cases.py.

TEST INFRASTRUCTURE ONLY - runs where the reference checkout exists (--reference), never on the GPU box.  Stubbed:
  - utils.renderer.render_texture_mesh: rp_cases.fake_render (seeded arrays), its calls recorded;
  - imageio: imread / imwrite through PIL (what imageio uses for PNG);
  - smplify.body_fitting.BodyFitting and smplify.texture_fitting.TextureFitting: recorders of their calls;
  - os.system: captured; an openpose.bin command writes rp_cases.people of every PNG it is pointed at, as openpose.bin would;
  - cv2: Rodrigues, projectPoints and circle are bodyfitting_amd.overlay's numpy restatement (circle: OpenCV's Circle, radius 1, fill);
  - tqdm, and utils.io_utils' heavy imports (scipy.misc.face, neural_renderer, torchvision, utils.imutils, utils.geometry).

The golden holds
  - defaults:                  the parser's defaults as JSON;
  - subjects:                  JSON set of (subject, mesh path relative to the tree) get_subjects finds;
  - rd_<m>_<branch>_*:         render_data's returns for use_mask m in the render and the reuse branch, its render call and the files;
  - calls_<case>:              JSON per subject: os.system commands, BodyFitting / TextureFitting call arguments (paths relative);
  - calls_<case>_keypoints_<subject>: the keypoints BodyFitting got, as [views, 25, 3] (NaN for a view without a person);
  - genders:                   the genders of the info csv case;
  - overlay_<k>:               check_smpl_fitting on rp_cases.overlay_cases()[k].

Usage:  python tools/gen_rp_golden.py [--reference /path/to/reference]
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import re
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = {"render": [], "fit": [], "tex": [], "system": []}


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def cv2_circle(img, center, radius, color, thickness=1, lineType=8, shift=0):
    """OpenCV's Circle(img, center, 1, color, fill) (drawing.cpp): the row cy from cx - 1 to cx + 1 clipped, (cx, cy -+ 1) when inside"""
    assert radius == 1 and thickness == -1 and lineType == 8 and shift == 0
    H, W = img.shape[:2]
    cx, cy = center
    for x in range(max(cx - 1, 0), min(cx + 1, W - 1) + 1):
        if 0 <= cy < H:
            img[cy, x] = color
    for y in (cy - 1, cy + 1):
        if 0 <= y < H and 0 <= cx < W:
            img[y, cx] = color
    return img


def install(reference):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, reference)
    from PIL import Image
    from bodyfitting_amd import overlay as OV
    import rp_cases as RC

    def projectPoints(pts, rvec, tvec, K, dist):
        assert not np.any(np.asarray(dist))
        p = OV.project_points(pts, OV.rodrigues_to_matrix(rvec), np.asarray(tvec, np.float64).reshape(3), np.asarray(K, np.float64))
        return p.reshape(-1, 1, 2), None

    stub("cv2", Rodrigues=lambda R: (OV.rodrigues_to_vector(R), None), projectPoints=projectPoints, circle=cv2_circle,
         INTER_CUBIC=2, INTER_NEAREST=0, INTER_LINEAR=1)
    stub("imageio", imread=lambda p: np.asarray(Image.open(p)), imwrite=lambda p, a: Image.fromarray(np.asarray(a)).save(p))
    stub("tqdm", tqdm=lambda x, *a, **k: x, trange=range)
    stub("scipy.misc", face=None)
    stub("neural_renderer")
    tv = stub("torchvision")
    tv.transforms = stub("torchvision.transforms", Normalize=object)
    stub("utils.imutils", crop=None)
    stub("utils.geometry", rotation_matrix_to_angle_axis=None, convert_hom_to_angle=None)
    stub("trimesh")
    stub("models", hmr=None, SMPL=None, Inpainter=None)

    def render(file, imgsize=512, viewnum=8, white_bkgd=False, pose_only=False):
        RECORD["render"].append(dict(file=file, imgsize=imgsize, viewnum=viewnum, white_bkgd=white_bkgd, pose_only=pose_only))
        return RC.fake_render(file, imgsize, viewnum, white_bkgd, pose_only)

    stub("utils.renderer", render_texture_mesh=render, gen_cam_views=None)
    stub("utils.cam_pose_vis", cam_pose_vis=None)
    sm = stub("smplify")
    sm.__path__ = []
    stub("smplify.smplify", SMPLify=None)

    # the reference's body_fitting.py itself, for check_smpl_fitting; the app then imports the recorder in its place
    spec = importlib.util.spec_from_file_location("ref_body_fitting", os.path.join(reference, "smplify", "body_fitting.py"))
    bf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bf)

    class BodyFitting:
        def __init__(self, options):
            self.options = options

        def __call__(self, images, c2ws, Ks, keypoints, **kw):
            RECORD["fit"].append(dict(images=images, c2ws=c2ws, Ks=Ks, keypoints=keypoints, **kw))
            out = kw["output_folder"]
            os.makedirs(out, exist_ok=True)
            for name in (f"{self.options.smpl_type}.obj", f"{self.options.smpl_type}_parameter.npy"):
                open(os.path.join(out, name), "w").close()
            if kw.get("disp") and os.path.basename(os.path.dirname(out)) != "bob":
                open(os.path.join(out, f"{self.options.smpl_type}+d.obj"), "w").close()

    class TextureFitting:
        def __init__(self, smpl_uv_dir, render=False, debug=None, **kw):
            RECORD["tex"].append(dict(init=dict(smpl_uv_dir=smpl_uv_dir, render=render, debug=bool(debug), **kw)))

        def __call__(self, output_dir, smpld_dir, scan_dir):
            RECORD["tex"].append(dict(output_dir=output_dir, smpld_dir=smpld_dir, scan_dir=scan_dir))

    stub("smplify.body_fitting", BodyFitting=BodyFitting, check_smpl_fitting=bf.check_smpl_fitting)
    stub("smplify.texture_fitting", TextureFitting=TextureFitting)

    def system(cmd):
        RECORD["system"].append(cmd)
        m = re.search(r"--image_dir (\S+)\s+--write_json (\S+)", cmd)
        if m:
            for name in sorted(os.listdir(m.group(1))):
                img = np.asarray(Image.open(os.path.join(m.group(1), name)))
                RC.write_people_json(os.path.join(m.group(2), os.path.splitext(name)[0] + "_keypoints.json"), RC.people(img))
        return 0

    os.system = system
    return bf


def load_app(reference):
    spec = importlib.util.spec_from_file_location("rp_fitting", os.path.join(reference, "apps", "rp_fitting.py"))
    app = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(app)                                   # the reference's module, unmodified
    return app


def rel(path, base):
    return os.path.relpath(path, base) if isinstance(path, str) and path.startswith(base) else path


def kp_array(kps):
    out = np.full((len(kps), 25, 3), np.nan)
    for i, k in enumerate(kps):
        if k is not None:
            out[i] = k["pose"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "rp_runner.npz"))
    args = ap.parse_args()
    bf = install(args.reference)
    import rp_cases as RC
    app = load_app(args.reference)
    out = {"defaults": np.asarray(json.dumps(vars(app.config_parser().parse_args([])), sort_keys=True))}

    with tempfile.TemporaryDirectory() as tmp:
        root = RC.write_tree(os.path.join(tmp, "scans"))
        base = ["--target_dir", root, "--load_size", str(RC.L), "--smpl_uv_dir", "uv/smpl_uv.obj"]
        a = app.config_parser().parse_args(base + ["--output_dir", os.path.join(tmp, "o0")])
        r = app.runner(a)
        out["subjects"] = np.asarray(json.dumps(sorted([s, rel(m, root)] for s, m in zip(r.subjects, r.meshfiles))))

        # render_data, both branches, with and without masks
        for m in (0, 1):
            od = os.path.join(tmp, f"rd{m}")
            a = app.config_parser().parse_args(base + ["--output_dir", od] + (["--use_mask"] if m else []))
            r = app.runner(a)
            mesh = os.path.join(root, "alice", "alice.obj")
            for branch in ("render", "reuse"):
                RECORD["render"].clear()
                images, masks, Ks, Rts, use_frames, mask_frames = r.render_data("alice", mesh)
                k = f"rd_{m}_{branch}"
                out[k + "_images"], out[k + "_Ks"], out[k + "_Rts"] = np.stack(images), np.stack(Ks), np.stack(Rts)
                out[k + "_masks"] = np.stack(masks) if masks else np.zeros((0, RC.L, RC.L), np.uint8)
                out[k + "_frames"] = np.asarray([use_frames, mask_frames])
                call = dict(RECORD["render"][0])
                call["file"] = rel(call["file"], root)
                out[k + "_call"] = np.asarray(json.dumps(call, sort_keys=True))
                out[k + "_files"] = np.asarray(json.dumps(sorted(os.path.relpath(os.path.join(p, f), od)
                                                                 for p, _, fs in os.walk(od) for f in fs)))

        # whole runs: (case, extra argv, pre-written JSON counts per subject)
        cases = {"smpl": (["--use_mask"], {"alice": 8, "bob": 3}),
                 "smplx": (["--smpl_type", "smplx", "--tasks", "openpose", "smplify", "texfit", "output"], {})}
        for case, (extra, pre) in cases.items():
            od = os.path.join(tmp, "run_" + case)
            for subject, n in pre.items():               # JSONs of an earlier run: 8 are enough to skip detection, 3 are not
                d = os.path.join(od, subject, "openpose")
                os.makedirs(d, exist_ok=True)
                imgs = RC.fake_render(os.path.join(root, subject, dict(RC.SCANS)[subject]), RC.L, white_bkgd=True)[0]
                for i in range(n):
                    RC.write_people_json(os.path.join(d, "%02d_keypoints.json" % i), RC.people(imgs[i]))
            for key in RECORD:
                RECORD[key].clear()
            a = app.config_parser().parse_args(base + ["--output_dir", od] + extra)
            r = app.runner(a)
            r.run()
            per = {}
            for call in RECORD["fit"]:
                subject = os.path.basename(os.path.dirname(call["output_folder"]))
                per[subject] = {"fit": {k: rel(v, od) if k == "output_folder" else rel(v, root) if k == "meshfile" else v
                                        for k, v in call.items() if k not in ("images", "c2ws", "Ks", "keypoints", "masks")},
                                "n_images": len(call["images"]), "n_masks": len(call["masks"] or [])}
                out[f"calls_{case}_keypoints_{subject}"] = kp_array(call["keypoints"])
                out[f"calls_{case}_Rts_{subject}"] = np.stack(call["c2ws"])
            per["_tex"] = [{k: rel(rel(v, od), root) for k, v in c.items()} if "init" not in c else c for c in RECORD["tex"]]
            per["_system"] = [re.sub(r"\s+", " ", c.replace(od, "<out>").replace(root, "<scans>")) for c in RECORD["system"]]
            per["_files"] = sorted(os.path.relpath(os.path.join(p, f), od) for p, _, fs in os.walk(od) for f in fs)
            out[f"calls_{case}"] = np.asarray(json.dumps(per, sort_keys=True))

        # the gender zip: a csv of two rows for three subjects
        info = os.path.join(tmp, "info.csv")
        with open(info, "w") as f:
            f.write("x,0\ny,1\n")
        od = os.path.join(tmp, "g")
        a = app.config_parser().parse_args(base + ["--output_dir", od, "--info_dir", info, "--tasks", "smplify"])
        r = app.runner(a)
        RECORD["fit"].clear()
        for subject in r.subjects:
            os.makedirs(os.path.join(od, subject, "openpose"), exist_ok=True)
        r.run()
        out["genders"] = np.asarray(json.dumps({"genders": r.genders, "fits": [c["gender"] for c in RECORD["fit"]]}))

    for k, (img, verts, c2w, K) in enumerate(RC.overlay_cases()):
        out[f"overlay_{k}"] = bf.check_smpl_fitting(img, verts, c2w, K)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
