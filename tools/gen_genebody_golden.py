"""Write tests/golden/genebody_prep.npz: the reference's own apps/genebody_fitting.py (imported unmodified) on the seeded synthetic
capture of tests/genebody_cases.py.

TEST INFRASTRUCTURE ONLY - runs where the reference checkout exists (--reference), never on the GPU box.  Stubbed:
  - cv2: `resize` is bodyfitting_amd.genebody.cv2_resize_linear behind OpenCV's (src, dsize, dst, fx, fy, interpolation) signature,
    and it asserts that the interpolation was left at its default - the app's INTER_CUBIC / INTER_NEAREST arrive as the positional dst;
  - imageio: imread / imwrite through PIL (what imageio uses for PNG);
  - smplify.body_fitting, tqdm, and utils.io_utils' heavy imports (scipy.misc.face, neural_renderer, torchvision, utils.imutils,
    utils.geometry).
`runner` is built with object.__new__ and its real get_views / get_sequence / get_data run.

The golden holds
  - data_<k>_*:  what get_data returns for genebody_cases.DATA_CASES[k] (images, masks, Ks, Rts, use_frames, mask_frames);
  - views_<subject>, seq_<subject>: get_views and get_sequence;
  - crop:        image_cropping on genebody_cases.crop_masks() (rebuilt from the seed by the tests);
  - defaults:    the parser's defaults as JSON.

Usage:  python tools/gen_genebody_golden.py [--reference /path/to/reference]
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def install(reference):
    sys.path.insert(0, REPO)
    sys.path.insert(0, reference)
    from PIL import Image
    from bodyfitting_amd.genebody import cv2_resize_linear

    def resize(src, dsize, dst=None, fx=None, fy=None, interpolation=None):
        assert interpolation is None and fx is None and fy is None, "the app was expected to leave the interpolation at its default"
        return cv2_resize_linear(src, dsize)

    stub("cv2", resize=resize, INTER_CUBIC=2, INTER_NEAREST=0, INTER_LINEAR=1)
    stub("imageio", imread=lambda p: np.asarray(Image.open(p)), imwrite=lambda p, a: Image.fromarray(np.asarray(a)).save(p))
    stub("tqdm", tqdm=lambda x, *a, **k: x)
    sm = stub("smplify")
    sm.__path__ = []
    sm.body_fitting = stub("smplify.body_fitting", BodyFitting=object)
    stub("scipy.misc", face=None)
    stub("neural_renderer")
    tv = stub("torchvision")
    tv.transforms = stub("torchvision.transforms", Normalize=object)
    # utils.io_utils imports these two for functions get_data never calls; utils.geometry pulls in utils.camera, whose ragged
    # np.array literals no longer import under numpy 2
    stub("utils.imutils", crop=None)
    stub("utils.geometry", rotation_matrix_to_angle_axis=None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "genebody_prep.npz"))
    args = ap.parse_args()
    install(args.reference)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import genebody_cases as G
    spec = importlib.util.spec_from_file_location("genebody_fitting", os.path.join(args.reference, "apps", "genebody_fitting.py"))
    app = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(app)                                   # the reference's module, unmodified
    from utils.io_utils import image_cropping

    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        root = G.write_capture(os.path.join(tmp, "capture"))
        annots = np.load(os.path.join(root, "annots.npy"), allow_pickle=True).item()["cams"]
        for subject in G.SUBJECTS:
            r = object.__new__(app.runner)
            r.subject = subject
            r.target_dir = os.path.join(root, subject)
            out[f"views_{subject}"] = np.asarray(r.get_views())
            out[f"seq_{subject}"] = np.asarray(r.get_sequence())
        for k, (subject, frame, use_mask, L) in enumerate(G.DATA_CASES):
            r = object.__new__(app.runner)
            r.subject, r.use_mask, r.load_size, r.annots = subject, use_mask, L, annots
            r.target_dir = os.path.join(root, subject)
            r.output_dir = os.path.join(tmp, "out", subject)
            r.views = r.get_views()
            r.mask_frames = [1, 7, 13, 19, 25, 31, 37, 43]          # set in __init__ (:88)
            images, masks, Ks, Rts, use_frames, mask_frames = r.get_data(frame)
            out[f"data_{k}_images"] = np.stack(images)
            out[f"data_{k}_masks"] = np.stack(masks) if masks else np.zeros((0, L, L), np.uint8)
            out[f"data_{k}_Ks"], out[f"data_{k}_Rts"] = np.stack(Ks), np.stack(Rts)
            out[f"data_{k}_use_frames"], out[f"data_{k}_mask_frames"] = np.asarray(use_frames), np.asarray(mask_frames, np.int64)
            print(f"case {k} {subject} frame {frame} use_mask {use_mask} L {L}: {len(use_frames)} views kept, masks {mask_frames}")
    out["crop"] = np.asarray([[int(x) for x in image_cropping(m)] for m in G.crop_masks()], np.int64)
    out["defaults"] = np.asarray(json.dumps(vars(app.config_parser().parse_args([])), sort_keys=True))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
