"""Write tests/golden/openpose_hand_synthetic.npz: the reference's own OpenPose hand estimator (openpose/model.py handpose_model,
openpose/hand.py Hand, openpose/util.py handDetect, imported unmodified) on the synthetic weights `synthetic.make_openpose_hand_weights(0)`.

TEST INFRASTRUCTURE ONLY - runs where the reference checkout exists (--reference), never on the GPU box.  Stubs:
  - cv2: a module whose only function is `resize`, bodyfitting_amd.openpose.cv2_resize (the numpy restatement of the INTER_CUBIC calls
    hand.py makes);
  - skimage (not installed): skimage.measure.label(binary, return_num=True, connectivity=2) is scipy.ndimage.label(binary,
    np.ones((3, 3))) with its count.  ASSUMED equal: both number the 8-connected components by the raster order of their first pixel
    (tests/test_openpose_hand_model.py holds bodyfitting_amd.openpose_hand.label8 to scipy).

The golden holds
  - net_*:     a 128 x 32 synthetic BGR crop and the network's outputs at the first scale (hand.py's 0.5 x 368 / h: 184 x 46, padded
               to 184 x 48) in fp32 and fp64 (`model.double()`), [Hp/8, Wp/8, 22].  They pin tests/openpose_hand_cases.handpose_forward,
               the torch restatement the GPU tests compare all four scales with;
  - planted_peaks: the [21, 2] array Hand.__call__ returns, with the model stubbed, for tests/openpose_hand_cases.planted_outputs on a
               184 x 184 crop: a single bump; a spike beside a wider blob of larger sum; two equal-sum blobs (the first label wins);
               an empty part; a component whose values are all negative (npmax lands on a zeroed pixel); bumps at the borders;
  - detect:    util.handDetect's [x, y, w, is_left] rows for tests/openpose_hand_cases.detect_inputs (both hands, left only, a box
               clamped at the corner, a box under 20 dropped, a person without arms).

Usage:  python tools/gen_openpose_hand_golden.py [--reference /path/to/reference]
"""
from __future__ import annotations

import argparse
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
    from scipy import ndimage
    from bodyfitting_amd import openpose as O
    stub("cv2", resize=O.cv2_resize, INTER_CUBIC=2)

    def label(binary, return_num=False, connectivity=None):
        assert connectivity == binary.ndim == 2
        lab, num = ndimage.label(binary, np.ones((3, 3), int))
        return (lab, num) if return_num else lab
    sk = stub("skimage")
    sk.measure = stub("skimage.measure", label=label)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "openpose_hand_synthetic.npz"))
    args = ap.parse_args()
    install(args.reference)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from openpose_hand_cases import NET_HW, PLANT_SIDE, DETECT_HW, planted_outputs, detect_inputs
    import torch
    torch.set_num_threads(max(1, os.cpu_count() or 1))
    from openpose.hand import Hand                              # the reference's modules, unmodified
    from openpose import util
    from bodyfitting_amd import synthetic as S

    sd = S.make_openpose_hand_weights(0)
    crop = S.make_hmr_images(9, (NET_HW,))[0][:, :, ::-1].copy()          # BGR
    out = {"net_crop": crop}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "hand_pose_model.pth")
        torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, path)
        hand = Hand(path)
    model = hand.model
    rec32, rec64 = [], []

    def recording(data):
        with torch.no_grad():
            o = model(data)
            d = model.double()(data.double())
            model.float()
        rec32.append(o[0].permute(1, 2, 0).numpy().astype(np.float32))
        rec64.append(d[0].permute(1, 2, 0).numpy().astype(np.float64))
        return o
    hand.model = recording
    hand(crop)                                                 # records each scale's outputs; the first is kept
    out["net_out32_0"], out["net_out64_0"] = rec32[0], rec64[0]

    queue = list(planted_outputs(PLANT_SIDE))

    def stubbed(data):
        o = torch.from_numpy(queue.pop(0)).permute(2, 0, 1)[None]
        assert tuple(o.shape[2:]) == tuple(d // 8 for d in data.shape[2:])
        return o
    hand.model = stubbed
    peaks = hand(np.zeros((PLANT_SIDE, PLANT_SIDE, 3), np.uint8))
    out["planted_peaks"] = np.asarray(peaks, np.int64)
    print("planted peaks:", peaks.tolist())

    cand, subset = detect_inputs()
    boxes = util.handDetect(cand, subset, np.zeros(DETECT_HW + (3,), np.uint8))
    out["detect"] = np.array([[x, y, w, int(left)] for x, y, w, left in boxes], np.int64).reshape(-1, 4)
    print("handDetect:", out["detect"].tolist())
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
