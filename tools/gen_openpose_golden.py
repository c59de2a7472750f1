"""Write tests/golden/openpose_synthetic.npz: the reference's own OpenPose body estimator (openpose/model.py bodypose_model and
openpose/body.py Body, imported unmodified) on the synthetic weights `synthetic.make_openpose_weights(0)`.

TEST INFRASTRUCTURE ONLY - runs where the reference checkout exists (--reference), never on the GPU box.  cv2 is absent, so it is
stubbed with a module whose only function is `resize`: bodyfitting_amd.openpose.cv2_resize, the numpy restatement of the INTER_CUBIC
calls body.py makes.  torchvision (imported, unused) is stubbed.

The golden holds
  - net_*:     a 128 x 32 synthetic BGR image and the network's stage-6 outputs at the first scale (body.py's 0.5 x 368 / H) in
               fp32 and fp64 (`model.double()`), in the layout [Hp/8, Wp/8, 57] (Mconv7_stage6_L1 0:38, Mconv7_stage6_L2 38:57).
               They pin tests/openpose_cases.bodypose_forward, the torch restatement the GPU tests compare all four scales with;
  - planted_*: the candidate / subset Body.__call__ returns, with the model stubbed, for tests/openpose_cases.planted_outputs
               (three synthetic people: a whole one, one without a neck - its face and arm subsets are merged (found == 2) - and
               a lone forearm whose subset is deleted).  The planted maps themselves are rebuilt by the tests.

Usage:  python tools/gen_openpose_golden.py [--reference /path/to/reference]
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET_HW = (128, 32)


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def install(reference):
    sys.path.insert(0, REPO)
    sys.path.insert(0, reference)
    from bodyfitting_amd import openpose as O
    stub("cv2", resize=O.cv2_resize, INTER_CUBIC=2)
    tv = stub("torchvision")
    tv.transforms = stub("torchvision.transforms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "openpose_synthetic.npz"))
    args = ap.parse_args()
    install(args.reference)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from openpose_cases import PLANT_HW, planted_outputs
    import torch
    torch.set_num_threads(max(1, os.cpu_count() or 1))
    from openpose.body import Body                              # the reference's modules, unmodified
    from bodyfitting_amd import openpose as O, synthetic as S

    sd = S.make_openpose_weights(0)
    image = S.make_hmr_images(7, (NET_HW,))[0][:, :, ::-1].copy()          # BGR
    out = {"net_image": image}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "body_pose_model.pth")
        torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, path)
        body = Body(path)
    model = body.model
    rec32, rec64 = [], []

    def recording(data):
        with torch.no_grad():
            l1, l2 = model(data)
            d1, d2 = model.double()(data.double())
            model.float()
        rec32.append(torch.cat([l1, l2], 1)[0].permute(1, 2, 0).numpy().astype(np.float32))
        rec64.append(torch.cat([d1, d2], 1)[0].permute(1, 2, 0).numpy().astype(np.float64))
        return l1, l2
    body.model = recording
    body(image)                                                # records each scale's outputs; the first is kept
    out["net_out32_0"], out["net_out64_0"] = rec32[0], rec64[0]

    planted = planted_outputs(*PLANT_HW)
    queue = list(planted)

    def stubbed(data):
        o = torch.from_numpy(queue.pop(0)).permute(2, 0, 1)[None]
        assert tuple(o.shape[2:]) == tuple(d // 8 for d in data.shape[2:])
        return o[:, :O.N_PAF], o[:, O.N_PAF:]
    body.model = stubbed
    cand, subset = body(np.zeros(PLANT_HW + (3,), np.uint8))
    out["planted_hw"] = np.array(PLANT_HW)
    out["planted_candidate"], out["planted_subset"] = np.asarray(cand, np.float64).reshape(-1, 4), subset
    print("planted: %d peaks, %d people; subset parts %s" % (len(cand), len(subset), subset[:, -1].tolist()))
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
