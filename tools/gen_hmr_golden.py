"""Write tests/golden/hmr_synthetic.npz: the reference's own HMR (models/hmr.py, imported unmodified) and its post-processing
(utils/geometry.py rot6d_to_rotmat / convert_hom_to_angle) on the synthetic weights `synthetic.make_hmr_weights(0)` and three
synthetic images, in fp32 and in fp64 (`model.double()`).

TEST INFRASTRUCTURE ONLY - runs where the reference checkout exists (REFERENCE below), never on the GPU box.  The reference's
imports are stubbed as oracle/gen_golden.py stubs them; `HMR(Bottleneck, [3, 4, 6, 3], ...)` is built directly, so no ImageNet
weights are fetched.  cv2 is absent, so the 224 x 224 input is bodyfitting_amd.hmr.resize_224's restatement of the cv2.resize
call (stored as `resized`).

Usage:  python tools/gen_hmr_golden.py [--reference /path/to/reference]
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((512, 512), (480, 640), (224, 224))


def c2w_pair():
    """two camera-to-world matrices (a ring camera's rotation and a tilted one)"""
    def rot(axis, ang):
        axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    out = []
    for axis, ang, t in (((0, 1, 0), 2.1, (0.3, 0.1, 3.0)), ((1, 0.2, 0.1), -0.7, (-1.0, 0.5, 2.5))):
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = rot(axis, ang), t
        out.append(m.astype(np.float32))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "hmr_synthetic.npz"))
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    from oracle import gen_golden
    gen_golden.REFERENCE = args.reference
    gen_golden.install_reference_imports()
    import torch
    torch.set_num_threads(max(1, os.cpu_count() or 1))
    from models.hmr import HMR, Bottleneck                      # the reference's module, unmodified
    from utils.geometry import convert_hom_to_angle
    from bodyfitting_amd import hmr as H, synthetic as S
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import hmr_oracle

    sd, mean = S.make_hmr_weights(0)
    images = S.make_hmr_images(0, SIZES)
    c2ws = c2w_pair()[[0, 1, 0]]
    resized, x = hmr_oracle.network_input(images)
    with tempfile.TemporaryDirectory() as tmp:
        npz = os.path.join(tmp, "smpl_mean_params.npz")
        np.savez(npz, **mean)
        model = HMR(Bottleneck, [3, 4, 6, 3], npz)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    assert sorted(missing) == ["init_cam", "init_pose", "init_shape"] and not unexpected, (missing, unexpected)
    model.eval()
    out = {"resized": resized, "c2w": c2ws, "weights_digest": np.array(H.weights_digest(H.match_state(sd, "model_checkpoint.pt", mean)))}
    for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
        m = model.to(dtype)
        feats = {}
        h1 = m.avgpool.register_forward_hook(lambda mod, inp, o: feats.update(xf=o.reshape(o.shape[0], -1), l4=inp[0]))
        with torch.no_grad():
            rotmat, betas, cam = m(x.to(dtype))
        h1.remove()
        # the regressor's final 6D state, re-run outside the module (HMR.forward returns only its rotation matrices)
        state = dict(sd, init_pose=m.init_pose.numpy(), init_shape=m.init_shape.numpy(), init_cam=m.init_cam.numpy())
        pose6d = hmr_oracle.regressor(state, feats["xf"], dtype)[0]
        poses = []
        for i in range(len(images)):                            # run_hmr, one image at a time (body_fitting.py:70-73)
            r = rotmat[i:i + 1].clone()
            c = torch.from_numpy(c2ws[i]).to(dtype)
            r[0, 0] = c[:3, :3] @ r[0, 0]
            poses.append(convert_hom_to_angle(r.float() if dtype == torch.float32 else r, 1, "cpu").to(dtype))
        out.update({f"xf_{tag}": feats["xf"].numpy(), f"pose6d_{tag}": pose6d.detach().numpy(), f"betas_{tag}": betas.numpy(),
                    f"cam_{tag}": cam.numpy(), f"rotmat_{tag}": rotmat.numpy(), f"pose_{tag}": torch.cat(poses).numpy()})
        if tag == "32":
            out["layer4_positive"] = np.array(float((feats["l4"] > 0).double().mean()))
    frac = float(out["layer4_positive"])
    assert 0.2 <= frac <= 0.8, f"degenerate golden: {frac:.3f} of the layer-4 activations are positive"
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: layer-4 positive fraction {frac:.3f}; max|xf32 - xf64| "
          f"{np.abs(out['xf_32'] - out['xf_64']).max():.3e}; betas {out['betas_64'][0][:3]}")


if __name__ == "__main__":
    main()
