#!/usr/bin/env python3
"""One evaluation of the silhouette loss with its gradient, on one GPU: a record, not part of the bench.py contract.
Writes profiles/mask_loss_bench.md (or --out).  The problem: the 6,890-vertex model at its initial estimate, 8 views, 8 masks of
512 x 512, contours followed on the device.
  * `bf_silhouette_loss` (native.Silhouette.loss): value, view terms and dverts[6890,3] for vertices the caller holds - one upload,
    three launches, one read-back;
  * `bf_batch_mask_loss` (FrameBatch.mask_loss) on the same problem: the model's forward from the batch's parameters, then five launches
    - it does strictly more work.
Both are timed with the host clock around the call (each ends in a blocking copy back to the host), alternating, after --warmup
calls of each: median, minimum and the 10th / 90th percentile of --repeats calls.
usage: python tools/bench_mask_loss.py [--repeats R] [--warmup W] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from bodyfitting_amd import native as N, synthetic as S   # noqa: E402

N_VIEWS = 8


def problem():
    """-> (model, gmm, problem, world-space vertices float32[6890,3] at the initial estimate, w2c[8,4,4], K[8,3,3], masks uint8[8,512,512])"""
    import torch
    from oracle import smplify_oracle as O
    model, gmm = S.make_model("smpl", seed=0), S.make_gmm(seed=0)
    prob = S.make_problem(model, frame=0, n_views=N_VIEWS, mask_frames=list(range(N_VIEWS)))
    out = O.smpl_forward(O.to_torch_model(model, torch.float32), torch.tensor(prob["init_betas"]), torch.tensor(prob["init_pose"][:, :3]),
                         torch.tensor(prob["init_pose"][:, 3:]))
    verts = (out["vertices"][0] * prob.get("constant_scale", 0.3)).numpy().astype(np.float32)
    w2cs, Ks, _ = O.prepare_views(prob["c2ws"], prob["Ks"], prob["keypoints"], torch.float32)
    idx = [prob["use_frames"].index(f) for f in prob["mask_frames"]]
    return model, gmm, prob, verts, w2cs[idx].numpy(), Ks[idx].numpy(), np.array(prob["masks"])


def stats(ts):
    ts = np.asarray(ts) * 1e6
    return {"median_us": round(float(np.median(ts)), 1), "min_us": round(float(ts.min()), 1), "p10_us": round(float(np.percentile(ts, 10)), 1),
            "p90_us": round(float(np.percentile(ts, 90)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mask_loss_bench.md"))
    a = ap.parse_args()
    model, gmm, prob, verts, w2c, K, masks = problem()
    sil = N.Silhouette(masks > 128, None, device=0)
    dm = N.DeviceModel(model, gmm, device=0)
    c2w, Kb, kp, ndiv, betas, pose = N.pack_problem([prob])
    b = N.FrameBatch(dm, 1, N_VIEWS)
    b.set_cameras(c2w, Kb); b.set_keypoints(kp, ndiv); b.set_init(betas, pose)
    b.set_masks(masks[None], [prob["use_frames"].index(f) for f in prob["mask_frames"]], None)

    def alone():
        return sil.loss(verts, w2c, K, imsize=prob["imsize"])

    def batch():
        return b.mask_loss()

    for _ in range(a.warmup):
        value, _, grad = alone()
        bvalue, bgrad = batch()
    t_alone, t_batch = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter(); alone(); t1 = time.perf_counter(); batch(); t2 = time.perf_counter()
        t_alone.append(t1 - t0); t_batch.append(t2 - t1)
    row = {"contour_points": [len(c) for c in sil.contours()], "bf_silhouette_loss": stats(t_alone), "bf_batch_mask_loss": stats(t_batch),
           "values": [float(value), float(bvalue[0])], "repeats": a.repeats, "warmup": a.warmup}
    print(json.dumps(row), flush=True)
    sil.close(); b.close(); dm.close()
    with open(a.out, "w") as f:
        f.write("# One silhouette-loss evaluation with its gradient, one MI355X (tools/bench_mask_loss.py)\n\n")
        f.write(f"6,890 vertices (1,723 sampled), {N_VIEWS} views, masks 512 x 512, contours of {row['contour_points']} points followed on the device.\n"
                f"Host clock around the call (it ends in a blocking copy to the host), the two calls alternating, {a.repeats} calls of each after "
                f"{a.warmup}.  `bf_silhouette_loss`: the caller's vertices go up, three launches, loss + view terms + dverts[6890,3] come back.\n"
                "`bf_batch_mask_loss`: the model's forward from the batch's parameters, five launches, loss + dverts come back.  A record, not a gate.\n\n")
        f.write("| call | median, us | minimum, us | 10th - 90th percentile, us |\n|---|---|---|---|\n")
        for k in ("bf_silhouette_loss", "bf_batch_mask_loss"):
            s = row[k]
            f.write(f"| `{k}` | {s['median_us']} | {s['min_us']} | {s['p10_us']} - {s['p90_us']} |\n")
        f.write(f"\nValues: {row['values'][0]:.4f} (stand-alone, on torch's float32 vertices) and {row['values'][1]:.4f} (batch, on the HIP forward's).\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
