#!/usr/bin/env python3
"""Kid (11 betas, age='kid') against adult (10 betas) on one GPU (not part of the bench.py contract): the 1 frame x 48 views x
100 iteration fit, the 32- and 256-frame batch steps, and the final mesh of each on its own.  Device times from the library's HIP
events (FrameBatch.last_timing: fit_ms = the fit launch(es), mesh_ms = the final mesh - bf_mesh_multi_kernel<1, *> at one frame,
bf_mesh_batch32_kernel<*> at 32, pack_feat + pose-blend GEMM + bf_mesh_epilogue_batch_kernel<*> at 256 - total_ms = the step).
Synthetic data (bodyfitting_amd/synthetic.py, the kid template of synthetic.make_kid_template); the median of --reps repetitions
after one warm-up, one JSON object per line.   usage: python tools/bench_kid.py [--reps R]"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from bodyfitting_amd import model_files, native as N, synthetic as S   # noqa: E402


def step(dev, problems, iters, reps):
    c2w, K, kp, ndiv, betas, pose = N.pack_problem(problems)
    b = N.FrameBatch(dev, len(problems), c2w.shape[1])
    b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv)
    runs = []
    for r in range(reps + 1):
        b.set_init(betas, pose)
        b.fit(iters)
        b.get_params()
        if r:
            runs.append(b.last_timing())
    b.close()
    return {k: float(np.median([t[k] for t in runs])) for k in runs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100)
    a = ap.parse_args()
    adult, gmm = S.make_model("smpl", seed=0), S.make_gmm(seed=0)
    kid = model_files.kid_model(adult, S.make_kid_template(adult))
    folded = S.kid_problem_model(kid, 0.4)
    devs = {"adult": N.DeviceModel(adult, gmm, device=0), "kid": N.DeviceModel(kid, gmm, device=0)}
    probs = {"adult": [S.make_problem(adult, frame=f, n_views=48) for f in range(256)],
             "kid": [S.as_kid_problem(S.make_problem(folded, frame=f, n_views=48), 0.4) for f in range(256)]}
    for F in (1, 32, 256):
        row = {"frames": F, "views": 48, "iters": a.iters, "reps": a.reps}
        for age in ("adult", "kid"):
            t = step(devs[age], probs[age][:F], a.iters, a.reps if F < 256 else max(2, a.reps // 3))
            row[age] = {**{k: round(v, 4) for k, v in t.items()}, "fit_instance": devs[age].fit_instance,
                        "frames_per_s": round(F * 1000.0 / t["total_ms"], 1)}
        row["kid_over_adult"] = {k: round(row["kid"][k] / row["adult"][k], 3) for k in ("fit_ms", "mesh_ms", "total_ms") if row["adult"][k] > 0}
        print(json.dumps(row), flush=True)
    for d in devs.values():
        d.close()


if __name__ == "__main__":
    main()
