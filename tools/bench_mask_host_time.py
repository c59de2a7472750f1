#!/usr/bin/env python3
"""Host time per call of bf_batch_stage_masks and bf_batch_set_masks(..., None) on config 3's shapes (SMPL-X, 1 frame x 48 views,
8 mask views of 512 x 512): a record, not part of the bench.py contract (profiles/mask_arenas.md).  Timed from Python around the call,
a sync() after every call outside the timed region, 10 untimed calls first; prints one JSON line with every call's microseconds.
BODYFIT_LIB selects the library.
usage: python tools/bench_mask_host_time.py N_CALLS"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from bodyfitting_amd import native as N, synthetic as S, _lib  # noqa: E402

n_calls = int(sys.argv[1])
model, gmm = S.make_model("smplx", seed=0), S.make_gmm(seed=0)
dev = N.DeviceModel(model, gmm, device=0)
mask_frames = list(range(0, 48, 6))[:8]
prob = S.make_problem_smplx(model, frame=0, n_views=48, mask_frames=mask_frames)
c2w, K, kp, ndiv, betas, pose = N.pack_problem([prob])
b = N.FrameBatch(dev, 1, 48)
b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose)
masks = np.ascontiguousarray(np.array(prob["masks"])[None], dtype=np.uint8)
b.set_masks(masks, mask_frames, None)
b.fit(20); b.sync()
out = {"lib": _lib.LIB_PATH, "calls": n_calls}
for name, call in (("stage_masks", lambda: b.stage_masks(masks, mask_frames)), ("set_masks", lambda: b.set_masks(masks, mask_frames, None))):
    for _ in range(10):
        call(); b.sync()
    us = []
    for _ in range(n_calls):
        t0 = time.perf_counter()
        call()
        us.append((time.perf_counter() - t0) * 1e6)
        b.sync()
    out[name + "_us"] = [round(x, 1) for x in us]
b.fit(20); b.sync()
assert np.isfinite(b.get_params()).all()
b.close(); dev.close()
print(json.dumps(out))
