"""The RenderPeople runner (bodyfitting_amd/renderpeople.py) end to end on the GPU: wall time per stage and subject for N seeded
synthetic textured scans (the synthetic SMPL body, UV atlas, 256 x 256 texture) at load size 512, with synthetic model, HMR and
OpenPose weights and the reference's iteration counts (600 fit iterations, 200 texture-fit iterations at 512).  No dataset needed.
Record: profiles/rp_bench.md.

Stages, seconds per subject (the first subject pays for weight uploads and allocations and is reported apart):
  render   render_texture_mesh (OBJ + texture load, 8 renders)
  openpose body detection on the 8 views (+ JSON writes)
  hmr      BodyFitting.run_hmr
  fit      the rest of BodyFitting: scan fit + SMPL+D and its OBJ / npy writes
  overlay  the fit-check overlay kernel (host camera work included)
  texfit   TextureFitting without its PNG writes (200 iterations, 36 compare renders, the UV map)
  io       host PNG encode / decode: the runner's views, masks and overlay, and TextureFitting's debug / render / smpl.png images

Usage:  python tools/bench_rp.py [--subjects 3] [--out results.json]
"""
from __future__ import annotations

import argparse
import collections
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
STAGES = ("render", "openpose", "hmr", "fit", "overlay", "texfit", "io")


def write_textured_obj(path, verts, faces, seed, tex=256):
    from PIL import Image
    d, stem = os.path.dirname(path), os.path.splitext(os.path.basename(path))[0]
    n = len(faces)
    cols = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    cell = np.stack([i % cols, i // cols], -1) / cols
    tri = np.array([[0.1, 0.1], [0.9, 0.1], [0.1, 0.9]]) / cols
    uv = (cell[:, None, :] + tri[None]).reshape(-1, 2)
    yy, xx = np.mgrid[0:tex, 0:tex]
    img = np.stack([(xx + 40 * seed) % 256, yy % 256, (xx ^ yy) % 256], -1).astype(np.uint8)
    Image.fromarray(img).save(os.path.join(d, stem + ".png"))
    with open(os.path.join(d, stem + ".mtl"), "w") as fh:
        fh.write(f"newmtl material_0\nKd 1 1 1\nmap_Kd {stem}.png\n")
    lines = [f"mtllib {stem}.mtl"] + ["v %.6f %.6f %.6f" % tuple(p) for p in verts] + ["vt %.6f %.6f" % tuple(p) for p in uv]
    lines += ["usemtl material_0"] + [f"f {a + 1}/{3 * k + 1} {b + 1}/{3 * k + 2} {c + 1}/{3 * k + 3}" for k, (a, b, c) in enumerate(faces)]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subjects", type=int, default=3)
    ap.add_argument("--load_size", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from bodyfitting_amd import assets, renderpeople as RP, synthetic as S, texture_dropin as TD

    model = S.make_model("smpl", seed=0)
    for g in ("neutral", "male", "female"):
        assets._MODELS[("smpl", g)] = model
    assets._GMM["gmm"] = S.make_gmm(seed=0)
    sd, mean = S.make_hmr_weights(0)
    assets.register_hmr(sd, mean)
    assets.register_openpose(S.make_openpose_weights(0))

    T = collections.defaultdict(float)
    per_subject = []
    tmp = tempfile.mkdtemp(prefix="bench_rp_")
    root, out = os.path.join(tmp, "scans"), os.path.join(tmp, "out")
    v, f = np.asarray(model["v_template"], np.float64), np.asarray(model["faces"], np.int64)
    for k in range(args.subjects):
        os.makedirs(os.path.join(root, "subject%02d" % k))
        write_textured_obj(os.path.join(root, "subject%02d" % k, "scan.obj"), v * (1 + 0.02 * k), f, k)
    os.makedirs(os.path.join(tmp, "uv"))
    write_textured_obj(os.path.join(tmp, "uv", "smpl_uv.obj"), v, f, 9)

    def timed(name, fn):
        def w(*a, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                T[name] += time.perf_counter() - t0
        return w

    TD._imwrite = timed("io_tex", TD._imwrite)
    a = RP.config_parser().parse_args(["--target_dir", root, "--output_dir", out, "--load_size", str(args.load_size),
                                       "--smpl_uv_dir", os.path.join(tmp, "uv", "smpl_uv.obj")])
    r = RP.runner(a)
    r.render = timed("render", r.render)
    r.overlay = timed("overlay", r.overlay)
    r._map = timed("io_runner", r._map)
    r.bodyfitter.run_hmr = timed("hmr", r.bodyfitter.run_hmr)
    for name in ("render_data", "run_openpose", "run_smplify", "run_texfit", "run_output"):
        setattr(r, name, timed(name, getattr(r, name)))
    try:
        for subject, meshfile, gender in zip(r.subjects, r.meshfiles, r.genders):
            before = dict(T)
            t0 = time.perf_counter()
            data = r.render_data(subject, meshfile)
            r.run_openpose(subject, data)
            keypoints = r.read_openpose(subject)
            r.run_smplify(subject, data, keypoints, gender, meshfile)
            r.run_texfit(subject, meshfile)
            r.run_output(subject)
            total = time.perf_counter() - t0
            d = {k: T[k] - before.get(k, 0.0) for k in T}
            io_runner = d.get("io_runner", 0.0)
            row = dict(render=d["render"], openpose=d["run_openpose"], hmr=d["hmr"],
                       overlay=d["overlay"], texfit=d["run_texfit"] - d.get("io_tex", 0.0), io=io_runner + d.get("io_tex", 0.0))
            # run_smplify holds HMR, the fit, the overlay and the overlay PNG write (the last _map of the subject)
            overlay_png = io_runner - (d["render_data"] - d["render"])        # render_data's other time is its PNG writes
            row["fit"] = d["run_smplify"] - d["hmr"] - d["overlay"] - overlay_png
            row["total"] = total
            row["texfit_debug_pngs"] = d.get("io_tex", 0.0)
            per_subject.append({k: round(x, 4) for k, x in row.items()})
            print(json.dumps({"subject": subject, **per_subject[-1]}), flush=True)
    finally:
        r.close()
    steady = per_subject[1:] or per_subject
    mean = {k: round(float(np.mean([p[k] for p in steady])), 4) for k in steady[0]}
    share = {k: round(mean[k] / mean["total"], 3) for k in STAGES}
    result = dict(subjects=args.subjects, load_size=args.load_size, first=per_subject[0], steady_mean=mean, steady_share=share,
                  dominant=max(STAGES, key=lambda k: mean[k]))
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
