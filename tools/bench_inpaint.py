"""LBAM texture inpainting throughput on one GPU (synthetic weights `synthetic.make_lbam_weights(0)`; the real LBAM_NoBN weights
are not on hand - the work per layer does not depend on the values).

Prints one JSON line: the batch-1 latency of Inpainter(image, mask) at 512^2 and 1024^2 and of the whole TextureFitting.inpaint at
512^2 (hole mask of a synthetic UV layout, network, quantization, erode / dilate post-processing), host copies included; the
network's useful FLOPs and its lower bound at the 157.3 TF fp32-MFMA peak.  With --trace, the kernel_trace.csv or results .db of a
rocprofv3 `--kernel-trace --stats` run of this same command, it also prints per-layer device times of the last 512^2 network (the
GEMM launch plus its split-K reduction), TF/s and the share of the peak, and per-kernel totals - without touching the GPU.

Usage:  python tools/bench_inpaint.py [--reps 20]
        python tools/bench_inpaint.py --trace out/kernel_trace.csv
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from bodyfitting_amd import inpaint as I                                   # noqa: E402

PEAK_TF = 157.3


def layers(H, W):
    """the network's GEMM launches in the order inpaint_api.hip issues them -> [(name, useful FLOPs)]"""
    out = []
    for l in range(1, 7):
        out.append((f"rc{l}", 2 * (H >> l) * (W >> l) * I.REV[l] * 16 * I.REV[l - 1]))
    for l in range(1, 8):
        cm = 3 if l == 1 else I.ENC[l - 1]
        out.append((f"ec{l}", 2 * (H >> l) * (W >> l) * I.ENC[l] * 16 * (I.ENC[l - 1] + cm)))
    for t, (cin, cout) in enumerate(I.DEC, 1):
        out.append((f"dc{t}", 2 * (H >> (7 - t)) * (W >> (7 - t)) * cout * 4 * cin))
    return out


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def read_trace(path):
    """(name, start, end) of every dispatch of a rocprofv3 kernel trace, in start order"""
    if path.endswith(".db"):
        import sqlite3
        con = sqlite3.connect(path)
        rows = con.execute("select name, start, end from kernels order by start").fetchall()
        return [(str(n), float(s), float(e)) for n, s, e in rows]
    with open(path) as fh:
        rows = [(r["Kernel_Name"], float(r["Start_Timestamp"]), float(r["End_Timestamp"])) for r in csv.DictReader(fh)]
    return sorted(rows, key=lambda r: r[1])


def analyse(path, H=512, W=512):
    rows = [r for r in read_trace(path) if r[0].startswith("bf_ip_")]
    per_kernel = {}
    for n, s, e in rows:
        k = n.split("(")[0]
        per_kernel[k] = per_kernel.get(k, 0.0) + (e - s)
    # the last 512^2 network: its 20 GEMM launches end with the last bf_ip_dec64_kernel before a bf_ip_quantize_kernel (the texture
    # call), each GEMM followed by its reduction when split
    lay = layers(H, W)
    gemm = [i for i, r in enumerate(rows) if r[0].startswith(("bf_ip_rev", "bf_ip_enc", "bf_ip_dec"))]
    quant = [i for i, r in enumerate(rows) if r[0].startswith("bf_ip_quantize")]
    last = max(i for i in gemm if i < quant[-1]) if quant else gemm[-1]
    idx = gemm[gemm.index(last) - len(lay) + 1:gemm.index(last) + 1]
    report, total_ns = [], 0.0
    for (name, flops), i in zip(lay, idx):
        end = rows[i][2]
        if i + 1 < len(rows) and rows[i + 1][0].startswith("bf_ip_reduce"):
            end = rows[i + 1][2]
        ns = end - rows[i][1]
        total_ns += ns
        tf = flops / ns / 1e3
        report.append({"layer": name, "us": round(ns / 1e3, 1), "tflops": round(tf, 1), "of_peak": round(tf / PEAK_TF, 3)})
    return {"layers_512": report, "network_device_ms_512": round(total_ns / 1e6, 3),
            "kernel_totals_ms": {k: round(v / 1e6, 3) for k, v in sorted(per_kernel.items(), key=lambda kv: -kv[1])}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", default=None)
    a = ap.parse_args()
    if a.trace:
        print(json.dumps(analyse(a.trace)))
        return
    import inpaint_cases as IC
    from bodyfitting_amd import synthetic as S
    net = I.Inpainter(S.make_lbam_weights(0), device=0, max_batch=1)
    res = {"weights": "synthetic (make_lbam_weights(0))"}
    for side in (512, 1024):
        img = IC.golden_image(side, side)
        mask = IC.masks(side, side)["large"]
        flops = sum(f for _, f in layers(side, side))
        res[f"inpainter_ms_{side}"] = round(timed(lambda: net(img, mask), a.reps), 3)
        res[f"gflop_{side}"] = round(flops / 1e9, 1)
        res[f"lower_bound_ms_{side}"] = round(flops / (PEAK_TF * 1e12) * 1e3, 3)
    text, nf = IC.uv_obj_text(n=96, seed=11)
    from bodyfitting_amd import texture_dropin as TD
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "uv.obj")
        with open(path, "w") as fh:
            fh.write(text)
        uv = TD.load_obj_uv(path) * 512
    tex = IC.texture_image(512, 512)
    res["texture_inpaint_ms_512"] = round(timed(lambda: net.texture(tex, uv), a.reps), 3)
    res["texture_faces"] = nf
    res["selected_faces"] = int(net.select_faces(tex, uv).sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
