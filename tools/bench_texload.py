"""Texture loading of a RenderPeople-sized scan, step by step: nr.load_obj(..., load_texture=True) on the HIP path
(bodyfitting_amd/obj_textures.py + bf_texfit_load_textures) and the 8-view render_texture_mesh of apps/rp_fitting.py's render_data.

A synthetic scan is written first: a latitude-longitude sphere of ~250k triangles with one `vt` per vertex, and an 8192^2 JPEG
written by PIL.  Reported separately: OBJ / MTL parsing, image decoding (PIL), upload, kernel (HIP events; bytes written per second
against the 8 TB/s HBM peak), download, and render_texture_mesh at 512 (8 views: whole call, and the renders alone).

    python tools/bench_texload.py [--faces 250000] [--image 8192] [--reps 5] [--dir DIR]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bodyfitting_amd import obj_textures as OT          # noqa: E402
from bodyfitting_amd import texture_dropin as TD        # noqa: E402
from bodyfitting_amd import texture_fitting as TF       # noqa: E402

HBM_PEAK = 8.0e12


def write_scan(d, n_faces, image_size):
    from PIL import Image
    n_lat = int(round(np.sqrt(n_faces / 4)))
    n_lon = 2 * n_lat
    th, ph = np.meshgrid(np.linspace(0.01, np.pi - 0.01, n_lat + 1), np.linspace(0, 2 * np.pi, n_lon + 1), indexing="ij")
    v = np.stack([0.4 * np.sin(th) * np.cos(ph), 0.9 * np.cos(th) + 0.9, 0.3 * np.sin(th) * np.sin(ph)], -1).reshape(-1, 3)
    uv = np.stack([ph / (2 * np.pi), 1 - th / np.pi], -1).reshape(-1, 2)
    idx = np.arange((n_lat + 1) * (n_lon + 1)).reshape(n_lat + 1, n_lon + 1) + 1
    a, b, c, e = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    tri = np.concatenate([np.stack([a, c, b], 1), np.stack([b, c, e], 1)])
    with open(os.path.join(d, "scan.obj"), "w") as fh:
        fh.write("mtllib scan.mtl\n")
        fh.write("".join("v %.6f %.6f %.6f\n" % tuple(p) for p in v))
        fh.write("".join("vt %.6f %.6f\n" % tuple(p) for p in uv))
        fh.write("usemtl skin\n")
        fh.write("".join(f"f {i}/{i} {j}/{j} {k}/{k}\n" for i, j, k in tri))
    with open(os.path.join(d, "scan.mtl"), "w") as fh:
        fh.write("newmtl skin\nKd 0.8 0.8 0.8\nmap_Kd scan.jpg\n")
    y, x = np.mgrid[0:image_size, 0:image_size].astype(np.float32) / image_size
    rng = np.random.default_rng(0)
    img = np.stack([128 + 100 * np.sin(40 * x), 128 + 100 * np.cos(33 * y), 128 + 60 * np.sin(25 * (x + y))], -1)
    img = np.clip(img + rng.normal(0, 8, img.shape[:2] + (1,)).astype(np.float32), 0, 255).astype(np.uint8)
    Image.fromarray(img).save(os.path.join(d, "scan.jpg"), quality=90)
    return os.path.join(d, "scan.obj"), len(tri)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=250_000)
    ap.add_argument("--image", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--render-size", type=int, default=512)
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    d = args.dir or tempfile.mkdtemp()
    t0 = time.perf_counter()
    path, nf = write_scan(d, args.faces, args.image)
    write_s = time.perf_counter() - t0
    ts = 4
    parse, decode, up, kern, down, total = [], [], [], [], [], []
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        lines = OT._read_lines(path)
        verts, faces = OT.load_vertices(path, lines), OT.load_faces(path, lines)
        tm = {}
        job = OT.parse_textures(path, OT.mtllib_files(path, lines)[-1], lines, timing=tm)
        t1 = time.perf_counter()
        tex = OT.run_load_textures(job, ts, timing=tm)
        t2 = time.perf_counter()
        if rep == 0:
            continue                                            # (first call: HIP initialisation)
        parse.append(t1 - t0 - tm["decode_s"]); decode.append(tm["decode_s"])
        up.append(tm["upload_ms"]); kern.append(tm["kernel_ms"]); down.append(tm["download_ms"]); total.append(t2 - t0)
    med = lambda a: float(np.median(a))                         # noqa: E731
    out_bytes = tex.nbytes
    t0 = time.perf_counter()
    imgs, masks, poses, Ks = TD.render_texture_mesh(path, imgsize=args.render_size)
    rtm_s = time.perf_counter() - t0
    center, dist = TD.scene_bound(verts)
    r = TF.Renderer(args.render_size, ts, near=0.0, far=2 * dist, background=(0, 0, 0), K=Ks[0], orig_size=args.render_size)
    r.set_mesh(r.TARGET, (verts, faces, tex))
    r.render_rgbd(r.TARGET, poses[0])
    t0 = time.perf_counter()
    for p in poses:
        r.render_rgbd(r.TARGET, p)
    render8_ms = (time.perf_counter() - t0) * 1e3
    r.close()
    res = dict(faces=nf, texture_size=ts, image=args.image, jpeg_bytes=os.path.getsize(os.path.join(d, "scan.jpg")), reps=args.reps,
               write_fixture_s=write_s, parse_s=med(parse), decode_s=med(decode), upload_ms=med(up), kernel_ms=med(kern),
               kernel_bytes_written=out_bytes, kernel_write_GBps=out_bytes / (med(kern) * 1e-3) / 1e9,
               kernel_write_frac_of_hbm_peak=out_bytes / (med(kern) * 1e-3) / HBM_PEAK, download_ms=med(down),
               load_obj_total_s=med(total), render_texture_mesh_512_s=rtm_s, render_8_views_512_ms=render8_ms,
               mask_coverage=float(np.mean([m.mean() / 255 for m in masks])))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
