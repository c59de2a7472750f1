"""Host time per call of the geometry gradient of the stand-alone renderer (bf_nr_render_taped with a geometry tape,
bf_nr_tape_vertex_grad) through native.Nr*, next to the plain render and the texture gradient of the same render: 512 x 512 with
2 x 2 super-sampling, the SMPL topology (13,776 faces) and an 81,920-face scan, for a silhouette, a depth and a lit colour render.
Synthetic meshes, fill_back on, the Renderer's default light.  Every call ends in a stream synchronisation, so the host clock around
it covers its copies and kernels.  Device time of the kernels: run this under
`rocprofv3 --kernel-trace --stats -- python tools/bench_nr_vertex.py --iters 10` (a run of its own) and read bf_nr_*.
A record, not a gate: profiles/nr_vertex_grad_bench.md."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))
from bodyfitting_amd import native                     # noqa: E402
from bodyfitting_amd import texture_fitting as TF      # noqa: E402
from bench_nr_render import scan_mesh, smpl_mesh       # noqa: E402

MODES = {"silhouette": ("alpha",), "depth": ("depth",), "lit colour": ("rgb", "depth", "alpha")}


def median_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--scan-level", type=int, default=6)      # 81,920 faces
    a = ap.parse_args()
    ts, n = 4, a.image
    meshes = {"smpl": smpl_mesh(ts), "scan": scan_mesh(a.scan_level, ts)}
    center, dist = TF.scene_bound(meshes["scan"][0])
    pose = TF.gen_cam_views(center, 18, dist, gl=True)[2]
    cam = dict(K=np.array([[n, 0, n // 2], [0, n, n // 2], [0, 0, 1]], np.float32), R=pose[:3, :3], t=pose[:3, 3], orig_size=n)
    rng = np.random.default_rng(0)
    cot = dict(rgb=rng.standard_normal((3, n, n)).astype(np.float32), depth=rng.standard_normal((n, n)).astype(np.float32),
               alpha=rng.standard_normal((n, n)).astype(np.float32))
    r = native.NrRenderer(n, True, 0.0, 2 * dist)
    rows = {}
    for name, (v, f, tex) in meshes.items():
        m = native.NrMesh(r, v, f, ts, tex)
        for mode, want in MODES.items():
            g = [cot[k] if k in want else None for k in ("rgb", "depth", "alpha")]
            flags = native.TAPE_GEOMETRY | (native.TAPE_TEXTURES if "rgb" in want else 0)
            row = {"render_ms": median_ms(lambda: r.render(m, want=want, **cam), a.iters)}

            def taped():
                r.render_taped(m, want=want, flags=flags, **cam)[3].close()

            row["render_taped_ms"] = median_ms(taped, a.iters)
            tape = r.render_taped(m, want=want, flags=flags, **cam)[3]
            row["vertex_grad_ms"] = median_ms(lambda: tape.vertex_grad(*g), a.iters)
            if "rgb" in want:
                row["texture_grad_ms"] = median_ms(lambda: tape.texture_grad(cot["rgb"]), a.iters)
            gv = tape.vertex_grad(*g)[0]
            row["grad_verts_nonzero"] = int(np.count_nonzero(np.abs(gv).sum(1)))
            tape.close()
            m.set_vertices(v)                                                # (what a step of the caller's optimiser costs on top)
            row["set_vertices_ms"] = median_ms(lambda: m.set_vertices(v), a.iters)
            rows[f"{name} / {mode}"] = row
        m.close()
    # the gather's worst case: two faces over the whole image, each record's box ~ is^2 pixels on ONE wave
    quad_v = np.array([[-0.98, -0.97, 1.0], [0.99, -0.98, 1.1], [0.98, 0.97, 1.2], [-0.99, 0.98, 1.05]], np.float32)
    quad_f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    m = native.NrMesh(r, quad_v, quad_f, ts, rng.uniform(0, 1, (2, ts, ts, ts, 3)).astype(np.float32))
    for mode, want in MODES.items():
        g = [cot[k] if k in want else None for k in ("rgb", "depth", "alpha")]
        tape = r.render_taped(m, want=want, ndc=True, flags=native.TAPE_GEOMETRY)[3]
        rows[f"two faces over the image / {mode}"] = {"vertex_grad_ms": median_ms(lambda: tape.vertex_grad(*g, camera=False), a.iters)}
        tape.close()
    m.close()
    r.close()
    print(json.dumps({"metric": "nr_vertex_grad_host_ms_per_call", "image": n, "faces": {k: len(v[1]) for k, v in meshes.items()}, "iters": a.iters,
                      "rows": rows}))


if __name__ == "__main__":
    main()
