"""Generate tests/golden/nr_lighting.npz: what the reference's own neural_renderer/lighting.py, vertices_to_faces.py and
projection.py (pure torch; loaded by file path from the reference checkout, unmodified, run on the CPU) return for a small mesh
under a dozen light settings and two cameras.  tests/test_nr_dropin.py holds tests/nr_oracle.py's light and oracle/texfit_oracle.py's
projection to it.

The triangles have a smallest angle of at least 15 degrees, so no cross product cancels; the degenerate face the tests check
separately is not in here.

    python tools/gen_nr_golden.py [--reference DIR] [--out tests/golden/nr_lighting.npz]
"""
import argparse
import importlib.util
import os

import numpy as np

PKG = os.path.join('thirdparty', 'neural_renderer', 'neural_renderer')

LIGHTS = [  # ambient, directional, color_ambient, color_directional, direction
    (0.5, 0.5, (1, 1, 1), (1, 1, 1), (0, 1, 0)),                      # Renderer's defaults
    (1.0, 0.0, (1, 1, 1), (1, 1, 1), (0, 1, 0)),                      # the texture-fitting loop's
    (0.0, 1.0, (1, 1, 1), (1, 1, 1), (0, 0, -1)),
    (0.0, 0.0, (1, 1, 1), (1, 1, 1), (0, 1, 0)),
    (0.3, 0.8, (1.0, 0.9, 0.7), (0.6, 1.0, 0.8), (0.3, 0.8, -0.5)),   # not a unit vector, coloured
    (0.7, 0.3, (0.2, 0.4, 0.6), (1.0, 0.5, 0.25), (1, 0, 0)),
    (0.25, 0.75, (1, 1, 1), (1, 1, 1), (-0.57735, -0.57735, 0.57735)),
    (0.1, 1.5, (0.9, 0.9, 1.0), (1.0, 0.8, 0.6), (0.0, -1.0, 0.2)),
    (2.0, 0.5, (0.5, 0.5, 0.5), (0.1, 0.2, 0.3), (0.6, 0.0, 0.8)),
    (0.5, 0.5, (0, 0, 0), (1, 1, 1), (0.2, 0.3, 0.4)),
    (0.5, 0.5, (1, 1, 1), (0, 0, 0), (0, 1, 0)),
    (0.05, 0.95, (0.3, 0.6, 0.9), (0.9, 0.6, 0.3), (-0.8, 0.1, -0.6)),
]


def load(ref, name):
    path = os.path.join(ref, PKG, name + '.py')
    spec = importlib.util.spec_from_file_location('nr_ref_' + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def mesh(n_faces=160, seed=0, min_angle=15.0):
    """independent triangles (3 vertices each) around the origin with every angle >= min_angle degrees"""
    rng = np.random.default_rng(seed)
    tris = []
    while len(tris) < n_faces:
        tri = rng.uniform(-1, 1, (3, 3)) * rng.uniform(0.05, 1.0) + rng.uniform(-0.5, 0.5, 3)
        ok = True
        for k in range(3):
            a, b = tri[(k + 1) % 3] - tri[k], tri[(k + 2) % 3] - tri[k]
            ok &= np.degrees(np.arccos(np.clip(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)), -1, 1))) >= min_angle
        if ok:
            tris.append(tri)
    verts = np.concatenate(tris).astype(np.float32)
    faces = np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)
    faces[::3] = faces[::3, ::-1]                                     # both windings
    return verts, faces


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('BF_REFERENCE', '/root/reference'))
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'nr_lighting.npz'))
    args = ap.parse_args()
    lighting = load(args.reference, 'lighting').lighting
    vertices_to_faces = load(args.reference, 'vertices_to_faces').vertices_to_faces
    projection = load(args.reference, 'projection').projection
    verts, faces = mesh()
    rng = np.random.default_rng(1)
    textures = rng.uniform(0, 1, (len(faces), 2, 2, 2, 3)).astype(np.float32)
    v, f, t = torch.from_numpy(verts)[None], torch.from_numpy(faces)[None], torch.from_numpy(textures)[None]
    fw = vertices_to_faces(v, f)
    out = dict(verts=verts, faces=faces, textures=textures, face_world=fw[0].numpy(),
               lights=np.array([[a, d, *ca, *cd, *dr] for a, d, ca, cd, dr in LIGHTS], np.float64))
    lit, light = [], []
    for a, d, ca, cd, dr in LIGHTS:
        lit.append(lighting(fw, t, a, d, list(ca), list(cd), list(dr))[0].numpy())
        light.append(lighting(fw, torch.ones_like(t), a, d, list(ca), list(cd), list(dr))[0, :, 0, 0, 0].numpy())
    out.update(lit=np.stack(lit).astype(np.float32), light=np.stack(light).astype(np.float32))
    cams, proj = [], []
    for k in range(2):
        ang = 0.4 + 1.1 * k
        R = np.array([[np.cos(ang), 0, np.sin(ang)], [0.1 * np.sin(ang), 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        R = np.linalg.qr(R)[0].astype(np.float32)
        tv = np.array([0.1 * k, -0.2, 3.0 + k], np.float32)
        K = np.array([[300 + 50 * k, 0, 128], [0, 310, 120 + 5 * k], [0, 0, 1]], np.float32)
        orig = 256 + 64 * k
        pv = projection(v, torch.from_numpy(K)[None], torch.from_numpy(R)[None], torch.from_numpy(tv)[None, None], torch.zeros(1, 5), orig)
        cams.append(np.concatenate([K.ravel(), R.ravel(), tv, [orig]]).astype(np.float32))
        proj.append(pv[0].numpy())
    out.update(cams=np.stack(cams), projected=np.stack(proj).astype(np.float32))
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
