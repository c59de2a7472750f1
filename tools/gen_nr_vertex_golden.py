"""Generate tests/golden/nr_vertex_grad.npz, what tests/test_nr_vertex_oracle.py holds tests/nr_vertex_oracle.py to:

  (a) the four gradient cases the reference records in its own tests (thirdparty/neural_renderer/tests/test_rasterize_silhouettes.py
      and test_rasterize.py, test_backward_case1 / case2), as data: vertices, face, pixel, which loss, and `grad_ref`.  The numbers
      are read out of those files' literals at generation time; none of their text is kept here;
  (b) for ~100 random triangles (every angle >= 15 degrees) and tools/gen_nr_golden.py's dozen lights: a random cotangent on the
      light rows, pulled back to the corners by torch autograd through the reference's lighting.py in float64;
  (c) for two cameras and ~100 vertices: a random cotangent on the projected vertices, pulled back to `vertices`, `R` and `t`
      through the reference's projection.py in float64.

lighting.py and projection.py are pure torch: loaded by file path from the reference checkout, unmodified, run on the CPU.

    python tools/gen_nr_vertex_golden.py --reference DIR [--out tests/golden/nr_vertex_grad.npz]      (or BF_REFERENCE=DIR)
"""
import argparse
import ast
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_nr_golden import LIGHTS, load, mesh      # noqa: E402

TESTS = os.path.join('thirdparty', 'neural_renderer', 'tests')


def recorded_cases(ref):
    """the literals of test_backward_case1 / case2 in the two test files -> one dict of arrays per case"""
    cases = []
    for fname, colour in (('test_rasterize_silhouettes.py', 0), ('test_rasterize.py', 1)):
        tree = ast.parse(open(os.path.join(ref, TESTS, fname)).read())
        for fn in ast.walk(tree):
            if not (isinstance(fn, ast.FunctionDef) and fn.name in ('test_backward_case1', 'test_backward_case2')):
                continue
            vals = {}
            for node in fn.body:
                name = node.targets[0].id if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name) else None
                if name in ('vertices', 'faces', 'pxi', 'pyi', 'grad_ref') and name not in vals:      # (the first assignment: the literal)
                    vals[name] = ast.literal_eval(ast.unparse(node.value))
            # case 1's loss is |image - 1| at the pixel, case 2's |image|
            cases.append(dict(vertices=np.array(vals['vertices'], np.float32), faces=np.array(vals['faces'], np.int32),
                              pixel=np.array([vals['pyi'], vals['pxi']], np.int32), grad_ref=np.array(vals['grad_ref'], np.float32),
                              minus_one=np.int32(fn.name.endswith('1')), colour=np.int32(colour)))
    assert len(cases) == 4
    return cases


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('BF_REFERENCE'), required='BF_REFERENCE' not in os.environ,
                    help='the reference checkout (default: $BF_REFERENCE)')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'nr_vertex_grad.npz'))
    args = ap.parse_args()
    lighting = load(args.reference, 'lighting').lighting
    projection = load(args.reference, 'projection').projection
    out = {}
    cases = recorded_cases(args.reference)
    for key in cases[0]:
        out['case_' + key] = np.stack([c[key] for c in cases])

    # (b) light rows -> corners
    verts, faces = mesh(n_faces=100, seed=5)
    rng = np.random.default_rng(6)
    fw = torch.from_numpy(verts[faces].astype(np.float64))[None]
    ones = torch.ones(1, len(faces), 1, 1, 1, 3, dtype=torch.float64)
    cot, pulled = [], []
    for a, d, ca, cd, dr in LIGHTS:
        x = fw.clone().requires_grad_(True)
        rows = lighting(x, ones, a, d, torch.tensor(ca, dtype=torch.float64), torch.tensor(cd, dtype=torch.float64),
                        torch.tensor(dr, dtype=torch.float64))[0, :, 0, 0, 0]
        g = rng.standard_normal((len(faces), 3)).astype(np.float32).astype(np.float64)      # (lighting.py:33 sums into a float32 `light`: a cotangent that float32 holds passes it unchanged)
        if rows.requires_grad:
            rows.backward(torch.from_numpy(g))
        cot.append(g)
        pulled.append(np.zeros((len(faces), 3, 3)) if x.grad is None else x.grad[0].numpy())
    out.update(light_face_world=verts[faces], lights=np.array([[a, d, *ca, *cd, *dr] for a, d, ca, cd, dr in LIGHTS], np.float64),
               light_cotangent=np.stack(cot), light_corner_grad=np.stack(pulled))

    # (c) projected vertices -> vertices, R, t
    pverts = (rng.uniform(-1, 1, (100, 3)) * 0.8).astype(np.float32)
    cams, pc, gv, gR, gt = [], [], [], [], []
    for k in range(2):
        ang = 0.4 + 1.1 * k
        R = np.array([[np.cos(ang), 0, np.sin(ang)], [0.1 * np.sin(ang), 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        R = np.linalg.qr(R)[0].astype(np.float32)
        tv = np.array([0.1 * k, -0.2, 3.0 + k], np.float32)
        K = np.array([[300 + 50 * k, 7 * k, 128], [0, 310, 120 + 5 * k], [0, 0, 1]], np.float32)
        orig = 256 + 64 * k
        v = torch.from_numpy(pverts.astype(np.float64))[None].requires_grad_(True)
        Rt = torch.from_numpy(R.astype(np.float64))[None].requires_grad_(True)
        tt = torch.from_numpy(tv.astype(np.float64))[None, None].requires_grad_(True)
        pv = projection(v, torch.from_numpy(K.astype(np.float64))[None], Rt, tt, torch.zeros(1, 5, dtype=torch.float64), orig)
        g = rng.standard_normal((100, 3))
        pv.backward(torch.from_numpy(g)[None])
        cams.append(np.concatenate([K.ravel(), R.ravel(), tv, [orig]]).astype(np.float32))
        pc.append(g); gv.append(v.grad[0].numpy()); gR.append(Rt.grad[0].numpy()); gt.append(tt.grad[0, 0].numpy())
    out.update(proj_verts=pverts, proj_cams=np.stack(cams), proj_cotangent=np.stack(pc), proj_grad_verts=np.stack(gv), proj_grad_R=np.stack(gR),
               proj_grad_t=np.stack(gt))
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
