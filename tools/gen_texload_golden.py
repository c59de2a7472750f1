"""Generate tests/golden/nr_load_obj_textures.npz: what the reference's own neural_renderer/load_obj.py and utils/renderer.py
(imported unmodified from the reference checkout) return on synthetic OBJ / MTL / image fixtures.

Three substitutions make them run without CUDA:
  * neural_renderer.cuda.load_textures -> tests/texload_oracle.load_textures (the numpy restatement of load_textures_cuda_kernel.cu);
  * skimage.io.imread -> PIL, the way imageio's pillow plugin hands images to skimage (grey 2-D, RGBA 4 channels, palette -> RGB(A));
  * torch.Tensor.cuda -> the identity.
For render_texture_mesh(..., pose_only=True) the float32 arrays the reference takes to numpy come back as float64 arrays of the same
values: that is numpy 1's promotion of `height / 0.8` (a float32 scalar over a Python float gives float64), the environment the
reference was written for; numpy 2 would divide in float32.

The fixtures themselves (the OBJ / MTL text and the image bytes) are stored in the npz, so the tests rebuild the same files.

    python tools/gen_texload_golden.py [--reference DIR] [--out tests/golden/nr_load_obj_textures.npz]
"""
import argparse
import importlib.util
import io
import os
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

WRAPS = ('REPEAT', 'MIRRORED_REPEAT', 'CLAMP_TO_EDGE', 'CLAMP_TO_BORDER')


def png(a, mode=None, **info):
    from PIL import Image
    im = Image.fromarray(a) if mode is None else Image.fromarray(a).convert(mode)
    buf = io.BytesIO()
    im.save(buf, format='PNG', **info)
    return buf.getvalue()


def palette_png(rng):
    from PIL import Image
    im = Image.fromarray(rng.integers(0, 6, (4, 6), dtype=np.uint8), mode='P')
    im.putpalette(list(rng.integers(0, 256, 6 * 3, dtype=np.uint8).astype(int)))
    buf = io.BytesIO()
    im.save(buf, format='PNG')
    return buf.getvalue()


def mixed_fixture():
    """every `f` token form, polygons, faces before any usemtl, Kd-only / image / bare / Kd+image materials, grey / RGB / RGBA /
    palette images, two mtllib lines (the second wins), vt values outside [0, 1], negative, and exact integers"""
    rng = np.random.default_rng(7)
    files = {}
    files['rgb.png'] = png(rng.integers(0, 256, (5, 7, 3), dtype=np.uint8))
    files['grey.png'] = png(rng.integers(0, 256, (6, 4), dtype=np.uint8))
    files['rgba.png'] = png(rng.integers(0, 256, (5, 5, 4), dtype=np.uint8))
    files['pal.png'] = palette_png(rng)
    files['first.mtl'] = b"newmtl other\nKd 0.9 0.9 0.9\nmap_Kd rgb.png\n"
    files['second.mtl'] = (b"# colour before any newmtl: material ''\nKd 0.1 0.2 0.3\n\n"
                           b"newmtl kd_only\nKd 0.25 0.5 0.7\n"
                           b"newmtl with_rgb\nKd 0.3 0.3 0.3\nmap_Kd rgb.png\n"
                           b"newmtl with_grey\nmap_Kd grey.png extra tokens\n"
                           b"newmtl with_rgba\nmap_Kd rgba.png\n"
                           b"newmtl with_pal\nmap_Kd pal.png\n"
                           b"newmtl bare\nNs 10\n")
    v = rng.uniform(-1, 2, (9, 3))
    vt = [(0.1, 0.2), (0.9, 0.15), (0.5, 0.95), (1.3, -0.2), (-0.7, 2.4), (0.0, 1.0), (1.0, 0.0), (2.0, -1.0), (0.33, 0.66),
          (-2.25, 0.5), (0.75, 3.5), (0.999, 0.001)]
    lines = ["# synthetic texture fixture", "mtllib first.mtl"]
    lines += ["v %.6f %.6f %.6f" % tuple(p) for p in v]
    lines += ["vt %.6f %.6f" % p for p in vt]
    lines += ["f 1/1 2/2 3/3", "f 4/4/1 5/5/1 6/6/1 7/7/1"]              # before any usemtl: material ''
    lines += ["usemtl with_rgb", "f 1/1 2/2 3/3 4/4", "f 2/5/2 3/6/2 4/7/2 5/8/2 6/9/2", "f 7/10 8/11 9/12", "f 1/4 3/7 5/10"]
    lines += ["mtllib second.mtl"]
    lines += ["usemtl kd_only", "f 1//1 2//1 3//1", "f 4/1 5/2 6/3"]
    lines += ["usemtl with_grey", "f 1 2 3", "f 4/2 5//1 6/-1", "f 7/-2 8/-5 9/-11", "f 3/3 4/8 5/9 6/10"]
    lines += ["usemtl with_rgba", "f 1/6 2/7 3/8", "f 2/11 3/12 4/1 5/2"]
    lines += ["usemtl with_pal", "f 6/3 7/4 8/5", "f 9/6 1/7 2/8"]
    lines += ["usemtl bare", "f 3/9 4/10 5/11", "usemtl not_in_mtl", "f 6/12 7/1 8/2", "usemtl with_rgb", "f 9/3 8/5 7/7"]
    files['mixed.obj'] = ("\n".join(lines) + "\n").encode()
    return 'mixed.obj', files


def scan_fixture():
    """a closed blob with one UV triangle per face, an RGB texture and a Kd material for a band of faces"""
    from texfit_cases import icosphere, uv_atlas
    rng = np.random.default_rng(11)
    v, f = icosphere(1)
    v = v * np.array([0.45, 0.8, 0.4], np.float32) + np.array([0.1, 0.9, -0.05], np.float32)
    uv, uvf = uv_atlas(len(f), seed=3)
    files = {'skin.png': png(rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)),
             'scan.mtl': b"newmtl skin\nKd 0.6 0.5 0.4\nmap_Kd skin.png\nnewmtl cloth\nKd 0.2 0.3 0.8\n"}
    lines = ["mtllib scan.mtl"] + ["v %.6f %.6f %.6f" % tuple(p) for p in v] + ["vt %.6f %.6f" % tuple(p) for p in uv]
    lines.append("usemtl skin")
    for i, (a, b, c) in enumerate(f):
        if i == len(f) - 10:
            lines.append("usemtl cloth")
        ta, tb, tc = uvf[i] + 1
        lines.append(f"f {a + 1}/{ta}/1 {b + 1}/{tb}/1 {c + 1}/{tc}/1")
    files['scan.obj'] = ("\n".join(lines) + "\n").encode()
    return 'scan.obj', files


def pil_imread(path):
    """skimage.io.imread through imageio's pillow plugin"""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode == 'P':
            im = im.convert('RGBA' if 'transparency' in im.info else 'RGB')
        return np.asarray(im)


def import_reference(ref):
    import torch
    import texload_oracle as TO

    def load_textures_stub(image, faces, textures, is_update, wrapping, use_bilinear):
        out = TO.load_textures(image.numpy(), faces.numpy(), textures.numpy(), is_update.numpy(), wrapping, use_bilinear)
        textures.copy_(torch.from_numpy(out))
        return textures
    torch.Tensor.cuda = lambda self, *a, **k: self
    nr = types.ModuleType('neural_renderer'); nr.__path__ = []
    cuda = types.ModuleType('neural_renderer.cuda'); cuda.__path__ = []
    lt = types.ModuleType('neural_renderer.cuda.load_textures'); lt.load_textures = load_textures_stub
    nr.cuda, cuda.load_textures = cuda, lt
    sk = types.ModuleType('skimage'); sk.__path__ = []
    skio = types.ModuleType('skimage.io'); skio.imread = pil_imread; sk.io = skio
    sys.modules.update({'neural_renderer': nr, 'neural_renderer.cuda': cuda, 'neural_renderer.cuda.load_textures': lt,
                        'skimage': sk, 'skimage.io': skio})

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    lo = load('nr_load_obj', os.path.join(ref, 'thirdparty/neural_renderer/neural_renderer/load_obj.py'))
    nr.load_obj = lo.load_obj
    rend = load('ref_utils_renderer', os.path.join(ref, 'utils/renderer.py'))
    return lo, rend


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('BF_REFERENCE', '/root/reference'))
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden', 'nr_load_obj_textures.npz'))
    args = ap.parse_args()
    import torch
    lo, rend = import_reference(args.reference)
    out = {}
    modes = [(ts, w, b) for ts in (4,) for w in WRAPS for b in (True, False)]
    modes += [(2, 'REPEAT', True), (2, 'MIRRORED_REPEAT', False), (6, 'REPEAT', True), (6, 'CLAMP_TO_EDGE', False)]
    with tempfile.TemporaryDirectory() as tmp:
        for fx_name, (obj, files) in (('mixed', mixed_fixture()), ('scan', scan_fixture())):
            d = os.path.join(tmp, fx_name)
            os.makedirs(d)
            names = sorted(files)
            out[f'{fx_name}__obj'] = np.array(obj)
            out[f'{fx_name}__files'] = np.array(names)
            for n in names:
                with open(os.path.join(d, n), 'wb') as fh:
                    fh.write(files[n])
                out[f'{fx_name}__file__{n}'] = np.frombuffer(files[n], np.uint8)
            path = os.path.join(d, obj)
            for norm in (False, True):
                vv, ff = lo.load_obj(path, normalization=norm)
                out[f'{fx_name}__vertices_{"norm" if norm else "raw"}'] = vv.numpy()
                out[f'{fx_name}__faces'] = ff.numpy()
            for ts, w, b in modes:
                _, _, tex = lo.load_obj(path, normalization=False, texture_size=ts, load_texture=True, texture_wrapping=w, use_bilinear=b)
                out[f'{fx_name}__tex__{ts}_{w}_{int(b)}'] = tex.numpy()
            numpy_f32 = torch.Tensor.numpy
            torch.Tensor.numpy = lambda self, *a, **k: (numpy_f32(self).astype(np.float64) if self.dtype == torch.float32
                                                        else numpy_f32(self))
            try:
                for size in (512, 37):
                    poses, Ks = rend.render_texture_mesh(path, imgsize=size, pose_only=True)
                    out[f'{fx_name}__poses_{size}'] = np.stack(poses)
                    out[f'{fx_name}__Ks_{size}'] = np.stack(Ks)
            finally:
                torch.Tensor.numpy = numpy_f32
    np.savez_compressed(args.out, **out)
    print(args.out, sum(v.nbytes for v in out.values()), 'bytes uncompressed,', len(out), 'arrays')


if __name__ == '__main__':
    main()
