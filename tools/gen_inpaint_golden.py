"""Write tests/golden/inpaint_synthetic.npz: the reference's own texture inpainter (models/inpaint.py LBAMModel, Inpainter and
smplify/texture_fitting.py TextureFitting.inpaint, imported unmodified) on the synthetic weights `synthetic.make_lbam_weights(SEED)`,
written with torch.save to a temporary file (the weights themselves are not committed; the seed is).

TEST INFRASTRUCTURE ONLY - runs where the reference checkout exists (--reference), never on the GPU box.  Stubs:
  - torchvision: imported at module level by models/inpaint.py for the training-only VGG16 loss, never used at inference;
  - `.cuda()` of tensors and modules is the identity (the CPU stands in for the GPU);
  - `models`: a package over the reference's models/ directory whose `Inpainter` is models/inpaint.py's (models/__init__.py also
    imports HMR and SMPL, which need smplx);
  - cv2: drawContours, erode and dilate are bodyfitting_amd.inpaint's restatements (fill_triangle, erode, dilate); cv2 is not
    installed here, as tools/gen_openpose_hand_golden.py stubs cv2.resize.  drawContours records the triangles it is given;
  - neural_renderer, imageio: imported at module level by texture_fitting.py / utils/renderer.py, unused by TextureFitting.inpaint.

The golden holds, at 128 x 128:
  - image, masks [3] (full, scattered, large): tests/inpaint_cases.golden_image / masks (the empty mask returns the input);
  - out32 [3, H, W, 3]: Inpainter(...)(image, mask), float32 as the reference returns it;
  - out64_delta [3, H, W, 3]: float32(out64 - out32), out64 the same call with the network in float64 (`netG.double()` on a freshly
    loaded model, so its GaussActivation clamps run in float64 - what tests/inpaint_cases.lbam_forward(..., torch.float64)
    restates).  out32 + out64_delta in float64 is out64 to ~1e-14 (the file stays small);
  - tex_*: TextureFitting(uv_obj, inpaint=True).inpaint(texture) on tests/inpaint_cases.texture_image and uv_obj_text: tex_img, tex_uv
    (load_obj_uv * 128, float32), tex_sel (the faces drawContours filled, in order), tex_mask (the mask Inpainter received),
    tex_net32 / tex_net64_delta (the network's result on it, float32, and float64 as above) and tex_out (the final uint8 image).

Usage:  python tools/gen_inpaint_golden.py [--reference /path/to/reference]
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def install(reference, drawn):
    sys.path.insert(0, REPO)
    sys.path.insert(0, reference)
    import torch
    from bodyfitting_amd import inpaint as I
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    tv = stub("torchvision")
    tv.models = stub("torchvision.models")

    def draw_contours(image, contours, idx, color, thickness):
        assert idx == 0 and thickness == -1 and tuple(color) == (255, 255, 255) and len(contours) == 1
        tri = np.asarray(contours[0])
        assert tri.dtype == np.int32 and tri.shape == (3, 2)
        drawn.append(tri.copy())
        I.fill_triangle(image, tri)

    def morph(fn):
        def f(img, kernel, iterations=1):
            k = np.asarray(kernel)
            assert iterations == 1 and k.shape[0] == k.shape[1] and (k == 1).all()
            out = fn(img, k.shape[0])
            return out[:, :, 0] if out.ndim == 3 and out.shape[2] == 1 else out       # cv2 drops a singleton channel
        return f
    stub("cv2", drawContours=draw_contours, erode=morph(I.erode), dilate=morph(I.dilate))
    stub("neural_renderer")
    stub("imageio")
    models = stub("models")
    models.__path__ = [os.path.join(reference, "models")]
    from models.inpaint import Inpainter                   # the reference's file, unmodified
    models.Inpainter = Inpainter
    return Inpainter


def run64(Inpainter, path, image, mask):
    """Inpainter(path)(image, mask) with netG in float64 (inputs prepared in float32 as __call__ does, then widened)"""
    inp = Inpainter(path)
    net64 = inp.netG.double()
    inp.netG = lambda x, m: net64(x.double(), m.double())
    return inp(image, mask)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "inpaint_synthetic.npz"))
    args = ap.parse_args()
    drawn = []
    Inpainter = install(args.reference, drawn)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    import inpaint_cases as IC
    from bodyfitting_amd import inpaint as I, synthetic as S
    torch.set_num_threads(max(1, os.cpu_count() or 1))
    sd = S.make_lbam_weights(SEED)
    H, W = IC.GOLDEN_HW
    image = IC.golden_image(H, W)
    masks = {k: v for k, v in IC.masks(H, W).items() if k != "empty"}
    out = {"seed": np.int64(SEED), "image": image, "mask_names": np.array(list(masks)), "masks": np.stack(list(masks.values()))}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
        os.makedirs(os.path.join(tmp, "external"))
        path = os.path.join(tmp, "external", "LBAM_NoBN_ParisStreetView.pth")
        torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, path)
        ref = Inpainter(path)
        out["out32"] = np.stack([ref(image, m) for m in masks.values()]).astype(np.float32)
        out64 = np.stack([run64(Inpainter, path, image, m) for m in masks.values()]).astype(np.float64)
        out["out64_delta"] = (out64 - out["out32"]).astype(np.float32)

        obj_text, nf = IC.uv_obj_text()
        obj = os.path.join(tmp, "uv.obj")
        with open(obj, "w") as fh:
            fh.write(obj_text)
        tex = IC.texture_image(H, W)
        os.chdir(tmp)                                      # texture_fitting.py:189 opens external/... relative to the working directory
        try:
            from smplify.texture_fitting import TextureFitting, load_obj_uv
            tf = TextureFitting(obj, inpaint=True)
            seen = {}
            real = tf.inpainter

            def recording(img, mask):
                seen["mask"] = mask.copy()
                r = real(img, mask)
                seen["net32"] = r
                return r
            tf.inpainter = recording
            tex_out = tf.inpaint(tex.copy())
        finally:
            os.chdir(cwd)
        uv = load_obj_uv(obj) * H
        sel = I.select_faces(tex, uv)
        assert len(drawn) == sel.sum() and all((d == f.astype(np.int32)).all() for d, f in zip(drawn, uv[sel])), \
            "the restated face test selects other faces than the reference drew"
        out.update(tex_img=tex, tex_uv=uv.astype(np.float32), tex_sel=np.flatnonzero(sel).astype(np.int32), tex_mask=seen["mask"],
                   tex_net32=seen["net32"].astype(np.float32),
                   tex_net64_delta=(run64(Inpainter, path, tex, seen["mask"]).astype(np.float64) - seen["net32"]).astype(np.float32),
                   tex_out=tex_out)
        print(f"texture case: {nf} faces, {sel.sum()} selected, {int((seen['mask'][:, :, 0] > 0).sum())} hole pixels")
    for k, d in zip(masks, out["out64_delta"]):
        print(k, "max |fp32 - fp64|", float(np.abs(d).max()))
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
