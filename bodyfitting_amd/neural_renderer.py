"""`import neural_renderer as nr` for callers of the reference (smplify/texture_fitting.py:8,240-275, utils/renderer.py, utils/io_utils.py,
test/correspondence.py): `Renderer`, `load_obj`, `save_obj` and `__version__` on the HIP path (libbodyfit's bf_nr_*; kernels:
csrc/nr_kernels.hip and the rasteriser shared with the fused texture-fitting loop).  `bodyfitting_amd/dropin_nr/neural_renderer`
re-exports this module under the reference's import name.

`Renderer` is thirdparty/neural_renderer/neural_renderer/renderer.py:11-346 for camera_mode='projection' with zero distortion:
fill-back, ambient + directional light, rgb / depth / alpha, and the gradient of any loss on the rgb image with respect to the
`textures` - what `loss.backward()` of the loop of texture_fitting.py:262-270 needs.  Every other name of the reference package
raises NotImplementedError on access.

The soft-edge gradient to `vertices`, `R` and `t` (backward_pixel_map, backward_depth_map, and the reverse of lighting.py and
projection.py; bf_nr_render_taped + bf_nr_tape_vertex_grad) is behind a switch that is off by default:
`GEOMETRY_GRAD`, read once at import from the environment variable BF_NR_GEOMETRY_GRAD ("1" = on), is what a new Renderer's
`geometry_grad` attribute starts as; set the attribute like the reference's callers set `renderer.image_size`.  Off, inputs that ask
for that gradient raise NotImplementedError instead of coming back detached.  On, `vertices`, `R`, `t` and `textures` that require
grad are the inputs of one autograd node per render (rgb, depth and alpha cotangents all count), a vertex tensor changed in place
(`optimizer.step()`) keeps its device mesh and only its positions go up again, and `K` that requires grad is still refused: K is
not differentiated.

Tensors in give float32 tensors out on the vertices' device; arrays in give arrays out.  The device meshes are remembered per
(vertices, faces) object and GPU - stamps and a table of _memo.py: a tensor by identity and version, an array by a digest, four at
a time - and a mesh's textures go up again only when their stamp no longer holds: in the reference's loop the scan's once, the
fitted ones once per `optimizer.step()`.  torch is imported on first use only.

The DEVICE route: when `vertices` - and `textures`, where the render uses them - are float32 tensors on
one GPU and `_autograd.route_for` says so, nothing above applies: the kernels read the tensors where they lie and write the images
and gradients into torch tensors on torch's current stream (bf_nr_render_dev, bf_nr_tape_*_dev); a mesh is remembered by its
faces, vertex count and GPU only, nothing is sent again, and `K`, `R`, `t` are each read by address (a float32 tensor on that GPU)
or taken by value (anything else).  DEVICE_ROUTE, read once from BF_NR_DEVICE_ROUTE ("0" = off; the default is
DEVICE_ROUTE_DEFAULT, on), switches it for this module; BF_TORCH_DEVICE_ROUTE=0 switches it off with every other drop-in's.
`render_texture` stays on the host route.
"""
from __future__ import annotations

import os

import numpy as np

from . import _autograd
from . import _memo
from . import native
from . import obj_textures as OT

__version__ = '1.1.3'            # thirdparty/neural_renderer/neural_renderer/__init__.py:14
name = 'neural_renderer_pytorch'

# the names of the reference package (__init__.py:1-12) that are not supplied
_NOT_BUILT = ("get_points_from_angles", "lighting", "look", "look_at", "Mesh", "perspective", "projection", "orthogonal", "rasterize_rgbad",
              "rasterize", "rasterize_silhouettes", "rasterize_depth", "Rasterize", "vertices_to_faces", "cuda")
_MESH_SLOTS = 4
GEOMETRY_GRAD = os.environ.get("BF_NR_GEOMETRY_GRAD", "") == "1"
# on: measured ahead of the parent commit's host route by more than both sides' ranges at the reference's loop size (profiles/nr_device_route.md)
DEVICE_ROUTE_DEFAULT = "1"
DEVICE_ROUTE = os.environ.get("BF_NR_DEVICE_ROUTE", DEVICE_ROUTE_DEFAULT).strip() != "0"
_NO_K_GRAD = ("neural_renderer.Renderer: K is not differentiated (geometry_grad covers `vertices`, `R` and `t`, not the intrinsics); "
              "detach K first")
_NO_VERTEX_GRAD = ("neural_renderer.Renderer: the soft-edge vertex gradient (backward_pixel_map, backward_depth_map of "
                   "cuda/rasterize_cuda_kernel.cu) is not built - only `textures` is differentiated; detach {what} first")


def __getattr__(attr):
    if attr in _NOT_BUILT:
        raise NotImplementedError(f"neural_renderer.{attr} is not supplied by bodyfitting_amd (Renderer, load_obj, save_obj and __version__ are)")
    raise AttributeError(f"module {__name__!r} has no attribute {attr!r}")


def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "_version")


def _host(x, dtype=np.float32):
    if x is None:
        return None
    if _is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=dtype)


def _gpu_of(x):
    return x.device.index or 0 if _is_tensor(x) and x.device.type == "cuda" else 0


def _readable_on(x, gpu):
    """can a kernel on GPU `gpu` read `x` where it lies: a float32 tensor there"""
    return _is_tensor(x) and x.device.type == "cuda" and (x.device.index or 0) == gpu and str(x.dtype) == "torch.float32" and hasattr(x, "data_ptr")


def _close_meshes(entry):
    for m in entry["meshes"]:
        m.close()


class _Tapes:
    """the tapes of one differentiable render (one per batch item), freed by the backward pass or with the graph"""

    def __init__(self):
        self.tapes = []

    def live(self):
        if not self.tapes:
            raise RuntimeError("neural_renderer.Renderer: this render's tape was freed by an earlier backward pass")
        return self.tapes

    def close(self):
        for tp in self.tapes:
            tp.close()
        self.tapes = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DeviceTapes(_Tapes):
    """... of the device route: each tape borrows one float32 tensor, held here and dropped with the tapes - torch's stream-ordered
    allocator owns its lifetime, so nothing waits"""

    def __init__(self):
        _Tapes.__init__(self)
        self.storage = []

    def close(self):
        _Tapes.close(self)
        self.storage = []


def _sum_in_item_order(rows):
    """((g0 + g1) + g2) ...: the order numpy's sum(0, dtype=float32) adds the rows of a small array in"""
    total = rows[0]
    for g in rows[1:]:
        total = total + g
    return total


class _DeviceRender:
    """the `device_route` object of _autograd.apply for one differentiable render: inputs (vertices, textures, R, t) in that order,
    None where one takes no gradient.  render(v, tex, R, t, flags, held) -> the outputs; it is the Renderer's closure"""

    def __init__(self, device, render, names, flags, ndc):
        self.device, self.render, self.names, self.flags, self.ndc = device, render, names, flags, ndc
        self.held = _DeviceTapes()

    def forward(self, tensors, stream):
        return self.render(tensors, self.flags, self.held, stream)

    def vjp(self, tensors, cotangents, want, stream):
        import torch
        tapes = self.held.live()
        v, tex, R, t = tensors
        g = dict(zip(self.names, cotangents))
        like = next(x for x in tensors if x is not None)
        grads = [None, None, None, None]
        B = len(tapes)
        if self.flags & native.TAPE_GEOMETRY and (want[0] or want[2] or want[3]):
            gv = torch.empty((B, tapes[0].n_verts, 3), dtype=torch.float32, device=like.device)
            gR = torch.empty((B, 3, 3), dtype=torch.float32, device=like.device) if R is not None else None
            gt = torch.empty((B, 3), dtype=torch.float32, device=like.device) if t is not None else None
            for b, tp in enumerate(tapes):
                cot = [0 if g.get(nm) is None else g[nm][b].data_ptr() for nm in ("rgb", "depth", "alpha")]
                tp.vertex_grad_dev(stream, gv[b].data_ptr(), cot[0], cot[1], cot[2], 0 if gR is None else gR[b].data_ptr(),
                                   0 if gt is None else gt[b].data_ptr())
            grads[0] = gv if v is not None else None
            for slot, x, each in ((2, R, gR), (3, t, gt)):
                if x is not None:                            # a camera shared by the batch takes the sum over its items
                    grads[slot] = each if x.numel() == each.numel() else _sum_in_item_order([each[b] for b in range(B)])
        if tex is not None and want[1]:
            if g.get("rgb") is None:
                grads[1] = torch.zeros_like(tex)
            else:
                grads[1] = torch.empty_like(tex)
                for b, tp in enumerate(tapes):
                    tp.texture_grad_dev(stream, g["rgb"][b].data_ptr(), grads[1][b].data_ptr())
        self.held.close()
        return grads


class Renderer:
    """renderer.py:11-63, the same constructor list and defaults"""

    def __init__(self, image_size=256, anti_aliasing=True, background_color=[0, 0, 0],
                 fill_back=True, camera_mode='projection',
                 K=None, R=None, t=None, dist_coeffs=None, orig_size=1024,
                 perspective=True, viewing_angle=30, camera_direction=[0, 0, 1],
                 near=0.1, far=100,
                 light_intensity_ambient=0.5, light_intensity_directional=0.5,
                 light_color_ambient=[1, 1, 1], light_color_directional=[1, 1, 1],
                 light_direction=[0, 1, 0]):
        if camera_mode in ('look', 'look_at', 'orthogonal'):
            raise NotImplementedError(f"neural_renderer.Renderer: camera_mode={camera_mode!r} is not built (only 'projection')")
        if camera_mode != 'projection':
            raise ValueError('Camera mode has to be one of projection, look or look_at')
        self.image_size, self.anti_aliasing, self.background_color, self.fill_back = image_size, anti_aliasing, background_color, fill_back
        self.camera_mode, self.K, self.R, self.t, self.orig_size = camera_mode, K, R, t, orig_size
        self.dist_coeffs = self._zero_distortion(dist_coeffs)
        self.perspective, self.viewing_angle, self.camera_direction = perspective, viewing_angle, camera_direction
        self.near, self.far = near, far
        self.light_intensity_ambient, self.light_intensity_directional = light_intensity_ambient, light_intensity_directional
        self.light_color_ambient, self.light_color_directional = light_color_ambient, light_color_directional
        self.light_direction = light_direction
        self.rasterizer_eps = 1e-3
        self.geometry_grad = GEOMETRY_GRAD     # not a constructor parameter (the list above is the reference's)
        self._native = {}           # gpu -> (configuration, native.NrRenderer)
        self._meshes = {}           # a table of _memo.py: key -> v, f, tex (last sent): stamps; gpu, ts, meshes [per batch item], closed when dropped

    # ---- nn.Module's surface the reference's callers touch ----
    def to(self, *args, **kwargs):
        return self

    def cuda(self, *args, **kwargs):
        return self

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)

    @staticmethod
    def _zero_distortion(dist_coeffs):
        if dist_coeffs is not None and np.any(_host(dist_coeffs) != 0):
            raise NotImplementedError("neural_renderer.Renderer: non-zero dist_coeffs are not built (projection.py:25-34)")
        return None

    def close(self):
        for key in list(self._meshes):
            _memo.drop(self._meshes, key, _close_meshes)
        for _, r in self._native.values():
            r.close()
        self._native = {}

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ---- device objects ----
    def _renderer_on(self, gpu):
        cfg = (int(self.image_size), bool(self.anti_aliasing), float(self.near), float(self.far), tuple(float(c) for c in _host(self.background_color).reshape(3)))
        have = self._native.get(gpu)
        if have is None or have[0] != cfg:
            if have is not None:                         # its meshes go with it
                for key in [k for k, e in self._meshes.items() if e["gpu"] == gpu]:
                    _memo.drop(self._meshes, key, _close_meshes)
                have[1].close()
            have = (cfg, native.NrRenderer(cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], device=gpu))
            self._native[gpu] = have
        have[1].set_light(self.light_intensity_ambient, self.light_intensity_directional, _host(self.light_color_ambient).reshape(3),
                          _host(self.light_color_directional).reshape(3), _host(self.light_direction).reshape(3))
        return have[1]

    def _meshes_for(self, r, gpu, vertices, faces, v_host, f_host, textures, tex_host):
        """the device meshes (one per batch item) of these vertices and faces, with `textures` (may be None) sent if they changed.
        v_host / f_host / tex_host: callables that give the host arrays, called only when something has to go up"""
        sv, sf = _memo.Stamp(vertices), _memo.Stamp(faces)
        key = (sv.part, sf.part, gpu)
        entry = _memo.find(self._meshes, key)
        ts = 0 if textures is None else int(textures.shape[2])
        usable = entry is not None and entry["f"].still(faces) and (textures is None or entry["ts"] == ts)
        if usable and self.geometry_grad and entry["v"].still(vertices, any_version=True) and not entry["v"].still(vertices):
            v = v_host()                                 # changed in place (optimizer.step()): the same topology, new positions
            for b, m in enumerate(entry["meshes"]):
                m.set_vertices(v[b])
            entry["v"] = sv
        if entry is not None and not (usable and entry["v"].still(vertices)):
            _memo.drop(self._meshes, key, _close_meshes)
            entry = None
        if entry is None:
            v, f = v_host(), f_host()
            _memo.room(self._meshes, _MESH_SLOTS, key, _close_meshes)          # (the oldest meshes go before the new ones are made)
            entry = {"v": sv, "f": sf, "gpu": gpu, "ts": ts, "tex": None, "meshes": [native.NrMesh(r, v[b], f[b], ts) for b in range(len(v))]}
            entry = _memo.store(self._meshes, _MESH_SLOTS, key, (), entry, closed=_close_meshes)
        if textures is not None and not (entry["tex"] is not None and entry["tex"].still(textures)):
            tex = tex_host()
            for b, m in enumerate(entry["meshes"]):
                m.set_textures(tex[b])
            entry["tex"] = _memo.Stamp(textures)
        return entry["meshes"]

    def _topology_meshes(self, r, gpu, faces, nv, ts, f_host):
        """the device route's meshes: the topology, texture size and tile lists of these faces - nothing of the vertices or textures,
        which the kernels read where the caller holds them.  Remembered by the faces' stamp, NV and GPU"""
        sf = _memo.Stamp(faces)
        key = (sf.part, int(nv), gpu, "device")
        entry = _memo.find(self._meshes, key)
        if entry is not None and not (entry["f"].still(faces) and (not ts or entry["ts"] == ts)):      # (_meshes_for's rule: a render without textures takes the mesh as it is)
            _memo.drop(self._meshes, key, _close_meshes)
            entry = None
        if entry is None:
            f = f_host()
            _memo.room(self._meshes, _MESH_SLOTS, key, _close_meshes)
            blank = np.zeros((int(nv), 3), np.float32)              # (never read: bf_nr_render_dev takes the caller's vertices)
            entry = {"v": None, "f": sf, "gpu": gpu, "ts": ts, "tex": None, "meshes": [native.NrMesh(r, blank, f[b], ts) for b in range(len(f))]}
            entry = _memo.store(self._meshes, _MESH_SLOTS, key, (), entry, closed=_close_meshes)
        return entry["meshes"]

    def _on_device_route(self, r, gpu, vertices, textures, differentiated=()):
        """_autograd.route_for's answer for this render: a renderer that offers the route, the switches, one HIP runtime, and float32
        tensors on the renderer's GPU - the vertices, the textures a render uses, and an `R` or `t` that takes a gradient"""
        offers = getattr(type(r), "offers_dev", None)
        if not DEVICE_ROUTE or offers is None or not offers():
            return False
        present = [x for x in (vertices, textures) if x is not None] + list(differentiated)
        return _autograd.takes_device_route(gpu, *present)

    def _render_device(self, r, gpu, vertices, faces, textures, K, R, t, orig_size, lightoff, want, fill_back, ndc, geometry, tex_in):
        """the device route of `_render`: see the module's text.  geometry: [vertices, R, t] that take a gradient (None: not);
        tex_in: the textures when they do"""
        import torch
        B, nv, n = int(vertices.shape[0]), int(vertices.shape[1]), int(self.image_size)
        ts = 0 if textures is None else int(textures.shape[2])
        names = [nm for nm in ("rgb", "depth", "alpha") if nm in want]
        device = vertices.device

        def camera_part(x, shape, nm):
            """-> (a contiguous [n, *shape] tensor of the GPU, None) to read by address, or (None, a host array) to take by value"""
            if _readable_on(x, gpu):
                x = x.detach().reshape((-1,) + shape).contiguous()
                count = int(x.shape[0])
            else:
                x = _host(x).reshape((-1,) + shape)
                count = len(x)
            if count not in (1, B):
                raise ValueError(f"{nm} must have batch size 1 or {B}, not {count}")
            return (x, None) if _is_tensor(x) else (None, x)

        fixed = None if ndc else [camera_part(K, (3, 3), "K"), camera_part(R, (3, 3), "R"), camera_part(t, (3,), "t")]

        def item(part, b, floats):
            tensor, array = part
            if tensor is not None:
                return tensor.data_ptr() + (b % int(tensor.shape[0])) * floats * 4
            return array[b % len(array)]

        def render(tensors, flags, held, stream):
            v, tex, R_in, t_in = tensors
            v = vertices.detach().contiguous() if v is None else v
            tex = (None if textures is None else textures.detach().contiguous()) if tex is None else tex
            cam = fixed
            if not ndc and (R_in is not None or t_in is not None):
                cam = list(fixed)
                if R_in is not None:
                    cam[1] = (R_in.reshape(-1, 3, 3), None)
                if t_in is not None:
                    cam[2] = (t_in.reshape(-1, 3), None)
            meshes = self._topology_meshes(r, gpu, faces, nv, ts, lambda: _host(faces, np.int32))
            out = {"rgb": torch.empty((B, 3, n, n), dtype=torch.float32, device=device) if "rgb" in want else None,
                   "depth": torch.empty((B, n, n), dtype=torch.float32, device=device) if "depth" in want else None,
                   "alpha": torch.empty((B, n, n), dtype=torch.float32, device=device) if "alpha" in want else None}
            lit = not lightoff and ("rgb" in want or bool(flags & native.TAPE_TEXTURES))
            for b, m in enumerate(meshes):
                args = dict(ndc=True) if ndc else dict(K=item(cam[0], b, 9), R=item(cam[1], b, 9), t=item(cam[2], b, 3), orig_size=float(orig_size))
                floats = r.tape_floats(m, fill_back, lit, flags, "rgb" in want)
                storage = torch.empty((floats,), dtype=torch.float32, device=device) if flags else None
                tp = r.render_dev(m, stream, v[b].data_ptr(), 0 if tex is None else tex[b].data_ptr(), fill_back=fill_back, lightoff=lightoff,
                                  rgb=0 if out["rgb"] is None else out["rgb"][b].data_ptr(),
                                  depth=0 if out["depth"] is None else out["depth"][b].data_ptr(),
                                  alpha=0 if out["alpha"] is None else out["alpha"][b].data_ptr(),
                                  flags=flags, storage=0 if storage is None else storage.data_ptr(), storage_floats=floats, **args)
                if flags:
                    held.tapes.append(tp)
                    held.storage.append(storage)
            return tuple(out[nm] for nm in names)

        if any(x is not None for x in geometry):
            flags = native.TAPE_GEOMETRY | (native.TAPE_TEXTURES if tex_in is not None else 0)
            route = _DeviceRender(gpu, render, names, flags, ndc)
            return _autograd.apply(None, None, [geometry[0], tex_in, geometry[1], geometry[2]], device_route=route)
        if tex_in is not None:
            route = _DeviceRender(gpu, render, names, native.TAPE_TEXTURES, ndc)
            return _autograd.apply(None, None, [None, tex_in, None, None], device_route=route)
        return render([None, None, None, None], 0, None, _autograd.stream_of(vertices))

    # ---- the one render path ----
    def _render(self, vertices, faces, textures, K, R, t, dist_coeffs, orig_size, lightoff, want, fill_back=None, ndc=False, like=None):
        self._zero_distortion(dist_coeffs)
        if self.camera_mode != 'projection':
            raise NotImplementedError(f"neural_renderer.Renderer: camera_mode={self.camera_mode!r} is not built (only 'projection')")
        like = vertices if like is None else like
        K, R, t = (self.K if K is None else K), (self.R if R is None else R), (self.t if t is None else t)
        orig_size = self.orig_size if orig_size is None else orig_size
        grad_on = False
        if any(_is_tensor(x) for x in (vertices, textures, K, R, t)):
            import torch
            grad_on = torch.is_grad_enabled()

        def wants_grad(x):
            return grad_on and _is_tensor(x) and x.requires_grad

        if wants_grad(K) and self.geometry_grad:
            raise NotImplementedError(_NO_K_GRAD)
        if not self.geometry_grad:
            for what, x in (("vertices", vertices), ("K", K), ("R", R), ("t", t)):
                if wants_grad(x):
                    raise NotImplementedError(_NO_VERTEX_GRAD.format(what=what))
        if getattr(vertices, "ndim", 0) != 3 or vertices.shape[2] != 3:
            raise ValueError(f"vertices must be [B, NV, 3], not {tuple(getattr(vertices, 'shape', ()))}")
        B = int(vertices.shape[0])
        if getattr(faces, "ndim", 0) != 3 or faces.shape[0] != B or faces.shape[2] != 3:
            raise ValueError(f"faces must be [B, NF, 3] with B = {B}, not {tuple(getattr(faces, 'shape', ()))}")
        if "rgb" in want:
            if textures is None:
                raise ValueError("textures are needed for an rgb render")
            sh = tuple(textures.shape)
            if len(sh) != 6 or sh[0] != B or sh[1] != faces.shape[1] or sh[5] != 3 or not (sh[2] == sh[3] == sh[4]):
                raise ValueError(f"textures must be [B, NF, ts, ts, ts, 3] with B = {B}, NF = {faces.shape[1]}, not {sh}")
        else:
            textures = None
        cams = None
        if not ndc and (K is None or R is None or t is None):
            raise ValueError("K, R and t are needed (as arguments or from the constructor) with camera_mode='projection'")
        gpu = _gpu_of(like)
        r = self._renderer_on(gpu)
        fill_back = self.fill_back if fill_back is None else fill_back
        geometry = [x if wants_grad(x) else None for x in (vertices, None if ndc else R, None if ndc else t)] if self.geometry_grad else [None] * 3
        if like is vertices:
            if self._on_device_route(r, gpu, vertices, textures, [x for x in geometry[1:] if x is not None]):
                return self._render_device(r, gpu, vertices, faces, textures, K, R, t, orig_size, lightoff, want, fill_back, ndc, geometry,
                                           textures if wants_grad(textures) else None)
        if not ndc:
            Kh, Rh, th = _host(K).reshape(-1, 3, 3), _host(R).reshape(-1, 3, 3), _host(t).reshape(-1, 3)
            for nm, a in (("K", Kh), ("R", Rh), ("t", th)):
                if len(a) not in (1, B):
                    raise ValueError(f"{nm} must have batch size 1 or {B}, not {len(a)}")
            cams = [(Kh[b % len(Kh)], Rh[b % len(Rh)], th[b % len(th)]) for b in range(B)]
        tex_ref = textures

        def run(tex_host, tape, flags=None):
            meshes = self._meshes_for(r, gpu, vertices, faces, lambda: _host(vertices), lambda: _host(faces, np.int32), tex_ref, tex_host)
            outs, tapes = [], []
            for b, m in enumerate(meshes):
                cam = dict(ndc=True) if ndc else dict(K=cams[b][0], R=cams[b][1], t=cams[b][2], orig_size=float(orig_size))
                if flags is None:
                    rgb, depth, alpha, tp = r.render(m, fill_back=fill_back, lightoff=lightoff, want=want, tape=tape, **cam)
                else:
                    rgb, depth, alpha, tp = r.render_taped(m, fill_back=fill_back, lightoff=lightoff, want=want, flags=flags, **cam)
                outs.append((rgb, depth, alpha))
                tapes.append(tp)
            stacked = tuple(np.stack([o[i] for o in outs]) for i, nm in enumerate(("rgb", "depth", "alpha")) if nm in want)
            return stacked, tapes

        if any(x is not None for x in geometry):
            held = _Tapes()
            tex_in = textures if wants_grad(textures) else None
            flags = native.TAPE_GEOMETRY | (native.TAPE_TEXTURES if tex_in is not None else 0)
            names = [nm for nm in ("rgb", "depth", "alpha") if nm in want]

            def forward(v_array, tex_array, R_array, t_array):
                out, held.tapes = run((lambda: tex_array) if tex_in is not None else (lambda: _host(tex_ref)), True, flags)
                return out

            def vjp(arrays, cotangents):
                held.live()
                g = dict(zip(names, cotangents))
                per_item = [tp.vertex_grad(*[None if g.get(nm) is None else g[nm][b] for nm in ("rgb", "depth", "alpha")], camera=not ndc)
                            for b, tp in enumerate(held.tapes)]
                grads = [np.stack([p[0] for p in per_item]), None, None, None]
                if tex_in is not None:
                    grads[1] = (np.zeros(arrays[1].shape, np.float32) if g.get("rgb") is None else
                                np.stack([tp.texture_grad(g["rgb"][b]) for b, tp in enumerate(held.tapes)]))
                for slot, i, x in ((2, 1, arrays[2]), (3, 2, arrays[3])):
                    if x is not None:                        # a camera shared by the batch takes the sum over its items
                        each = np.stack([p[i] for p in per_item])
                        grads[slot] = each if x.size == each.size else each.sum(0, dtype=np.float32)
                held.close()
                return grads

            out = _autograd.apply(forward, vjp, [geometry[0], tex_in, geometry[1], geometry[2]])
            out = tuple(o.to(like.device) for o in out) if _is_tensor(like) else out
        elif grad_on and _is_tensor(textures) and textures.requires_grad:
            held = _Tapes()

            def forward(tex_array):
                out, held.tapes = run(lambda: tex_array, True)
                return out

            def vjp(arrays, cotangents):
                held.live()
                g_rgb = cotangents[0] if "rgb" in want else None        # depth and alpha cotangents: zero
                if g_rgb is None:
                    grad = np.zeros(arrays[0].shape, np.float32)
                else:
                    grad = np.stack([tp.texture_grad(g_rgb[b]) for b, tp in enumerate(held.tapes)])
                held.close()
                return [grad]

            out = _autograd.apply(forward, vjp, [textures])
            out = tuple(o.to(like.device) for o in out) if _is_tensor(like) else out
        else:
            out, _ = run(lambda: _host(tex_ref), False)
            if _is_tensor(like):
                import torch
                out = tuple(torch.from_numpy(o).to(like.device) for o in out)
        return out

    # ---- the reference's methods ----
    def forward(self, vertices, faces, textures=None, mode=None, K=None, R=None, t=None, dist_coeffs=None, orig_size=None, lightoff=False):
        """renderer.py:65-80"""
        if mode is None:
            return self.render(vertices, faces, textures, K, R, t, dist_coeffs, orig_size, lightoff=lightoff)
        elif mode == 'rgb':
            return self.render_rgb(vertices, faces, textures, K, R, t, dist_coeffs, orig_size, lightoff=lightoff)
        elif mode == 'silhouettes':
            return self.render_silhouettes(vertices, faces, K, R, t, dist_coeffs, orig_size)
        elif mode == 'depth':
            return self.render_depth(vertices, faces, K, R, t, dist_coeffs, orig_size)
        raise ValueError("mode should be one of None, 'silhouettes' or 'depth'")

    def render_silhouettes(self, vertices, faces, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        """renderer.py:82-126 -> alpha [B, H, W]"""
        return self._render(vertices, faces, None, K, R, t, dist_coeffs, orig_size, True, ("alpha",))[0]

    def render_depth(self, vertices, faces, K=None, R=None, t=None, dist_coeffs=None, orig_size=None):
        """renderer.py:128-172 -> depth [B, H, W] (far where nothing is drawn)"""
        return self._render(vertices, faces, None, K, R, t, dist_coeffs, orig_size, True, ("depth",))[0]

    def render_rgb(self, vertices, faces, textures, K=None, R=None, t=None, dist_coeffs=None, orig_size=None, lightoff=False):
        """renderer.py:174-232 -> rgb [B, 3, H, W]"""
        return self._render(vertices, faces, textures, K, R, t, dist_coeffs, orig_size, lightoff, ("rgb",))[0]

    def render(self, vertices, faces, textures, K=None, R=None, t=None, dist_coeffs=None, orig_size=None, lightoff=False):
        """renderer.py:234-292 -> (rgb [B, 3, H, W], depth [B, H, W], alpha [B, H, W])"""
        return self._render(vertices, faces, textures, K, R, t, dist_coeffs, orig_size, lightoff, ("rgb", "depth", "alpha"))

    def render_texture(self, filename_obj, textures):
        """renderer.py:294-346: the UV-space image of `textures` [1, NF, ts, ts, ts, 3] over the OBJ's `vt` triangles, front and
        back, unlit -> (rgb [1, 3, H, W], depth [1, H, W])"""
        from .texture_dropin import _uv_obj
        uv, uv_faces = _uv_obj(filename_obj)
        verts = np.ascontiguousarray(np.concatenate([uv * 2.0 - 1.0, np.ones((len(uv), 1))], 1), dtype=np.float32)[None]      # :303-304
        return self._render(verts, np.ascontiguousarray(uv_faces, dtype=np.int32)[None], textures, None, None, None, None, None, True,
                            ("rgb", "depth"), fill_back=True, ndc=True, like=textures)


def _torch_device():
    import torch
    return torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")      # (the reference's .cuda(); host tensors where there is no GPU to hold them)


def load_obj(filename_obj, normalization=False, texture_size=4, load_texture=False, texture_wrapping='REPEAT', use_bilinear=True):
    """load_obj.py:98-152 through obj_textures.load_obj -> (vertices float32 [NV, 3], faces int32 [NF, 3]) or, with load_texture,
    (vertices, faces, textures float32 [NF, ts, ts, ts, 3]): tensors on the GPU as the reference returns them"""
    import torch
    out = OT.load_obj(filename_obj, normalization=normalization, texture_size=texture_size, load_texture=load_texture,
                      texture_wrapping=texture_wrapping, use_bilinear=use_bilinear)
    dev = _torch_device()
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in out)


def save_obj(filename, vertices, faces, textures=None):
    """save_obj.py:40-83 without textures: `v` and `f` lines as the reference writes them"""
    if textures is not None:
        raise NotImplementedError("neural_renderer.save_obj: the textured form (create_texture_image, save_obj.py:10-37,44-49) is not built")
    v, f = _host(vertices, np.float64), _host(faces, np.int64)
    assert v.ndim == 2
    assert f.ndim == 2
    with open(filename, 'w') as fh:
        fh.write('# %s\n' % os.path.basename(filename))
        fh.write('#\n')
        fh.write('\n')
        for vertex in v:
            fh.write('v %.8f %.8f %.8f\n' % (vertex[0], vertex[1], vertex[2]))
        fh.write('\n')
        for face in f:
            fh.write('f %d %d %d\n' % (face[0] + 1, face[1] + 1, face[2] + 1))
