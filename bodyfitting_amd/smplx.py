"""`smplx.create(model_type='smplx', ...)` of the reference (smplify/smplify.py:59-80) on the HIP path.

`SMPLX` takes smplx's forward keywords and returns `bodyfitting_amd.smpl.ModelOutput`.  `joints` are smplx's 144 joints (55
chain joints, 21 selector vertices, 51 face landmarks and - with `use_face_contour=True` - the 17 contour landmarks picked by
the neck chain's yaw), put through `joint_mapper` when one was given, as smplx does.

Two paths, as `bodyfitting_amd.smpl.SMPL` has them:
* numpy in -> numpy out, no gradient.
* torch tensors in -> torch tensors out on the inputs' device, differentiable w.r.t. betas, global_orient, body_pose, jaw_pose,
  leye_pose, reye_pose, left_hand_pose, right_hand_pose and expression through the HIP forward and its vector-Jacobian
  product (bf_smplx_forward / bf_smplx_vjp and their _expr variants), once.  The contour landmarks' row is an integer look-up:
  no gradient flows through the choice.  torch is imported on this path only.  float32 tensors on the model's GPU go into
  the kernels where they lie, on torch's current stream (bf_smplx_forward_dev / bf_smplx_vjp_dev: the device route of
  _autograd.py) - an argument not passed is a NULL pointer there, and `dyn_row` is then an int32 tensor on that GPU, not read
  back; everything else goes through host memory.

`num_betas` (10 .. 300) and `num_expression_coeffs` (0 .. 100) are smplx.create's: other counts than the registered model's own get
a device model of their own (`assets.get_device_model(..., num_betas=, num_expression_coeffs=)`: the registered dict's columns when
it holds them, else the model file's), `betas` is then [B, num_betas] and `expression` [B, num_expression_coeffs].  The betas beyond
the tenth ride with the expression coefficients around the model's passes (bf_model_set_shape_space).

`expression` [B, n_expression] is an input of its own on a device model with expression directions (a model file's shapedirs
columns behind the 10 shape directions, `DeviceModel.n_expression` of them): zero or not, it goes through the device and, as a
tensor that requires grad, gets its gradient.  `expression=None` is the call without it.  On a device model without directions
zeros pass and are ignored, anything else is refused.

What the device model cannot do is refused, not approximated: `use_pca=False`, another number of PCA components or expression
coefficients than the model's, `flat_hand_mean=True`, `age='kid'`, a dtype other than float32, an `expression` of another width
or dtype than the device model's (float32).
"""
from __future__ import annotations

import numpy as np

from . import _autograd, assets, layout
from .smpl import SMPL, ModelOutput, _is_tensor, address, require_elements

N_CONTOUR = 17          # the landmarks `use_face_contour` adds at the end of smplx's joints
_INPUTS = ("betas", "global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose")


def smpl_to_openpose(model_type="smplx", use_hands=True, use_face=True, use_face_contour=False, openpose_format="coco25"):
    return layout.smpl_to_openpose(model_type, use_hands=use_hands, use_face=use_face, use_face_contour=use_face_contour,
                                   openpose_format=openpose_format)


class JointMapper:
    """Picks `joint_maps` along the joint axis of [B, J, 3] tensors or arrays; `joint_maps=None` is the identity."""

    def __init__(self, joint_maps=None):
        self.joint_maps = None if joint_maps is None else np.asarray(joint_maps, dtype=np.int64)

    def __call__(self, joints, **kwargs):
        if self.joint_maps is None:
            return joints
        if _is_tensor(joints):
            import torch
            return torch.index_select(joints, 1, torch.as_tensor(self.joint_maps, dtype=torch.long, device=joints.device))
        return np.asarray(joints)[:, self.joint_maps]

    forward = __call__

    def to(self, *args, **kwargs):
        return self


def vertices2joints(J_regressor, vertices):
    """smplx.lbs.vertices2joints: J_regressor[J, V], vertices[B, V, 3] -> [B, J, 3]"""
    if _is_tensor(vertices) or _is_tensor(J_regressor):
        import torch
        return torch.einsum("bik,ji->bjk", vertices, J_regressor)
    return np.einsum("bik,ji->bjk", np.asarray(vertices), np.asarray(J_regressor))


def _is_float32(dtype):
    if dtype is None:
        return True
    name = getattr(dtype, "__name__", None) or str(dtype)
    return name.split(".")[-1] == "float32"


class SMPLX:
    def __init__(self, model_path=None, gender="neutral", joint_mapper=None, use_face_contour=False, use_pca=True, num_pca_comps=6,
                 flat_hand_mean=False, age="adult", dtype=None, batch_size=1, ext="npz", device=0, num_expression_coeffs=None, num_betas=10,
                 **kwargs):
        # (create_* and the initial-value keywords of smplx arrive in kwargs: arguments not passed to forward are zeros, smplx's
        #  zero-initialised parameters)
        if not use_pca:
            raise ValueError("use_pca=False: the device model takes the hands as PCA coefficients only")
        if flat_hand_mean:
            raise ValueError("flat_hand_mean=True: the device model's pose_mean carries the hand means")
        if age != "adult":
            raise ValueError(f"age={age!r}: there is no SMPL-X kid model on the device")
        if not _is_float32(dtype):
            raise ValueError(f"dtype={dtype}: the HIP model computes in float32")
        self.batch_size, self.gender = batch_size, gender
        self.joint_mapper, self.use_face_contour = joint_mapper, bool(use_face_contour)
        if int(num_betas) < 10:
            raise ValueError(f"num_betas={num_betas}: the device model carries the ten core betas; 10 .. 300 are supported")
        # (the default construction asks for the model as before; other counts get a device model of their own)
        space = {}
        if int(num_betas) != 10:
            space["num_betas"] = int(num_betas)
        if num_expression_coeffs is not None:
            space["num_expression_coeffs"] = int(num_expression_coeffs)
        self._dev = assets.get_device_model("smplx", gender, device, **space)
        if int(self._dev.n_betas) != 10 and "num_betas" not in space:       # a model registered with more: its first ten, as smplx cuts a file's
            self._dev = assets.get_device_model("smplx", gender, device, num_betas=10, **space)
        if int(self._dev.n_betas) != int(num_betas):
            raise ValueError(f"num_betas={num_betas}: the device model takes {self._dev.n_betas} betas")
        self.num_betas = int(num_betas)
        if int(num_pca_comps) != int(self._dev.n_hand_pca):
            raise ValueError(f"num_pca_comps={num_pca_comps}: the model has {self._dev.n_hand_pca} hand PCA components")
        self.num_pca_comps = int(num_pca_comps)
        # expression directions of the device model (0: none - zeros pass and are ignored, anything else is refused)
        self.num_expression_coeffs = int(getattr(self._dev, "n_expression", 0))
        if self.num_expression_coeffs and num_expression_coeffs is not None and int(num_expression_coeffs) != self.num_expression_coeffs:
            raise ValueError(f"num_expression_coeffs={num_expression_coeffs}: the model has {self.num_expression_coeffs} expression directions")
        self.faces = np.asarray(assets.get_model("smplx", gender)["faces"])
        self.dyn_row = None             # the contour-table rows of the last forward

    def _batch(self, given):
        for name, width in (("betas", self._dev.n_betas), ("global_orient", 3), ("body_pose", 63), ("jaw_pose", 3), ("leye_pose", 3),
                            ("reye_pose", 3), ("left_hand_pose", self.num_pca_comps), ("right_hand_pose", self.num_pca_comps)):
            if given[name] is not None:
                x = given[name]
                return int(np.prod(tuple(x.shape))) // width if hasattr(x, "shape") else np.asarray(x).size // width
        return self.batch_size

    def _check_expression(self, expression, n):
        """-> is `expression` an input of the device call.  None never is; on a device model without expression directions zeros
        pass (and are ignored) and anything else is refused; with directions it must be [n, n_expression] in the device model's
        dtype (float32 for the HIP model)."""
        if expression is None:
            return False
        ne = self.num_expression_coeffs
        if ne == 0:
            e = expression.detach().cpu().numpy() if _is_tensor(expression) else np.asarray(expression)
            if np.any(e != 0):
                raise ValueError("expression: the device model carries no expression directions - expression coefficients must be zero")
            return False
        e = expression if hasattr(expression, "shape") and hasattr(expression, "dtype") else np.asarray(expression)
        shape = tuple(e.shape)
        if shape != (n, ne):
            raise ValueError(f"expression: shape {shape}, the model takes [{n}, {ne}]")
        want = np.dtype(getattr(self._dev, "dtype", np.float32)).name
        if str(e.dtype).split(".")[-1] != want:
            raise ValueError(f"expression: dtype {e.dtype}, the device model computes in {want}")
        return True

    def forward(self, betas=None, global_orient=None, body_pose=None, left_hand_pose=None, right_hand_pose=None, transl=None,
                expression=None, jaw_pose=None, leye_pose=None, reye_pose=None, return_verts=True, return_full_pose=False, **kwargs):
        given = dict(betas=betas, global_orient=global_orient, body_pose=body_pose, jaw_pose=jaw_pose, leye_pose=leye_pose,
                     reye_pose=reye_pose, left_hand_pose=left_hand_pose, right_hand_pose=right_hand_pose)
        n = self._batch(given)
        with_expr = self._check_expression(expression, n)
        if any(_is_tensor(x) for x in list(given.values()) + [transl] + ([expression] if with_expr else [])):
            return self._forward_torch(n, given, transl, expression, with_expr, return_verts, return_full_pose)
        widths = {"betas": self._dev.n_betas, "body_pose": 63, "left_hand_pose": self.num_pca_comps, "right_hand_pose": self.num_pca_comps}
        for k in ("betas", "global_orient", "body_pose"):
            if given[k] is None:
                given[k] = np.zeros((n, widths.get(k, 3)), np.float32)
        extra = {"expression": np.asarray(expression)} if with_expr else {}          # (None: the eight-argument call)
        out = self._dev.forward_smplx(*[given[k] for k in _INPUTS], **extra)
        self.dyn_row = out["dyn_row"]
        verts, joints = out["vertices"], self._map(out["joints_all"])
        if transl is not None:
            t = np.asarray(transl, verts.dtype).reshape(-1, 1, 3)
            verts, joints = verts + t, joints + t
        given = {k: (np.zeros((n, widths.get(k, 3)), np.float32) if v is None else np.asarray(v, np.float32)) for k, v in given.items()}
        return ModelOutput(vertices=verts if return_verts else None, joints=joints, full_pose=out["full_pose"] if return_full_pose else None,
                           betas=given["betas"], global_orient=given["global_orient"], body_pose=given["body_pose"], jaw_pose=given["jaw_pose"],
                           left_hand_pose=given["left_hand_pose"], right_hand_pose=given["right_hand_pose"], expression=expression)

    __call__ = forward

    def _map(self, joints_all):
        joints = joints_all if self.use_face_contour else joints_all[:, :-N_CONTOUR]
        return joints if self.joint_mapper is None else self.joint_mapper(joints)

    def _forward_torch(self, n, given, transl, expression, with_expr, return_verts, return_full_pose):
        import torch
        like = next(x for x in list(given.values()) + [transl, expression] if _is_tensor(x))
        widths = {"betas": self._dev.n_betas, "body_pose": 63}
        x = {}
        for k, v in given.items():
            if v is None and k in ("betas", "global_orient", "body_pose"):
                v = torch.zeros(n, widths.get(k, 3), dtype=like.dtype, device=like.device)
            elif v is not None and not _is_tensor(v):
                v = torch.as_tensor(np.asarray(v), dtype=like.dtype, device=like.device)
            x[k] = v
        dev = self._dev

        # with expression the Function has a ninth input, the device calls a keyword more; without, they are the eight-argument calls
        def forward(*arrays):
            out = dev.forward_smplx(*arrays[:8], **({"expression": arrays[8]} if with_expr else {}))
            self.dyn_row = out["dyn_row"]
            return out["vertices"], out["joints_all"], out["full_pose"]

        def vjp(arrays, cot):
            return dev.vjp_smplx(*arrays[:8], dverts=cot[0], djoints_all=cot[1], dfull_pose=cot[2],
                                 **({"expression": arrays[8]} if with_expr else {}))

        inputs = [x[k] for k in _INPUTS]
        if with_expr:
            inputs.append(expression if _is_tensor(expression) else torch.as_tensor(np.asarray(expression), device=like.device))
        verts, joints_all, full_pose = _autograd.apply(forward, vjp, inputs, device_route=_DeviceRoute(self, with_expr))
        joints = self._map(joints_all)
        if transl is not None:                          # smplx: joints += transl.unsqueeze(1); vertices += transl.unsqueeze(1)
            t = transl if _is_tensor(transl) else torch.as_tensor(np.asarray(transl), dtype=verts.dtype, device=verts.device)
            t = t.reshape(-1, 1, 3)
            verts, joints = verts + t, joints + t
        return ModelOutput(vertices=verts if return_verts else None, joints=joints, full_pose=full_pose if return_full_pose else None,
                           betas=x["betas"], global_orient=x["global_orient"], body_pose=x["body_pose"], jaw_pose=x["jaw_pose"],
                           left_hand_pose=x["left_hand_pose"], right_hand_pose=x["right_hand_pose"], expression=expression)

    def to(self, *args, **kwargs):
        """nn.Module.to's place in smplify.py:80: the HIP model stays on the constructor's `device`"""
        return self


class _DeviceRoute:
    """`DeviceModel.forward_smplx` / `vjp_smplx` on tensors of the model's GPU (_autograd.apply's device_route): the eight
    parameter blocks, and with_expr the coefficients behind them"""

    def __init__(self, owner, with_expr):
        self.owner, self.dev, self.with_expr = owner, owner._dev, with_expr
        self.device = getattr(self.dev, "device", None) if hasattr(self.dev, "forward_smplx_dev") else None      # (a stand-in offers no device route)

    def _n(self, x):
        d = self.dev
        n = x[0].numel() // d.n_betas
        widths = (d.n_betas, 3, 63, 3, 3, 3, d.n_hand_pca, d.n_hand_pca) + ((d.n_expression,) if self.with_expr else ())
        require_elements("SMPLX.forward", tuple(zip(_INPUTS + ("expression",), x, widths)), n)
        return n, widths

    def forward(self, x, stream):
        import torch
        d, (n, _) = self.dev, self._n(x)
        verts, joints_all, full_pose = (torch.empty(shape, dtype=torch.float32, device=x[0].device)
                                        for shape in ((n, d.n_verts, 3), (n, d.n_joints_all, 3), (n, 3 * d.n_joints)))
        dyn_row = torch.empty(n, dtype=torch.int32, device=x[0].device)
        d.forward_smplx_dev(n, stream, [address(t) for t in x[:8]], expression=address(x[8]) if self.with_expr else 0,
                            vertices=address(verts), joints_all=address(joints_all), full_pose=address(full_pose), dyn_row=address(dyn_row))
        self.owner.dyn_row = dyn_row
        return verts, joints_all, full_pose

    def vjp(self, x, cotangents, want, stream):
        import torch
        d, (n, widths) = self.dev, self._n(x)
        grads = [torch.empty((n, w), dtype=torch.float32, device=x[0].device) if t is not None and wanted else None
                 for t, w, wanted in zip(x, widths, want)]
        d.vjp_smplx_dev(n, stream, [address(t) for t in x[:8]], expression=address(x[8]) if self.with_expr else 0,
                        dverts=address(cotangents[0]), djoints_all=address(cotangents[1]), dfull_pose=address(cotangents[2]),
                        grads=[address(g) for g in grads[:8]], dexpression=address(grads[8]) if self.with_expr else 0)
        return grads


def create(model_path=None, model_type="smpl", **kwargs):
    """smplx.create: 'smplx' -> SMPLX, 'smpl' -> bodyfitting_amd.smpl.SMPL (other body models are not on the device)."""
    kind = str(model_type).lower()
    if kind == "smplx":
        return SMPLX(model_path, **kwargs)
    if kind == "smpl":
        return SMPL(model_path, **kwargs)
    raise NotImplementedError(f"model_type={model_type!r}: 'smpl' and 'smplx' run on the device")
