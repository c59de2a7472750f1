"""`models.smpl.SMPL` of the reference (models/smpl.py:56-90) on the HIP path.

Same constructor / forward keyword names and the same `ModelOutput` fields.  `joints` are the 49 joints of JOINT_MAP,
`joints_ori` the 45 smplx joints, `vertices` the LBS output.

Two paths:
* numpy in -> numpy out, in model space (`transl` is ignored there: INTEGRATION.md).
* torch tensors in -> torch tensors out on the inputs' device, differentiable w.r.t. betas / global_orient / body_pose through
  the HIP forward and its vector-Jacobian product (bf_smpl_vjp), and w.r.t. transl as smplx + the wrapper apply it.  torch
  is imported on this path only.  float32 tensors on the model's GPU go into the kernels where they lie, on torch's current
  stream (bf_smpl_forward_dev / bf_smpl_vjp_dev: the device route of _autograd.py); everything else goes through host memory.
"""
from __future__ import annotations

from dataclasses import dataclass, asdict

import numpy as np

from . import _autograd, assets


@dataclass
class ModelOutput:                       # models/smpl.py:38-54 (whose __getitem__ forgot to import asdict)
    vertices: np.ndarray = None
    joints: np.ndarray = None
    full_pose: np.ndarray = None
    betas: np.ndarray = None
    expression: np.ndarray = None
    global_orient: np.ndarray = None
    body_pose: np.ndarray = None
    left_hand_pose: np.ndarray = None
    right_hand_pose: np.ndarray = None
    jaw_pose: np.ndarray = None
    joints_ori: np.ndarray = None

    def __getitem__(self, key):
        return asdict(self)[key]


class SMPL:
    def __init__(self, model_path=None, batch_size=1, gender="neutral", age="adult", create_transl=True,
                 kid_template_path=None, device=0, **kwargs):
        # age='kid': the 11-direction model of smplx's kid branch (model_files.kid_model), betas[B, 11]
        self.batch_size = batch_size
        self.gender, self.age = gender, age
        self._dev = assets.get_device_model("smpl", gender, device, age=age, kid_template_path=kid_template_path)
        model = assets.get_model("smpl", gender, age, kid_template_path)
        self.faces = np.asarray(model["faces"]) if "faces" in model else None
        self.J_regressor_extra = np.asarray(model["J_regressor_extra"], dtype=np.float32)
        self.J_regressor_h36m = np.asarray(model["J_regressor_h36m"], dtype=np.float32) if "J_regressor_h36m" in model else None
        self.joint_map = np.asarray(model["joint_map"])
        self.joints = None

    def forward(self, global_orient=None, body_pose=None, betas=None, transl=None, **kwargs):
        if any(_is_tensor(x) for x in (global_orient, body_pose, betas, transl)):
            return self._forward_torch(global_orient, body_pose, betas, transl)
        n = np.asarray(betas).reshape(-1, self._dev.n_betas).shape[0]
        verts, joints, jori = self._dev.forward(betas, global_orient, body_pose)
        self.joints = jori
        go = np.asarray(global_orient, np.float32).reshape(n, 3)
        bp = np.asarray(body_pose, np.float32).reshape(n, -1)
        return ModelOutput(vertices=verts, global_orient=go, body_pose=bp, joints=joints, joints_ori=jori,
                           betas=np.asarray(betas, np.float32).reshape(n, -1), full_pose=np.concatenate([go, bp], 1))

    __call__ = forward

    def _forward_torch(self, global_orient, body_pose, betas, transl):
        import torch
        like = next(x for x in (betas, global_orient, body_pose, transl) if _is_tensor(x))
        betas, global_orient, body_pose = (x if _is_tensor(x) else torch.as_tensor(np.asarray(x), dtype=like.dtype, device=like.device)
                                           for x in (betas, global_orient, body_pose))
        dev = self._dev
        verts, joints, jori = _autograd.apply(dev.forward, lambda x, cot: dev.vjp(*x, *cot), (betas, global_orient, body_pose),
                                              device_route=_DeviceRoute(dev))
        if transl is not None:
            # smplx adds transl to the vertices and its 45 joints; the wrapper's 9 extra joints are J_regressor_extra (v + t), i.e. each
            # moves by its regressor row's sum times t (models/smpl.py:71-75)
            t = transl if _is_tensor(transl) else torch.as_tensor(np.asarray(transl), dtype=verts.dtype, device=verts.device)
            t = t.reshape(-1, 1, 3)
            coef = np.concatenate([np.ones(jori.shape[1]), self.J_regressor_extra.astype(np.float64).sum(1)])[self.joint_map]
            verts = verts + t
            jori = jori + t
            joints = joints + torch.as_tensor(coef, dtype=joints.dtype, device=joints.device).reshape(1, -1, 1) * t
        self.joints = jori
        return ModelOutput(vertices=verts, global_orient=global_orient, body_pose=body_pose, joints=joints, joints_ori=jori,
                           betas=betas, full_pose=torch.cat([global_orient, body_pose], 1))

    def to(self, *args, **kwargs):
        """nn.Module.to's place in smplify.py:51-56: the HIP model stays on the constructor's `device`"""
        return self

    def get_joints_h36m(self, vertices):
        if _is_tensor(vertices):
            import torch
            return torch.einsum("bik,ji->bjk", vertices, torch.as_tensor(self.J_regressor_h36m, dtype=vertices.dtype, device=vertices.device))
        return np.einsum("bik,ji->bjk", np.asarray(vertices), self.J_regressor_h36m)

    def get_joints_ori(self):
        return self.joints


def _is_tensor(x):
    return hasattr(x, "detach") and hasattr(x, "requires_grad")


def require_elements(who, named, n):
    """every (name, tensor or None, width) holds n * width elements: the kernels index by these sizes"""
    for name, t, width in named:
        if t is not None and t.numel() != n * width:
            raise ValueError(f"{who}: {name} has {t.numel()} elements, [{n}, {width}] are expected")


def address(t):
    return 0 if t is None else t.data_ptr()


class _DeviceRoute:
    """`DeviceModel.forward` / `vjp` on tensors of the model's GPU (_autograd.apply's device_route)"""

    def __init__(self, dev):
        # (a device model without the *_dev calls - a stand-in - offers no device route)
        self.dev, self.device = dev, getattr(dev, "device", None) if hasattr(dev, "forward_dev") else None

    def _n(self, x):
        d = self.dev
        n = x[0].numel() // d.n_betas
        require_elements("SMPL.forward", (("betas", x[0], d.n_betas), ("global_orient", x[1], 3), ("body_pose", x[2], 3 * (d.n_joints - 1))), n)
        return n

    def forward(self, x, stream):
        import torch
        d, n = self.dev, self._n(x)
        out = [torch.empty((n, rows, 3), dtype=torch.float32, device=x[0].device)
               for rows in (d.n_verts, d.n_joint_map, d.n_joints + d.n_selector)]
        d.forward_dev(n, stream, *[address(t) for t in x], *[address(t) for t in out])
        return tuple(out)

    def vjp(self, x, cotangents, want, stream):
        import torch
        d, n = self.dev, self._n(x)
        grads = [torch.empty((n, t.numel() // n), dtype=torch.float32, device=t.device) if w else None for t, w in zip(x, want)]
        d.vjp_dev(n, stream, *[address(t) for t in x], *[address(c) for c in cotangents], *[address(g) for g in grads])
        return grads
