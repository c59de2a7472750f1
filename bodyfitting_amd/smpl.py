"""`models.smpl.SMPL` of the reference (models/smpl.py:56-90) on the HIP path.

Same constructor / forward keyword names and the same `ModelOutput` fields.  `joints` are the 49 joints of JOINT_MAP,
`joints_ori` the 45 smplx joints, `vertices` the LBS output.

Two paths:
* numpy in -> numpy out, in model space (`transl` is ignored there: INTEGRATION.md).
* torch tensors in -> torch tensors out on the inputs' device, differentiable w.r.t. betas / global_orient / body_pose through
  the HIP forward and its vector-Jacobian product (bf_smpl_vjp), and w.r.t. transl as smplx + the wrapper apply it.  torch
  is imported on this path only.
"""
from __future__ import annotations

from dataclasses import dataclass, asdict

import numpy as np

from . import assets


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
        verts, joints, jori = _smpl_function().apply(self._dev, betas, global_orient, body_pose)
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


_FUNCTION = []


def _smpl_function():
    """The torch.autograd.Function of the torch path, defined on first use: forward = DeviceModel.forward, backward =
    DeviceModel.vjp, both through host memory.  Outputs come back as the device model returns them (float32 for the HIP model)
    on the inputs' device.  Once differentiable."""
    if _FUNCTION:
        return _FUNCTION[0]
    import torch
    from torch.autograd.function import once_differentiable

    def host(t):
        return None if t is None else t.detach().cpu().numpy()

    class SMPLFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, dev, betas, global_orient, body_pose):
            ctx.set_materialize_grads(False)            # (an unused output's cotangent stays None = zero: nothing is copied for it)
            ctx.dev = dev
            ctx.save_for_backward(betas, global_orient, body_pose)
            out = dev.forward(host(betas), host(global_orient), host(body_pose))
            return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(betas.device) for a in out)

        @staticmethod
        @once_differentiable
        def backward(ctx, dverts, djoints, djoints_ori):
            betas, global_orient, body_pose = ctx.saved_tensors
            want = ctx.needs_input_grad[1:]
            if not any(want) or (dverts is None and djoints is None and djoints_ori is None):
                return None, None, None, None
            grads = ctx.dev.vjp(host(betas), host(global_orient), host(body_pose), host(dverts), host(djoints), host(djoints_ori))
            return (None,) + tuple(torch.from_numpy(np.ascontiguousarray(g)).reshape(x.shape).to(x.device) if w else None
                                   for g, x, w in zip(grads, (betas, global_orient, body_pose), want))

    _FUNCTION.append(SMPLFunction)
    return SMPLFunction
