"""`smplify.prior.MaxMixturePrior` of the reference (smplify/prior.py:100-231) on the HIP path: the merged likelihood
min_m (0.5 d' P_m d - log w_m) and its gradient with respect to the pose, through bf_keypoint_loss with no views, the pose prior's
weight 1 and the other weights 0.

numpy in -> numpy out; torch tensors in -> a differentiable float32 tensor on the pose's device (torch is imported on that path
only); a float32 tensor on the prior's GPU goes into the kernel where it lies, on torch's current stream (bf_keypoint_loss_dev:
the device route of _autograd.py).  `use_merged=False` (prior.py:198-225) and dtypes other than float32 are refused, not approximated.
"""
from __future__ import annotations

import weakref

import numpy as np

from . import _autograd, assets

_FLOAT32_NAMES = ("torch.float32", "float32", "<class 'numpy.float32'>")
_FOREIGN = weakref.WeakKeyDictionary()        # the reference's own prior module -> {device: native.Gmm}


def _is_tensor(x):
    return hasattr(x, "detach") and hasattr(x, "requires_grad")


def is_gmm_like(obj):
    return all(hasattr(obj, k) for k in ("means", "precisions", "nll_weights"))


def _host(a):
    return np.asarray(a.detach().cpu().numpy() if _is_tensor(a) else a, np.float32)


def _require_float32(who, name, x):
    if _is_tensor(x):
        import torch
        ok = x.dtype == torch.float32
    else:
        ok = np.asarray(x).dtype == np.float32
    if not ok:
        raise ValueError(f"{who}: {name} must be float32 (the HIP kernel's type), not {x.dtype}")


def device_gmm(obj, device=None):
    """The buffers of a prior object - this module's MaxMixturePrior or anything with means / precisions / nll_weights, such as
    the reference's own nn.Module - on `device` (None: the object's own, else 0), uploaded once per object and device."""
    from . import native
    if device is None:
        device = obj.device if isinstance(obj, MaxMixturePrior) else 0
    device = int(device)
    if isinstance(obj, MaxMixturePrior):
        cache = obj._on_device
    else:
        try:
            cache = _FOREIGN.setdefault(obj, {})
        except TypeError:                          # (not weakly referenceable: keep the handles on the object itself)
            cache = obj.__dict__.setdefault("_bodyfit_gmm", {})
    if device not in cache:
        cache[device] = native.Gmm(_host(obj.means), _host(obj.precisions), _host(obj.nll_weights).reshape(-1), device=device)
    return cache[device]


class _DeviceRoute:
    """merged_log_likelihood on a pose of the prior's GPU (_autograd.apply's device_route): bf_keypoint_loss_dev with no views"""

    def __init__(self, gmm, hyper):
        self.gmm, self.hyper, self.device = gmm, hyper, gmm.device

    def forward(self, x, stream):
        import torch
        from . import native
        p = x[0]
        terms = torch.empty((p.shape[0], 4), dtype=torch.float32, device=p.device)
        native.keypoint_loss_dev(stream, p.shape[0], pose_dim=p.shape[1], poses=p.data_ptr(), gmm=self.gmm, hyper=self.hyper,
                                 terms=terms.data_ptr())
        return (terms[:, 1],)

    def vjp(self, x, cotangents, want, stream):
        import torch
        from . import native
        p = x[0]
        dterms = torch.zeros((p.shape[0], 4), dtype=torch.float32, device=p.device)
        dterms[:, 1] = cotangents[0].reshape(-1)
        dposes = torch.empty_like(p)
        native.keypoint_loss_dev(stream, p.shape[0], pose_dim=p.shape[1], poses=p.data_ptr(), gmm=self.gmm, hyper=self.hyper,
                                 dterms=dterms.data_ptr(), dposes=dposes.data_ptr())
        return (dposes,)


class MaxMixturePrior:
    def __init__(self, prior_folder="prior", num_gaussians=6, dtype="torch.float32", epsilon=1e-16, use_merged=True, **kwargs):
        if str(dtype) not in _FLOAT32_NAMES:
            raise ValueError(f"MaxMixturePrior: dtype {dtype} is not supported, the HIP kernels are float32")
        if not use_merged:
            raise ValueError("MaxMixturePrior: use_merged=False (prior.py:198-225) is not supported")
        self.num_gaussians, self.epsilon, self.use_merged = num_gaussians, epsilon, use_merged
        self.device = int(kwargs.get("device", 0))
        gmm = assets.get_gmm(prior_folder, num_gaussians)
        means, precisions, nll_weights = assets.gmm_buffers(gmm)
        self.means, self.precisions = means, precisions
        self.nll_weights = nll_weights.reshape(1, -1)                  # (prior.py:159: unsqueeze(dim=0))
        self.weights = np.asarray(gmm["weights"], np.float32).reshape(1, -1)
        self.random_var_dim = means.shape[1]
        self._on_device = {}

    def to(self, *args, **kwargs):
        """nn.Module.to's place in smplify.py:46: the buffers stay on the constructor's `device`"""
        return self

    def get_mean(self):
        return self.weights @ self.means

    def merged_log_likelihood(self, pose, betas):
        """pose[B, D' <= D] (zero-padded to the GMM's dimension, D' > 55) -> [B]"""
        from . import native
        gmm = device_gmm(self)
        hyper = native.make_hyper(pose_prior_weight=1.0, angle_prior_weight=0.0, shape_prior_weight=0.0)

        def forward(p):
            return (native.keypoint_loss(None, poses=p, gmm=gmm, hyper=hyper, want=("terms",))["terms"][:, 1],)

        def vjp(arrays, cotangents):
            p = arrays[0]
            dterms = np.zeros((len(p), 4), p.dtype)
            dterms[:, 1] = np.asarray(cotangents[0]).reshape(-1)
            return (native.keypoint_loss(None, poses=p, gmm=gmm, hyper=hyper, dterms=dterms, want=("dposes",))["dposes"],)

        if not _is_tensor(pose):
            pose = np.asarray(pose)
        _require_float32("MaxMixturePrior", "pose", pose)
        if pose.ndim != 2:
            raise ValueError("MaxMixturePrior: pose must be [B, D]")
        if not _is_tensor(pose):
            return forward(pose)[0]
        return _autograd.apply(forward, vjp, (pose,), device_route=_DeviceRoute(gmm, hyper))[0]

    def forward(self, pose, betas):
        return self.merged_log_likelihood(pose, betas)

    __call__ = forward
