"""The torch.autograd.Function behind the torch paths of `smpl.SMPL` and `smplx.SMPLX`: a device model's forward and its
vector-Jacobian product, both through host memory.  Built on first use; torch is imported only there."""
from __future__ import annotations

import numpy as np

_FUNCTION = []


def apply(forward, vjp, inputs):
    """`inputs`: tensors, or None for an argument that was not passed (it takes no gradient).
    `forward(*arrays)` -> tuple of arrays, `vjp(arrays, cotangents)` -> one gradient array per input; both see numpy arrays where
    there is a tensor and None where there is none (a cotangent that is None is zero).
    -> the outputs as tensors on the inputs' device, in the dtype `forward` returns them (float32 for the HIP model).  Once
    differentiable; a gradient comes back in its input's shape, device and dtype."""
    return _function().apply(forward, vjp, *inputs)


def _function():
    if _FUNCTION:
        return _FUNCTION[0]
    import torch
    from torch.autograd.function import once_differentiable

    def host(t):
        return None if t is None else t.detach().cpu().numpy()

    class HostFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, forward, vjp, *inputs):
            ctx.set_materialize_grads(False)            # (an unused output's cotangent stays None = zero: nothing is copied for it)
            ctx.vjp = vjp
            ctx.present = [t is not None for t in inputs]
            ctx.save_for_backward(*[t for t in inputs if t is not None])
            out = forward(*[host(t) for t in inputs])
            device = next(t for t in inputs if t is not None).device
            return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in out)

        @staticmethod
        @once_differentiable
        def backward(ctx, *cotangents):
            saved = iter(ctx.saved_tensors)
            inputs = [next(saved) if p else None for p in ctx.present]
            want = ctx.needs_input_grad[2:]
            if not any(want) or all(c is None for c in cotangents):
                return (None,) * (2 + len(inputs))
            grads = ctx.vjp([host(t) for t in inputs], [host(c) for c in cotangents])
            return (None, None) + tuple(
                torch.from_numpy(np.ascontiguousarray(g)).reshape(x.shape).to(device=x.device, dtype=x.dtype) if w else None
                for g, x, w in zip(grads, inputs, want))

    _FUNCTION.append(HostFunction)
    return HostFunction
