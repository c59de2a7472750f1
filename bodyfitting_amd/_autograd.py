"""The torch.autograd.Functions behind the torch paths of `smpl.SMPL`, `smplx.SMPLX`, `loss` and `prior`: a native forward and its
vector-Jacobian product.  Built on first use; torch is imported only there.

Two routes.  The HOST route takes every input and cotangent through host memory (`.cpu().numpy()` in, `torch.from_numpy().to()` out)
into the library's host entry points.  The DEVICE route hands the tensors' addresses and torch's current stream to the *_dev entry
points: no host copy, no synchronisation.  It needs torch and the library to share ONE HIP runtime, which a process has when torch
was imported before the library was first loaded (the loader then resolves the library's libamdhip64 to the copy torch brought) and
lacks in the other order.  That is found out at run time (`bf_device_pointer_check` on an input's address, once per process and
GPU), never assumed; `route_for` holds the whole decision.  Whenever the device route is not available the host route runs, as it
always has: nothing raises because of it.  BF_TORCH_DEVICE_ROUTE=0 switches the device route off."""
from __future__ import annotations

import os
import sys

import numpy as np

_FUNCTION = []
_DEVICE_FUNCTION = []
_ENABLED = []           # BF_TORCH_DEVICE_ROUTE, read once
_SHARED = {}            # GPU index -> do torch and the library share a HIP runtime


def enabled():
    """BF_TORCH_DEVICE_ROUTE is not 0 (read once; default: on)"""
    if not _ENABLED:
        _ENABLED.append(os.environ.get("BF_TORCH_DEVICE_ROUTE", "1").strip() != "0")
    return _ENABLED[0]


def route_for(inputs, device_index, enabled, shares_runtime, dtypes=("torch.float32",)):
    """-> "device" or "host".  inputs: tensors, arrays or None (an argument not passed); device_index: the GPU of the native object
    that offers a device route (None: it offers none); enabled: the switch; shares_runtime: torch's memory is the library's.
    "device" only when a route is offered, the switch is on, the runtimes are shared and every present input is a float32 tensor
    on cuda:device_index - and there is one.  dtypes: what the entry reads instead of float32 (the silhouette's masks)."""
    if device_index is None or not enabled or not shares_runtime:
        return "host"
    present = [t for t in inputs if t is not None]
    if not present:
        return "host"
    for t in present:
        device = getattr(t, "device", None)
        if getattr(device, "type", None) != "cuda" or device.index != int(device_index) or str(getattr(t, "dtype", None)) not in dtypes:
            return "host"
    return "device"


def shares_runtime(device_index, address):
    """does the library know `address` - memory torch allocated on GPU device_index - as its own runtime's?  Asked once per process
    and GPU; a refusal is said once on stderr."""
    device_index = int(device_index)
    if device_index not in _SHARED:
        from . import native
        _SHARED[device_index] = native.device_pointer_check(device_index, address)
        if not _SHARED[device_index]:
            print(f"bodyfitting_amd: tensors on cuda:{device_index} take the host route - the library was loaded before torch was "
                  "imported, so the process holds two HIP runtimes (import torch first for the device route)", file=sys.stderr)
    return _SHARED[device_index]


def takes_device_route(device_index, *tensors, dtypes=("torch.float32",)):
    """do these go the device route of a native object on GPU device_index (None: it offers none)?  `route_for`'s rule, `shares_runtime`
    asked only once everything else says "device"; arrays, None and objects without `data_ptr` (no address to hand over): False"""
    if route_for(tensors, device_index, enabled(), True, dtypes) != "device" or not all(hasattr(t, "data_ptr") for t in tensors):
        return False
    return shares_runtime(device_index, tensors[0].data_ptr())


def chosen_route(inputs, device_route, dtypes=("torch.float32",)):
    """the route `apply` takes for these inputs"""
    present = [t for t in inputs if t is not None]
    return "device" if takes_device_route(getattr(device_route, "device", None), *present, dtypes=dtypes) else "host"


def stream_of(tensor):
    """the handle of torch's current stream on the tensor's GPU: what a *_dev entry point queues its work on"""
    import torch
    return torch.cuda.current_stream(tensor.device).cuda_stream


def apply(forward, vjp, inputs, device_route=None):
    """`inputs`: tensors, or None for an argument that was not passed (it takes no gradient).
    `forward(*arrays)` -> tuple of arrays, `vjp(arrays, cotangents)` -> one gradient array per input; both see numpy arrays where
    there is a tensor and None where there is none (a cotangent that is None is zero).
    -> the outputs as tensors on the inputs' device, in the dtype `forward` returns them (float32 for the HIP model).  Once
    differentiable; a gradient comes back in its input's shape, device and dtype.

    device_route: None, or an object with `device` (a GPU index), `forward(tensors, stream)` -> tuple of tensors and
    `vjp(tensors, cotangents, want, stream)` -> one gradient tensor (or None) per input - contiguous tensors of that GPU in, None where
    `forward` / `vjp` above see None, `want[i]`: input i needs its gradient; stream: torch's current stream's handle, on which the
    results must be ordered.  Taken when `route_for` says so, else `forward` / `vjp` run through host memory."""
    if chosen_route(inputs, device_route) == "device":
        return _device_function().apply(device_route, *inputs)
    return _function().apply(forward, vjp, *inputs)


class ScalarLossRoute:
    """The `device_route` of a scalar loss whose native call returns the gradient for cotangent 1 with the value (loss.py:
    _scalar_loss).  call(tensor, want_grad, stream) -> (value: a float32 tensor [1] on the GPU, gradient: a tensor like `tensor`, or
    None); the forward keeps the gradient tensor, the reverse scales it on the device by the cotangent where it lies
    (bf_scale_gradient_dev: one launch, the bits of numpy's float32 `g * c` and `+ 0.0` with plus_zero) - the cotangent is never read
    back.  device: the GPU of the native object, None when it offers no device route."""

    def __init__(self, who, device, call, want_grad, plus_zero=False):
        self.who, self.device, self.call, self.want_grad, self.plus_zero = who, device, call, want_grad, plus_zero
        self.grad = None

    def forward(self, tensors, stream):
        value, self.grad = self.call(tensors[0], self.want_grad, stream)
        return (value,)

    def vjp(self, tensors, cotangents, want, stream):
        import torch
        from . import native
        if self.grad is None:
            raise RuntimeError(f"{self.who}: no gradient was computed with the forward")
        out = torch.empty_like(self.grad)
        native.scale_gradient_dev(self.device, stream, self.grad.numel(), self.grad.data_ptr(), cotangents[0].data_ptr(), out.data_ptr(),
                                  plus_zero=self.plus_zero)
        return (out,)


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


def _device_function():
    if _DEVICE_FUNCTION:
        return _DEVICE_FUNCTION[0]
    import torch
    from torch.autograd.function import once_differentiable

    def route_stream(route):
        return torch.cuda.current_stream(route.device).cuda_stream

    class DeviceFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, route, *inputs):
            ctx.set_materialize_grads(False)
            ctx.route = route
            ctx.present = [t is not None for t in inputs]
            ctx.save_for_backward(*[t for t in inputs if t is not None])
            return tuple(route.forward([None if t is None else t.detach().contiguous() for t in inputs], route_stream(route)))

        @staticmethod
        @once_differentiable
        def backward(ctx, *cotangents):
            saved = iter(ctx.saved_tensors)
            inputs = [next(saved) if p else None for p in ctx.present]
            want = ctx.needs_input_grad[1:]
            if not any(want) or all(c is None for c in cotangents):
                return (None,) * (1 + len(inputs))
            route = ctx.route
            grads = route.vjp([None if t is None else t.detach().contiguous() for t in inputs],
                              [None if c is None else c.contiguous() for c in cotangents], want, route_stream(route))
            return (None,) + tuple(g.reshape(x.shape) if w and g is not None else None for g, x, w in zip(grads, inputs, want))

    _DEVICE_FUNCTION.append(DeviceFunction)
    return DeviceFunction
