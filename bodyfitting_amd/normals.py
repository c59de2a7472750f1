"""`utils.io_utils.compute_normal_torch` of the reference (utils/io_utils.py:406-428) on the HIP path: vertex normals of a triangle
mesh (bf_vertex_normals) and, for torch tensors, their vector-Jacobian product (bf_vertex_normals_vjp) behind the project's
torch.autograd.Function - the first line of a user's own SMPL+D loop (smplify.py:236-245).

torch tensors in -> a float32 tensor [NV,3] on the vertices' device, differentiable (once) with respect to `vertices`; numpy in ->
numpy out.  torch is imported only when tensors arrive.

The topology - the faces and the vertex -> (face, corner) lists - is uploaded once per faces object and GPU (`topology_for`, a
table of _memo.py): a loop that passes the same tensor builds it once - a hit reads nothing of the tensor back, wherever it lives -
an in-place edit of the tensor is seen, arrays are told apart by a digest of their int32 bytes.

float32 vertices on the topology's GPU go into the kernels where they lie, on torch's current stream (bf_vertex_normals_dev /
bf_vertex_normals_vjp_dev: the device route of _autograd.py, on the topology's own workspace); everything else goes through host memory.
"""
from __future__ import annotations

import numpy as np

from . import _autograd
from . import _memo
from . import prior as _prior

_TOPOLOGY_SLOTS = 8         # meshes kept at a time; the oldest goes first
_TOPOLOGIES = {}            # a table of _memo.py: (faces, n_verts, GPU) -> topo (native.Topology); a faces tensor is not held

FUSED_PATH = ("only numpy arrays and torch tensors (and this project's MeshGridSearcher) are supported here; SMPLify's fused stage "
              "(bodyfitting_amd.smplify) is the other path")


def _is_tensor(x):
    return hasattr(x, "detach") and hasattr(x, "requires_grad")


def require_array(who, name, x):
    """An argument that is neither an array nor a tensor: NotImplementedError (what the stand-alone stubs raised for anything)"""
    if not (_is_tensor(x) or isinstance(x, np.ndarray)):
        raise NotImplementedError(f"{who}: {name} is a {type(x).__name__}; {FUSED_PATH}")


def require_same_kind(who, named):
    """all tensors or all arrays"""
    kinds = {_is_tensor(x) for _, x in named}
    if len(kinds) > 1:
        raise ValueError(f"{who}: {', '.join(n for n, _ in named)} mix torch tensors and numpy arrays")


def require_rows3(who, name, x):
    """-> the row count of what the reference's x.view(-1, 3) yields"""
    if x.ndim < 1 or x.shape[-1] != 3:
        raise ValueError(f"{who}: {name} must end in a dimension of 3, not {tuple(x.shape)}")
    return int(np.prod(x.shape[:-1]))


def require_no_grad(who, name, x):
    if _is_tensor(x) and x.requires_grad:
        raise ValueError(f"{who}: {name} requires grad; no gradient flows to it")


def device_index(x):
    """the GPU of a tensor (a CPU tensor or an array: 0)"""
    d = getattr(x, "device", None)
    if d is None or getattr(d, "type", "cpu") == "cpu":
        return 0
    return 0 if d.index is None else int(d.index)


def _faces_host(who, faces):
    """what the reference's faces.view(-1, 3) yields, as int32 on the host"""
    if _is_tensor(faces):
        if faces.is_floating_point() or faces.is_complex():
            raise ValueError(f"{who}: faces must be an integer tensor, not {faces.dtype}")
        host = faces.detach().cpu().numpy()
    else:
        host = faces
        if host.dtype.kind not in "iu":
            raise ValueError(f"{who}: faces must be an integer array, not {host.dtype}")
    if host.size == 0 or host.size % 3:
        raise ValueError(f"{who}: faces must hold a positive multiple of 3 indices, not {host.size}")
    return np.ascontiguousarray(host.reshape(-1, 3), dtype=np.int32)


def topology_for(who, faces, n_verts, device):
    """The `native.Topology` of `faces` for a mesh of n_verts vertices on GPU `device`, built on first use."""
    require_array(who, "faces", faces)
    require_no_grad(who, "faces", faces)
    host = None if _is_tensor(faces) else _faces_host(who, faces)
    seen = []
    key = (_memo.part(faces, seen, None if host is None else host.tobytes()), int(n_verts), int(device))
    hit = _memo.find(_TOPOLOGIES, key, seen)
    if hit is not None:
        return hit["topo"]
    from . import native
    if host is None:
        host = _faces_host(who, faces)
    if host.min() < 0 or host.max() >= n_verts:
        raise ValueError(f"{who}: a face index lies outside [0, {n_verts})")
    return _memo.store(_TOPOLOGIES, _TOPOLOGY_SLOTS, key, seen, {"topo": native.Topology(n_verts, host, device=device)})["topo"]


def compute_normal_torch(vertices, faces):
    """vertices[..., 3] (read as the reference's vertices.view(-1, 3)), faces: integer indices (read as faces.view(-1, 3)) ->
    normals[NV,3]: face normals n / (|n| + 1e-8), summed per vertex, divided by (|sum| + 1e-8) again.  The gradient goes to
    `vertices`."""
    from . import native
    who = "compute_normal_torch"
    require_array(who, "vertices", vertices)
    require_array(who, "faces", faces)
    require_same_kind(who, (("vertices", vertices), ("faces", faces)))
    _prior._require_float32(who, "vertices", vertices)
    n_verts = require_rows3(who, "vertices", vertices)
    if n_verts == 0:
        raise ValueError(f"{who}: no vertices")
    topo = topology_for(who, faces, n_verts, device_index(vertices))

    def forward(v):
        return (native.vertex_normals(topo, v.reshape(-1, 3)),)

    def vjp(arrays, cotangents):
        return (native.vertex_normals_vjp(topo, arrays[0].reshape(-1, 3), cotangents[0]),)

    if not _is_tensor(vertices):
        return forward(vertices)[0]
    return _autograd.apply(forward, vjp, (vertices,), device_route=_NormalsRoute(topo))[0]


class _NormalsRoute:
    """compute_normal_torch on vertices of the topology's GPU (_autograd.apply's device_route): bf_vertex_normals_dev and
    bf_vertex_normals_vjp_dev on the tensors' addresses, the results in tensors made here"""

    def __init__(self, topo):
        self.topo, self.device = topo, getattr(topo, "dev_route_device", None)

    def forward(self, tensors, stream):
        import torch
        from . import native
        v = tensors[0]
        out = torch.empty((self.topo.n_verts, 3), dtype=torch.float32, device=v.device)
        native.vertex_normals_dev(self.topo, stream, v.data_ptr(), out.data_ptr())
        return (out,)

    def vjp(self, tensors, cotangents, want, stream):
        import torch
        from . import native
        v = tensors[0]
        out = torch.empty((self.topo.n_verts, 3), dtype=torch.float32, device=v.device)
        native.vertex_normals_vjp_dev(self.topo, stream, v.data_ptr(), cotangents[0].data_ptr(), out.data_ptr())
        return (out,)
