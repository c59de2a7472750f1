"""The device route of the SMPL+D stage's losses, the parts that need no GPU: the new entry points as include/bodyfit.h declares them
against the binding's signatures and the library's exports (in the manner of tests/test_abi.py), the query memo's hit / miss rule as a
pure function on stand-in tensors, and that a library without the new entry points is not taken to offer the route."""
import ctypes as C
import os
import re

import pytest

from bodyfitting_amd import _autograd, _lib
from bodyfitting_amd import native as N
from bodyfitting_amd.mesh_grid_searcher import MeshGridSearcher, memo_hit

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what the issue names, and the scaling launch behind the scalar losses' backward
NEW = ("bf_vertex_normals_dev", "bf_vertex_normals_vjp_dev", "bf_normal_laplacian_dev", "bf_scan_point_loss_dev", "bf_scan_nearest_dev",
       "bf_normal_loss_dev", "bf_scale_gradient_dev")
TWINS = {"bf_vertex_normals_dev": "bf_vertex_normals", "bf_vertex_normals_vjp_dev": "bf_vertex_normals_vjp",
         "bf_normal_laplacian_dev": "bf_normal_laplacian", "bf_scan_point_loss_dev": "bf_scan_point_loss",
         "bf_scan_nearest_dev": "bf_scan_nearest"}


def _prototypes():
    """name -> [parameter declarations] of every function include/bodyfit.h declares"""
    text = open(os.path.join(REPO, "include", "bodyfit.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"\b(int|void|float|int64_t)\s+(bf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        out[name] = (ret, [" ".join(p.split()) for p in params.split(",")])
    return out


def _ctype(decl):
    """the ctypes kind of a parameter declaration: every pointer is an address on this route, the counts and flags are ints"""
    return "pointer" if "*" in decl else {"int": "int"}[decl.rsplit(" ", 1)[0]]


def test_the_header_declares_the_new_entry_points_with_the_bindings_signatures():
    protos = _prototypes()
    assert tuple(N.MESH_LOSS_DEV_SYMBOLS) == NEW
    for name in NEW:
        assert name in protos and name in _lib.SIGNATURES, name
        ret, params = protos[name]
        res, args = _lib.SIGNATURES[name]
        assert ret == "int" and res is C.c_int, name
        assert len(params) == len(args), (name, params, args)
        for decl, arg in zip(params, args):
            assert _ctype(decl) == ("int" if arg is C.c_int else "pointer"), (name, decl, arg)
            assert arg in (C.c_int, C.c_void_p), (name, decl, arg)          # device addresses go in as integers
    # a twin's arguments first, in its order, then the workspace and the stream
    for name, twin in TWINS.items():
        params, host = protos[name][1], protos[twin][1]
        assert params[:len(host)] == host, (name, params, host)
        assert params[len(host):] == ["bf_workspace *ws", "void *stream"], (name, params)
    assert protos["bf_normal_loss_dev"][1][-2:] == ["bf_workspace *ws", "void *stream"]
    assert protos["bf_normal_loss_dev"][1][:5] == ["int device", "int n", "const int32_t *face_ids", "const float *face_norm_table", "int n_faces"]


def test_the_library_exports_the_new_entry_points():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built - run __graft_entry__.build()")
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    assert N.offers_mesh_loss_dev(lib)


def test_every_new_kernel_is_declared_in_the_checked_header():
    header = open(os.path.join(REPO, "bodyfitting_amd", "csrc", "mesh_loss_kernels.h")).read()
    source = open(os.path.join(REPO, "bodyfitting_amd", "csrc", "mesh_loss_kernels.hip")).read()
    defined = set(re.findall(r"^(bf_ml_[a-z_]+_kernel)\(", source, flags=re.M))
    assert {"bf_ml_normal_gather_partial_kernel", "bf_ml_scale_kernel"} <= defined
    assert defined == set(re.findall(r"\b(bf_ml_[a-z_]+_kernel)\(", header))


class _Tensor:
    """what the memo looks at: identity and `_version`"""

    def __init__(self, version=0):
        self._version = version


def test_the_memo_hits_only_the_same_tensor_at_the_same_version():
    p = _Tensor()
    memo = (p, p._version, "ids", "nearest")
    assert memo_hit(memo, p)
    assert not memo_hit(None, p)
    assert not memo_hit(memo, _Tensor())                    # equal contents, another object: a miss, never a comparison
    p._version += 1                                         # an in-place edit
    assert not memo_hit(memo, p)
    assert memo_hit((p, p._version, "ids", "nearest"), p)
    # the memo holds its tensor: as long as it lives, no other object can have that identity
    held = _Tensor()
    memo = (held, 0, "ids", "nearest")
    ident = id(held)
    del held
    assert id(memo[0]) == ident and not memo_hit(memo, _Tensor())


class _NoGrid:
    closed = 0

    def close(self):
        type(self).closed += 1


def test_set_mesh_and_close_drop_the_memo(monkeypatch):
    from bodyfitting_amd import mesh_grid_searcher as M

    class Grid(_NoGrid):
        def __init__(self, verts, faces, device=0):
            pass

        def grid_info(self):
            import numpy as np
            return np.ones(3, np.int32), np.zeros(3, np.float32), 1.0

    monkeypatch.setattr(M, "Scan", Grid)
    import numpy as np
    verts, faces = np.eye(3, dtype=np.float32), np.array([[0, 1, 2]], np.int32)
    s = MeshGridSearcher(verts, faces)
    p = _Tensor()
    s._remember_query_dev(p, "ids", "nearest")
    assert memo_hit(s._last_query_dev, p) and s._query_dev(p, None) == "ids"          # a hit searches nothing (Grid cannot)
    s.set_mesh(verts, faces)
    assert s._last_query_dev is None
    s._remember_query_dev(p, "ids", "nearest")
    s.close()
    assert s._last_query_dev is None and Grid.closed == 2


class _CudaTensor(_Tensor):
    """a float32 tensor on cuda:0, as _autograd.route_for reads one"""
    dtype = "torch.float32"

    class device:
        type, index = "cuda", 0

    def detach(self):
        return self

    def cpu(self):
        return self

    requires_grad = False

    def data_ptr(self):
        return 4096


def test_a_library_without_the_new_symbols_does_not_offer_the_route(monkeypatch):
    class Old:
        """a library from before this route: the host entry points and the keypoint stage's device route only"""
        bf_vertex_normals = bf_scan_nearest = bf_keypoint_loss_dev = bf_workspace_create = staticmethod(lambda *a: 0)

    assert not N.offers_mesh_loss_dev(Old())
    for missing in NEW:                                     # ... and every one of them is needed

        class Partial:
            pass
        for name in NEW:
            if name != missing:
                setattr(Partial, name, staticmethod(lambda *a: 0))
        assert not N.offers_mesh_loss_dev(Partial()), missing
    # what such a library's objects say, and what follows from it: the host route, for tensors that would qualify otherwise
    monkeypatch.setattr(_autograd, "_ENABLED", [True])
    monkeypatch.setattr(_autograd, "_SHARED", {0: True})
    t = _CudaTensor()
    from bodyfitting_amd.normals import _NormalsRoute

    class Topo:
        dev_route_device = None
        n_verts = 3

    assert _autograd.chosen_route([t], _NormalsRoute(Topo())) == "host"
    assert _autograd.chosen_route([t], _NormalsRoute(object())) == "host"          # (a stand-in without the attribute)
    Topo.dev_route_device = 0
    assert _autograd.chosen_route([t], _NormalsRoute(Topo())) == "device"
    s = MeshGridSearcher()
    s._scan = type("Grid", (_NoGrid,), {"dev_route_device": None})()
    assert not s._takes_device_route(t)
    s._scan = type("Grid", (_NoGrid,), {})()
    assert not s._takes_device_route(t)
    s._scan = type("Grid", (_NoGrid,), {"dev_route_device": 0})()
    assert s._takes_device_route(t)
    from bodyfitting_amd import loss as L
    assert not L._takes_device_route(None, t) and L._takes_device_route(0, t) and not L._takes_device_route(1, t)
    s._scan = None
