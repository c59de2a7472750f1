"""The device route of neural_renderer.Renderer without a GPU: when it is taken (_autograd.route_for's rule, never an error when
it is unavailable), and the Python plumbing around bf_nr_render_dev / bf_nr_tape_*_dev - per-item slices, cameras by value or by
address, the tape's borrowed tensor, the shared camera's sum - over a stand-in backend that reads and writes CPU tensors at the
addresses it is handed and computes with tests/nr_vertex_oracle.py.  The route itself runs in tests/test_gpu_nr_device_route.py."""
import ctypes
import itertools
import os
import types

import numpy as np
import pytest
import torch

from bodyfitting_amd import _autograd, _lib, native
from bodyfitting_amd import neural_renderer as nr
from texfit_cases import icosphere
import nr_vertex_oracle as VO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("bf_nr_render_dev", "bf_nr_tape_texture_grad_dev", "bf_nr_tape_vertex_grad_dev", "bf_nr_tape_layout", "bf_nr_route_stats")
SIZE = 12


def _at(address, shape):
    """the float32 array at `address` (memory of a live CPU tensor)"""
    n = int(np.prod(shape))
    return np.ctypeslib.as_array((ctypes.c_float * n).from_address(address)).reshape(shape)


class DevTape(VO.OracleTape):
    def __init__(self, keep, log, flags, nv, tex_shape):
        super().__init__(keep, log, flags)
        self.n_verts, self.tex_shape = nv, tex_shape

    def vertex_grad_dev(self, stream, grad_verts, grad_rgb=0, grad_depth=0, grad_alpha=0, grad_R=0, grad_t=0):
        shapes = ((3, SIZE, SIZE), (SIZE, SIZE), (SIZE, SIZE))
        g = [_at(a, s).copy() if a else None for a, s in zip((grad_rgb, grad_depth, grad_alpha), shapes)]
        gv, gR, gt = self.vertex_grad(*g, camera=bool(grad_R or grad_t))
        _at(grad_verts, gv.shape)[...] = gv
        if grad_R:
            _at(grad_R, (3, 3))[...] = gR
        if grad_t:
            _at(grad_t, (3,))[...] = gt
        self.log["dev_calls"] += 1

    def texture_grad_dev(self, stream, grad_rgb, grad_textures):
        _at(grad_textures, self.tex_shape)[...] = self.texture_grad(_at(grad_rgb, (3, SIZE, SIZE)).copy())
        self.log["dev_calls"] += 1


class DevRenderer(VO.OracleRenderer):
    """the oracle backend with the device route's entry points, on CPU tensors' memory"""
    LOG = VO.OracleRenderer.LOG

    @classmethod
    def offers_dev(cls, lib=None):
        return True

    def tape_floats(self, mesh, fill_back, lit, flags, has_rgb):
        return 64 if flags else 0

    def render(self, *args, **kwargs):
        self.log["host_calls"] += 1
        return super().render(*args, **kwargs)

    def render_taped(self, *args, **kwargs):
        self.log["host_calls"] += 1
        return super().render_taped(*args, **kwargs)

    def render_dev(self, mesh, stream, verts, textures=0, K=None, R=None, t=None, orig_size=1.0, fill_back=True, lightoff=False, ndc=False,
                   rgb=0, depth=0, alpha=0, flags=0, storage=0, storage_floats=0):
        assert bool(flags) == bool(storage) and storage_floats == (64 if flags else 0)
        self.log["by_address"].append(tuple(isinstance(x, int) for x in (K, R, t)))
        K, R, t = (_at(x, s).copy() if isinstance(x, int) else x for x, s in ((K, (3, 3)), (R, (3, 3)), (t, (3,))))
        v = _at(verts, mesh.verts.shape).copy()
        tex = _at(textures, mesh.textures_shape).copy() if textures else None
        want = tuple(nm for nm, a in (("rgb", rgb), ("depth", depth), ("alpha", alpha)) if a)
        out = VO.render(v, mesh.faces, tex, K, R, t, orig_size, fill_back=fill_back, lightoff=lightoff, light=self.light, ndc=ndc, want=want, **self.cfg)
        for a, o, shape in zip((rgb, depth, alpha), out[:3], ((3, SIZE, SIZE), (SIZE, SIZE), (SIZE, SIZE))):
            if a:
                _at(a, shape)[...] = o
        self.log["dev_calls"] += 1
        return DevTape(out[3], self.log, flags, len(v), mesh.textures_shape) if flags else None


class _Device:
    def __init__(self, kind, index):
        self.type, self.index = kind, index


class _Like:
    """what the routing rule reads of a tensor"""
    requires_grad = False
    _version = 0

    def __init__(self, kind="cuda", index=0, dtype="torch.float32"):
        self.device, self.dtype = _Device(kind, index), dtype

    def data_ptr(self):
        return 4096


@pytest.fixture
def backend(monkeypatch):
    monkeypatch.setattr(native, "NrRenderer", DevRenderer)
    monkeypatch.setattr(native, "NrMesh", VO.OracleMesh)
    monkeypatch.setattr(native, "NrTape", VO.OracleTape)
    monkeypatch.setattr(nr, "DEVICE_ROUTE", True)
    DevRenderer.LOG.update(meshes=0, uploads=0, tapes_open=0, vertex_uploads=0, host_calls=0, dev_calls=0, by_address=[])
    return DevRenderer.LOG


@pytest.fixture
def on_device(backend, monkeypatch):
    """CPU float32 tensors stand for tensors of cuda:0: the decision says "device", and their memory is what the backend reads"""
    held = []

    class Tapes(nr._DeviceTapes):
        def __init__(self):
            super().__init__()
            held.append(self)

    monkeypatch.setattr(nr, "_DeviceTapes", Tapes)
    monkeypatch.setattr(nr, "_readable_on", lambda x, gpu: nr._is_tensor(x) and str(x.dtype) == "torch.float32")
    monkeypatch.setattr(_autograd, "takes_device_route", lambda gpu, *tensors, dtypes=("torch.float32",): gpu is not None and all(nr._is_tensor(x) and str(x.dtype) == "torch.float32" for x in tensors))
    monkeypatch.setattr(_autograd, "stream_of", lambda tensor: 0)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    return held


def _mesh(ts=2, seed=0):
    v, f = icosphere(1)
    rng = np.random.default_rng(seed)
    v = (v * 0.8 + np.array([0.05, -0.03, 2.6])).astype(np.float32)
    return v, f.astype(np.int32), rng.uniform(0.1, 1.0, (len(f), ts, ts, ts, 3)).astype(np.float32)


def _K():
    return np.array([[SIZE, 0, SIZE // 2], [0, SIZE, SIZE // 2], [0, 0, 1]], np.float32)


def _camera(k=0):
    a = 0.1 + 0.15 * k
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    return R, np.array([0.02 * k, -0.01, 0.1 * k], np.float32)


def _renderer(**kw):
    r = nr.Renderer(image_size=SIZE, K=_K()[None], orig_size=SIZE, near=0.1, far=10.0, **kw)
    return r


# ---- the decision ---------------------------------------------------------------------------------------------------------------------

def test_the_route_is_taken_exactly_under_route_fors_rule(backend, monkeypatch):
    """vertices - and textures, where a render uses them - float32 tensors on the renderer's GPU, BF_TORCH_DEVICE_ROUTE not 0, one
    shared runtime, a backend that offers the entries, the module's own switch on: every other combination is the host route"""
    r = _renderer()
    native_r = r._renderer_on(0)
    kinds = (("cuda", 0), ("cuda", 1), ("cpu", None))
    dtypes = ("torch.float32", "torch.float64", "torch.float16")
    for (kind, index), dtype, enabled, shared, offered, switch in itertools.product(kinds, dtypes, (True, False), (True, False), (True, False), (True, False)):
        monkeypatch.setattr(_autograd, "_ENABLED", [enabled])
        monkeypatch.setattr(_autograd, "_SHARED", {0: shared, 1: shared})
        monkeypatch.setattr(nr, "DEVICE_ROUTE", switch)
        rr = native_r if offered else VO.OracleRenderer(SIZE)
        rule = kind == "cuda" and index == 0 and dtype == "torch.float32" and enabled and shared and offered
        want = rule and switch
        what = (kind, index, dtype, enabled, shared, offered, switch)
        assert r._on_device_route(rr, 0, _Like(kind, index, dtype), None) == want, what                       # a silhouette: the vertices decide
        assert r._on_device_route(rr, 0, _Like(), _Like(kind, index, dtype)) == want, what                    # ... the textures with them
        assert r._on_device_route(rr, 0, _Like(), _Like(), [_Like(kind, index, dtype)]) == want, what         # ... an R or t that takes a gradient
        assert (_autograd.route_for([_Like(kind, index, dtype)], 0 if offered else None, enabled, shared) == "device") == rule, what
    monkeypatch.setattr(_autograd, "_ENABLED", [True])
    monkeypatch.setattr(_autograd, "_SHARED", {0: True})
    monkeypatch.setattr(nr, "DEVICE_ROUTE", True)
    # K, R, t never decide: a numpy K with R, t on the GPU, or all five there, is the device route; numpy vertices are not
    assert r._on_device_route(native_r, 0, _Like(), _Like())
    assert not r._on_device_route(native_r, 0, np.zeros((1, 4, 3), np.float32), None)
    assert not r._on_device_route(native_r, 0, _Like(), np.zeros((1, 4, 2, 2, 2, 3), np.float32))
    r.close()


def test_nothing_raises_where_the_route_is_unavailable(backend):
    """CPU tensors, float64 and numpy inputs run the host route with a backend that offers the entries"""
    v, f, tex = _mesh()
    R, t = _camera()
    r = _renderer()
    ref = r.render(v[None], f[None], tex[None], R=R[None], t=t[None])
    assert all(isinstance(o, np.ndarray) for o in ref)
    for dtype in (torch.float32, torch.float64):
        out = r.render(torch.tensor(v, dtype=dtype)[None], torch.tensor(f)[None], torch.tensor(tex, dtype=dtype)[None], R=torch.tensor(R)[None],
                       t=torch.tensor(t)[None])
        for o, w in zip(out, ref):
            assert o.dtype == torch.float32 and np.array_equal(o.numpy(), w)
    assert backend["dev_calls"] == 0 and backend["host_calls"] == 3
    r.close()


# ---- the plumbing ---------------------------------------------------------------------------------------------------------------------

def _tensors(v, f, tex, B=1):
    return (torch.tensor(np.stack([v] * B)), torch.tensor(np.stack([f] * B)), torch.tensor(np.stack([tex] * B)))


def test_cameras_come_by_value_or_by_address_each_on_its_own(on_device, backend):
    """the reference's loop: K a numpy array in the constructor, R and t fresh tensors of the GPU -> K by value, R and t by address;
    all five on the GPU -> all by address; the results are the host route's"""
    v, f, tex = _mesh()
    R, t = _camera(1)
    host = _renderer()
    ref = host.render(v[None], f[None], tex[None], R=R[None], t=t[None])
    assert backend["dev_calls"] == 0
    tv, tf, tt = _tensors(v, f, tex)
    for K, want in ((None, (False, True, True)), (torch.tensor(_K())[None], (True, True, True))):
        r = _renderer()
        backend["by_address"].clear()
        out = r.render(tv, tf, tt, K=K, R=torch.tensor(R)[None], t=torch.tensor(t).reshape(1, 1, 3))
        assert backend["by_address"] == [want]
        for o, w in zip(out, ref):
            assert isinstance(o, torch.Tensor) and o.dtype == torch.float32 and np.array_equal(o.numpy(), w)
        for mode, k in (("silhouettes", 2), ("depth", 1)):
            np.testing.assert_array_equal(r.forward(tv, tf, mode=mode, K=K, R=torch.tensor(R)[None], t=torch.tensor(t)[None]).numpy(), ref[k])
        np.testing.assert_array_equal(r.forward(tv, tf, tt, mode="rgb", K=K, R=R[None], t=torch.tensor(t, dtype=torch.float64)[None]).numpy(), ref[0])
        assert backend["by_address"][-1] == (want[0], False, False)                  # an array, a float64 tensor: by value
        r.close()
    assert backend["host_calls"] == 1 and backend["uploads"] == 1 and backend["vertex_uploads"] == 0     # (the yardstick's own)
    with pytest.raises(ValueError, match="R must have batch size 1 or 1, not 2"):
        _renderer().render(tv, tf, tt, R=torch.tensor(np.stack([R, R])), t=torch.tensor(t)[None])
    host.close()


def test_K_requiring_grad_is_refused_on_both_routes(on_device, backend, monkeypatch):
    v, f, tex = _mesh()
    R, t = _camera()
    tv, tf, tt = _tensors(v, f, tex)
    K = torch.tensor(_K())[None].requires_grad_(True)
    for device_route in (True, False):
        monkeypatch.setattr(nr, "DEVICE_ROUTE", device_route)
        r = _renderer()
        r.geometry_grad = True
        with pytest.raises(NotImplementedError, match="K is not differentiated"):
            r.render(tv, tf, tt, K=K, R=torch.tensor(R)[None], t=torch.tensor(t)[None])
        r.geometry_grad = False
        with pytest.raises(NotImplementedError, match="detach K first"):
            r.render(tv, tf, tt, K=K, R=torch.tensor(R)[None], t=torch.tensor(t)[None])
        r.close()
    assert backend["dev_calls"] == 0 and backend["host_calls"] == 0


def test_with_geometry_grad_off_vertex_gradients_are_refused_with_the_old_message(on_device, backend):
    v, f, tex = _mesh()
    R, t = _camera()
    tv, tf, tt = _tensors(v, f, tex)
    r = _renderer()
    assert r.geometry_grad is False
    for what, kw in (("vertices", dict(v=tv.clone().requires_grad_(True))), ("R", dict(R=torch.tensor(R)[None].requires_grad_(True))),
                     ("t", dict(t=torch.tensor(t)[None].requires_grad_(True)))):
        with pytest.raises(NotImplementedError, match=f"soft-edge vertex gradient.*detach {what} first"):
            r.render(kw.get("v", tv), tf, tt, R=kw.get("R", torch.tensor(R)[None]), t=kw.get("t", torch.tensor(t)[None]))
    assert backend["dev_calls"] == 0
    r.close()


def _grads(r, v, f, tex, R, t, cot, retain=False):
    x = dict(v=v.clone().requires_grad_(True), tex=tex.clone().requires_grad_(True), R=R.clone().requires_grad_(True), t=t.clone().requires_grad_(True))
    out = r.render(x["v"], f, x["tex"], R=x["R"], t=x["t"])
    loss = sum((o * c).sum() for o, c in zip(out, cot))
    loss.backward(retain_graph=retain)
    return [o.detach().numpy() for o in out], {k: a.grad.numpy().copy() for k, a in x.items()}, loss


def test_gradients_are_the_host_routes_and_the_tape_tensor_is_released(on_device, backend, monkeypatch):
    v, f, tex = _mesh()
    R, t = _camera(1)
    tv, tf, tt = _tensors(v, f, tex)
    cot = [torch.tensor(np.random.default_rng(k).standard_normal(s).astype(np.float32)) for k, s in enumerate(((1, 3, SIZE, SIZE), (1, SIZE, SIZE), (1, SIZE, SIZE)))]
    monkeypatch.setattr(nr, "DEVICE_ROUTE", False)
    host = _renderer()
    host.geometry_grad = True
    want_out, want, _ = _grads(host, tv, tf, tt, torch.tensor(R)[None], torch.tensor(t)[None], cot)
    assert backend["dev_calls"] == 0 and not on_device
    monkeypatch.setattr(nr, "DEVICE_ROUTE", True)
    r = _renderer()
    r.geometry_grad = True
    got_out, got, loss = _grads(r, tv, tf, tt, torch.tensor(R)[None], torch.tensor(t)[None], cot, retain=True)
    assert backend["dev_calls"] == 3 and backend["vertex_uploads"] == 0             # one render, one vertex and one texture gradient
    for a, b in zip(got_out, want_out):
        np.testing.assert_array_equal(a, b)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    # the tape and the tensor it borrowed went with the backward pass; a second one raises the existing error
    held = on_device[-1]
    assert held.tapes == [] and held.storage == [] and backend["tapes_open"] == 0
    with pytest.raises(RuntimeError, match="tape was freed by an earlier backward pass"):
        loss.backward()
    # a textures-only render: one node, its tape freed with the graph when no backward runs
    tex2 = tt.clone().requires_grad_(True)
    out = r.render_rgb(tv, tf, tex2, R=torch.tensor(R)[None], t=torch.tensor(t)[None])
    assert out.requires_grad and len(on_device[-1].tapes) == 1 and len(on_device[-1].storage) == 1 and on_device[-1].storage[0].numel() == 64
    assert backend["tapes_open"] == 1
    del out
    on_device.clear()
    import gc
    gc.collect()
    assert backend["tapes_open"] == 0
    # the mesh is remembered by its faces, vertex count and GPU: new vertex and texture tensors, and edits in place, make no new one
    meshes, uploads = backend["meshes"], backend["uploads"]
    r.render(tv.clone(), tf, tt.clone(), R=torch.tensor(R)[None], t=torch.tensor(t)[None])
    tv2 = tv.clone()
    tv2.add_(0.01)
    r.render(tv2, tf, tt, R=torch.tensor(R)[None], t=torch.tensor(t)[None])
    assert backend["meshes"] == meshes and backend["uploads"] == uploads == 1         # (the one upload: the host-route yardstick's)
    r.close(); host.close()


def test_the_shared_cameras_sum_is_taken_in_item_order(on_device, backend):
    """a [1,3,3] camera shared by B = 3 items takes ((g0 + g1) + g2): the bits of numpy's sum(0, dtype=float32) over the items'
    gradients, which the host route returns"""
    rng = np.random.default_rng(3)
    for shape in ((3, 3, 3), (7, 3), (2, 9)):
        rows = (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(np.float32)
        got = nr._sum_in_item_order([torch.tensor(r_) for r_ in rows]).numpy()
        want = rows[0]
        for r_ in rows[1:]:
            want = want + r_
        assert got.tobytes() == want.tobytes() == rows.sum(0, dtype=np.float32).tobytes()
    v, f, tex = _mesh()
    R, t = _camera(2)
    B = 3
    vs = np.stack([v + np.float32(0.02 * b) for b in range(B)])
    tv, tf, tt = torch.tensor(vs), torch.tensor(np.stack([f] * B)), torch.tensor(np.stack([tex] * B))
    cot = [torch.tensor(np.random.default_rng(7 + k).standard_normal(s).astype(np.float32)) for k, s in enumerate(((B, 3, SIZE, SIZE), (B, SIZE, SIZE), (B, SIZE, SIZE)))]
    r = _renderer()
    r.geometry_grad = True
    _, shared, _ = _grads(r, tv, tf, tt, torch.tensor(R)[None], torch.tensor(t)[None], cot)
    _, each, _ = _grads(r, tv, tf, tt, torch.tensor(np.stack([R] * B)), torch.tensor(np.stack([t] * B)), cot)
    assert shared["R"].shape == (1, 3, 3) and each["R"].shape == (B, 3, 3) and shared["t"].shape == (1, 3)
    assert shared["R"][0].tobytes() == ((each["R"][0] + each["R"][1]) + each["R"][2]).tobytes() == each["R"].sum(0, dtype=np.float32).tobytes()
    assert shared["t"][0].tobytes() == ((each["t"][0] + each["t"][1]) + each["t"][2]).tobytes()
    assert np.array_equal(shared["v"], each["v"]) and backend["host_calls"] == 0
    r.close()


def test_the_new_names_are_in_header_signatures_and_exports():
    text = open(os.path.join(REPO, "include", "bodyfit.h")).read()
    for name in NEW_NAMES:
        assert f"int {name}(" in text, name
        assert name in _lib.SIGNATURES, name
    assert tuple(native.NR_DEV_SYMBOLS) == NEW_NAMES
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built - run __graft_entry__.build()")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_NAMES:
        assert hasattr(lib, name), name


def test_the_modules_switch_is_read_at_import_and_on_unless_switched_off():
    """BF_NR_DEVICE_ROUTE=0 keeps the Renderer alone on the host route; unset or anything else leaves its device route on (measured
    ahead of the parent commit's host route at the reference's loop size: profiles/nr_device_route.md)"""
    import subprocess
    import sys
    code = "import sys; sys.path.insert(0, %r); from bodyfitting_amd import neural_renderer as nr; print(int(nr.DEVICE_ROUTE))" % REPO
    for value, want in ((None, "1"), ("1", "1"), ("0", "0"), (" 0 ", "0"), ("yes", "1")):
        env = {k: v for k, v in os.environ.items() if k != "BF_NR_DEVICE_ROUTE"}
        if value is not None:
            env["BF_NR_DEVICE_ROUTE"] = value
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.strip() == want, (value, out.stdout, out.stderr[-500:])
    assert nr.DEVICE_ROUTE_DEFAULT == "1"
