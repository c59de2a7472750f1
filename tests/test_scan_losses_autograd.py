"""`utils.io_utils.compute_normal_torch` and `smplify.loss.point_cloud_loss_mesh_grid` / `normal_loss_mesh_grid` /
`normal_laplacian_smoothness` of the drop-in packages (bodyfitting_amd/normals.py, bodyfitting_amd/loss.py) on the CPU: parameter
lists, import names, the autograd Function, the caches, what is accepted and what is refused - with the native calls replaced by
float64 stand-ins over oracle.mesh_oracle and the closest-point search by oracle.mesh_oracle.nearest_bruteforce
(tests/scan_loss_cases.py; the HIP kernels themselves are held to the same oracle in tests/test_gpu_scan_losses.py)."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scan_loss_cases as SC
from oracle import mesh_oracle as MO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = inspect.Parameter.empty


@pytest.fixture
def L(monkeypatch):
    """bodyfitting_amd.loss with the stand-ins behind the native calls"""
    from bodyfitting_amd import loss
    SC.install_stand_ins(monkeypatch)
    return loss


@pytest.fixture
def searcher(L):
    from bodyfitting_amd.mesh_grid_searcher import MeshGridSearcher
    _, sv, sf, _ = SC.scan()
    return MeshGridSearcher(sv, sf)


def _freeze(searcher, pts):
    """the closest points of `pts`, held fixed for every later query (they are detached: finite differences must not move them)"""
    ids, near, _ = MO.nearest_bruteforce(searcher.verts, searcher.faces, np.asarray(pts, np.float32).reshape(-1, 3))
    searcher._scan.frozen = (ids, near.astype(np.float64))
    return ids, near


def test_the_four_parameter_lists_are_the_references():
    from bodyfitting_amd import loss as L
    from bodyfitting_amd import normals as NM

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    assert sig(NM.compute_normal_torch) == [("vertices", E), ("faces", E)]                                  # io_utils.py:410
    assert sig(L.point_cloud_loss_mesh_grid) == [("mesh_grid_searcher", E), ("points", E)]                  # loss.py:233
    # loss.py:260-261: the reference's four names in its order; the last two default to None here so that a call with two arguments
    # is refused by the function itself (NotImplementedError), as the stub it replaces did
    assert sig(L.normal_loss_mesh_grid) == [("mesh_grid_searcher", E), ("points", E), ("face_norm_mesh", None), ("point_norm", None)]
    assert sig(L.normal_laplacian_smoothness) == [("norms", E), ("faces", E)]                               # loss.py:273


def test_dropin_packages_resolve_by_the_reference_import_names(tmp_path):
    """smplify.py:14-16's import lines with dropin/ first on sys.path, in a child process; importing them does not import torch,
    and a name this project does not provide still comes from the caller's own utils/io_utils.py"""
    (tmp_path / "utils").mkdir()
    (tmp_path / "utils" / "__init__.py").write_text("")
    (tmp_path / "utils" / "io_utils.py").write_text("def compute_normal(*a):\n    return 'theirs'\ncompute_normal_torch = load_obj_mesh = None\n")
    code = """
import os, sys
import bodyfitting_amd
root = os.path.dirname(bodyfitting_amd.__file__)
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(root, "dropin"))
from utils.io_utils import load_obj_mesh, compute_normal, compute_normal_torch
from utils.mesh_grid_searcher import MeshGridSearcher
from smplify.loss import point_cloud_loss_mesh_grid, normal_loss_mesh_grid, normal_laplacian_smoothness
import utils.io_utils as IU
import bodyfitting_amd.loss as L, bodyfitting_amd.normals as NM, bodyfitting_amd.io as IO
assert IU.__file__.startswith(os.path.join(root, "dropin")), IU.__file__
assert compute_normal_torch is NM.compute_normal_torch and load_obj_mesh is IO.load_obj_mesh
assert compute_normal() == 'theirs'
assert point_cloud_loss_mesh_grid is L.point_cloud_loss_mesh_grid and normal_loss_mesh_grid is L.normal_loss_mesh_grid
assert normal_laplacian_smoothness is L.normal_laplacian_smoothness
assert not hasattr(IU, "no_such_name")
assert "torch" not in sys.modules
print("ok")
""" % str(tmp_path)
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=REPO, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


def test_compute_normal_torch_value_shape_and_gradcheck(L):
    from bodyfitting_amd.normals import compute_normal_torch
    verts, faces = SC.meshes()["fan9_lonely_vertex"]
    v = torch.tensor(verts, dtype=torch.float64).reshape(1, -1, 3).requires_grad_(True)          # [1,NV,3], as smplify.py:237 passes it
    f = torch.as_tensor(faces.astype(np.int64)).reshape(1, -1, 3)                                # (and smpl_faces may carry a batch axis)
    n = compute_normal_torch(v, f)
    assert n.shape == (len(verts), 3) and n.dtype == torch.float64 and n.requires_grad
    want = MO.compute_normal_torch(v.detach().reshape(-1, 3), f.reshape(-1, 3))
    torch.testing.assert_close(n, want, rtol=1e-12, atol=1e-14)
    assert not n[-1].any()                                                                      # the vertex in no face
    assert torch.autograd.gradcheck(lambda x: compute_normal_torch(x, f), (v,), eps=1e-6, atol=1e-5, rtol=1e-5)
    # a flat int32 faces tensor reads as faces.view(-1, 3) too
    torch.testing.assert_close(compute_normal_torch(v, torch.as_tensor(faces.reshape(-1))), want, rtol=1e-12, atol=1e-14)


def test_losses_values_and_gradcheck(L, searcher):
    _, sv, sf, fn = SC.scan()
    pts = torch.tensor(SC.points(65), dtype=torch.float64).reshape(1, -1, 3).requires_grad_(True)
    ids, near = _freeze(searcher, pts.detach().numpy())
    loss = L.point_cloud_loss_mesh_grid(searcher, pts)
    assert loss.shape == () and loss.dtype == torch.float64
    torch.testing.assert_close(loss, torch.norm(pts.detach().reshape(-1, 3) - torch.tensor(near, dtype=torch.float64)), rtol=1e-12, atol=0)
    assert torch.autograd.gradcheck(lambda p: L.point_cloud_loss_mesh_grid(searcher, p), (pts,), eps=1e-6, atol=1e-6, rtol=1e-5)

    fnt = torch.tensor(fn, dtype=torch.float64)
    pn = torch.tensor(SC.cotangent("pn", (65, 3)), dtype=torch.float64, requires_grad=True)
    nl = L.normal_loss_mesh_grid(searcher, pts, fnt, pn)
    assert nl.shape == ()
    torch.testing.assert_close(nl, torch.mean(1 - torch.sum(fnt[torch.as_tensor(ids.astype(np.int64))] * pn.detach(), -1)), rtol=1e-12, atol=1e-15)
    assert torch.autograd.gradcheck(lambda x: L.normal_loss_mesh_grid(searcher, pts, fnt, x), (pn,), eps=1e-6, atol=1e-7, rtol=1e-5)

    verts, faces = SC.meshes()["fan17"]
    norms = torch.tensor(SC.cotangent("lap", verts.shape), dtype=torch.float64).reshape(1, -1, 3).requires_grad_(True)
    ft = torch.as_tensor(faces.astype(np.int64))
    sm = L.normal_laplacian_smoothness(norms, ft)
    assert sm.shape == ()
    torch.testing.assert_close(sm, MO.normal_laplacian_smoothness(norms.detach().reshape(-1, 3), ft), rtol=1e-12, atol=0)
    assert torch.autograd.gradcheck(lambda x: L.normal_laplacian_smoothness(x, ft), (norms,), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_the_loop_of_smplify_py_236_245_end_to_end(L, searcher):
    """the gradient of the SMPL+D objective through all four functions equals autograd of the oracle"""
    from bodyfitting_amd.normals import compute_normal_torch
    model, base, faces = SC.body690()
    _, sv, sf, fn = SC.scan()
    body = torch.tensor(sv, dtype=torch.float64).reshape(1, -1, 3) * 1.01
    ids, near = _freeze(searcher, body.numpy())
    ft, fnt = torch.as_tensor(faces.astype(np.int64)), torch.tensor(fn, dtype=torch.float64)
    grads = []
    for fns in ((compute_normal_torch, L.point_cloud_loss_mesh_grid, L.normal_loss_mesh_grid, L.normal_laplacian_smoothness), None):
        disp = torch.zeros_like(body, requires_grad=True)
        deformed = body + disp
        if fns is not None:
            norms = fns[0](deformed, ft)
            loss = fns[1](searcher, deformed) + (fns[2](searcher, deformed, fnt, norms) + fns[3](norms, ft)) * 0.9 * 0.1
        else:
            norms = MO.compute_normal_torch(deformed.reshape(-1, 3), ft)
            loss = MO.point_cloud_loss(deformed, torch.tensor(near, dtype=torch.float64)) + (
                MO.normal_loss(fnt[torch.as_tensor(ids.astype(np.int64))], norms) + MO.normal_laplacian_smoothness(norms, ft)) * 0.9 * 0.1
        loss.backward()
        grads.append(disp.grad)
    assert grads[0].shape == body.shape
    torch.testing.assert_close(grads[0], grads[1], rtol=1e-9, atol=1e-12)


def test_gradients_only_where_asked_and_once(L, searcher):
    from bodyfitting_amd.normals import compute_normal_torch
    _, sv, sf, fn = SC.scan()
    verts, faces = SC.meshes()["fan8"]
    ft = torch.as_tensor(faces.astype(np.int64))
    v = torch.tensor(verts)
    assert not compute_normal_torch(v, ft).requires_grad
    pts, pn, fnt = torch.tensor(SC.points(64)), torch.tensor(SC.cotangent("pn", (64, 3))), torch.tensor(fn)
    before = SC.StandInScan.grads
    assert not L.point_cloud_loss_mesh_grid(searcher, pts).requires_grad
    assert not L.normal_loss_mesh_grid(searcher, pts, fnt, pn).requires_grad
    assert not L.normal_laplacian_smoothness(v, ft).requires_grad
    with torch.no_grad():
        assert not L.point_cloud_loss_mesh_grid(searcher, pts.clone().requires_grad_(True)).requires_grad
    assert SC.StandInScan.grads == before                                      # no gradient is computed when nothing asks for one
    # the normal loss: to point_norm only, although points requires grad
    p2, pn2 = pts.clone().requires_grad_(True), pn.clone().requires_grad_(True)
    L.normal_loss_mesh_grid(searcher, p2, fnt, pn2).backward()
    assert p2.grad is None and pn2.grad is not None and pn2.grad.shape == pn2.shape and pn2.grad.dtype == torch.float32
    # a cotangent scales the gradient that came with the forward; zero gives zeros
    p3 = pts.clone().requires_grad_(True)
    (L.point_cloud_loss_mesh_grid(searcher, p3) * 2.5).backward()
    p4 = pts.clone().requires_grad_(True)
    L.point_cloud_loss_mesh_grid(searcher, p4).backward()
    torch.testing.assert_close(p3.grad, 2.5 * p4.grad, rtol=1e-6, atol=0)
    p5 = pts.clone().requires_grad_(True)
    (L.point_cloud_loss_mesh_grid(searcher, p5) * 0.0).backward()
    assert not p5.grad.any()
    # once differentiable
    for f, x in ((lambda t: compute_normal_torch(t, ft).sum(), v), (lambda t: L.point_cloud_loss_mesh_grid(searcher, t), pts),
                 (lambda t: L.normal_loss_mesh_grid(searcher, pts, fnt, t), pn), (lambda t: L.normal_laplacian_smoothness(t, ft), v)):
        with pytest.raises(RuntimeError):
            z = x.clone().requires_grad_(True)
            g, = torch.autograd.grad(f(z), z, create_graph=True)
            g.sum().backward()


def test_numpy_in_gives_floats_and_arrays_out(L, searcher):
    from bodyfitting_amd.normals import compute_normal_torch
    _, sv, sf, fn = SC.scan()
    verts, faces = SC.meshes()["fan16"]
    n = compute_normal_torch(verts, faces)
    assert isinstance(n, np.ndarray) and n.shape == verts.shape and n.dtype == np.float32
    np.testing.assert_allclose(n, compute_normal_torch(torch.tensor(verts), torch.as_tensor(faces)).numpy(), rtol=0, atol=0)
    pts, pn = SC.points(63), SC.cotangent("pn", (63, 3))
    a, b, c = L.point_cloud_loss_mesh_grid(searcher, pts), L.normal_loss_mesh_grid(searcher, pts, fn, pn), L.normal_laplacian_smoothness(n, faces)
    assert all(isinstance(x, float) for x in (a, b, c))
    t = (L.point_cloud_loss_mesh_grid(searcher, torch.tensor(pts)), L.normal_loss_mesh_grid(searcher, torch.tensor(pts), torch.tensor(fn), torch.tensor(pn)),
         L.normal_laplacian_smoothness(torch.tensor(n), torch.as_tensor(faces)))
    assert all(x.shape == () and x.dtype == torch.float32 for x in t)
    np.testing.assert_allclose([a, b, c], [float(x) for x in t], rtol=0, atol=0)


def test_refusals(monkeypatch):
    from bodyfitting_amd import loss as L
    from bodyfitting_amd import mesh_grid_searcher, native
    from bodyfitting_amd.normals import compute_normal_torch
    SC.install_stand_ins(monkeypatch)
    monkeypatch.undo()                                                          # (float32 is enforced again ...)
    for name, fn_ in (("Topology", SC.StandInTopology), ("vertex_normals", SC.stand_in_vertex_normals), ("normal_laplacian", SC.stand_in_normal_laplacian),
                      ("normal_loss", SC.stand_in_normal_loss)):
        monkeypatch.setattr(native, name, fn_)                                  # (... the native calls are still the stand-ins)
    monkeypatch.setattr(mesh_grid_searcher, "Scan", SC.StandInScan)
    _, sv, sf, fn = SC.scan()
    s = mesh_grid_searcher.MeshGridSearcher(sv, sf)
    pts, pn, fnt = torch.tensor(SC.points(64)), torch.tensor(SC.cotangent("pn", (64, 3))), torch.tensor(fn)
    verts, faces = SC.meshes()["fan7"]
    v, ft = torch.tensor(verts), torch.as_tensor(faces.astype(np.int64))
    assert L.normal_loss_mesh_grid(s, pts, fnt, pn).shape == ()
    # neither an array nor a tensor, or a foreign searcher: NotImplementedError naming SMPLify's fused stage
    for name in ("point_cloud_loss_mesh_grid", "normal_loss_mesh_grid", "normal_laplacian_smoothness"):
        with pytest.raises(NotImplementedError, match="SMPLify"):
            getattr(L, name)(None, None)
    for call in (lambda: L.point_cloud_loss_mesh_grid(object(), pts), lambda: L.point_cloud_loss_mesh_grid(s, [[0.0, 0.0, 0.0]]),
                 lambda: L.normal_loss_mesh_grid(s, pts), lambda: L.normal_loss_mesh_grid(s, pts, fnt, None),
                 lambda: L.normal_loss_mesh_grid(SC.StandInScan(sv, sf), pts, fnt, pn), lambda: L.normal_laplacian_smoothness(v, faces.tolist()),
                 lambda: compute_normal_torch(verts.tolist(), faces), lambda: compute_normal_torch(v, None)):
        with pytest.raises(NotImplementedError, match="SMPLify"):
            call()
    # every other refusal is a ValueError
    bad = [
        ("float32", lambda: compute_normal_torch(v.double(), ft)),
        ("float32", lambda: L.point_cloud_loss_mesh_grid(s, pts.double())),
        ("float32", lambda: L.normal_loss_mesh_grid(s, pts, fnt.double(), pn)),
        ("float32", lambda: L.normal_loss_mesh_grid(s, pts, fnt, pn.half())),
        ("float32", lambda: L.normal_laplacian_smoothness(verts.astype(np.float64), faces)),
        ("mix", lambda: compute_normal_torch(v, faces)),
        ("mix", lambda: L.normal_laplacian_smoothness(verts, ft)),
        ("mix", lambda: L.normal_loss_mesh_grid(s, pts, fn, pn)),
        ("dimension of 3", lambda: compute_normal_torch(v.reshape(-1, 2), ft)),
        ("dimension of 3", lambda: L.point_cloud_loss_mesh_grid(s, pts.reshape(-1, 2))),
        ("dimension of 3", lambda: L.normal_loss_mesh_grid(s, pts, fnt, pn.reshape(-1))),
        ("dimension of 3", lambda: L.normal_laplacian_smoothness(v.reshape(-1, 6), ft)),
        ("one row per face", lambda: L.normal_loss_mesh_grid(s, pts, fnt[:-1], pn)),
        ("rows", lambda: L.normal_loss_mesh_grid(s, pts, fnt, pn[:-1])),
        ("requires grad", lambda: compute_normal_torch(v, ft.float().requires_grad_(True))),
        ("requires grad", lambda: L.normal_loss_mesh_grid(s, pts, fnt.clone().requires_grad_(True), pn)),
        ("requires grad", lambda: L.point_cloud_loss_mesh_grid(mesh_grid_searcher.MeshGridSearcher(torch.tensor(sv, requires_grad=True), sf), pts)),
        ("set_mesh", lambda: L.point_cloud_loss_mesh_grid(mesh_grid_searcher.MeshGridSearcher(), pts)),
        ("set_mesh", lambda: L.normal_loss_mesh_grid(mesh_grid_searcher.MeshGridSearcher(), pts, fnt, pn)),
        ("integer", lambda: L.normal_laplacian_smoothness(v, ft.float())),
        ("multiple of 3", lambda: compute_normal_torch(v, ft.reshape(-1)[:-1])),
        ("outside", lambda: compute_normal_torch(v, ft + 1)),
        ("outside", lambda: L.normal_laplacian_smoothness(v, ft - 1)),
    ]
    for match, call in bad:
        with pytest.raises(ValueError, match=match):
            call()


def test_topology_cache_hit_miss_and_in_place_edit(L):
    from bodyfitting_amd.normals import compute_normal_torch
    verts, faces = SC.meshes()["fan9"]
    v, ft = torch.tensor(verts, requires_grad=True), torch.as_tensor(faces.astype(np.int64))
    start = SC.StandInTopology.created
    for _ in range(3):                                                          # a loop that passes the same tensor builds it once,
        n = compute_normal_torch(v + 0.0, ft)
        L.normal_laplacian_smoothness(n, ft)                                    # ... and the Laplacian of the same mesh shares it
    assert SC.StandInTopology.created == start + 1
    compute_normal_torch(v, ft.clone())                                         # another tensor: a miss
    assert SC.StandInTopology.created == start + 2
    before = compute_normal_torch(v, ft).detach().clone()
    ft[0] = ft[0][[1, 0, 2]]                                                    # an in-place edit is seen: face 0 flipped
    after = compute_normal_torch(v, ft).detach()
    assert SC.StandInTopology.created == start + 3
    assert not torch.equal(before, after)
    torch.testing.assert_close(after, MO.compute_normal_torch(v.detach().double(), ft).float(), rtol=0, atol=1e-7)
    # arrays: told apart by their bytes
    created = SC.StandInTopology.created
    compute_normal_torch(verts, faces); compute_normal_torch(verts, faces.copy())
    assert SC.StandInTopology.created == created + 1
    other = faces.copy(); other[0] = other[0][[1, 0, 2]]
    compute_normal_torch(verts, other)
    assert SC.StandInTopology.created == created + 2
    # the same faces for a mesh of another size is another topology
    compute_normal_torch(np.concatenate([verts, verts[:1]]), faces)
    assert SC.StandInTopology.created == created + 3


def test_search_reuse_one_search_for_two_losses(L, searcher):
    _, sv, sf, fn = SC.scan()
    pts, pn, fnt = torch.tensor(SC.points(65), requires_grad=True), torch.tensor(SC.cotangent("pn", (65, 3)), requires_grad=True), torch.tensor(fn)
    start = SC.StandInScan.searches
    deformed = pts.reshape(1, -1, 3) + 0.0
    (L.point_cloud_loss_mesh_grid(searcher, deformed) + L.normal_loss_mesh_grid(searcher, deformed, fnt, pn)).backward()
    assert SC.StandInScan.searches == start + 1                                 # smplify.py:239-240: the same points
    assert SC.NORMAL_LOSS_CALLS[-1] == ((65, 3), True, 0)                       # 65 gathered rows went up, not the scan's table
    L.normal_loss_mesh_grid(searcher, deformed.detach() + 1e-3, fnt, pn)        # other points: a search of its own
    assert SC.StandInScan.searches == start + 2
    L.normal_loss_mesh_grid(searcher, deformed.detach() + 1e-3, fnt, pn)
    assert SC.StandInScan.searches == start + 2
    L.point_cloud_loss_mesh_grid(searcher, deformed)                            # the point loss always searches (one call does both)
    assert SC.StandInScan.searches == start + 3
    ids = searcher.nearest_points(deformed.detach().reshape(-1, 3))[1]          # nearest_points itself neither reads nor feeds the cache
    assert SC.StandInScan.searches == start + 4 and len(ids) == 65
    searcher.set_mesh(sv, sf)                                                   # a new mesh forgets the last query
    L.normal_loss_mesh_grid(searcher, deformed, fnt, pn)
    assert SC.StandInScan.searches == start + 5


@pytest.mark.parametrize("name", SC.MESH_NAMES)
def test_every_gpu_mesh_case_is_well_posed(name):
    """float32 autograd of the oracle within 1e-5 of float64, per block: tests/test_gpu_scan_losses.py needs no skip and no filter"""
    verts, faces = SC.all_meshes()[name]
    dn = SC.cotangent(name, verts.shape)
    n64, g64 = SC.ref_normals(verts, faces, dn, torch.float64)
    n32, g32 = SC.ref_normals(verts, faces, dn, torch.float32)
    SC.well_posed(name + " normals", n64, n32)
    SC.well_posed(name + " dverts", g64, g32)
    assert np.isfinite(g64).all() and np.abs(g64).max() > 0
    if name == SC.ZERO_AREA:
        others = np.abs(SC.ref_normals(*SC.fan(9, 5), dn[:-1], torch.float64)[1]).max()
        assert np.abs(g64).max() > 1e6 * others                                 # the degenerate face's dn / 1e-8
    if name == "fan9_lonely_vertex":
        assert not n64[-1].any() and not g64[-1].any()
    norms = SC.cotangent(name + " lap", verts.shape)
    v64, l64 = SC.ref_laplacian(norms, faces, torch.float64)
    v32, l32 = SC.ref_laplacian(norms, faces, torch.float32)
    SC.well_posed(name + " dnorms", l64, l32)
    assert abs(v32 - v64) <= SC.WELL_POSED * abs(v64)


@pytest.mark.parametrize("n", SC.POINT_COUNTS + ("on_vertices",))
def test_every_gpu_point_case_is_well_posed(n):
    _, sv, sf, fn = SC.scan()
    pts = SC.points_on_scan_vertices() if n == "on_vertices" else SC.points(n)
    ids, near, _ = MO.nearest_bruteforce(sv, sf, pts)
    v64, g64 = SC.ref_point_loss(pts, near, torch.float64)
    v32, g32 = SC.ref_point_loss(pts, near, torch.float32)
    SC.well_posed(f"points {n} dpoints", g64, g32)
    assert abs(v32 - v64) <= SC.WELL_POSED * abs(v64)
    if n == "on_vertices":
        assert v64 == 0 and not g64.any() and not g32.any() and np.isfinite(g32).all()           # torch: zero gradient at a zero norm
    else:
        assert v64 > 0 and (np.abs(pts - near).sum(1) == 0).sum() >= len(pts) // 5               # some points lie exactly on the scan
    pn = SC.cotangent(f"pn {n}", pts.shape)
    w64, h64 = SC.ref_normal_loss(fn[ids], pn, torch.float64)
    w32, h32 = SC.ref_normal_loss(fn[ids], pn, torch.float32)
    SC.well_posed(f"points {n} dpoint_norm", h64, h32)
    assert abs(w32 - w64) <= SC.WELL_POSED * abs(w64)
