"""The device route of the SMPL+D stage's losses and of the closest-point search in FRESH processes
(tests/test_gpu_scan_device_route.py).  Like tests/device_route_child.py, which this module imports first, torch is imported before the
library, so that both share one HIP runtime, and every function asserts the route it means to measure before it measures anything.

The yardstick is the host route of the same build - the numpy calls of `native` and the drop-in functions on CPU tensors, which
tests/test_gpu_scan_losses.py holds to the float64 oracle: the device route issues the same launches and must give the same BITS
(compared as uint32, so that -0.0 is not +0.0)."""
import os

import numpy as np
import torch                    # (first: see above)

from device_route_child import GPU, _busy, _guard_kept, _guarded, _repo, _took, _two_calls
from lanes_child import _run

COTANGENTS = (1.0, 2.5, -1.5)          # 1, one that is not 1, a negative one


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32) if a.dtype.kind == "f" else np.ascontiguousarray(a)


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), f"{what}: {int((g != w).sum())} of {g.size} words differ from the host route"


def _gpu(a, grad=False):
    return torch.tensor(a, device=GPU, requires_grad=grad)


def _stats():
    from bodyfitting_amd import native as N
    return N.dev_route_stats()


def _searcher():
    import scan_loss_cases as SC
    from bodyfitting_amd.mesh_grid_searcher import MeshGridSearcher
    _, sv, sf, fn = SC.scan()
    return MeshGridSearcher(sv, sf), fn


def _topologies():
    """name -> (verts, faces): the 690-vertex body; fans of nv - 2 faces around ONE hub with a vertex in no face, nv = 255, 256, 257
    (the vertex count on both sides of a block, the hub's list many adjacency batches long); strips of 255, 256, 257 faces (the face
    count on both sides of a block)"""
    import scan_loss_cases as SC
    out = {"body690": SC.body690()[1:]}
    for nv in (255, 256, 257):
        out[f"fan_nv{nv}"] = SC.fan(nv - 2, 2000 + nv, lonely=True)
        assert len(out[f"fan_nv{nv}"][0]) == nv
    for nf in (255, 256, 257):
        out[f"strip_nf{nf}"] = SC.strip(nf, 3000 + nf)
    return out


def _many_points(n, seed):
    """n query points near the scan (scan_loss_cases.points stops at the scan's 690 vertices)"""
    import scan_loss_cases as SC
    sv = SC.scan()[1]
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(sv[rng.integers(0, len(sv), n)] + rng.normal(0, 0.01, (n, 3)), np.float32)


def _loss_both_routes(f, x0, what, cotangents=COTANGENTS):
    """f(tensor) -> a scalar loss; on a CPU tensor (the host route) and on a GPU tensor (the device route): value and gradient bits
    for every cotangent.  -> the GPU value"""
    value = None
    for c in cotangents:
        res = {}
        for where in ("cpu", GPU):
            before = _stats()
            x = torch.tensor(x0, device=where, requires_grad=True)
            out = f(x)
            (out * c).backward()
            after = _stats()
            if where == GPU:
                assert out.device.type == "cuda" and x.grad.device.type == "cuda"
                assert after["host_calls"] == before["host_calls"] and after["dev_calls"] > before["dev_calls"], (what, before, after)
            else:
                assert after["dev_calls"] == before["dev_calls"] and after["host_calls"] > before["host_calls"], (what, before, after)
            assert out.shape == () and out.dtype == torch.float32
            res[where] = (out, x.grad)
        _same(res[GPU][0], res["cpu"][0], f"{what} value")
        _same(res[GPU][1], res["cpu"][1], f"{what} gradient x {c}")
        value = res[GPU][0]
    return value


def same_bits(out_path, which):
    def body():
        _repo()
        import scan_loss_cases as SC
        from bodyfitting_amd import loss as L, native as N
        from bodyfitting_amd.normals import compute_normal_torch
        _took("device")
        if which in ("normals", "laplacian"):
            for name, (verts, faces) in _topologies().items():
                topo = N.Topology(len(verts), faces)
                faces_gpu = torch.as_tensor(faces.astype(np.int64)).to(GPU)
                if which == "normals":
                    dn = SC.cotangent(name + " route", verts.shape)
                    want_n, want_g = N.vertex_normals(topo, verts), N.vertex_normals_vjp(topo, verts, dn)
                    before = _stats()
                    v = _gpu(verts.reshape(1, -1, 3), True)
                    n = compute_normal_torch(v, faces_gpu)
                    (n * _gpu(dn)).sum().backward()
                    after = _stats()
                    assert n.device.type == "cuda" and n.shape == (len(verts), 3) and v.grad.shape == v.shape
                    assert after["dev_calls"] == before["dev_calls"] + 2 and after["host_calls"] == before["host_calls"], (before, after)
                    _same(n, want_n, f"{name} normals")
                    _same(v.grad.reshape(-1, 3), want_g, f"{name} dverts")
                    if name.startswith("fan"):
                        assert not _bits(n[-1]).any() and not _bits(v.grad[0, -1]).any()          # the vertex in no face
                else:
                    norms = SC.cotangent(name + " lap route", verts.shape)
                    faces_cpu = torch.as_tensor(faces.astype(np.int64))
                    _loss_both_routes(lambda x: L.normal_laplacian_smoothness(x, faces_gpu if x.is_cuda else faces_cpu), norms,
                                      f"{name} laplacian")
                topo.close()
            return {"ok": np.ones(1)}
        searcher, fn = _searcher()
        if which == "point":
            # the closest-point launch is (n + 3) / 4 groups, the reductions are 256 wide
            for n in (1, 3, 4, 5, 255, 256, 257):
                _loss_both_routes(lambda x: L.point_cloud_loss_mesh_grid(searcher, x), SC.points(n), f"point loss n={n}")
            # points ON the scan: the loss is 0 and the gradient exactly 0
            on = SC.points_on_scan_vertices()
            value = _loss_both_routes(lambda x: L.point_cloud_loss_mesh_grid(searcher, x), on, "points on the scan")
            assert float(value.detach()) == 0.0
            x = _gpu(on, True)
            (L.point_cloud_loss_mesh_grid(searcher, x) * 3.0).backward()
            assert not _bits(x.grad).any()
        elif which == "point_large":
            # 65,537 points: 257 block sums, so bf_ml_finish_kernel's threads loop
            _loss_both_routes(lambda x: L.point_cloud_loss_mesh_grid(searcher, x), _many_points(65537, 9), "point loss n=65537", (2.5,))
        else:
            assert which == "normal"
            # face_norm_mesh un-normalised, as smplify.py:149 builds it
            assert np.abs(np.linalg.norm(fn, axis=1) - 1).max() > 0.5
            fn_t = {"cpu": torch.tensor(fn), GPU: _gpu(fn)}
            for n in (1, 256, 257):
                pts = SC.points(n)
                pts_t = {"cpu": torch.tensor(pts), GPU: _gpu(pts)}
                key = lambda x: GPU if x.is_cuda else "cpu"
                _loss_both_routes(lambda x: L.normal_loss_mesh_grid(searcher, pts_t[key(x)], fn_t[key(x)], x),
                                  SC.cotangent(f"pn route {n}", pts.shape), f"normal loss n={n}")
        searcher.close()
        return {"ok": np.ones(1)}

    _run(out_path, body)


def oracle_band(out_path):
    """independent of the host route: one case per function against float64 autograd of oracle/mesh_oracle.py, in
    tests/scan_loss_cases.py's band (the one tests/test_gpu_scan_losses.py uses)"""
    def body():
        _repo()
        import scan_loss_cases as SC
        from bodyfitting_amd import loss as L
        from bodyfitting_amd.normals import compute_normal_torch
        _took("device")
        band = SC.Band()
        _, verts, faces = SC.body690()
        faces_gpu = torch.as_tensor(faces.astype(np.int64)).to(GPU)
        dn = SC.cotangent("band route", verts.shape)
        v = _gpu(verts, True)
        n = compute_normal_torch(v, faces_gpu)
        (n * _gpu(dn)).sum().backward()
        n64, g64 = SC.ref_normals(verts, faces, dn, torch.float64)
        n32, g32 = SC.ref_normals(verts, faces, dn, torch.float32)
        band.block("normals", n.detach().cpu().numpy(), n64, n32)
        band.block("dverts", v.grad.cpu().numpy(), g64, g32)
        x = _gpu(dn, True)
        value = L.normal_laplacian_smoothness(x, faces_gpu)
        value.backward()
        v64, l64 = SC.ref_laplacian(dn, faces, torch.float64)
        v32, l32 = SC.ref_laplacian(dn, faces, torch.float32)
        band.value("laplacian", float(value.detach()), v64, v32)
        band.block("dnorms", x.grad.cpu().numpy(), l64, l32)
        searcher, fn = _searcher()
        pts = SC.points(257)
        p = _gpu(pts, True)
        near, ids = searcher.nearest_points(p)
        assert near.device.type == "cuda"
        near, ids = near.cpu().numpy(), ids.cpu().numpy()
        value = L.point_cloud_loss_mesh_grid(searcher, p)
        value.backward()
        v64, g64 = SC.ref_point_loss(pts, near, torch.float64)
        v32, g32 = SC.ref_point_loss(pts, near, torch.float32)
        band.value("point loss", float(value.detach()), v64, v32)
        band.block("dpoints", p.grad.cpu().numpy(), g64, g32)
        pn0 = SC.cotangent("pn band route", pts.shape)
        pn = _gpu(pn0, True)
        value = L.normal_loss_mesh_grid(searcher, p.detach(), _gpu(fn), pn)
        value.backward()
        w64, h64 = SC.ref_normal_loss(fn[ids], pn0, torch.float64)
        w32, h32 = SC.ref_normal_loss(fn[ids], pn0, torch.float32)
        band.value("normal loss", float(value.detach()), w64, w32)
        band.block("dpoint_norm", pn.grad.cpu().numpy(), h64, h32)
        searcher.close()
        return {"ok": np.ones(1)}

    _run(out_path, body)


def gather_alone(out_path):
    """bf_normal_loss_dev by itself against table[ids] in numpy followed by the host bf_normal_loss: ids that hit face 0 and face
    NF - 1, repeated ids, n no multiple of 256; an id outside the table is not read and contributes what the header says.  Then the
    scaling launch against numpy's float32 g * c and g * c + 0.0."""
    def body():
        _repo()
        from bodyfitting_amd import native as N
        _took("device")
        rng = np.random.default_rng(21)
        nf, stream = 1000, torch.cuda.current_stream().cuda_stream
        table = rng.normal(0, 2.0, (nf, 3)).astype(np.float32)
        table_t = _gpu(table)
        ws = N.Workspace(0)
        for n in (1, 300, 513):
            ids = rng.integers(0, nf, n).astype(np.int32)
            ids[0] = nf - 1
            if n > 1:
                ids[1], ids[2:40] = 0, 7                      # face 0; one face many times
                ids[-1] = 0
            pn = rng.normal(size=(n, 3)).astype(np.float32)
            want, dwant = N.normal_loss(table[ids], pn)
            loss, dpn = torch.empty(1, device=GPU), torch.empty((n, 3), device=GPU)
            ids_t, pn_t = _gpu(ids), _gpu(pn)                 # (held: the launch reads them after this line)
            N.normal_loss_dev(ws, stream, n, ids_t.data_ptr(), table_t.data_ptr(), nf, pn_t.data_ptr(), loss=loss.data_ptr(),
                              dpoint_norms=dpn.data_ptr())
            _same(loss, np.asarray(want).reshape(1), f"gather n={n} loss")
            _same(dpn, dwant, f"gather n={n} dpoint_norms")
            only = torch.empty(1, device=GPU)
            N.normal_loss_dev(ws, stream, n, ids_t.data_ptr(), table_t.data_ptr(), nf, pn_t.data_ptr(), loss=only.data_ptr())
            _same(only, loss, f"gather n={n} loss without the gradient")
        # ids outside [0, nf): the row adds 0 to the sum (the mean divides by n) and its gradient row is zero
        n = 300
        ids = rng.integers(0, nf, n).astype(np.int32)
        ids[3], ids[299] = -1, nf
        pn = rng.normal(size=(n, 3)).astype(np.float32)
        inside = np.ones(n, bool)
        inside[[3, 299]] = False
        rows = 1.0 - (table[ids[inside]].astype(np.float64) * pn[inside]).sum(1)
        loss, dpn = torch.empty(1, device=GPU), torch.full((n, 3), 9.0, device=GPU)
        ids_t, pn_t = _gpu(ids), _gpu(pn)
        N.normal_loss_dev(ws, stream, n, ids_t.data_ptr(), table_t.data_ptr(), nf, pn_t.data_ptr(), loss=loss.data_ptr(),
                          dpoint_norms=dpn.data_ptr())
        assert abs(float(loss) - rows.sum() / n) <= 1e-5 * np.abs(rows).sum() / n
        assert not _bits(dpn[3]).any() and not _bits(dpn[299]).any()
        beside = N.normal_loss(table[np.clip(ids, 0, nf - 1)], pn)[1]          # (the same n: the other rows' gradients are the host call's)
        _same(dpn.cpu().numpy()[inside], beside[inside], "rows beside an id outside the table")
        # the scaling launch: zeros of both signs, a denormal product, counts on both sides of a block
        for n in (1, 255, 256, 257, 2070):
            g = rng.normal(size=n).astype(np.float32)
            g[::7] = 0.0
            g[3::11] = -0.0
            g[5::13] = 1e-30
            for c in (2.5, -1.5, 0.0, -0.0, 1e-10):
                c32 = np.float32(c)
                for plus_zero, want in ((False, g * c32), (True, g * c32 + np.float32(0.0))):
                    out, g_t, c_t = torch.empty(n, device=GPU), _gpu(g), _gpu(np.array(c32))
                    N.scale_gradient_dev(0, stream, n, g_t.data_ptr(), c_t.data_ptr(), out.data_ptr(), plus_zero=plus_zero)
                    _same(out, want, f"scale n={n} c={c} plus_zero={plus_zero}")
        torch.cuda.synchronize()
        ws.close()
        return {"ok": np.ones(1)}

    _run(out_path, body)


def optional_outputs(out_path):
    """the NULL / non-NULL choices of the outputs through the *_dev entries: bf_scan_point_loss_dev at 1, 5 and 257 points (all 16),
    bf_normal_laplacian_dev on the 257-vertex fan and bf_normal_loss_dev at 257 points (loss only, gradient only, both, neither).
    Every output asked for holds the bits of the host route's all-outputs call and nothing is written behind it"""
    def body():
        _repo()
        import scan_loss_cases as SC
        from bodyfitting_amd import native as N
        _took("device")
        searcher, fn = _searcher()
        scan, stream = searcher._scan, torch.cuda.current_stream().cuda_stream
        for n in (1, 5, 257):
            pts = SC.points(n)
            value, ids, near, dp = scan.point_loss(pts)
            want = {"loss": np.asarray(value).reshape(1), "face_ids": ids, "nearest": near, "dpoints": dp}
            pts_t = _gpu(pts)
            for mask in range(16):
                names = [k for i, k in enumerate(want) if (mask >> i) & 1]

                def call():
                    out = {k: _guarded(want[k].size) for k in names}
                    scan.point_loss_dev(n, stream, pts_t.data_ptr(), **{k: a for k, (_, a) in out.items()})
                    return out
                for k, (t, _) in _two_calls(call, f"point loss n={n} {names}").items():
                    got = t[:want[k].size].cpu().numpy()
                    assert got.tobytes() == np.ascontiguousarray(want[k]).tobytes(), f"point loss n={n} {names}: {k} differs from the host route"
                    _guard_kept(t, want[k].size, f"point loss n={n} {names} {k}")
        verts, faces = SC.fan(255, 2257, lonely=True)
        topo = N.Topology(len(verts), faces)
        norms = SC.cotangent("fan257 optional", verts.shape)
        pts, pn = SC.points(257), SC.cotangent("pn optional", (257, 3))
        ids = scan.point_loss(pts)[1]
        host = {"laplacian": N.normal_laplacian(topo, norms), "normal loss": N.normal_loss(fn[ids], pn)}
        norms_t, pn_t, ids_t, fn_t = _gpu(norms), _gpu(pn), _gpu(ids), _gpu(fn)
        ws = N.Workspace(0)
        entries = {"laplacian": lambda loss, grad: N.normal_laplacian_dev(topo, stream, norms_t.data_ptr(), loss=loss, dnorms=grad),
                   "normal loss": lambda loss, grad: N.normal_loss_dev(ws, stream, 257, ids_t.data_ptr(), fn_t.data_ptr(), len(fn), pn_t.data_ptr(),
                                                                       loss=loss, dpoint_norms=grad)}
        for name, entry in entries.items():
            for want_loss, want_grad in ((True, False), (False, True), (True, True), (False, False)):
                def call():
                    loss, grad = _guarded(1) if want_loss else (None, 0), _guarded(257 * 3) if want_grad else (None, 0)
                    entry(loss[1], grad[1])
                    return loss[0], grad[0]
                what = f"{name} loss={want_loss} gradient={want_grad}"
                loss, grad = _two_calls(call, what)
                for t, w, on in ((loss, np.asarray(host[name][0]).reshape(1), want_loss), (grad, host[name][1], want_grad)):
                    if on:
                        assert t[:w.size].cpu().numpy().tobytes() == np.ascontiguousarray(w).tobytes(), f"{what}: differs from the host route"
                        _guard_kept(t, w.size, what)
        torch.cuda.synchronize()
        ws.close()
        topo.close()
        searcher.close()
        return {"ok": np.ones(1)}

    _run(out_path, body)


def nearest_tensors(out_path):
    """nearest_points / nearest_points_with_coefficients on CUDA tensors: the numpy call's bits, on the tensors' device"""
    def body():
        _repo()
        import scan_loss_cases as SC
        _took("device")
        searcher, _ = _searcher()
        for n in (1, 5, 257, 690):
            pts = SC.points(n)
            want = searcher.nearest_points_with_coefficients(pts)
            before = _stats()
            near, ids = searcher.nearest_points(_gpu(pts))
            near2, ids2, bary = searcher.nearest_points_with_coefficients(_gpu(pts.reshape(1, n, 3)))
            after = _stats()
            assert after["dev_calls"] == before["dev_calls"] + 2 and after["host_calls"] == before["host_calls"]
            for t in (near, ids, near2, ids2, bary):
                assert t.device == torch.device(GPU) and not t.requires_grad
            assert ids.dtype == torch.int32 and ids2.dtype == torch.int32 and near.shape == (n, 3) and bary.shape == (n, 3)
            for got, w, name in ((near, want[0], "nearest"), (ids, want[1], "ids"), (near2, want[0], "nearest (coefficients call)"),
                                 (ids2, want[1], "ids (coefficients call)"), (bary, want[2], "coefficients")):
                _same(got, w, f"n={n} {name}")
        searcher.close()
        return {"ok": np.ones(1)}

    _run(out_path, body)


def _smpld_loop(steps, after_step=None):
    """smplify.py:229-245 as written, on the 690-vertex body against the 1376-face scan, everything on cuda:0 -> disp"""
    import scan_loss_cases as SC
    from bodyfitting_amd.loss import normal_laplacian_smoothness, normal_loss_mesh_grid, point_cloud_loss_mesh_grid
    from bodyfitting_amd.mesh_grid_searcher import MeshGridSearcher
    from bodyfitting_amd.normals import compute_normal_torch
    device = torch.device(GPU)
    _, verts, faces = SC.body690()
    _, scan_verts, scan_faces, _ = SC.scan()
    tris = scan_verts[scan_faces]
    face_norms = torch.from_numpy(np.cross(tris[::, 1] - tris[::, 0], tris[::, 2] - tris[::, 0])).float().to(device)
    constant_scale = float((scan_verts.max(0) - scan_verts.min(0))[1] / 1.7)
    pointsearcher = MeshGridSearcher(verts=scan_verts, faces=scan_faces)
    body_vertices = torch.from_numpy(verts).reshape(1, -1, 3).to(device)
    disp = torch.zeros_like(body_vertices)
    body_vertices = body_vertices.detach()
    disp.requires_grad = True
    optimizer = torch.optim.Adam([disp], lr=5e-2, betas=(0.9, 0.999))
    smpl_faces = torch.from_numpy(faces).long().to(device)
    for i in range(steps):
        deformed_verts = body_vertices + disp
        deformed_norms = compute_normal_torch(deformed_verts, smpl_faces)
        icp_loss = point_cloud_loss_mesh_grid(pointsearcher, deformed_verts)
        norm_loss = normal_loss_mesh_grid(pointsearcher, deformed_verts, face_norms, deformed_norms)
        smoothness = normal_laplacian_smoothness(deformed_norms, smpl_faces)
        loss = icp_loss + (norm_loss + smoothness) * constant_scale * 0.1
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        if after_step:
            after_step(i)
    out = disp.detach().cpu().numpy()
    pointsearcher.close()
    return out


# per step of the SMPL+D loop, in its order: bf_vertex_normals_dev (compute_normal_torch), bf_scan_point_loss_dev (the ONE search of the
# step and the point loss), bf_normal_loss_dev (its ids are the memo's: no bf_scan_nearest_dev), bf_normal_laplacian_dev; then the
# backward: one bf_scale_gradient_dev per scalar loss (three) and bf_vertex_normals_vjp_dev once, on the summed cotangent of the normals
DEV_CALLS_PER_STEP = 4 + 3 + 1


def smpld_loop(out_path, switched_off):
    """ten iterations; switched_off: the same loop on the host route (BF_TORCH_DEVICE_ROUTE=0), for the parent to compare"""
    if switched_off:
        os.environ["BF_TORCH_DEVICE_ROUTE"] = "0"
    else:
        os.environ.pop("BF_TORCH_DEVICE_ROUTE", None)

    def body():
        _repo()
        _took("host" if switched_off else "device")
        seen = []
        start = _stats()
        disp = _smpld_loop(10, lambda i: seen.append(_stats()))
        end = seen[-1]
        assert np.isfinite(disp).all() and np.abs(disp).max() > 1e-3
        if switched_off:
            assert end["dev_calls"] == start["dev_calls"] and end["host_calls"] > start["host_calls"], (start, end)
            return {"disp": disp}
        assert end["host_calls"] == start["host_calls"], (start, end)
        assert [s["dev_calls"] - start["dev_calls"] for s in seen] == [DEV_CALLS_PER_STEP * (i + 1) for i in range(10)], (start, seen)
        assert seen[0]["allocations"] > start["allocations"]
        assert all(s["allocations"] == seen[0]["allocations"] for s in seen), [s["allocations"] for s in seen]
        assert end["stream_switches"] == start["stream_switches"]
        return {"disp": disp}

    _run(out_path, body)


def memo(out_path):
    """the device route's memo: a hit only for the same tensor at the same version, never a stale answer"""
    def body():
        _repo()
        import scan_loss_cases as SC
        from bodyfitting_amd import loss as L
        from bodyfitting_amd.mesh_grid_searcher import MeshGridSearcher
        _took("device")
        searcher, fn = _searcher()
        fn_gpu = _gpu(fn)
        pts_a = SC.points(257)
        pn = SC.cotangent("pn memo", (257, 3))
        pn_gpu = _gpu(pn)

        def host_normal_loss(s, pts, face_norms, normals):
            return L.normal_loss_mesh_grid(s, torch.tensor(pts), torch.tensor(face_norms), torch.tensor(normals))

        def dev_calls(f):
            before = _stats()
            out = f()
            after = _stats()
            assert after["host_calls"] == before["host_calls"]
            return out, after["dev_calls"] - before["dev_calls"]

        want_a = host_normal_loss(searcher, pts_a, fn, pn)
        # the same tensor, untouched: one search for the two losses
        p = _gpu(pts_a)
        _, calls = dev_calls(lambda: L.point_cloud_loss_mesh_grid(searcher, p))
        assert calls == 1
        got, calls = dev_calls(lambda: L.normal_loss_mesh_grid(searcher, p, fn_gpu, pn_gpu))
        assert calls == 1, "the memo missed the tensor it was made for"
        _same(got, want_a, "memo hit")
        # modified in place between the two losses: a second search, the answer for the NEW contents
        moved = pts_a + np.float32(0.02)
        want_moved = host_normal_loss(searcher, moved, fn, pn)
        L.point_cloud_loss_mesh_grid(searcher, p)
        p.add_(0.02)
        _same(p, moved, "the in-place edit")
        got, calls = dev_calls(lambda: L.normal_loss_mesh_grid(searcher, p, fn_gpu, pn_gpu))
        assert calls == 2, "an in-place edit must search again"
        _same(got, want_moved, "after an in-place edit")
        # a fresh tensor with equal contents: a second search, the same result
        L.point_cloud_loss_mesh_grid(searcher, p)
        twin = p.clone()
        got, calls = dev_calls(lambda: L.normal_loss_mesh_grid(searcher, twin, fn_gpu, pn_gpu))
        assert calls == 2, "a different tensor must search again"
        _same(got, want_moved, "a fresh tensor with equal contents")
        # the previous tensor deleted, a new one allocated - the memo holds the old one, so the new one cannot be taken for it
        q = _gpu(pts_a)
        L.point_cloud_loss_mesh_grid(searcher, q)
        address = q.data_ptr()
        del q
        q2 = _gpu(moved)
        got, calls = dev_calls(lambda: L.normal_loss_mesh_grid(searcher, q2, fn_gpu, pn_gpu))
        assert calls == 2 and q2.data_ptr() != address, "the memo keeps its tensor alive: its address cannot come back"
        _same(got, want_moved, "a new tensor after the old one was deleted")
        # set_mesh with another scan: no stale ids
        sv, sf = SC.scan()[1:3]
        sv2 = np.ascontiguousarray(sv[:, [1, 2, 0]] * np.float32(1.1))
        tris = sv2[sf]
        fn2 = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]).astype(np.float32)
        other = MeshGridSearcher(sv2, sf)
        want_other = host_normal_loss(other, pts_a, fn2, pn)
        other.close()
        q4 = _gpu(pts_a)
        L.point_cloud_loss_mesh_grid(searcher, q4)
        searcher.set_mesh(sv2, sf)
        assert searcher._last_query_dev is None and searcher._last_query is None
        got, calls = dev_calls(lambda: L.normal_loss_mesh_grid(searcher, q4, _gpu(fn2), pn_gpu))
        assert calls == 2
        _same(got, want_other, "after set_mesh")
        searcher.close()
        assert searcher._last_query_dev is None
        return {"ok": np.ones(1)}

    _run(out_path, body)


def stream_order(out_path):
    def body():
        _repo()
        import scan_loss_cases as SC
        from bodyfitting_amd import loss as L
        from bodyfitting_amd.normals import compute_normal_torch
        _took("device")
        searcher, fn = _searcher()
        _, verts, faces = SC.body690()
        faces_gpu, fn_gpu = torch.as_tensor(faces.astype(np.int64)).to(GPU), _gpu(fn)

        def step(v):
            n = compute_normal_torch(v, faces_gpu)
            loss = L.point_cloud_loss_mesh_grid(searcher, v) * 0.7 + L.normal_loss_mesh_grid(searcher, v, fn_gpu, n) * -1.3 + \
                L.normal_laplacian_smoothness(n, faces_gpu) * 2.1
            loss.backward()
            return loss

        # the reference: the same step on the current stream, drained
        ref_v = _gpu(verts, True)
        ref_loss = step(ref_v)
        torch.cuda.synchronize()
        ref = ref_loss.detach().cpu().numpy(), ref_v.grad.cpu().numpy()

        def on_stream(s):
            """vertices produced on `s` behind a long chain, forward and backward queued with no synchronisation in between"""
            with torch.cuda.stream(s):
                zero = _busy()
                v = (_gpu(verts) + zero).requires_grad_(True)
                return v, step(v)

        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        before = _stats()
        v, loss = on_stream(s1)
        torch.cuda.synchronize()
        _same(loss, ref[0], "loss on a side stream")
        _same(v.grad, ref[1], "gradient on a side stream")
        mid = _stats()
        assert mid["host_calls"] == before["host_calls"] and mid["dev_calls"] == before["dev_calls"] + 8
        # two streams alternating on one searcher and one topology: each call waits for the one before it on the other stream
        runs = [on_stream(s) for s in (s2, s1, s2, s1)]
        torch.cuda.synchronize()
        for v, loss in runs:
            _same(loss, ref[0], "loss, alternating streams")
            _same(v.grad, ref[1], "gradient, alternating streams")
        after = _stats()
        assert after["stream_switches"] >= mid["stream_switches"] + 4, (mid, after)
        searcher.close()
        return {"ok": np.ones(1)}

    _run(out_path, body)


def fallbacks(out_path, switched_off):
    """switched_off: BF_TORCH_DEVICE_ROUTE=0 - GPU tensors give the host route's bits through the host entry points alone.  Else: CPU
    tensors and float64 take the host route (or are refused as before), tensors of another GPU than the scan's take it too (where
    there are two), and the *_dev entries refuse a NULL workspace, n = 0 and n beyond the limit before anything is queued."""
    if switched_off:
        os.environ["BF_TORCH_DEVICE_ROUTE"] = "0"
    else:
        os.environ.pop("BF_TORCH_DEVICE_ROUTE", None)

    def body():
        _repo()
        import ctypes as C
        import scan_loss_cases as SC
        from bodyfitting_amd import _lib, loss as L, native as N
        from bodyfitting_amd.normals import compute_normal_torch
        _took("host" if switched_off else "device")
        searcher, fn = _searcher()
        _, verts, faces = SC.body690()
        pts, pn = SC.points(257), SC.cotangent("pn fallbacks", (257, 3))
        dn = SC.cotangent("dn fallbacks", verts.shape)

        def everything(where, dtype=torch.float32):
            """the four functions and the searcher on tensors of `where` -> their values and gradients"""
            t = lambda a, grad=False: torch.tensor(a, device=where, dtype=dtype, requires_grad=grad)
            f = torch.as_tensor(faces.astype(np.int64)).to(where)
            v, p, q = t(verts, True), t(pts, True), t(pn, True)
            n = compute_normal_torch(v, f)
            (n * t(dn)).sum().backward()
            out = [n, v.grad]
            for loss, x in ((L.point_cloud_loss_mesh_grid(searcher, p), p), (L.normal_loss_mesh_grid(searcher, p.detach(), t(fn), q), q)):
                (loss * -2.5).backward()
                out += [loss, x.grad]
            x = t(dn, True)
            loss = L.normal_laplacian_smoothness(x, f)
            (loss * 1.5).backward()
            out += [loss, x.grad]
            near, ids, bary = searcher.nearest_points_with_coefficients(p.detach())
            assert all(o.device.type == torch.device(where).type for o in out + [near, ids, bary])
            return out + [near, ids, bary]

        before = _stats()
        want = everything("cpu")
        after = _stats()
        assert after["dev_calls"] == before["dev_calls"] and after["host_calls"] > before["host_calls"], "CPU tensors"
        if switched_off:
            got = everything(GPU)
            assert _stats()["dev_calls"] == before["dev_calls"], "the switch is off"
            for i, (g, w) in enumerate(zip(got, want)):
                _same(g, w, f"switched off, output {i}")
            searcher.close()
            return {"ok": np.ones(1)}
        got = everything(GPU)
        assert _stats()["dev_calls"] > before["dev_calls"]
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"output {i}")
        # float64: the searcher converts and goes through the host, the losses refuse it, as they always have
        before = _stats()
        near, ids = searcher.nearest_points(torch.tensor(pts, device=GPU, dtype=torch.float64))
        _same(near, want[-3], "float64 nearest")
        _same(ids, want[-2], "float64 ids")
        for call in (lambda: L.point_cloud_loss_mesh_grid(searcher, torch.tensor(pts, device=GPU, dtype=torch.float64)),
                     lambda: compute_normal_torch(torch.tensor(verts, device=GPU, dtype=torch.float64), torch.as_tensor(faces.astype(np.int64)))):
            try:
                call()
            except ValueError:
                continue
            raise AssertionError("float64 was not refused")
        assert _stats()["dev_calls"] == before["dev_calls"], "float64"
        # tensors on another GPU than the scan's
        if torch.cuda.device_count() > 1:
            got = everything("cuda:1")
            assert _stats()["dev_calls"] == before["dev_calls"], "another GPU"
            for i, (g, w) in enumerate(zip(got, want)):
                _same(g, w, f"cuda:1, output {i}")
        else:
            print("one GPU: tensors of another GPU not tried")
        # refusals, each before anything is queued
        lib = _lib.load()
        topo = N.Topology(len(verts), faces)
        ws = N.Workspace(0)
        stream = torch.cuda.current_stream().cuda_stream
        a_t, i32_t = torch.zeros(4 * len(verts), device=GPU), torch.zeros(16, device=GPU, dtype=torch.int32)
        a, i32 = C.c_void_p(a_t.data_ptr()), C.c_void_p(i32_t.data_ptr())
        scan, big = searcher._scan._h, (1 << 28) + 1
        calls = _stats()
        INVALID, UNSUPPORTED = -1, -3
        refusals = [
            (lib.bf_vertex_normals_dev(topo._h, a, a, None, None), INVALID),
            (lib.bf_vertex_normals_vjp_dev(topo._h, a, a, a, None, None), INVALID),
            (lib.bf_normal_laplacian_dev(topo._h, a, a, a, None, None), INVALID),
            (lib.bf_scan_point_loss_dev(scan, 1, a, a, None, None, None, None, None), INVALID),
            (lib.bf_scan_nearest_dev(scan, 1, a, i32, a, None, None, None), INVALID),
            (lib.bf_normal_loss_dev(0, 1, i32, a, 4, a, a, None, None, None), INVALID),
            (lib.bf_scan_point_loss_dev(scan, 0, a, a, None, None, None, ws._h, None), INVALID),
            (lib.bf_scan_nearest_dev(scan, 0, a, i32, a, None, ws._h, None), INVALID),
            (lib.bf_normal_loss_dev(0, 0, i32, a, 4, a, a, None, ws._h, None), INVALID),
            (lib.bf_scale_gradient_dev(0, 0, a, a, 0, a, None), INVALID),
            (lib.bf_scan_point_loss_dev(scan, big, a, a, None, None, None, ws._h, None), UNSUPPORTED),
            (lib.bf_scan_nearest_dev(scan, big, a, i32, a, None, ws._h, None), UNSUPPORTED),
            (lib.bf_normal_loss_dev(0, big, i32, a, 4, a, a, None, ws._h, None), UNSUPPORTED),
            (lib.bf_normal_loss_dev(0, 1, i32, a, big, a, a, None, ws._h, None), UNSUPPORTED),
            (lib.bf_scale_gradient_dev(0, big, a, a, 0, a, None), UNSUPPORTED),
            (lib.bf_vertex_normals_dev(None, a, a, ws._h, None), INVALID),
            (lib.bf_scan_point_loss_dev(None, 1, a, a, None, None, None, ws._h, None), INVALID),
            (lib.bf_normal_loss_dev(0, 1, None, a, 4, a, a, None, ws._h, None), INVALID),
        ]
        assert [r for r, _ in refusals] == [w for _, w in refusals], refusals
        assert b"bf_normal_loss_dev" in lib.bf_last_error()
        now = _stats()
        assert now["dev_calls"] == calls["dev_calls"] and now["allocations"] == calls["allocations"], "a refused call counted or allocated"
        torch.cuda.synchronize()                                  # (raises if a HIP error was left behind in the shared runtime)
        assert torch.cuda.current_device() == 0
        # ... and the next call succeeds
        out, v_t = torch.empty((len(verts), 3), device=GPU), _gpu(verts)
        N.vertex_normals_dev(topo, stream, v_t.data_ptr(), out.data_ptr(), ws=ws)
        _same(out, want[0], "bf_vertex_normals_dev after the refusals")
        ws.close()
        topo.close()
        searcher.close()
        return {"ok": np.ones(1)}

    _run(out_path, body)


def nearest_outputs(out_path):
    """bf_scan_nearest and bf_scan_nearest_dev at n = 1, 3, 4, 5 and 257 points (the launch is (n + 3) / 4 groups) with each non-empty
    subset of (face_ids, nearest, bary): the words of the all-outputs call, the host call and the *_dev call agreeing word for word,
    nothing written behind an output of the device route and no allocation on a second identical call.  bf_scan_nearest counts one
    host call and nothing else.  Then the refusals of both entries, each before anything is queued or counted."""
    def body():
        _repo()
        import ctypes as C
        import scan_loss_cases as SC
        from bodyfitting_amd import _lib, native as N
        _took("device")
        lib = _lib.load()
        searcher, _ = _searcher()
        scan, stream = searcher._scan, torch.cuda.current_stream().cuda_stream
        names = ("face_ids", "nearest", "bary")
        words = lambda a: np.ascontiguousarray(a).reshape(-1).view(np.uint32)          # noqa: E731

        def host_call(n, pts, out):
            before = _stats()
            _lib.check(lib.bf_scan_nearest(scan._h, n, _lib.fptr(pts), _lib.iptr(out.get("face_ids")), _lib.fptr(out.get("nearest")),
                                           _lib.fptr(out.get("bary"))), "bf_scan_nearest")
            after = _stats()
            assert after["host_calls"] == before["host_calls"] + 1, (before, after)
            assert all(after[k] == before[k] for k in ("dev_calls", "allocations", "stream_switches")), (before, after)

        for n in (1, 3, 4, 5, 257):
            pts = SC.points(n)
            near, ids, bary = scan.nearest_points(pts)
            want = {"face_ids": ids, "nearest": near, "bary": bary}
            assert ids.dtype == np.int32 and (ids >= 0).all() and np.isfinite(near).all() and np.isfinite(bary).all()
            pts_t = _gpu(pts)
            for mask in range(1, 8):
                asked = [k for i, k in enumerate(names) if (mask >> i) & 1]
                out = {k: np.full(want[k].shape, -7, want[k].dtype) for k in asked}
                host_call(n, pts, out)

                def call():
                    o = {k: _guarded(want[k].size) for k in asked}
                    scan.nearest_points_dev(n, stream, pts_t.data_ptr(), **{k: a for k, (_, a) in o.items()})
                    return o
                got = _two_calls(call, f"nearest n={n} {asked}")
                for k in asked:
                    t = got[k][0]
                    _same(words(out[k]), words(want[k]), f"host route n={n} {asked}: {k} against the all-outputs call")
                    _same(words(t[:want[k].size].cpu().numpy()), words(out[k]), f"n={n} {asked}: {k}, device route against host route")
                    _guard_kept(t, want[k].size, f"nearest n={n} {asked} {k}")
        torch.cuda.synchronize()
        # refusals
        INVALID, UNSUPPORTED = -1, -3
        ws = scan.workspace()
        a_t = torch.zeros(64, device=GPU)
        a, h, s = C.c_void_p(a_t.data_ptr()), _lib.fptr(np.zeros(64, np.float32)), scan._h
        before = _stats()
        for args in ((None, 1, h), (s, 0, h), (s, -1, h), (s, 1, None)):
            assert lib.bf_scan_nearest(*args, None, h, None) == INVALID and lib.bf_last_error() == b"bf_scan_nearest: bad argument", args
        who = b"bf_scan_nearest_dev: "
        for args, code, text in (((None, 1, a, None, a, None, ws._h, None), INVALID, b"bad argument"),
                                 ((s, 1, None, None, a, None, ws._h, None), INVALID, b"bad argument"),
                                 ((s, 1, a, None, a, None, None, None), INVALID, b"the workspace is NULL"),
                                 ((s, 0, a, None, a, None, ws._h, None), INVALID, b"points must be positive"),
                                 ((s, (1 << 28) + 1, a, None, a, None, ws._h, None), UNSUPPORTED, b"more than 268435456 points")):
            assert lib.bf_scan_nearest_dev(*args) == code and lib.bf_last_error() == who + text, (args, lib.bf_last_error())
        if torch.cuda.device_count() > 1:
            far = N.Workspace(1)
            assert lib.bf_scan_nearest_dev(s, 1, a, None, a, None, far._h, None) == INVALID
            assert lib.bf_last_error() == who + b"the workspace lives on another device", lib.bf_last_error()
            far.close()
        else:
            print("one GPU: a workspace of another device not tried")
        assert _stats() == before, "a refused call was counted or allocated"
        torch.cuda.synchronize()
        searcher.close()
        return {"ok": np.ones(1)}

    _run(out_path, body)
