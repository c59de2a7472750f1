"""The stand-alone scan / SMPL+D losses on the GPU: bf_vertex_normals(_vjp), bf_normal_laplacian, bf_scan_point_loss and
bf_normal_loss (csrc/mesh_loss_kernels.hip) through `native` and through the drop-in functions, against torch autograd of
oracle/mesh_oracle.py from the same float32 inputs.  The cases, the references and the band are tests/scan_loss_cases.py's (the band
is DESIGN.md section 2.3's rule; tests/test_scan_losses_autograd.py shows every case well posed, so nothing is skipped or filtered
here).  Each check prints its position inside its band, the last test the worst of all."""
import numpy as np
import pytest
import torch

import scan_loss_cases as SC
from conftest import load_golden
from bodyfitting_amd import _lib
from bodyfitting_amd import native as N
from bodyfitting_amd import synthetic as S
from oracle import mesh_oracle as MO

pytestmark = pytest.mark.gpu
BAND = SC.Band()


@pytest.fixture(scope="module")
def searcher():
    from bodyfitting_amd.mesh_grid_searcher import MeshGridSearcher
    _, sv, sf, _ = SC.scan()
    s = MeshGridSearcher(sv, sf)
    yield s
    s.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", SC.MESH_NAMES)
def test_normals_their_vjp_and_the_laplacian(name):
    """one triangle, the block edge in faces and in vertices, both sides of the adjacency batch, a vertex in no face, 690, and the
    mesh with a zero-area face; random dnormals; two calls give equal bits"""
    verts, faces = SC.all_meshes()[name]
    dn = SC.cotangent(name, verts.shape)
    topo = N.Topology(len(verts), faces)
    n = N.vertex_normals(topo, verts)
    g = N.vertex_normals_vjp(topo, verts, dn)
    n64, g64 = SC.ref_normals(verts, faces, dn, torch.float64)
    n32, g32 = SC.ref_normals(verts, faces, dn, torch.float32)
    BAND.block(name + " normals", n, n64, n32)
    BAND.block(name + " dverts", g, g64, g32)
    if name == "fan9_lonely_vertex":
        assert not _bits(n[-1]).any() and not _bits(g[-1]).any()               # normal exactly zero, gradient bit-zero
    np.testing.assert_array_equal(_bits(N.vertex_normals(topo, verts)), _bits(n))
    np.testing.assert_array_equal(_bits(N.vertex_normals_vjp(topo, verts, dn)), _bits(g))
    assert not N.vertex_normals_vjp(topo, verts, np.zeros_like(dn)).any()      # a zero cotangent
    norms = SC.cotangent(name + " lap", verts.shape)
    value, dnorms = N.normal_laplacian(topo, norms)
    v64, l64 = SC.ref_laplacian(norms, faces, torch.float64)
    v32, l32 = SC.ref_laplacian(norms, faces, torch.float32)
    BAND.value(name + " laplacian", value, v64, v32)
    BAND.block(name + " dnorms", dnorms, l64, l32)
    again, dagain = N.normal_laplacian(topo, norms)
    assert _bits(again) == _bits(value)
    np.testing.assert_array_equal(_bits(dagain), _bits(dnorms))
    assert _bits(N.normal_laplacian(topo, norms, want_grad=False)[0]) == _bits(value)
    topo.close()


@pytest.mark.parametrize("n", SC.POINT_COUNTS)
def test_scan_losses_over_point_counts(searcher, n):
    """1, the wave edge, the block edge and 690 points, some of them exactly on the scan; evaluated with the ids and closest points
    the searcher's own nearest_points returns"""
    _, sv, sf, fn = SC.scan()
    pts = SC.points(n)
    near, ids = searcher.nearest_points(pts)
    value, ids2, near2, g = searcher._scan.point_loss(pts)
    np.testing.assert_array_equal(ids2, ids)
    np.testing.assert_array_equal(_bits(near2), _bits(near))                   # the existing launch: the same bits
    v64, g64 = SC.ref_point_loss(pts, near, torch.float64)
    v32, g32 = SC.ref_point_loss(pts, near, torch.float32)
    BAND.value(f"points {n} point loss", value, v64, v32)
    BAND.block(f"points {n} dpoints", g, g64, g32)
    on = np.abs(pts - near).sum(1) == 0
    assert on.sum() >= n // 5 and not g[on].any()              # (zero, of either sign: a scan coordinate of -0.0 gives -0.0 - 0.0 = -0.0, as in torch)
    again = searcher._scan.point_loss(pts)
    assert _bits(again[0]) == _bits(value)
    np.testing.assert_array_equal(_bits(again[3]), _bits(g))
    assert _bits(searcher._scan.point_loss(pts, want_grad=False)[0]) == _bits(value)
    pn = SC.cotangent(f"pn {n}", pts.shape)
    w, h = N.normal_loss(fn[ids], pn)
    w64, h64 = SC.ref_normal_loss(fn[ids], pn, torch.float64)
    w32, h32 = SC.ref_normal_loss(fn[ids], pn, torch.float32)
    BAND.value(f"points {n} normal loss", w, w64, w32)
    BAND.block(f"points {n} dpoint_norm", h, h64, h32)
    w2, h2 = N.normal_loss(fn[ids], pn)
    assert _bits(w2) == _bits(w)
    np.testing.assert_array_equal(_bits(h2), _bits(h))


def test_points_on_scan_vertices_give_zero_loss_and_bit_zero_gradient(searcher):
    pts = SC.points_on_scan_vertices()
    value, ids, near, g = searcher._scan.point_loss(pts)
    np.testing.assert_array_equal(near, pts)
    assert value == 0 and np.isfinite(g).all() and not _bits(g).any()
    p = torch.tensor(pts, requires_grad=True)
    from bodyfitting_amd import loss as L
    (L.point_cloud_loss_mesh_grid(searcher, p) * 3.0).backward()
    assert torch.isfinite(p.grad).all() and not p.grad.any()


def test_torch_path_is_bit_equal_to_the_native_calls_and_scales_cotangents(searcher):
    from bodyfitting_amd import loss as L
    from bodyfitting_amd.normals import compute_normal_torch
    _, sv, sf, fn = SC.scan()
    _, verts, faces = SC.body690()
    ft, fnt = torch.as_tensor(faces.astype(np.int64)), torch.tensor(fn)
    topo = N.Topology(len(verts), faces)
    dn = SC.cotangent("torch path", verts.shape)
    # compute_normal_torch, with a random cotangent
    v = torch.tensor(verts).reshape(1, -1, 3).requires_grad_(True)
    n = compute_normal_torch(v, ft)
    assert n.shape == (690, 3) and n.dtype == torch.float32
    np.testing.assert_array_equal(_bits(n.detach().numpy()), _bits(N.vertex_normals(topo, verts)))
    (n * torch.tensor(dn)).sum().backward()
    assert v.grad.shape == v.shape
    np.testing.assert_array_equal(_bits(v.grad.numpy().reshape(-1, 3)), _bits(N.vertex_normals_vjp(topo, verts, dn)))
    # the three losses: cotangent 1 gives the native call's bits, 2.5 scales them, 0 gives zeros
    pts, pn = SC.points(257), SC.cotangent("pn torch", (257, 3))
    near, ids = searcher.nearest_points(pts)
    native = {"point": searcher._scan.point_loss(pts)[::3], "normal": N.normal_loss(fn[ids], pn), "laplacian": N.normal_laplacian(topo, dn)}
    calls = {"point": (lambda x: L.point_cloud_loss_mesh_grid(searcher, x), pts),
             "normal": (lambda x: L.normal_loss_mesh_grid(searcher, torch.tensor(pts), fnt, x), pn),
             "laplacian": (lambda x: L.normal_laplacian_smoothness(x, ft), dn)}
    for key, (f, x0) in calls.items():
        value, grad = native[key]
        for cot in (1.0, 2.5, 0.0):
            x = torch.tensor(x0, requires_grad=True)
            out = f(x)
            assert out.shape == () and out.dtype == torch.float32 and _bits(out.detach().numpy()) == _bits(value), key
            (out * cot).backward()
            np.testing.assert_array_equal(_bits(x.grad.numpy()), _bits(grad * np.float32(cot)), err_msg=f"{key} x {cot}")
    # numpy in: floats out, the same bits
    floats = {"point": L.point_cloud_loss_mesh_grid(searcher, pts), "normal": L.normal_loss_mesh_grid(searcher, pts, fn, pn),
              "laplacian": L.normal_laplacian_smoothness(dn, faces)}
    for key, value in floats.items():
        assert isinstance(value, float) and _bits(np.float32(value)) == _bits(native[key][0]), key
    topo.close()


def test_limits_and_their_error_codes(searcher):
    tri = np.array([[0, 1, 2]], np.int32)
    for faces, n_verts, code in ((np.array([[0, 1, 3]], np.int32), 3, -1), (np.array([[0, -1, 2]], np.int32), 3, -1),
                                 (tri, 0, -1), (tri, (1 << 28) + 1, -3)):
        with pytest.raises(_lib.BodyfitError, match=rf"bf_topo_create failed \({code}\)"):
            N.Topology(n_verts, faces)
    lib = _lib.load()
    import ctypes as C
    h = C.c_void_p()
    assert lib.bf_topo_create(0, 3, 0, _lib.iptr(tri), C.byref(h)) == -1 and not h.value               # no faces
    assert lib.bf_topo_create(0, 3, (1 << 28) + 1, _lib.iptr(tri), C.byref(h)) == -3                  # (refused before anything is read)
    assert lib.bf_topo_create(0, 3, 1, None, C.byref(h)) == -1
    one = np.zeros(3, np.float32)
    out = np.zeros(3, np.float32)
    assert lib.bf_vertex_normals(None, _lib.fptr(one), _lib.fptr(out)) == -1
    assert lib.bf_vertex_normals_vjp(None, _lib.fptr(one), _lib.fptr(one), _lib.fptr(out)) == -1
    assert lib.bf_normal_laplacian(None, _lib.fptr(one), _lib.fptr(out), None) == -1
    scan = searcher._scan
    assert lib.bf_scan_point_loss(scan._h, 0, _lib.fptr(one), _lib.fptr(out), None, None, None) == -1
    assert lib.bf_scan_point_loss(scan._h, (1 << 28) + 1, _lib.fptr(one), _lib.fptr(out), None, None, None) == -3
    assert lib.bf_scan_point_loss(None, 1, _lib.fptr(one), _lib.fptr(out), None, None, None) == -1
    assert lib.bf_normal_loss(0, 0, _lib.fptr(one), _lib.fptr(one), _lib.fptr(out), None) == -1
    assert lib.bf_normal_loss(0, (1 << 28) + 1, _lib.fptr(one), _lib.fptr(one), _lib.fptr(out), None) == -3
    assert lib.bf_normal_loss(0, 1, None, _lib.fptr(one), _lib.fptr(out), None) == -1
    assert b"bf_normal_loss" in lib.bf_last_error()
    # every output is optional
    topo = N.Topology(3, tri)
    assert lib.bf_normal_laplacian(topo._h, _lib.fptr(np.zeros(9, np.float32)), None, None) == 0
    assert lib.bf_scan_point_loss(scan._h, 1, _lib.fptr(one), None, None, None, None) == 0
    topo.close()


def _host_calls():
    return N.dev_route_stats()["host_calls"]


@pytest.mark.parametrize("n", [1, 5, 257])
def test_scan_point_loss_optional_outputs_in_every_combination(searcher, n):
    """bf_scan_point_loss at the C ABI: all 16 NULL / non-NULL choices of (loss, face_ids, nearest, dpoints).  Every output asked for
    holds the bits of the all-outputs call; every call counts once on the host route"""
    lib, scan, pts = _lib.load(), searcher._scan, SC.points(n)
    names = ("loss", "face_ids", "nearest", "dpoints")

    def call(mask):
        out = {"loss": np.full(1, np.nan, np.float32), "face_ids": np.full(n, -7, np.int32), "nearest": np.full((n, 3), np.nan, np.float32),
               "dpoints": np.full((n, 3), np.nan, np.float32)}
        out = {k: v for i, (k, v) in enumerate(out.items()) if (mask >> i) & 1}
        before = _host_calls()
        rc = lib.bf_scan_point_loss(scan._h, n, _lib.fptr(pts), _lib.fptr(out.get("loss")), _lib.iptr(out.get("face_ids")),
                                    _lib.fptr(out.get("nearest")), _lib.fptr(out.get("dpoints")))
        assert rc == 0 and _host_calls() == before + 1, (mask, rc)
        return out

    full = call(15)
    assert np.isfinite(full["loss"]).all() and np.isfinite(full["dpoints"]).all() and (full["face_ids"] >= 0).all()
    for mask in range(16):
        got = call(mask)
        assert set(got) == {k for i, k in enumerate(names) if (mask >> i) & 1}
        for k, v in got.items():
            assert v.tobytes() == full[k].tobytes(), (mask, k)


def test_normal_laplacian_and_normal_loss_optional_outputs(searcher):
    """bf_normal_laplacian on the 257-vertex fan and bf_normal_loss at 257 points, at the C ABI: loss only, gradient only, both and
    neither.  What is asked for holds the bits of the call for both; neither returns BF_OK and counts once on the host route"""
    lib = _lib.load()
    verts, faces = SC.fan(255, 2257, lonely=True)
    assert len(verts) == 257
    topo = N.Topology(len(verts), faces)
    norms = SC.cotangent("fan257 optional", verts.shape)
    pts, pn = SC.points(257), SC.cotangent("pn optional", (257, 3))
    fn = np.ascontiguousarray(SC.scan()[3][searcher.nearest_points(pts)[1]])

    def laplacian(loss, grad):
        return lib.bf_normal_laplacian(topo._h, _lib.fptr(norms), _lib.fptr(loss), _lib.fptr(grad))

    def normal(loss, grad):
        return lib.bf_normal_loss(0, 257, _lib.fptr(fn), _lib.fptr(pn), _lib.fptr(loss), _lib.fptr(grad))

    for name, call in (("laplacian", laplacian), ("normal loss", normal)):
        both = np.full(1, np.nan, np.float32), np.full((257, 3), np.nan, np.float32)
        assert call(*both) == 0 and np.isfinite(both[0]).all() and np.isfinite(both[1]).all(), name
        for want_loss, want_grad in ((True, False), (False, True), (True, True), (False, False)):
            loss = np.full(1, np.nan, np.float32) if want_loss else None
            grad = np.full((257, 3), np.nan, np.float32) if want_grad else None
            before = _host_calls()
            assert call(loss, grad) == 0, (name, want_loss, want_grad)
            assert _host_calls() == before + 1, (name, want_loss, want_grad)
            if want_loss:
                assert loss.tobytes() == both[0].tobytes(), (name, want_grad)
            if want_grad:
                assert grad.tobytes() == both[1].tobytes(), (name, want_loss)
    topo.close()


def test_the_users_own_smpl_d_loop_on_the_dropins():
    """smplify.py:236-245 with torch.optim.Adam(lr=5e-2) on the drop-in functions, from the base mesh of
    test_gpu_scan.py::test_displacement_stage_first_steps: its first gradient against the float64 oracle's and its first step
    against the reference's own (that test's bounds)"""
    from bodyfitting_amd import loss as L
    from bodyfitting_amd.mesh_grid_searcher import MeshGridSearcher
    from bodyfitting_amd.normals import compute_normal_torch
    model = SC.body690()[0]
    dev = N.DeviceModel(model, S.make_gmm(seed=0), device=0)
    g = load_golden("scan_nv690_30it.npz")
    prob, sv, sf = S.make_scan_problem(model, frame=0, n_views=8)
    scan = N.Scan(sv, sf)
    c2w, K, kp, ndiv, betas, pose = N.pack_problem([prob])
    b = N.FrameBatch(dev, 1, 8)
    b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose); b.set_scans([scan])
    b.fit(30)
    base = b.get_result()[0][0]
    b.close(); scan.close(); dev.close()
    # the user's side: smplify.py:147-156, 229-245
    tris = sv[sf]
    face_norms = torch.from_numpy(np.cross(tris[::, 1] - tris[::, 0], tris[::, 2] - tris[::, 0])).float()
    constant_scale = float((sv.max(0) - sv.min(0))[1] / 1.7)
    pointsearcher = MeshGridSearcher(verts=sv, faces=sf)
    body_vertices = torch.tensor(base).reshape(1, -1, 3)
    disp = torch.zeros_like(body_vertices)
    disp.requires_grad = True
    optimizer = torch.optim.Adam([disp], lr=5e-2, betas=(0.9, 0.999))
    smpl_faces = torch.from_numpy(np.asarray(model["faces"])).long()
    deformed_verts = body_vertices + disp
    deformed_norms = compute_normal_torch(deformed_verts, smpl_faces)
    icp_loss = L.point_cloud_loss_mesh_grid(pointsearcher, deformed_verts)
    norm_loss = L.normal_loss_mesh_grid(pointsearcher, deformed_verts, face_norms, deformed_norms)
    smoothness = L.normal_laplacian_smoothness(deformed_norms, smpl_faces)
    loss = icp_loss + (norm_loss + smoothness) * constant_scale * 0.1
    optimizer.zero_grad()
    loss.backward()
    grad = disp.grad.numpy()[0].copy()
    optimizer.step()
    pointsearcher.close()
    # autograd gradient of the same objective at disp = 0 on the same base mesh (fp64 oracle pieces), as that test forms it
    bv = torch.tensor(base, dtype=torch.float64)
    d64 = torch.zeros_like(bv, requires_grad=True)
    ids, cpts, _ = MO.ReferenceSearcher(sv, sf).nearest(base)
    t64 = sv.astype(np.float64)[sf]
    fnorm = torch.tensor(np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0]).astype(np.float32), dtype=torch.float64)
    P = bv + d64
    norms = MO.compute_normal_torch(P, smpl_faces)
    c = float((sv[:, 1].max() - sv[:, 1].min()) / 1.7)
    want_loss = MO.point_cloud_loss(P, torch.tensor(cpts, dtype=torch.float64)) + (
        MO.normal_loss(fnorm[torch.as_tensor(ids, dtype=torch.long)], norms) + MO.normal_laplacian_smoothness(norms, smpl_faces)) * c * 0.1
    want_loss.backward()
    want = d64.grad.numpy()
    err, allowed = float(np.abs(grad - want).max()), 1e-4 * float(np.abs(want).max())
    print(f"    first gradient: error {err:.3e} of {allowed:.3e} allowed = {err / allowed:.3f} of the band")
    BAND.rows.append(("loop first gradient", err, allowed, err / allowed))
    assert err <= allowed
    step = float(np.abs(disp.detach().numpy()[0] - g["disp1"]).max())
    print(f"    disp after step 1: error {step:.3e} of 2e-5 allowed = {step / 2e-5:.3f} of the band")
    BAND.rows.append(("loop disp after step 1", step, 2e-5, step / 2e-5))
    assert step <= 2e-5


def test_zz_the_worst_position_inside_a_band():
    worst = BAND.worst()
    assert worst is not None
    print(f"    {len(BAND.rows)} checks; the worst: {worst[0]}: error {worst[1]:.3e} of {worst[2]:.3e} allowed = {worst[3]:.3f} of the band")
    assert worst[3] <= 1.0
