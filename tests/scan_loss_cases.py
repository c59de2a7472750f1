"""What tests/test_scan_losses_autograd.py (CPU) and tests/test_gpu_scan_losses.py (GPU) share: the meshes and point sets the
stand-alone scan / SMPL+D losses are tried on, their references - torch autograd of oracle/mesh_oracle.py in float64 and float32
from the same float32 inputs - the error band, and float64 stand-ins for the native calls.

The band is DESIGN.md section 2.3's rule and is calibrated against nothing the HIP kernels give:
  per gradient block  max|hip - g64| <= max(5e-6 M, 8 err32),  M = max|g64|, err32 = max|g32 - g64|
  per value           |hip - v64| <= max(3e-6, 8 rel32) |v64|,  rel32 = |v32 - v64| / |v64|
i.e. a float32 kernel may be eight times as far from the float64 truth as torch's own float32 evaluation of the same formulas is, with
a floor of a few units in the last place of the block's largest entry (5e-6 ~ 40 ulp, 3e-6 ~ 25 ulp of float32) for blocks where
torch's float32 happens to be exact.  The normals themselves ([NV,3], not a scalar) are held to the block rule.
The CPU file checks that every case is well posed: err32 <= 1e-5 M for every block, so the band never degenerates.
"""
import functools

import numpy as np
import torch

from bodyfitting_amd import synthetic as S
from oracle import mesh_oracle as MO

ADJ_BATCH = 8                      # BF_ADJ_BATCH of csrc/mesh_normal_bodies.h: incident faces walked together
BLOCK = 256                        # threads per block = faces, vertices or points per block sum
WELL_POSED = 1e-5


# ----------------------------------------------------------------------------------------------------------------------------
# meshes
# ----------------------------------------------------------------------------------------------------------------------------

def fan(k, seed, lonely=False):
    """a closed fan: hub 0 with k incident faces, the rim below it; lonely: one more vertex that is in no face"""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(k) / k
    rim = np.stack([np.cos(ang), np.sin(ang), np.zeros(k)], 1) * (1 + 0.2 * rng.uniform(-1, 1, (k, 1)))
    verts = np.concatenate([[[0.0, 0.0, 0.6]], rim]) + 0.05 * rng.normal(size=(k + 1, 3))
    if lonely:
        verts = np.concatenate([verts, [[3.0, 1.0, 2.0]]])
    faces = np.array([[0, 1 + i, 1 + (i + 1) % k] for i in range(k)], np.int32)
    return verts.astype(np.float32), faces


def strip(nf, seed):
    """a triangle strip of nf faces over nf + 2 vertices on a wavy sheet, consistently oriented"""
    rng = np.random.default_rng(seed)
    i = np.arange(nf + 2)
    verts = np.stack([0.1 * (i // 2) + 0.02 * rng.uniform(-1, 1, nf + 2), 0.1 * (i % 2) + 0.02 * rng.uniform(-1, 1, nf + 2),
                      0.03 * np.sin(0.7 * i) + 0.01 * rng.normal(size=nf + 2)], 1)
    faces = np.array([[f, f + 1, f + 2] if f % 2 == 0 else [f + 1, f, f + 2] for f in range(nf)], np.int32)
    return verts.astype(np.float32), faces


def with_zero_area_face(verts, faces):
    """one more face whose third corner is a NEW vertex at its first corner's position: both edge products are exactly zero in every
    arithmetic, so |n| = 0 and the face's gradient is dn / 1e-8"""
    a, b = int(faces[0, 0]), int(faces[0, 1])
    verts = np.concatenate([verts, verts[a:a + 1]])
    faces = np.concatenate([faces, [[a, b, len(verts) - 1]]]).astype(np.int32)
    return verts, faces


@functools.lru_cache(maxsize=None)
def body690():
    model = S.make_model("smpl", seed=0, nv=690)
    rng = np.random.default_rng(11)
    verts = np.asarray(model["v_template"], np.float64) + 0.002 * rng.normal(size=(690, 3))
    return model, verts.astype(np.float32), np.asarray(model["faces"], np.int32).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def meshes():
    """name -> (verts float32[nv,3], faces int32[nf,3]): the smallest shapes at which the kernels can go wrong"""
    out = {"one_triangle": (np.array([[0.1, 0.2, 0.3], [1.0, 0.1, 0.2], [0.3, 0.9, 0.5]], np.float32), np.array([[0, 1, 2]], np.int32))}
    for nf in (BLOCK - 1, BLOCK, BLOCK + 1):                       # the block edge in faces ...
        out[f"strip_nf{nf}"] = strip(nf, nf)
    for nv in (BLOCK - 1, BLOCK, BLOCK + 1):                       # ... and in vertices
        out[f"strip_nv{nv}"] = strip(nv - 2, 1000 + nv)
    for k in (ADJ_BATCH - 1, ADJ_BATCH, ADJ_BATCH + 1, 2 * ADJ_BATCH, 2 * ADJ_BATCH + 1):        # both sides of the adjacency batch
        out[f"fan{k}"] = fan(k, k)
    out["fan9_lonely_vertex"] = fan(9, 77, lonely=True)
    out["body690"] = body690()[1:]
    return out


ZERO_AREA = "fan9_zero_area_face"            # its own case: its gradient is 1e8 times the others'


@functools.lru_cache(maxsize=None)
def zero_area_mesh():
    return with_zero_area_face(*fan(9, 5))


def all_meshes():
    return dict(meshes(), **{ZERO_AREA: zero_area_mesh()})


MESH_NAMES = ("one_triangle", "strip_nf255", "strip_nf256", "strip_nf257", "strip_nv255", "strip_nv256", "strip_nv257", "fan7", "fan8",
              "fan9", "fan16", "fan17", "fan9_lonely_vertex", "body690", ZERO_AREA)


def cotangent(name, shape):
    """random dnormals / norms / point normals of a case, float32"""
    rng = np.random.default_rng(sum(map(ord, name)))
    return rng.normal(size=shape).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------------
# the scan and the point sets
# ----------------------------------------------------------------------------------------------------------------------------

POINT_COUNTS = (1, 63, 64, 65, 255, 256, 257, 690)


@functools.lru_cache(maxsize=None)
def scan():
    """-> (problem, scan verts float32[690,3], scan faces int32[1376,3], face normals float32 as smplify.py:149 builds them)"""
    prob, sv, sf = S.make_scan_problem(body690()[0], frame=0, n_views=8)
    tris = sv[sf]
    fn = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]).astype(np.float32)
    return prob, sv, np.asarray(sf, np.int32), fn


def points(n):
    """n query points near the scan; every fifth one lies exactly on a scan vertex"""
    _, sv, _, _ = scan()
    rng = np.random.default_rng(300 + n)
    p = sv[rng.permutation(len(sv))[:n]] + rng.normal(0, 0.01, (n, 3)).astype(np.float32)
    on = np.arange(n) % 5 == 4
    p[on] = sv[rng.integers(0, len(sv), int(on.sum()))]
    return np.ascontiguousarray(p, np.float32)


def points_on_scan_vertices(n=64):
    return np.ascontiguousarray(scan()[1][7:7 + n])


# ----------------------------------------------------------------------------------------------------------------------------
# references: torch autograd of oracle/mesh_oracle.py
# ----------------------------------------------------------------------------------------------------------------------------

def _t(a, dtype, grad=False):
    return torch.tensor(np.asarray(a), dtype=dtype, requires_grad=grad)


def _faces_t(faces):
    return torch.as_tensor(np.asarray(faces, np.int64))


@torch.enable_grad()          # (also called inside an autograd Function's forward, where grad mode is off)
def ref_normals(verts, faces, dnormals, dtype):
    """-> (normals, dverts for the cotangent dnormals) as float64 arrays, evaluated in `dtype`"""
    v = _t(verts, dtype, True)
    n = MO.compute_normal_torch(v, _faces_t(faces))
    (n * _t(dnormals, dtype)).sum().backward()
    return n.detach().double().numpy(), v.grad.double().numpy()


@torch.enable_grad()          # (also called inside an autograd Function's forward, where grad mode is off)
def ref_laplacian(norms, faces, dtype):
    n = _t(norms, dtype, True)
    loss = MO.normal_laplacian_smoothness(n, _faces_t(faces))
    loss.backward()
    return float(loss.detach().double()), n.grad.double().numpy()


@torch.enable_grad()          # (also called inside an autograd Function's forward, where grad mode is off)
def ref_point_loss(pts, closest, dtype):
    p = _t(pts, dtype, True)
    loss = MO.point_cloud_loss(p, _t(closest, dtype))
    loss.backward()
    return float(loss.detach().double()), p.grad.double().numpy()


@torch.enable_grad()          # (also called inside an autograd Function's forward, where grad mode is off)
def ref_normal_loss(closest_face_norms, point_norms, dtype):
    pn = _t(point_norms, dtype, True)
    loss = MO.normal_loss(_t(closest_face_norms, dtype), pn)
    loss.backward()
    return float(loss.detach().double()), pn.grad.double().numpy()


# ----------------------------------------------------------------------------------------------------------------------------
# the band
# ----------------------------------------------------------------------------------------------------------------------------

class Band:
    """collects every check's position inside its band (error / allowed; <= 1 passes)"""

    def __init__(self):
        self.rows = []

    def block(self, what, got, g64, g32):
        got, g64, g32 = (np.asarray(a, np.float64) for a in (got, g64, g32))
        assert got.shape == g64.shape, (what, got.shape, g64.shape)
        assert np.isfinite(got).all(), what
        M = float(np.abs(g64).max())
        allowed = max(5e-6 * M, 8 * float(np.abs(g32 - g64).max()))
        err = float(np.abs(got - g64).max())
        return self._row(what, err, allowed)

    def value(self, what, got, v64, v32):
        assert np.isfinite(got), what
        allowed = max(3e-6 * abs(v64), 8 * abs(v32 - v64))
        return self._row(what, abs(float(got) - v64), allowed)

    def _row(self, what, err, allowed):
        at = 0.0 if err == 0.0 else (np.inf if allowed == 0.0 else err / allowed)
        self.rows.append((what, err, allowed, at))
        print(f"    {what}: error {err:.3e} of {allowed:.3e} allowed = {at:.3f} of the band")
        assert err <= allowed, (what, err, allowed)
        return at

    def worst(self):
        return max(self.rows, key=lambda r: r[3]) if self.rows else None


def well_posed(what, g64, g32):
    g64, g32 = np.asarray(g64, np.float64), np.asarray(g32, np.float64)
    M, err = float(np.abs(g64).max()), float(np.abs(g32 - g64).max())
    assert err <= WELL_POSED * M, (what, err, M)


# ----------------------------------------------------------------------------------------------------------------------------
# float64 stand-ins for the native calls (the CPU file)
# ----------------------------------------------------------------------------------------------------------------------------

def _like(a, ref):
    return np.asarray(a, np.float64 if np.asarray(ref).dtype == np.float64 else np.float32)


class StandInTopology:
    created = 0

    def __init__(self, n_verts, faces, device=0):
        type(self).created += 1
        self.n_verts, self.faces, self.device = int(n_verts), np.asarray(faces, np.int64).reshape(-1, 3), int(device)
        self.n_faces = len(self.faces)
        assert self.faces.min() >= 0 and self.faces.max() < n_verts

    def close(self):
        pass


def stand_in_vertex_normals(topo, verts):
    assert np.asarray(verts).shape == (topo.n_verts, 3)
    return _like(ref_normals(verts, topo.faces, np.zeros((topo.n_verts, 3)), torch.float64)[0], verts)


def stand_in_vertex_normals_vjp(topo, verts, dnormals):
    return _like(ref_normals(verts, topo.faces, np.asarray(dnormals).reshape(topo.n_verts, 3), torch.float64)[1], verts)


def stand_in_normal_laplacian(topo, norms, want_grad=True):
    value, grad = ref_laplacian(norms, topo.faces, torch.float64)
    return _like(value, norms), (_like(grad, norms) if want_grad else None)


NORMAL_LOSS_CALLS = []          # (rows uploaded, gradient wanted, device) per call


def stand_in_normal_loss(closest_face_norms, point_norms, want_grad=True, device=0):
    NORMAL_LOSS_CALLS.append((np.asarray(closest_face_norms).shape, bool(want_grad), int(device)))
    value, grad = ref_normal_loss(closest_face_norms, point_norms, torch.float64)
    return _like(value, point_norms), (_like(grad, point_norms) if want_grad else None)


class StandInScan:
    """native.Scan by brute force (oracle.mesh_oracle.nearest_bruteforce); `frozen` = (ids, nearest) answers every query with
    these (the closest points are detached: finite differences must not move them)"""
    searches = 0
    grads = 0

    def __init__(self, verts, faces, device=0):
        self.verts, self.faces, self.device = np.asarray(verts, np.float32), np.asarray(faces, np.int32), int(device)
        self.n_verts, self.n_faces = len(self.verts), len(self.faces)
        self.frozen = None

    def grid_info(self):
        return np.ones(3, np.int32), np.zeros(3, np.float32), 1.0

    def close(self):
        pass

    def _search(self, p):
        type(self).searches += 1
        if self.frozen is not None:
            return self.frozen
        ids, pts, _ = MO.nearest_bruteforce(self.verts, self.faces, np.asarray(p, np.float32))
        return ids, pts

    def nearest_points(self, p):
        ids, pts = self._search(p)
        return pts, ids, None

    def point_loss(self, p, want_grad=True):
        ids, pts = self._search(p)
        type(self).grads += bool(want_grad)
        value, grad = ref_point_loss(p, pts, torch.float64)
        return _like(value, p), ids, pts, (_like(grad, p) if want_grad else None)


def install_stand_ins(monkeypatch):
    """the native calls of normals.py / loss.py / mesh_grid_searcher.py replaced, float64 let through (gradcheck needs it)"""
    from bodyfitting_amd import mesh_grid_searcher, native, normals, prior
    monkeypatch.setattr(native, "Topology", StandInTopology)
    monkeypatch.setattr(native, "vertex_normals", stand_in_vertex_normals)
    monkeypatch.setattr(native, "vertex_normals_vjp", stand_in_vertex_normals_vjp)
    monkeypatch.setattr(native, "normal_laplacian", stand_in_normal_laplacian)
    monkeypatch.setattr(native, "normal_loss", stand_in_normal_loss)
    monkeypatch.setattr(mesh_grid_searcher, "Scan", StandInScan)
    monkeypatch.setattr(prior, "_require_float32", lambda who, name, x: None)
    monkeypatch.setattr(normals, "_TOPOLOGIES", {})
