"""Cases of the fused SMPL+D stage (bf_fit_displacement, csrc/disp_kernels.hip), shared by tests/test_disp_stage_cases.py (CPU: every
case is what it claims to be and well posed) and tests/test_gpu_disp_stage.py (MI355X: the stage's gradient, its Adam step by step and
the zero-distance rule).  test_gpu_dense_grad.py's step-4 check takes its reference and its tie handling from here too.

A topology case is the 690-vertex SMPL model with only `faces` replaced (bf_model_create range-checks the faces of an SMPL model and
nothing but this stage reads them), so that the three walks over a vertex's incident faces - BF_ADJ_BATCH = 8 at a time, padded
entries -1 - meet what a body template never gives them: a full second batch, a third one, a vertex in no face; and so that the face
count sits on both sides of a block edge.  Every case needs its own DeviceModel: the adjacency is built once per model.

The reference is torch autograd of oracle/mesh_oracle.py's SMPL+D objective (smplify.py:228-247) in float64 and float32 from the
same float32 inputs.  The band is DESIGN.md 2.3's block rule as scan_loss_cases.Band implements it, max(5e-6 M, 8 err32), plus the
rounding of the read-out of a gradient from Adam's first moments; nothing in it is calibrated on what the kernels return.
Nothing here touches a GPU.
"""
import functools

import numpy as np
import torch

import dense_grad_cases as DC
import scan_loss_cases as SC
from oracle import mesh_oracle as MO
from oracle import nearest_ref as NR

MODEL = "smpl690"                    # dense_grad_cases' name of S.make_model("smpl", seed=0, nv=690)
NV = 690
ADJ_BATCH = SC.ADJ_BATCH             # BF_ADJ_BATCH of csrc/mesh_normal_bodies.h
FACE_BLOCK_EDGE = 5 * SC.BLOCK       # 1280: five full blocks of bf_disp_face_kernel / bf_disp_fgrad_kernel
HUBS = (8, 9, 16, 17, 25)            # one full batch, one entry more, two full batches, a third batch, a fourth
FACE_COUNTS = (FACE_BLOCK_EDGE - 1, FACE_BLOCK_EDGE, FACE_BLOCK_EDGE + 1)
REPEATED_CORNER = "repeated_corner"  # its own case (like scan_loss_cases.ZERO_AREA): its gradient is 1e8 times the others'
CASES = ("body",) + tuple(f"hub{k}" for k in HUBS) + ("lonely",) + tuple(f"nf{n}" for n in FACE_COUNTS) + (REPEATED_CORNER,)
FRAMES = DC.SCAN_FRAMES              # two scans of different height in one batch
THIRD_FRAME = (2, 0.75)
THREE_FRAME_CASE = "hub17"
TIE_CAP = 0.1                        # share of vertices whose closest face may be the device's instead of the reference's: a cap
U = 2.0 ** -24                       # unit roundoff of float32


# ----------------------------------------------------------------------------------------------------------------------------
# topology
# ----------------------------------------------------------------------------------------------------------------------------

def base_model():
    return DC.model(MODEL)


@functools.lru_cache(maxsize=None)
def body_faces():
    f = np.asarray(base_model()["faces"], np.int32).reshape(-1, 3)
    f.setflags(write=False)
    return f


def valence(faces, nv=NV):
    """incident (face, corner) entries per vertex: the length of its adjacency list"""
    return np.bincount(np.asarray(faces).reshape(-1), minlength=nv)


@functools.lru_cache(maxsize=None)
def topology(case):
    """-> dict(faces int32[nf,3], marked: name -> vertex ids held on their own, valence: vertex -> claimed valence, nf)"""
    body = body_faces()
    val = valence(body)
    marked, claims = {}, {}
    if case == "body":
        faces = body
    elif case.startswith("hub"):
        k = int(case[3:])
        hub = int(np.argmin(val))
        need = k - int(val[hub])
        assert need > 0
        rng = np.random.default_rng(9000 + k)
        ring = rng.permutation(np.setdiff1d(np.arange(NV), [hub]))[:need + 1]
        extra = np.array([[hub, ring[i], ring[i + 1]] for i in range(need)], np.int32)
        faces = np.concatenate([body, extra]).astype(np.int32)
        rim = np.setdiff1d(np.unique(faces[(faces == hub).any(1)]), [hub])
        marked, claims = {"hub": np.array([hub]), "rim": rim}, {hub: k}
    elif case == "lonely":
        v = int(np.argmax(val))
        faces = body[~(body == v).any(1)]
        marked, claims = {"lonely": np.array([v])}, {v: 0}
    elif case.startswith("nf"):
        faces = body[:int(case[2:])]
    elif case == REPEATED_CORNER:
        a, b = int(body[0, 0]), int(body[0, 1])
        faces = np.concatenate([body, [[a, a, b]]]).astype(np.int32)
    else:
        raise KeyError(case)
    faces = np.ascontiguousarray(faces, np.int32)
    faces.setflags(write=False)
    return {"faces": faces, "marked": marked, "valence": claims, "nf": len(faces)}


def model(case):
    """the 690-vertex model with the case's faces, in the template's own layout and type"""
    m = base_model()
    own = np.asarray(m["faces"])
    f = topology(case)["faces"].astype(own.dtype)
    return dict(m, faces=f if own.ndim == 2 else f.reshape(-1))


def scan(frame, scale):
    """-> (problem, scan vertices float32, scan faces int32)"""
    return DC.scan_problem(MODEL, frame, scale)


def cpu_base(frame, scale, seed=0):
    """A base mesh without a GPU: the ground-truth body of the frame in the scan's world plus 2 mm (at scale 1) of seeded noise - as
    near the scan as a fit leaves it, and on no scan vertex.  float32"""
    from bodyfitting_amd import synthetic as S
    prob = scan(frame, scale)[0]
    gt = prob["gt"]
    verts, _ = S.smpl_joints64(base_model(), gt["betas"], gt["pose"])
    world = (verts + gt["transl"]) * gt["scale"] * scale
    rng = np.random.default_rng(DC.LC._seed("disp base", frame, seed))
    return (world + 0.002 * scale * rng.normal(size=world.shape)).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------------------------------------------------------

def scan_face_normals(sv, sf):
    """un-normalised scan face normals as smplify.py:149 builds them, float32"""
    tris = np.asarray(sv, np.float64)[np.asarray(sf)]
    return np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]).astype(np.float32)


def tie_share(sv, sf, P32):
    """The share of the vertices whose closest scan face is tied in the reference's own arithmetic: some other face returns the
    winner's float32 distance bit for bit (the closest point lies on a scan edge or corner).  Only at such a vertex can the device's
    search return another face than the reference's; measured with the reference alone"""
    ties = NR.nearest_allfaces(sv, sf, P32)[4]
    return float((np.asarray(ties) > 0).mean())


def settle_ties(sv, sf, ids_ref, ids_dev, P32, cap=TIE_CAP):
    """A vertex whose closest point lies on a scan edge or corner is equally far from the faces around it, bit for bit in the
    reference's own arithmetic, and the reference's answer there hangs on the order of its cell lists (test_gpu_scan.py).  The normal
    term reads the face's normal, so among such tied faces the oracle takes the one the device's search returns - after checking that
    it IS a tie (the reference's rule gives both faces the same float32 distance) and that such vertices are fewer than `cap` of all
    (None: no cap - the zero-distance case, where every vertex sits on a scan corner and is tied by construction).
    -> (face ids for the oracle, share of vertices taken from the device)"""
    ids_ref, ids_dev = np.asarray(ids_ref), np.asarray(ids_dev)
    tied = np.nonzero(ids_dev != ids_ref)[0]
    if not len(tied):
        return ids_ref, 0.0
    _, d_dev, _ = NR.rule(sv, sf, ids_dev[tied], P32[tied])
    _, d_ref, _ = NR.rule(sv, sf, ids_ref[tied], P32[tied])
    assert (d_dev.view(np.uint32) == d_ref.view(np.uint32)).all(), "the device's search chose a face the reference ranks behind its own"
    assert cap is None or len(tied) < cap * len(ids_ref), (len(tied), len(ids_ref))
    return np.where(ids_dev != ids_ref, ids_dev, ids_ref), len(tied) / len(ids_ref)


def objective_gradient(faces, base32, disp32, closest, face_norms, cscale, dtype):
    """d/d(disp) of point_cloud_loss + (normal_loss + normal_laplacian_smoothness) * c * 0.1 at base + disp (smplify.py:236-242), the
    closest points and their faces' normals constant -> float64 array [NV,3], evaluated in `dtype`"""
    faces_t = torch.as_tensor(np.asarray(faces, np.int64).reshape(-1, 3))
    disp = torch.tensor(np.asarray(disp32), dtype=dtype, requires_grad=True)
    P = torch.tensor(np.asarray(base32), dtype=dtype) + disp
    norms = MO.compute_normal_torch(P, faces_t)
    loss = MO.point_cloud_loss(P, torch.tensor(np.asarray(closest), dtype=dtype)) + (
        MO.normal_loss(torch.tensor(np.asarray(face_norms), dtype=dtype), norms) + MO.normal_laplacian_smoothness(norms, faces_t)) * cscale * 0.1
    loss.backward()
    return disp.grad.numpy().astype(np.float64)


def reference(faces, sv, sf, base32, disp32, ids_dev=None, cap=TIE_CAP):
    """The float64 and float32 gradient of the stage's objective at the device's float32 base + disp; closest points and face ids from
    the reference's search there (MO.ReferenceSearcher), the face ids settled against the device's where it gives them.
    -> dict(g64, g32, ids, share: vertices whose face was taken from the device)"""
    base32, disp32 = np.asarray(base32, np.float32), np.asarray(disp32, np.float32)
    P32 = base32 + disp32                                                 # (float32, as the stage forms it)
    ids, closest = DC.closest_points(sv, sf, P32)
    share = 0.0
    if ids_dev is not None:
        ids, share = settle_ties(sv, sf, ids, ids_dev, P32, cap)
    fn = scan_face_normals(sv, sf)[np.asarray(ids, np.int64)]
    c = DC.scan_cscale(sv)
    g = {dt: objective_gradient(faces, base32, disp32, closest, fn, c, dt) for dt in (torch.float64, torch.float32)}
    return {"g64": g[torch.float64], "g32": g[torch.float32], "ids": ids, "share": share, "closest": closest}


# ----------------------------------------------------------------------------------------------------------------------------
# the read-out of a gradient from Adam's first moments, and the bands
# ----------------------------------------------------------------------------------------------------------------------------

def one_minus(beta):
    """1 - beta as the kernel forms it: a float32 difference"""
    return float(np.float32(1.0) - np.float32(beta))


def gradient_from_moments(m_prev, m_now, beta1=0.9):
    """The stage keeps m_k = m_{k-1} + (g_k - m_{k-1}) (1 - beta1), so g_k = m_{k-1} + (m_k - m_{k-1}) / (1 - beta1) with the constant
    as the kernel holds it in float32; m_prev None: step 1, m_0 = 0.  float64"""
    w = one_minus(beta1)
    if m_prev is None:
        return np.asarray(m_now, np.float64) / w
    return np.asarray(m_prev, np.float64) + (np.asarray(m_now, np.float64) - np.asarray(m_prev, np.float64)) / w


def readout_rounding(m_prev, m_now, beta1=0.9):
    """The read-out's own rounding as test_displacement_gradient_after_three_steps derives it: (2 / (1 - beta1) - 1) * 2^-24 * max|m|,
    19 * 2^-24 * max|m| at beta1 = 0.9; at step 1 (m_0 = 0 exactly) the one rounding of m_1, 2^-24 max|m_1| / (1 - beta1)"""
    w = one_minus(beta1)
    if m_prev is None:
        return U / w * float(np.abs(m_now).max())
    return (2.0 / w - 1.0) * U * float(max(np.abs(m_prev).max(), np.abs(m_now).max()))


def hold(band, what, got, g64, g32, readout, rows=None, M=None):
    """scan_loss_cases.Band's block rule plus the read-out's rounding: max|got - g64| <= max(5e-6 M, 8 err32) + readout.  rows: the check
    on these rows alone, with their own err32 and the floor of the block they belong to (M: that block's max|g64|) - a rounding error
    in one row is of the size of the numbers the whole computation handles, not of the row's own result.  -> position in the band"""
    got, g64, g32 = (np.asarray(a, np.float64) for a in (got, g64, g32))
    assert got.shape == g64.shape, (what, got.shape, g64.shape)
    M = float(np.abs(g64).max()) if M is None else M
    if rows is not None:
        got, g64, g32 = got[rows], g64[rows], g32[rows]
    assert np.isfinite(got).all(), what + ": not finite"
    allowed = max(5e-6 * M, 8 * float(np.abs(g32 - g64).max())) + readout
    return band._row(what, float(np.abs(got - g64).max()), allowed)
