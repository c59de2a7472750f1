"""Cases of the dense iterations' parameter gradient, shared by tests/test_dense_grad_cases.py (CPU: the oracle is right and every
case is well posed) and tests/test_gpu_dense_grad.py (MI355X: bf_dense_iter_grad against float64 autograd of the oracle).

What bf_fit descends in its last two thirds is keypoints + 5 x silhouette + 5 * imsize / scan_height x closest-point, taken through
the whole mesh back to the parameters.  A case here = a model, a frame's problem, a parameter point away from the
initial estimate (non-zero translation, scale != 1, moved betas: loss_grad_cases.point) and, for the reverse mesh pass alone, a
cotangent on the body vertices: seeded normal numbers, scaled so that their parameter gradient is of the keypoint gradient's
magnitude.  Everything is built from fixed seeds; nothing here touches a GPU.
"""
import functools

import numpy as np
import torch

from bodyfitting_amd import synthetic as S
from oracle import mesh_oracle as MO
from oracle import smplify_oracle as O
import loss_grad_cases as LC
from scan_loss_cases import WELL_POSED                       # noqa: F401  (err32 <= WELL_POSED * M, block by block)

N_VIEWS = 4
# name -> (kind of loss_grad_cases, size or the bones per vertex of the 690-vertex SMPL variants of test_gpu_skinning_width.py)
MODELS = {"smpl690": ("smpl", "small"), "smpl6890": ("smpl", "full"), "kid690": ("kid", "small"), "nv690_B8": ("smpl", (5, 8)),
          "nv690_BD": ("smpl", (9, 12)), "smplx1200": ("smplx", "small"), "smplx10475": ("smplx", "full")}
# frames per batch of the reverse-pass checks: both sides of every frames-per-workgroup instance (1 / 2 / 4 / 8) with partly filled
# last groups, on both sides of BF_MFMA_MIN_FRAMES = 16
REVERSE_F = {"smpl690": (1, 2, 3, 4, 5, 8, 9, 15, 16, 17), "smpl6890": (1, 3, 8, 17), "kid690": (1, 5), "nv690_B8": (1, 4),
             "nv690_BD": (1, 4), "smplx1200": (1, 2, 7), "smplx10475": (1, 2)}
SUB_F = (1, 3)                      # one frame: the split tiles where the launch chooses them; three: a partly filled group of four
SUB_SAMPLED, SUB_KP = 0, 1          # bf_model_sub_vertices' `which`
TERMS4 = LC.TERMS
# the frames of a batch are 0, 1, 2, ... except where a frame's case is not well posed (chosen on the CPU: at smplx10475's frame 1 the
# float32 torch gradient of the scale, a sum that cancels, is 1.9e-5 of the block's maximum off the float64 one)
SKIP_FRAMES = {"smplx10475": (1,)}


def frames(name, n):
    """the frame numbers of a batch of n frames of the model"""
    out = [f for f in range(n + len(SKIP_FRAMES.get(name, ()))) if f not in SKIP_FRAMES.get(name, ())]
    return tuple(out[:n])


def kind(name):
    return MODELS[name][0]


def blocks(name):
    return O.SMPLX_PARAMS if kind(name) == "smplx" else LC.SMPL_BLOCKS


@functools.lru_cache(maxsize=None)
def model(name):
    k, size = MODELS[name]
    if isinstance(size, tuple):
        return S.make_model("smpl", seed=0, nv=690, bones=size)
    return LC.model(k, size)


def n_verts(name):
    return int(np.asarray(model(name)["v_template"]).shape[0])


@functools.lru_cache(maxsize=None)
def problem(name, frame):
    k, size = MODELS[name]
    if isinstance(size, tuple):
        return S.make_problem(model(name), frame=frame, n_views=N_VIEWS)
    return LC.problem(k, size, frame, N_VIEWS)


@functools.lru_cache(maxsize=None)
def _params(name, frame):
    return LC.point(kind(name), problem(name, frame), ("dense", name, frame))


def params(name, frame):
    return {k: v.copy() for k, v in _params(name, frame).items()}


def hyper_keywords(prob, **kw):
    """keyword arguments of native.make_hyper for a problem: exact silhouette distances on both sides"""
    return {"imsize": prob["imsize"], "constant_scale": prob.get("constant_scale", 0.3), "mask_cdist_form": 0, **kw}


@functools.lru_cache(maxsize=None)
def sub_vertices(name, which):
    """The vertices of a sub-model of the dense iterations, in its order (csrc/model_api.hip derive_sub): every fourth vertex first
    (SUB_SAMPLED only), then what the dense keypoint loss reads - selector vertices, the corners of the landmark faces, the support of
    the extra joint regressor - in ascending order.  Empty when the library builds none: more than 6 (5) tenths of the vertices, and
    the keypoint-only one for SMPL-X alone.  The GPU file holds the library's own list to this."""
    m = model(name)
    nv = n_verts(name)
    kv = np.zeros(nv, bool)
    kv[np.asarray(m["selector_ids"])] = True
    if "J_regressor_extra" in m:
        kv |= (np.asarray(m["J_regressor_extra"]) != 0).any(0)
    if kind(name) == "smplx":
        f = np.asarray(m["faces"])
        kv[f[np.asarray(m["lmk_faces_idx"])].ravel()] = True
        kv[f[np.asarray(m["dynamic_lmk_faces_idx"]).ravel()].ravel()] = True
    if which == SUB_KP and kind(name) != "smplx":
        return np.zeros(0, np.int32)
    first = np.arange(0, nv, 4) if which == SUB_SAMPLED else np.zeros(0, int)
    rest = np.nonzero(kv & ~np.isin(np.arange(nv), first))[0]
    ids = np.concatenate([first, rest]).astype(np.int32)
    return ids if len(ids) * 10 <= nv * (6 if which == SUB_SAMPLED else 5) else np.zeros(0, np.int32)


def sub_models(name):
    return tuple(w for w in (SUB_SAMPLED, SUB_KP) if len(sub_vertices(name, w)))


def _max(g, names):
    return max(float(np.abs(g[k]).max()) for k in names)


@functools.lru_cache(maxsize=None)
def _cotangent(name, frame, which):
    rng = np.random.default_rng(LC._seed("cotangent", name, frame, which))
    raw = rng.normal(size=(n_verts(name), 3))
    if which is not None:
        keep = np.zeros(n_verts(name), bool)
        keep[sub_vertices(name, which)] = True
        raw[~keep] = 0.0
    # scale: the cotangent's own pose gradient as large as the keypoint objective's (the objective is linear in the cotangent)
    m, pr, p = model(name), problem(name, frame), _params(name, frame)
    _, g_kp, _ = O.dense_loss_and_grad(m, LC.gmm_bufs(), pr, p)
    _, g_both, _ = O.dense_loss_and_grad(m, LC.gmm_bufs(), pr, p, cot=raw)
    g_raw = {k: g_both[k] - g_kp[k] for k in g_kp}
    return raw * (_max(g_kp, ("pose",)) / _max(g_raw, ("pose",)))


def cotangent(name, frame, which=None):
    """[NV,3] float64; which: None, or the sub-model off whose vertices it is zero"""
    return _cotangent(name, frame, which).copy()


def evaluate(name, frame, cot=None, dtype=torch.float64, **kw):
    """-> (terms dict over O.DENSE_TERMS, grads dict over blocks(name), body vertices) of the oracle at the case's point"""
    return O.dense_loss_and_grad(model(name), LC.gmm_bufs(), problem(name, frame), _params(name, frame), dtype=dtype, cot=cot, **kw)


@functools.lru_cache(maxsize=None)
def reverse_reference(name, frame, which=None):
    """the reverse-pass case of (model, frame): float64 and float32 torch evaluation of keypoints + sum(cot * vertices)"""
    cot = _cotangent(name, frame, which)
    t64, g64, _ = evaluate(name, frame, cot)
    t32, g32, _ = evaluate(name, frame, cot, dtype=torch.float32)
    return {"terms64": t64, "grads64": g64, "terms32": t32, "grads32": g32}


band, term_band = LC.band, LC.term_band


# ----------------------------------------------------------------------------------------------------------------------------
# scan term
# ----------------------------------------------------------------------------------------------------------------------------

SCAN_MODELS = ("smpl690", "smplx1200")
SCAN_FRAMES = ((0, 1.0), (1, 0.5))          # (frame, scan_scale): two scans of different height in one batch


@functools.lru_cache(maxsize=None)
def scan_problem(name, frame, scan_scale):
    """-> (problem, scan vertices, scan faces): synthetic.make_scan_problem(_smplx); SMPL-X scans keep the model's own faces and are
    scaled here (world, cameras and scan about the origin, so the keypoints stay where they are)"""
    m = model(name)
    if kind(name) != "smplx":
        return S.make_scan_problem(m, frame=frame, n_views=N_VIEWS, scan_scale=scan_scale)
    prob, sv, sf = S.make_scan_problem_smplx(m, frame, n_views=N_VIEWS, subdivide=0)
    sv = np.round(sv.astype(np.float64) * scan_scale, 4).astype(np.float32)
    c2ws = np.array(prob["c2ws"], np.float32)
    c2ws[:, :3, 3] *= np.float32(scan_scale)
    return dict(prob, c2ws=c2ws, constant_scale=float((sv[:, 1].max() - sv[:, 1].min()) / 1.7)), sv, sf


def scan_height(sv):
    return float(sv[:, 1].max() - sv[:, 1].min())


def scan_cscale(sv):
    """the constant scale the library derives from a scan, scan_height / 1.7 (smplify.py:156) - a float32 quotient there, and an input
    of the objective like every hyper-parameter: both sides use this number"""
    return float(np.float32(scan_height(sv)) / np.float32(1.7))


@functools.lru_cache(maxsize=None)
def _scan_params(name, frame, scan_scale):
    return LC.point(kind(name), scan_problem(name, frame, scan_scale)[0], ("scan", name, frame))


def scan_params(name, frame, scan_scale):
    return {k: v.copy() for k, v in _scan_params(name, frame, scan_scale).items()}


@functools.lru_cache(maxsize=None)
def _scan_cotangent(name, frame, scan_scale):
    rng = np.random.default_rng(LC._seed("scan cotangent", name, frame))
    raw = rng.normal(size=(n_verts(name), 3))
    prob = scan_problem(name, frame, scan_scale)[0]
    p = _scan_params(name, frame, scan_scale)
    _, g_kp, _ = O.dense_loss_and_grad(model(name), LC.gmm_bufs(), prob, p)
    _, g_both, _ = O.dense_loss_and_grad(model(name), LC.gmm_bufs(), prob, p, cot=raw)
    return raw * (_max(g_kp, ("pose",)) / max(float(np.abs(g_both["pose"] - g_kp["pose"]).max()), 1e-300))


def scan_cotangent(name, frame, scan_scale):
    return _scan_cotangent(name, frame, scan_scale).copy()


def scan_evaluate(name, frame, scan_scale, closest, cot=None, dtype=torch.float64):
    """the oracle with the scan term at closest points the caller found (constant, as the reference detaches them)"""
    prob, sv, _ = scan_problem(name, frame, scan_scale)
    return O.dense_loss_and_grad(model(name), LC.gmm_bufs(), prob, _scan_params(name, frame, scan_scale), dtype=dtype, cot=cot,
                                 closest=closest, scan_height=scan_height(sv), constant_scale=scan_cscale(sv))


def closest_points(sv, sf, vertices32):
    """the reference's search in its own float32 arithmetic at float32 vertices -> (face ids, points)"""
    ids, cpts, _ = MO.ReferenceSearcher(sv, sf).nearest(np.ascontiguousarray(vertices32, np.float32))
    return ids, cpts


# ----------------------------------------------------------------------------------------------------------------------------
# silhouette term
# ----------------------------------------------------------------------------------------------------------------------------

# The silhouette loss is piecewise smooth: every contour point pulls the nearest projected vertex (first minimum), weighted 1 or 10 by
# the mask pixel under that vertex (its coordinates truncated), and only vertices that project inside the image count.  A float32
# evaluation can be compared with float64 autograd only where both take the same pieces, so the case is chosen, on the CPU, such that in
# float64 (a) the nearest and the second-nearest projected vertex of every contour point, (b) the chosen vertices' pixel coordinates
# and the nearest integer and (c) every sampled vertex's projection and the image border are all farther apart than MASK_MARGIN.
# MASK_MARGIN is 8 x MASK_UV_ERR32, the largest |uv32 - uv64| of the case over its sampled vertices and mask views, measured with the
# oracle alone (test_dense_grad_cases.py prints and bounds it): float32 against float64 torch evaluation of the projection.
MASK_MODEL = "smpl6890"                      # the model of tests/test_gpu_mask.py
MASK_IMSIZE = 64
MASK_FRAME, MASK_VIEWS, MASK_POINT_SEED = 0, (1, 3), 0
MASK_UV_ERR32 = 8.5e-6                       # measured 4.70e-6 alone, 8.42e-6 with the scan's constant scale (test_silhouette_case_margins)
MASK_MARGIN = 8 * MASK_UV_ERR32


@functools.lru_cache(maxsize=None)
def mask_problem(frame=MASK_FRAME, views=MASK_VIEWS, imsize=MASK_IMSIZE):
    return S.make_problem(model(MASK_MODEL), frame=frame, n_views=N_VIEWS, imsize=imsize, mask_frames=list(views))


@functools.lru_cache(maxsize=None)
def _mask_params(frame=MASK_FRAME, views=MASK_VIEWS, imsize=MASK_IMSIZE, seed=MASK_POINT_SEED):
    return LC.point("smpl", mask_problem(frame, views, imsize), ("mask", frame, seed))


def mask_params(*a):
    return {k: v.copy() for k, v in _mask_params(*a).items()}


@functools.lru_cache(maxsize=None)
def mask_inputs(frame=MASK_FRAME, views=MASK_VIEWS, imsize=MASK_IMSIZE):
    """-> dict(contours, masks (0 / 1 float32 [M,H,W]), views) for O.dense_loss_and_grad, plus masks_u8 [M,H,W] as the library takes them"""
    from oracle.contour_oracle import border_pixels_rowmajor_all as extract_contours
    prob = mask_problem(frame, views, imsize)
    u8 = np.array(prob["masks"])
    mk = (u8 > 128).astype(np.float32)
    return {"contours": [np.asarray(c, np.float32) for c in extract_contours(mk)], "masks": mk,
            "views": [prob["use_frames"].index(f) for f in prob["mask_frames"]], "masks_u8": u8}


@functools.lru_cache(maxsize=None)
def mask_scan():
    """a scan for the silhouette case: its ground-truth body in the problem's world (constant scale 0.3: half a metre tall) with
    make_scan_problem's noise, rounded to the 4 decimals of an OBJ -> (vertices, faces)"""
    prob = mask_problem()
    gt, c = prob["gt"], prob["constant_scale"]
    verts, _ = S.smpl_joints64(model(MASK_MODEL), gt["betas"], gt["pose"])
    world = (verts + gt["transl"]) * gt["scale"] * c
    rng = np.random.default_rng(LC._seed("mask scan"))
    sv = np.round(world + 0.003 * c * S._scan_noise(world / c, rng), 4).astype(np.float32)
    return sv, np.asarray(model(MASK_MODEL)["faces"], np.int32)


def mask_evaluate(dtype=torch.float64, cot=None, closest=None, height=None, cscale=None, case=()):
    """the oracle at the silhouette case; closest / height: with a scan term as well; cscale: the constant scale (with a scan
    attached the library takes scan_cscale of it), default the problem's"""
    mi = mask_inputs(*case[:3])
    return O.dense_loss_and_grad(model(MASK_MODEL), LC.gmm_bufs(), mask_problem(*case[:3]), _mask_params(*case), dtype=dtype, cot=cot,
                                 masks={k: mi[k] for k in ("contours", "masks", "views")}, closest=closest, scan_height=height,
                                 constant_scale=mask_problem(*case[:3])["constant_scale"] if cscale is None else cscale)


def mask_margins(case=(), cscale=None):
    """-> dict(uv_err32, gap, pixel, border): the float32 projection's largest error and the three smallest float64 margins of the case"""
    prob, mi = mask_problem(*case[:3]), mask_inputs(*case[:3])
    out = {"uv_err32": 0.0, "gap": np.inf, "pixel": np.inf, "border": np.inf}
    uv = {}
    for dt in (torch.float64, torch.float32):
        _, _, bv = mask_evaluate(dt, cscale=cscale, case=case)
        w2cs = torch.inverse(torch.as_tensor(np.asarray(prob["c2ws"]), dtype=torch.float32).to(dt))
        Kt = torch.as_tensor(np.asarray(prob["Ks"]), dtype=torch.float32).to(dt)
        v4 = torch.as_tensor(bv, dtype=dt)[::4]
        uv[dt] = [O.perspective_projection(v4[None], w2cs[i][None, :3, :3], w2cs[i][None, :3, 3], Kt[i])[0].numpy().astype(np.float64)
                  for i in mi["views"]]
    for i, (a, b) in enumerate(zip(uv[torch.float64], uv[torch.float32])):
        out["uv_err32"] = max(out["uv_err32"], float(np.abs(a - b).max()))
        out["border"] = min(out["border"], float(np.minimum(np.abs(a), np.abs(a - prob["imsize"])).min()))
        inside = ((a < prob["imsize"]) & (a >= 0)).all(1)
        pin, c = a[inside], np.asarray(mi["contours"][i], np.float64)
        if len(pin) < 2 or len(c) == 0:
            continue
        d = np.sqrt(((c[:, None, :] - pin[None, :, :]) ** 2).sum(-1))
        order = np.argsort(d, axis=1)[:, :2]
        rows = np.arange(len(c))
        out["gap"] = min(out["gap"], float((d[rows, order[:, 1]] - d[rows, order[:, 0]]).min()))
        chosen = pin[np.unique(order[:, 0])]
        out["pixel"] = min(out["pixel"], float(np.abs(chosen - np.round(chosen)).min()))
    return out
