"""What tests/test_mask_loss_autograd.py (CPU) and tests/test_gpu_mask_loss.py (GPU) share: the synthetic silhouette problems the
stand-alone multview_mask_loss is tried on, their references - torch autograd of oracle.smplify_oracle.multview_mask_loss in float64
(exact distances: the truth) and in float32 from the same float32 inputs - the error band (scan_loss_cases.Band: DESIGN.md 2.3's
rule, imported, not copied) and float64 stand-ins for the native calls.

A case needs no body model: its vertices are points on an ellipsoid in front of M cameras on a ring, a view's mask is a shape drawn
where a coarser version of the same ellipsoid projects, and its contour is oracle/contour_oracle.py's.

The loss is piecewise smooth, so a float32 evaluation can be held to float64 autograd only where both take the same pieces.  Every
case is therefore built, on the CPU and from its seed alone, so that three float64 margins (dense_grad_cases.mask_margins' three,
restated here for caller-held vertices) all exceed the case's margin:
  gap     nearest against second-nearest inside vertex of every contour point
  pixel   the chosen vertices' pixel coordinates against the nearest integer
  border  every sampled vertex's projection against the image border (0 and imsize)
  margin  the larger of  8 x the largest |uv32 - uv64| of the case (what the exact form needs)  and  16 x the largest difference,
          over the case's (contour point, inside vertex) pairs, between torch's float32 cdist-form distance and the float64 distance
          (what the cdist form needs) - both measured with torch and the oracle's projection alone.
The builder draws the vertices from the seed and then draws the sampled vertices that stand too close to a decision again (with the
same generator) until the margins hold: no case is skipped, filtered or compared by share.  A vertex closer than NEAR pixels to a
contour point is drawn again too: the cdist form's error grows as 1 / distance, and with it the margin.
"""
import functools

import numpy as np
import torch

from oracle import contour_oracle as CO
from oracle import smplify_oracle as O
from scan_loss_cases import Band          # noqa: F401  (the band: imported, not copied)

STRIDE = 4                         # loss.py:99
NEAR = 0.4                         # pixels: no sampled vertex this close to a contour point
SLACK = 1.5                        # the builder keeps this factor between the margins and the case's margin
RADII = np.array([0.25, 0.40, 0.20])
RING = 3.0


class Case:
    def __init__(self, name, ns, M=2, size=32, H=None, W=None, imsize=None, eps=10.0, mask="ellipse", away=(), seed=0, r=None, repeat=1):
        self.name, self.ns, self.M, self.eps, self.mask, self.away, self.seed, self.repeat = name, ns, M, float(eps), mask, tuple(away), seed, repeat
        self.H, self.W = H or size, W or size
        self.imsize = float(imsize or min(self.H, self.W))
        self.r = (ns % 4 if r is None else r) if ns > 1 else (3 if r is None else r)      # n_verts = 4 Ns - r: mostly no multiple of 4
        self.n_verts = 4 * ns - self.r

    def __repr__(self):
        return self.name


def _cases():
    out = []
    # sampled-vertex counts: the contour scan's 16 lanes and record pairs, the wave, the LDS tile and the project block, the 690 of the
    # small model; n_verts 255 / 256 / 257: the finish kernel's vertex block
    for ns in (1, 2, 15, 16, 17):
        out.append(Case(f"ns{ns}", ns, size=16))
    for ns in (31, 32, 33, 63, 64, 65):
        out.append(Case(f"ns{ns}", ns, size=32))
    for ns in (255, 256, 257, 690):
        out.append(Case(f"ns{ns}", ns, size=64))
    out += [Case("nverts255", 64, r=1), Case("nverts256", 64, r=0), Case("nverts257", 65, r=3)]
    # contour lengths: one point, the 16 points of a 256-thread block, about 200, and more than 64 blocks of them (the finish
    # kernel's lanes take every 64th block sum): the border repeated, as a caller may pass it
    out += [Case("contour1", 33, mask="pixel"), Case("contour15", 33, mask="rect15"), Case("contour16", 33, mask="rect16"),
            Case("contour17", 33, mask="rect17"), Case("contour200", 65, size=64, mask="big"),
            Case("contour1100", 33, size=64, mask="big", repeat=6)]
    # views
    out += [Case("views1", 33, M=1), Case("views3", 33, M=3), Case("views8", 17, M=8, size=16),
            Case("view_without_inside_vertex", 33, M=3, away=(1,))]
    # image shapes and hypers
    out += [Case("imsize32_in_64x64", 33, H=64, W=64, imsize=32), Case("h48_w80", 33, H=48, W=80, imsize=48),
            Case("eps1", 33, eps=1.0), Case("eps37.5", 33, eps=37.5), Case("two_components", 33, mask="two"),
            Case("all_foreground", 33, size=16, mask="full")]
    return out


CASES = _cases()
CASE_NAMES = [c.name for c in CASES]
GRADCHECK_CASES = ("ns17", "view_without_inside_vertex", "h48_w80")


def case(name):
    return CASES[CASE_NAMES.index(name)]


# ----------------------------------------------------------------------------------------------------------------------------
# geometry
# ----------------------------------------------------------------------------------------------------------------------------

def _cameras(c, rng):
    """M cameras on a ring of radius RING looking at the origin (a view in c.away: past it, so nothing projects inside) ->
    w2c float32[M,4,4], K float32[M,3,3]"""
    w2c, K = np.zeros((c.M, 4, 4)), np.zeros((c.M, 3, 3))
    for i in range(c.M):
        a = 2 * np.pi * (i + 0.3 * rng.uniform(-1, 1)) / c.M
        pos = RING * np.array([np.cos(a), 0.15 * rng.uniform(-1, 1), np.sin(a)])
        target = np.array([4.0, 0.3, 0.0]) + pos if i in c.away else 0.05 * rng.uniform(-1, 1, 3)
        z = (target - pos) / np.linalg.norm(target - pos)
        x = np.cross([0.0, 1.0, 0.0], z); x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])
        w2c[i, :3, :3], w2c[i, :3, 3], w2c[i, 3, 3] = R, -R @ pos, 1.0
        f = 0.55 * c.imsize * RING / (2 * RADII[1])                 # the ellipsoid spans about 55 % of the image
        K[i] = [[f, 0.0, c.imsize / 2 + rng.uniform(-1, 1)], [0.0, f * (1 + 0.05 * rng.uniform(-1, 1)), c.imsize / 2 + rng.uniform(-1, 1)], [0, 0, 1]]
    return w2c.astype(np.float32), K.astype(np.float32)


def _on_ellipsoid(rng, n, scale=1.0):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * RADII * scale * (1 + 0.05 * rng.uniform(-1, 1, (n, 1)))


def project(verts, w2c, K, dtype):
    """the oracle's projection of verts[::STRIDE] in every view -> float64 [M,Ns,2], evaluated in `dtype`"""
    v = torch.as_tensor(np.asarray(verts), dtype=torch.float32).to(dtype)[::STRIDE]
    w, k = torch.as_tensor(w2c).to(dtype), torch.as_tensor(K).to(dtype)
    return np.stack([O.perspective_projection(v[None], w[i][None, :3, :3], w[i][None, :3, 3], k[i])[0].numpy().astype(np.float64)
                     for i in range(len(w))])


def _masks(c, w2c, K):
    """per view the shape drawn where a coarser ellipsoid (a fixed 12 x 6 grid of points on it, 85 % of the size) projects"""
    lon, lat = np.meshgrid(np.linspace(0, 2 * np.pi, 12, endpoint=False), np.linspace(0.15, np.pi - 0.15, 6))
    coarse = 0.85 * RADII * np.stack([np.sin(lat) * np.cos(lon), np.cos(lat), np.sin(lat) * np.sin(lon)], -1).reshape(-1, 3)
    uv = project(np.repeat(coarse, STRIDE, 0), w2c, K, torch.float64)
    masks = np.zeros((c.M, c.H, c.W), np.uint8)
    yy, xx = np.mgrid[:c.H, :c.W]
    for i in range(c.M):
        lo, hi = uv[i].min(0), uv[i].max(0)
        if i in c.away:
            lo, hi = np.array([0.3, 0.3]) * c.imsize, np.array([0.7, 0.75]) * c.imsize
        mid, rad = (lo + hi) / 2, (hi - lo) / 2
        cx, cy = int(round(mid[0])), int(round(mid[1]))
        if c.mask == "big":                                      # a rounded box over most of the image: a border of about 200 points
            masks[i] = ((xx - mid[0]) / (0.38 * c.W)) ** 4 + ((yy - mid[1]) / (0.44 * c.H)) ** 4 <= 1
        elif c.mask in ("ellipse", "two"):
            masks[i] = ((xx - mid[0]) / rad[0]) ** 2 + ((yy - mid[1]) / rad[1]) ** 2 <= 1
            if c.mask == "two":                                   # a second, smaller component further down: the border met last
                masks[i, c.H - 4:c.H - 2, 2:6] = 1
        elif c.mask == "pixel":
            masks[i, cy, cx] = 1
        elif c.mask in ("rect15", "rect16", "rect17"):            # w x h: 2 (w + h) - 4 points; one corner less: one point less
            w = {"rect15": 6, "rect16": 6, "rect17": 7}[c.mask]
            masks[i, cy - 2:cy + 2, cx - 3:cx - 3 + w] = 1
            if c.mask != "rect16":
                masks[i, cy - 2, cx - 3] = 0
        elif c.mask == "full":
            masks[i] = 1
        else:
            raise ValueError(c.mask)
    return masks


def _decisions(uv, contours, imsize):
    """the float64 margins of projections uv[M,Ns,2] -> (dict(gap, pixel, border, near), the sampled vertices that set them)"""
    out = {"gap": np.inf, "pixel": np.inf, "border": np.inf, "near": np.inf}
    who = {k: [] for k in out}

    def note(key, value, s):
        who[key].append((float(value), int(s)))
        out[key] = min(out[key], float(value))

    for i, a in enumerate(uv):
        b = np.minimum(np.abs(a), np.abs(a - imsize)).min(1)
        for s in np.argsort(b):
            note("border", b[s], s)
        inside = ((a < imsize) & (a >= 0)).all(1)
        ids, pin, c = np.flatnonzero(inside), a[inside], np.asarray(contours[i], np.float64)
        if len(pin) == 0 or len(c) == 0:
            continue
        d = np.sqrt(((c[:, None, :] - pin[None, :, :]) ** 2).sum(-1))
        near = d.min(0)
        for s in np.argsort(near):
            note("near", near[s], ids[s])
        order = np.argsort(d, axis=1, kind="stable")[:, :2]
        rows = np.arange(len(c))
        if len(pin) > 1:
            gap = d[rows, order[:, 1]] - d[rows, order[:, 0]]
            for q in np.argsort(gap):
                note("gap", gap[q], ids[order[q, 1]])
        for s in np.unique(order[:, 0]):
            note("pixel", np.abs(pin[s] - np.round(pin[s])).min(), ids[s])
    return out, who


def _cdist_err32(uv32, uv64, contours, imsize):
    """the largest difference between torch's float32 cdist-form distance (the matmul form, forced) and the float64 distance, over
    the (contour point, inside vertex) pairs"""
    worst = 0.0
    for a32, a64, c in zip(uv32, uv64, contours):
        inside = ((a64 < imsize) & (a64 >= 0)).all(1)
        if not inside.any() or len(c) == 0:
            continue
        d32 = torch.cdist(torch.as_tensor(a32[inside], dtype=torch.float32)[None], torch.as_tensor(np.asarray(c), dtype=torch.float32)[None],
                          compute_mode="use_mm_for_euclid_dist")[0].numpy().astype(np.float64)
        d64 = np.sqrt(((a64[inside][:, None, :] - np.asarray(c, np.float64)[None, :, :]) ** 2).sum(-1))
        worst = max(worst, float(np.abs(d32 - d64).max()))
    return worst


def margins_of(uv64, uv32, contours, imsize, cdist=True):
    """-> (dict(uv_err32, cdist_err32, margin, gap, pixel, border, near), the sampled vertices that set them) of the float64 and
    float32 projections uv[M,Ns,2]; cdist False: a case that is evaluated with exact distances only"""
    out, who = _decisions(uv64, contours, imsize)
    out["uv_err32"] = float(np.abs(uv32 - uv64).max())
    out["cdist_err32"] = _cdist_err32(uv32, uv64, contours, imsize) if cdist else 0.0
    out["margin"] = max(8 * out["uv_err32"], 16 * out["cdist_err32"])
    return out, who


def margins(c, verts, w2c, K, contours):
    return margins_of(project(verts, w2c, K, torch.float64), project(verts, w2c, K, torch.float32), contours, c.imsize)


def well_posed(m):
    return min(m["gap"], m["pixel"], m["border"]) > m["margin"]


@functools.lru_cache(maxsize=None)
def build(name):
    """-> dict(case, verts float32[n_verts,3], w2c, K, masks uint8[M,H,W], contours list of float32[C,2], margins)"""
    c = case(name)
    rng = np.random.default_rng([c.seed, sum(map(ord, name))])
    w2c, K = _cameras(c, rng)
    masks = _masks(c, w2c, K)
    contours = [np.tile(CO.extract_contour(m, "opencv_first"), (c.repeat, 1)) for m in masks]
    assert all(len(k) > 0 for k in contours)
    verts = _on_ellipsoid(rng, c.n_verts).astype(np.float32)
    for _ in range(400):
        m, who = margins(c, verts, w2c, K, contours)
        want = SLACK * m["margin"]
        again = {s for key in ("gap", "pixel", "border") for value, s in who[key] if value <= want}
        again |= {s for value, s in who["near"] if value < NEAR}
        if not again:
            break
        for s in sorted(again):
            verts[s * STRIDE] = _on_ellipsoid(rng, 1)[0]
    else:
        raise AssertionError(f"{name}: no well-posed vertices found: {m}")
    assert well_posed(m), (name, m)
    uv = project(verts, w2c, K, torch.float64)
    for i in range(c.M):
        assert (((uv[i] < c.imsize) & (uv[i] >= 0)).all(1).sum() == 0) == (i in c.away), (name, i)
    return {"case": c, "verts": verts, "w2c": w2c, "K": K, "masks": masks, "contours": contours, "margins": m}


# ----------------------------------------------------------------------------------------------------------------------------
# references: torch autograd of oracle.smplify_oracle.multview_mask_loss
# ----------------------------------------------------------------------------------------------------------------------------

@torch.enable_grad()          # (also called inside an autograd Function's forward, where grad mode is off)
def oracle_loss(verts, w2c, K, masks, contours, imsize, eps, dtype, pairwise, views=None):
    """-> (value, dverts float64[n_verts,3]) of the views `views` (default all), evaluated in `dtype`"""
    views = range(len(masks)) if views is None else views
    v = torch.tensor(np.asarray(verts), dtype=dtype, requires_grad=True)
    cs = [torch.as_tensor(np.asarray(contours[i]), dtype=dtype).reshape(-1, 2) for i in views]
    mk = torch.as_tensor(np.asarray(masks, np.float64)[list(views)], dtype=dtype)
    w = torch.as_tensor(np.asarray(w2c)[list(views)], dtype=dtype)
    k = torch.as_tensor(np.asarray(K)[list(views)], dtype=dtype)
    loss = O.multview_mask_loss(cs, mk, v, w, k, imsize=imsize, epsilon=eps, pairwise=pairwise)
    loss.backward()
    return float(loss.detach().double()), v.grad.double().numpy()


@functools.lru_cache(maxsize=None)
def references(name):
    """-> dict: "f64" the truth (exact distances, float64), "exact" and "cdist" the same function in float32 (pairwise "exact" and
    "torch"), each (value, dverts)"""
    b = build(name)
    c = b["case"]
    args = (b["verts"], b["w2c"], b["K"], b["masks"], b["contours"], c.imsize, c.eps)
    return {"f64": oracle_loss(*args, torch.float64, "exact"), "exact": oracle_loss(*args, torch.float32, "exact"),
            "cdist": oracle_loss(*args, torch.float32, "torch")}


# ----------------------------------------------------------------------------------------------------------------------------
# one step of a user's loop (smplify.py:177-213 with use_mask=True) on the 690-vertex model
# ----------------------------------------------------------------------------------------------------------------------------

LOOP_IMSIZE, LOOP_VIEWS, LOOP_MASK_FRAMES = 64, 4, (1, 3)
LOOP_BLOCKS = ("global_transl", "scale", "pose", "betas", "global_orient")


@functools.lru_cache(maxsize=None)
def loop_problem():
    import loss_grad_cases as LC
    from bodyfitting_amd import synthetic as S
    model = LC.model("smpl", "small")
    prob = S.make_problem(model, frame=0, n_views=LOOP_VIEWS, imsize=LOOP_IMSIZE, mask_frames=list(LOOP_MASK_FRAMES))
    mk = (np.array(prob["masks"]) > 128).astype(np.uint8)
    masks = {"contours": [CO.extract_contour(m, "opencv_first") for m in mk], "masks": mk.astype(np.float32),
             "views": [prob["use_frames"].index(f) for f in prob["mask_frames"]]}
    return model, prob, masks


def loop_evaluate(params, dtype):
    """the oracle's expression of one iteration - keypoint terms + 5 x multview_mask_loss (exact distances) - and its autograd ->
    (total, dict of the parameter blocks' gradients, body vertices)"""
    import loss_grad_cases as LC
    model, prob, masks = loop_problem()
    terms, grads, bv = O.dense_loss_and_grad(model, LC.gmm_bufs(), prob, params, dtype=dtype, masks=masks,
                                             constant_scale=prob.get("constant_scale", 0.3))
    return float(sum(terms.values())), grads, bv


def loop_margins(params):
    _, prob, masks = loop_problem()
    uv = {}
    for dt in (torch.float64, torch.float32):
        bv = loop_evaluate(params, dt)[2]
        w2cs = torch.inverse(torch.as_tensor(np.asarray(prob["c2ws"]), dtype=torch.float32).to(dt))
        Kt = torch.as_tensor(np.asarray(prob["Ks"]), dtype=torch.float32).to(dt)
        v4 = torch.as_tensor(bv, dtype=dt)[::STRIDE]
        uv[dt] = np.stack([O.perspective_projection(v4[None], w2cs[i][None, :3, :3], w2cs[i][None, :3, 3], Kt[i])[0].numpy().astype(np.float64)
                           for i in masks["views"]])
    return margins_of(uv[torch.float64], uv[torch.float32], masks["contours"], prob["imsize"], cdist=False)[0]


@functools.lru_cache(maxsize=None)
def loop_case():
    """-> (seed, params, margins): the first seed whose parameter point (loss_grad_cases.point: away from the initial estimate) is
    well posed"""
    import loss_grad_cases as LC
    _, prob, _ = loop_problem()
    for seed in range(64):
        params = LC.point("smpl", prob, ("mask loop", seed))
        m = loop_margins(params)
        if well_posed(m):
            return seed, params, m
    raise AssertionError("no well-posed parameter point among 64 seeds")


# ----------------------------------------------------------------------------------------------------------------------------
# float64 stand-ins for the native calls (the CPU file)
# ----------------------------------------------------------------------------------------------------------------------------

class StandInSilhouette:
    """native.Silhouette over the oracle, in float64"""
    created = 0
    followed = 0              # objects whose contours were extracted (contours=None)

    def __init__(self, masks, contours=None, device=0, contour_select=0):
        type(self).created += 1
        m = np.asarray(masks) != 0
        self.masks = (m[None] if m.ndim == 2 else m).astype(np.uint8)
        self.n_views, self.H, self.W = self.masks.shape
        self.device = int(device)
        if contours is None:
            type(self).followed += 1
            assert contour_select == 0
            self._contours = [CO.extract_contour(k, "opencv_first") for k in self.masks]
        else:
            self._contours = [np.asarray(k, np.float64).reshape(-1, 2) for k in contours]
            assert len(self._contours) == self.n_views

    def contours(self):
        return [np.asarray(k, np.float32) for k in self._contours]

    def loss(self, verts, w2c, K, imsize=512, epsilon=10, stride=4, cdist_form=True, want_grad=True):
        assert stride == STRIDE
        v = np.asarray(verts)
        value, grad = oracle_loss(v.astype(np.float64), w2c, K, self.masks, self._contours, imsize, epsilon, torch.float64, "exact")
        like = np.float64 if v.dtype == np.float64 else np.float32
        return np.asarray(value, like), None, (np.asarray(grad, like) if want_grad else None)

    def close(self):
        pass


def install_stand_ins(monkeypatch):
    """the native calls of loss.py's silhouette functions replaced, float64 let through (gradcheck needs it)"""
    from bodyfitting_amd import loss, native, prior
    monkeypatch.setattr(native, "Silhouette", StandInSilhouette)
    monkeypatch.setattr(prior, "_require_float32", lambda who, name, x: None)
    monkeypatch.setattr(loss, "_SILHOUETTES", {})
    StandInSilhouette.created = StandInSilhouette.followed = 0
