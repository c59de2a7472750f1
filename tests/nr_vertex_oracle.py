"""CPU oracle of the geometry gradient of `neural_renderer.Renderer` (bf_nr_render_taped, bf_nr_tape_vertex_grad).  TEST
INFRASTRUCTURE ONLY.

A numpy restatement of thirdparty/neural_renderer's backward_pixel_map and backward_depth_map (cuda/rasterize_cuda_kernel.cu:245-503,
543-592), of the reverse of lighting.py:41-52 and of projection.py:19-42 with zero distortion, on top of tests/nr_oracle.py's render
(imported, not edited).  The DECISIONS - floor / ceil of a crossing, record equality, `diff_grad <= 0`, the winding test - are
taken in the float32 / double mix the source writes, so the same terms enter the sums as on the device; the SUMS are float64.
Every gradient comes back as (grad, n, S): the value, the number of terms and the sum of their magnitudes - what a float32 sum in
any order is held to.  Where a term is itself a difference that may cancel (diff_grad, the depth pass's sum over inv / z, the
projection's reverse) S is formed from the magnitudes of ITS terms.  A line of an edge that is exactly axis-parallel at an integer
pixel coordinate is 0 / 0 in the source: skipped here and on the device.

`OracleRenderer / OracleMesh / OracleTape` extend nr_oracle's with set_vertices, render_taped and vertex_grad: what
bodyfitting_amd/neural_renderer.py calls on native.Nr* with geometry_grad on.
"""
import math

import numpy as np

from oracle import texfit_oracle as TO
import nr_oracle as NO

F32, F64 = np.float32, np.float64
TAPE_TEXTURES, TAPE_GEOMETRY = 1, 2
EPS = F32(1e-3)                      # rasterizer_eps


# ---- forward, keeping what the reverse pass reads ------------------------------------------------------------------------------------

def render(verts, faces, textures, K=None, R=None, t=None, orig_size=None, image_size=16, near=0.1, far=100.0, background=(0, 0, 0),
           anti_aliasing=True, fill_back=True, lightoff=False, light=None, ndc=False, want=("rgb", "depth", "alpha")):
    """nr_oracle.render's steps (its helpers, texfit_oracle's rasteriser) -> (rgb | None, depth | None, alpha | None, keep)"""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    light = dict(light or NO.DEFAULT_LIGHT)
    with_rgb = "rgb" in want
    rec_faces, rec_tex = NO.fill_back_records(faces, textures if with_rgb else None) if fill_back else \
        (faces, np.asarray(textures, F32) if with_rgb else None)
    rec_faces = rec_faces.astype(np.int64)
    lit = with_rgb and not lightoff
    rows = NO.light_rows(verts[rec_faces], **light) if lit else None
    pv = verts if ndc else TO.project(verts, K, R, t, orig_size)
    fv = pv[rec_faces]
    is2 = image_size * 2 if anti_aliasing else image_size
    fi, w, d = TO.rasterize(fv, is2, near, far)
    keep = dict(verts=verts, n_faces=len(faces), rec_faces=rec_faces, fv=fv.astype(F32), face_index=fi, weight=w, depth=d, is2=is2,
                image_size=image_size, anti_aliasing=anti_aliasing, light=rows, light_cfg=light, lit=lit, ndc=ndc, want=tuple(want),
                cam=None if ndc else (np.asarray(K, F32).reshape(3, 3), np.asarray(R, F32).reshape(3, 3), np.asarray(t, F32).reshape(3), F32(orig_size)),
                rgb_map=None, unlit=None)
    rgb = None
    if with_rgb:
        mask = (fi >= 0).astype(F32)[:, :, None]
        unlit, sidx, sw = TO.sample_textures(fv, rec_tex, fi, w, d)
        raw = unlit if rows is None else TO.sample_textures(fv, (rec_tex * rows[:, None, None, None, :]).astype(F32), fi, w, d)[0]
        raw = (raw * mask + (F32(1) - mask) * np.asarray(background, F32)[None, None, :]).astype(F32)
        rgb = NO.pool(raw.transpose(2, 0, 1), image_size, anti_aliasing)
        keep.update(rgb_map=raw, unlit=unlit, sampling_index=sidx, sampling_weight=sw, ts=np.asarray(textures).shape[1])
    return (rgb, NO.pool(d, image_size, anti_aliasing) if "depth" in want else None,
            NO.pool((fi >= 0).astype(F32), image_size, anti_aliasing) if "alpha" in want else None, keep)


def unpool(g, keep, dtype=F32):
    """the cotangent of a pooled, flipped map [..., is, is] at the super-sampled pixels [..., is2, is2] (x 0.25 with anti-aliasing:
    exact in float32)"""
    g = np.asarray(g, dtype)
    if keep["anti_aliasing"]:
        g = (np.repeat(np.repeat(g, 2, axis=-2), 2, axis=-1) * dtype(0.25)).astype(dtype)
    return np.ascontiguousarray(g[..., ::-1, :])


# ---- backward_pixel_map --------------------------------------------------------------------------------------------------------------

def _to_int(v, lo, hi):
    """float -> int as the source's target converts: NaN -> 0, saturating (the callers clamp to [lo, hi] anyway)"""
    return 0 if v != v else int(min(max(v, lo), hi))


def _cross(a0, a1, b0, b1, d0):
    with np.errstate(divide="ignore", invalid="ignore"):
        return F32(F32(F32(F32(b1 - a1) / F32(b0 - a0)) * F32(d0 - a0)) + a1)


def _dist(num, den, off, is_):
    d = F32(F64(F32(F32(num / den) * off)) * 2.0 / F64(is_))
    return F32(d + EPS) if 0 < d else F32(d - EPS)


def pixel_map_vjp(keep, g_rgb=None, g_alpha=None):
    """-> (grad_frec[nrec,3,3], n, S) for the cotangents of the pooled rgb [3,is,is] and alpha [is,is] (None: that term is absent)"""
    fv, fi, is_ = keep["fv"], keep["face_index"], keep["is2"]
    nrec = len(fv)
    grad, n, S = np.zeros((nrec, 3, 3)), np.zeros((nrec, 3, 3), np.int64), np.zeros((nrec, 3, 3))
    if g_rgb is None and g_alpha is None:
        return grad, n, S
    ga = None if g_alpha is None else unpool(g_alpha, keep)
    gc = None if g_rgb is None else unpool(g_rgb, keep).transpose(1, 2, 0)
    rgb_map = keep["rgb_map"]
    alpha = (fi >= 0).astype(F32)

    def diff_grad(y, x, a_ref, c_ref):
        """(float32 value as the source sums it, sum of the magnitudes of its terms)"""
        diff, mag = F32(0), 0.0
        if ga is not None:
            term = F32(F32(alpha[y, x] - a_ref) * ga[y, x])
            diff, mag = F32(diff + term), mag + abs(float(term))
        if gc is not None:
            for c in range(3):
                term = F32(F32(rgb_map[y, x, c] - c_ref[c]) * gc[y, x, c])
                diff, mag = F32(diff + term), mag + abs(float(term))
        return diff, mag

    for k in range(nrec):
        f = fv[k].reshape(9)
        if F32(f[7] - f[1]) * F32(f[3] - f[0]) < F32(f[4] - f[1]) * F32(f[6] - f[0]):
            continue
        pp = (F32(0.5) * (fv[k][:, :2] * F32(is_) + F32(is_) - F32(1))).astype(F32)
        for e in range(3):
            pi = [(e + m) % 3 for m in range(3)]
            for axis in range(2):
                p = [[pp[pi[m]][(dim + axis) % 2] for dim in range(2)] for m in range(3)]
                if p[0][0] == p[1][0]:
                    continue
                direction = (-1 if p[0][0] < p[1][0] else 1) if axis == 0 else (1 if p[0][0] < p[1][0] else -1)
                lo, hi = min(p[0][0], p[1][0]), max(p[0][0], p[1][0])
                if not (lo == lo and hi == hi):
                    continue
                d0_from, d0_to = int(max(math.ceil(min(max(lo, -1.0), is_)), 0.0)), int(min(max(hi, -2.0), is_ - 1.0))
                for d0 in range(d0_from, d0_to + 1):
                    fd0 = F32(d0)
                    cross = _cross(p[0][0], p[0][1], p[1][0], p[1][1], fd0)
                    if not (cross > -2 and cross < is_ + 1):
                        continue
                    d1_in = int(math.floor(cross)) if direction > 0 else int(math.ceil(cross))
                    d1_out = d1_in + direction
                    if d1_in < 0 or is_ <= d1_in or d1_out < 0 or is_ <= d1_out:
                        continue
                    at = (lambda d1: (d1, d0)) if axis == 0 else (lambda d1: (d0, d1))
                    y_in, x_in = at(d1_in)
                    y_out, x_out = at(d1_out)

                    def walk(d1_from, d1_to, own, a_ref, c_ref):
                        for d1 in range(d1_from, d1_to + 1):
                            y, x = at(d1)
                            if own and fi[y, x] != k:
                                continue
                            diff, mag = diff_grad(y, x, a_ref, c_ref)
                            if diff <= 0:
                                continue
                            off = F32(F32(d1) - cross)
                            for end, den in ((0, F32(p[1][0] - fd0)), (1, F32(fd0 - p[0][0]))):
                                if (p[1][0] if end == 0 else p[0][0]) == fd0:
                                    continue
                                dist = F64(_dist(F32(p[1][0] - p[0][0]), den, off, is_))
                                grad[k, pi[end], 1 - axis] -= F64(diff) / dist
                                n[k, pi[end], 1 - axis] += 1
                                S[k, pi[end], 1 - axis] += mag / abs(dist)

                    c_in = rgb_map[y_in, x_in] if gc is not None else None
                    c_out = rgb_map[y_out, x_out] if gc is not None else None
                    if fi[y_in, x_in] == k:
                        lim = is_ - 1 if direction > 0 else 0
                        walk(max(min(d1_out, lim), 0), min(max(d1_out, lim), is_ - 1), False, alpha[y_in, x_in], c_in)
                    if F32(fd0 - p[0][0]) * F32(fd0 - p[2][0]) < 0:
                        c2 = _cross(p[0][0], p[0][1], p[2][0], p[2][1], fd0)
                    else:
                        c2 = _cross(p[2][0], p[2][1], p[1][0], p[1][1], fd0)
                    lim = _to_int(c2 if not np.isfinite(c2) else (math.ceil(c2) if direction > 0 else math.floor(c2)), -1, is_)
                    walk(max(min(d1_in, lim), 0), min(max(d1_in, lim), is_ - 1), True, alpha[y_out, x_out], c_out)
    return grad, n, S


# ---- backward_depth_map and dL/dlight, over the pixels each record owns --------------------------------------------------------------------

def _face_inv(fv9, is_):
    """forward_face_index_map_cuda_kernel_1's inverted pixel-space triangle, float32"""
    p = (F32(0.5) * (fv9.reshape(3, 3)[:, :2] * F32(is_) + F32(is_) - F32(1))).astype(F32)
    inv = np.array([p[1, 1] - p[2, 1], p[2, 0] - p[1, 0], p[1, 0] * p[2, 1] - p[2, 0] * p[1, 1],
                    p[2, 1] - p[0, 1], p[0, 0] - p[2, 0], p[2, 0] * p[0, 1] - p[0, 0] * p[2, 1],
                    p[0, 1] - p[1, 1], p[1, 0] - p[0, 0], p[0, 0] * p[1, 1] - p[1, 0] * p[0, 1]], F32)
    den = F32(p[2, 0] * (p[0, 1] - p[1, 1]) + p[0, 0] * (p[1, 1] - p[2, 1]) + p[1, 0] * (p[2, 1] - p[0, 1]))
    return (inv / den).astype(F32)


def depth_vjp(keep, g_depth):
    """-> (grad_frec[nrec,3,3], n, S) for the cotangent of the pooled depth [is,is]"""
    fv, fi, is_ = keep["fv"], keep["face_index"], keep["is2"]
    nrec = len(fv)
    grad, n, S = np.zeros((nrec, 3, 3)), np.zeros((nrec, 3, 3), np.int64), np.zeros((nrec, 3, 3))
    if g_depth is None:
        return grad, n, S
    g = unpool(g_depth, keep, F64)
    inv = {}
    for yi, xi in zip(*np.nonzero(fi >= 0)):
        k = int(fi[yi, xi])
        f = fv[k].astype(F64)
        if k not in inv:
            m = _face_inv(fv[k], is_).astype(F64).reshape(3, 3)
            inv[k] = ((-m / f[:, 2:3]).sum(0), (np.abs(m) / np.abs(f[:, 2:3])).sum(0))
        tmp, tmp_mag = inv[k]
        d2 = F64(keep["depth"][yi, xi]) ** 2
        w = keep["weight"][yi, xi].astype(F64)
        gp = g[yi, xi]
        for c in range(3):
            term = gp * w[c] * d2 / (f[c, 2] * f[c, 2])
            grad[k, c, 2] += term; n[k, c, 2] += 1; S[k, c, 2] += abs(term)
            for l in range(2):
                grad[k, c, l] += -gp * tmp[l] * w[c] * d2 * is_ / 2
                n[k, c, l] += 1
                S[k, c, l] += abs(gp) * tmp_mag[l] * w[c] * d2 * is_ / 2
    return grad, n, S


def light_vjp(keep, g_rgb):
    """dL/dlight[nrec,3] = sum over the pixels a record owns of unlit x g -> (grad, n, S)"""
    fi = keep["face_index"]
    nrec = len(keep["fv"])
    grad, n, S = np.zeros((nrec, 3)), np.zeros((nrec, 3), np.int64), np.zeros((nrec, 3))
    g = unpool(g_rgb, keep, F64).transpose(1, 2, 0)
    for yi, xi in zip(*np.nonzero(fi >= 0)):
        k = int(fi[yi, xi])
        term = keep["unlit"][yi, xi].astype(F64) * g[yi, xi]
        grad[k] += term; n[k] += 1; S[k] += np.abs(term)
    return grad, n, S


def light_corner_jacobian(face_world, directional=0.5, color_directional=(1, 1, 1), direction=(0, 1, 0), **_):
    """M[NR,3,3,3]: d light[c] / d corner[i][j] of lighting.py:41-52 in float64 - cross product, F.normalize with max(|n|, 1e-5)
    (constant denominator below it), relu with derivative 0 at 0"""
    f = np.asarray(face_world, F64).reshape(-1, 3, 3)
    d, cd = np.asarray(direction, F64).reshape(3), np.asarray(color_directional, F64).reshape(3)
    M = np.zeros((len(f), 3, 3, 3))
    if directional == 0:
        return M
    a, b = f[:, 0] - f[:, 1], f[:, 2] - f[:, 1]
    nrm = np.cross(a, b)
    norm = np.linalg.norm(nrm, axis=1)
    length = np.maximum(norm, 1e-5)
    nh = nrm / length[:, None]
    s = nh @ d
    dn = np.broadcast_to(d, nrm.shape).copy()                          # d s / d n^
    proj = np.where((norm >= 1e-5)[:, None], nh * (nh @ d)[:, None], 0.0)
    dn = (dn - proj) / length[:, None]                                 # d s / d n
    dn = np.where((s > 0)[:, None], dn, 0.0)
    da, db = np.cross(b, dn), np.cross(dn, a)                          # d s / d a, d s / d b
    ds = np.stack([da, -(da + db), db], 1)                             # [NR, corner, xyz]
    return F64(directional) * cd[None, :, None, None] * ds[:, None, :, :]


def light_corner_magnitude(face_world, directional=0.5, color_directional=(1, 1, 1), direction=(0, 1, 0), **_):
    """what a float32 evaluation of `light_corner_jacobian` is held to, same shape: every difference replaced by the sum of its
    terms' magnitudes (d - n^ (n^ . d) cancels for a face that looks at the light), times what the cross product's own cancellation
    amplifies, |a| |b| / |n| >= 1"""
    f = np.asarray(face_world, F64).reshape(-1, 3, 3)
    d, cd = np.abs(np.asarray(direction, F64).reshape(3)), np.abs(np.asarray(color_directional, F64).reshape(3))
    a, b = f[:, 0] - f[:, 1], f[:, 2] - f[:, 1]
    norm = np.linalg.norm(np.cross(a, b), axis=1)
    length = np.maximum(norm, 1e-5)
    nh = np.abs(np.cross(a, b)) / length[:, None]
    cond = np.maximum(np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1) / length, 1.0)
    dn = (d[None, :] + nh * (nh @ d)[:, None]) / length[:, None]

    def abs_cross(u, v):
        u, v = np.abs(u), np.abs(v)
        return np.stack([u[:, 1] * v[:, 2] + u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] + u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] + u[:, 1] * v[:, 0]], 1)

    da, db = abs_cross(b, dn), abs_cross(dn, a)
    ds = np.stack([da, da + db, db], 1) * cond[:, None, None]
    return abs(F64(directional)) * cd[None, :, None, None] * ds[:, None, :, :]


# ---- projection.py:19-42, reversed ---------------------------------------------------------------------------------------------------

def projection_vjp(verts, K, R, t, orig_size, g, S=None):
    """g[NV,3]: cotangent of the projected (u, v, z) -> ((grad_verts, S_v), (grad_R, S_R), (grad_t, S_t)) in float64; S (the
    magnitudes behind g) goes through the absolute values of the same coefficients"""
    v, g = np.asarray(verts, F64).reshape(-1, 3), np.asarray(g, F64).reshape(-1, 3)
    S = np.abs(g) if S is None else np.asarray(S, F64).reshape(-1, 3)
    K, R, t, o = np.asarray(K, F64).reshape(3, 3), np.asarray(R, F64).reshape(3, 3), np.asarray(t, F64).reshape(3), F64(orig_size)
    p = v @ R.T + t
    zi = p[:, 2] + 1e-9
    A = np.zeros((len(v), 3, 3))                                       # A[:, i, j] = d out_i / d p_j
    su, sw = 2.0 / o, -2.0 / o
    A[:, 0, 0], A[:, 0, 1] = su * K[0, 0] / zi, su * K[0, 1] / zi
    A[:, 0, 2] = -su * (K[0, 0] * p[:, 0] + K[0, 1] * p[:, 1]) / zi ** 2
    A[:, 1, 0], A[:, 1, 1] = sw * K[1, 0] / zi, sw * K[1, 1] / zi
    A[:, 1, 2] = -sw * (K[1, 0] * p[:, 0] + K[1, 1] * p[:, 1]) / zi ** 2
    A[:, 2, 2] = 1.0
    dp = np.einsum("vij,vi->vj", A, g)
    S_dp = np.einsum("vij,vi->vj", np.abs(A), S)
    gv, S_v = dp @ R, S_dp @ np.abs(R)
    gR, S_R = np.einsum("vi,vj->ij", dp, v), np.einsum("vi,vj->ij", S_dp, np.abs(v))
    return (gv, S_v), (gR, S_R), (dp.sum(0), S_dp.sum(0))


# ---- the whole reverse pass ------------------------------------------------------------------------------------------------------------

def frec_grad(keep, g_rgb=None, g_depth=None, g_alpha=None):
    """-> (grad_frec[nrec,3,3], n, S): backward_pixel_map + backward_depth_map"""
    a, b = pixel_map_vjp(keep, g_rgb, g_alpha), depth_vjp(keep, g_depth)
    return a[0] + b[0], a[1] + b[1], a[2] + b[2]


def vertex_vjp(keep, g_rgb=None, g_depth=None, g_alpha=None):
    """-> dict(verts=(grad, n, S), R=(grad, n, S) | None, t=... | None, frec=(grad, n, S)).  With an ndc render `verts` is with
    respect to the vertices as given, and `parts` = its two summands, each (grad, n, S): the folded record rows and the light's
    reverse"""
    for g, nm in ((g_rgb, "rgb"), (g_depth, "depth"), (g_alpha, "alpha")):
        assert g is None or nm in keep["want"], f"a cotangent for {nm}, which the render did not produce"
    verts, rec_faces = keep["verts"], keep["rec_faces"]
    nv = len(verts)
    frec = frec_grad(keep, g_rgb, g_depth, g_alpha)
    gn, nn, Sn = np.zeros((nv, 3)), np.zeros((nv, 3), np.int64), np.zeros((nv, 3))
    gw, nw, Sw = np.zeros((nv, 3)), np.zeros((nv, 3), np.int64), np.zeros((nv, 3))
    for c in range(3):
        np.add.at(gn, rec_faces[:, c], frec[0][:, c]); np.add.at(nn, rec_faces[:, c], frec[1][:, c] + 1); np.add.at(Sn, rec_faces[:, c], frec[2][:, c])
    if keep["lit"] and g_rgb is not None and keep["light_cfg"]["directional"] != 0:
        dl, ndl, Sdl = light_vjp(keep, g_rgb)
        M = light_corner_jacobian(verts[rec_faces], **keep["light_cfg"])
        gc, Sc = np.einsum("kcij,kc->kij", M, dl), np.einsum("kcij,kc->kij", light_corner_magnitude(verts[rec_faces], **keep["light_cfg"]), Sdl)
        for c in range(3):
            np.add.at(gw, rec_faces[:, c], gc[:, c]); np.add.at(nw, rec_faces[:, c], ndl.max(1)[:, None] + 1); np.add.at(Sw, rec_faces[:, c], Sc[:, c])
    if keep["ndc"]:
        return dict(verts=(gn + gw, nn + nw, Sn + Sw), R=None, t=None, frec=frec, parts=((gn, nn, Sn), (gw, nw, Sw)))
    K, R, t, orig = keep["cam"]
    (gv, S_v), (gR, S_R), (gt, S_t) = projection_vjp(verts, K, R, t, orig, gn, Sn)
    n_v = nn.sum(1, keepdims=True) + nw
    n_all = int(nn.sum())
    return dict(verts=(gv + gw, np.broadcast_to(n_v, (nv, 3)).copy(), S_v + Sw), R=(gR, np.full((3, 3), n_all + nv), S_R), t=(gt, np.full(3, n_all + nv), S_t),
                frec=frec)


# ---- stand-ins for native.Nr* ----------------------------------------------------------------------------------------------------------

class OracleTape(NO.OracleTape):
    def __init__(self, keep, log, flags=TAPE_TEXTURES):
        super().__init__(keep, log)
        self.flags = flags

    def vertex_grad(self, grad_rgb=None, grad_depth=None, grad_alpha=None, camera=True):
        assert not self.closed and self.flags & TAPE_GEOMETRY
        out = vertex_vjp(self.keep, grad_rgb, grad_depth, grad_alpha)
        assert not (camera and self.keep["ndc"])
        return (out["verts"][0].astype(F32), out["R"][0].astype(F32) if camera else None, out["t"][0].astype(F32) if camera else None)


class OracleMesh(NO.OracleMesh):
    def set_vertices(self, verts):
        self.verts = np.array(verts, F32).reshape(self.verts.shape)
        self.log["vertex_uploads"] = self.log.get("vertex_uploads", 0) + 1


class OracleRenderer(NO.OracleRenderer):
    def render_taped(self, mesh, K=None, R=None, t=None, orig_size=1.0, fill_back=True, lightoff=False, ndc=False, want=("rgb", "depth", "alpha"),
                     flags=TAPE_GEOMETRY):
        rgb, depth, alpha, keep = render(mesh.verts, mesh.faces, mesh.textures, K, R, t, orig_size, fill_back=fill_back, lightoff=lightoff,
                                         light=self.light, ndc=ndc, want=want, **self.cfg)
        return rgb, depth, alpha, OracleTape(keep, self.log, flags)
