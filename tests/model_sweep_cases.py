"""The joint-angle sweep of tests/loss_grad_cases.py (axis R) laid out as the frames of ONE batch for the differentiable models: the
pose-state forward (pose_state_body.h's m_rodrigues: OCML sincosf, plain division) and the reverse of the chain
(model_grad_kernels.hip's vjp_rodrigues, which divides by a and a * a).  Shared by tests/test_gpu_parity.py, tests/test_gpu_smplx.py
(forward) and tests/test_gpu_smpl_autograd.py, tests/test_gpu_smplx_autograd.py (VJP); nothing here touches a GPU.

Frame f carries loss_grad_cases.sweep()[f]: its joints hold axis * angle (float32 values), every other joint a seeded N(0, 0.15)
pose, the betas N(0, 0.5).  SMPL-X adds frames with the left eye and the jaw swept - the jaw is no parameter of the fit, so only
this sweep reaches it.

Bands.  Forward, per frame and output: max(3e-6, 8 * err32), 3e-6 being the suite's band at small angles and err32 the float32 run
of the same oracle on the same frame (at large angles the reference's own float32 drifts along the chain as well).  VJP: the
autograd files' _band_check per frame and block, and for the rows of the swept joints the same expression with the ROW's own float64
maximum and the row's own float32 error - a leaf at 2e-4 rad has a gradient far below its block's maximum."""
import functools

import numpy as np
import torch

import loss_grad_cases as LC
from oracle import smplify_oracle as O

KINDS = ("smpl", "kid", "smplx")
FWD_BASE = 3e-6
SMPLX_INPUTS = ("betas", "global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose")
ROW_MARGIN = 1e-3          # degrees between -yaw and the nearest rounding boundary of the contour row (tests/test_gpu_smplx_autograd.py)


@functools.lru_cache(maxsize=None)
def frames(kind):
    """the sweep points of the batch, one per frame"""
    out = list(LC.sweep())
    if kind == "smplx":
        out += [LC.Sweep(1e-3, "general", "leye"), LC.Sweep(4.7, "-y", "leye"), LC.Sweep(1e-3, "+x", "jaw"), LC.Sweep(2e-4, "general", "jaw"),
                LC.Sweep(4.7, "general", "jaw"), LC.Sweep(2 * LC.PI + 1e-3, "+z", "jaw")]
    assert len(out) >= 16                     # a matrix-core mesh pass behind the pose state
    return tuple(out)


def model(kind):
    return LC.model(kind, "small")


@functools.lru_cache(maxsize=None)
def params(kind):
    """{input name: float32 [n, width]} in the argument names of DeviceModel.forward / vjp (SMPL, kid) or forward_smplx / vjp_smplx"""
    fr = frames(kind)
    n = len(fr)
    rng = np.random.default_rng(LC._seed("model-sweep", kind))
    nb = 11 if kind == "kid" else 10
    nj = 55 if kind == "smplx" else 24
    full = rng.normal(0, 0.15, (n, nj, 3))
    for f, s in enumerate(fr):
        for j, th in LC.sweep_thetas(kind, s).items():
            full[f, j] = th
    p = {"betas": rng.normal(0, 0.5, (n, nb)), "global_orient": full[:, 0]}
    if kind == "smplx":
        p.update(body_pose=full[:, 1:22].reshape(n, 63), jaw_pose=full[:, 22], leye_pose=full[:, 23], reye_pose=full[:, 24],
                 left_hand_pose=rng.normal(0, 0.15, (n, 6)), right_hand_pose=rng.normal(0, 0.15, (n, 6)))
    else:
        p["body_pose"] = full[:, 1:].reshape(n, 69)
    p = {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}
    for v in p.values():
        v.setflags(write=False)
    return p


def swept_rows(kind):
    """[(frame, joint index in the full pose, input name, slice into that input's row)] of every swept joint"""
    out = []
    for f, s in enumerate(frames(kind)):
        for j in LC.sweep_thetas(kind, s):
            if j == 0:
                out.append((f, j, "global_orient", slice(0, 3)))
            elif kind == "smplx" and j >= 22:
                out.append((f, j, {22: "jaw_pose", 23: "leye_pose"}[j], slice(0, 3)))
            else:
                out.append((f, j, "body_pose", slice(3 * (j - 1), 3 * j)))
    return out


def _forward(kind, dtype, grad=False):
    m = O.to_torch_model(model(kind), dtype)
    p = params(kind)
    if kind == "smplx":
        x = {k: torch.tensor(p[k], dtype=dtype, requires_grad=grad) for k in SMPLX_INPUTS}
        args = (x["betas"], x["global_orient"], x["body_pose"], x["leye_pose"], x["reye_pose"], x["left_hand_pose"], x["right_hand_pose"])
        out = O.smplx_forward(m, *args, jaw_pose=x["jaw_pose"], mapped=False)
        mapped = O.smplx_forward(m, *args, jaw_pose=x["jaw_pose"], mapped=True)
        return x, {"vertices": out["vertices"], "joints": mapped["joints"], "joints_all": out["joints"], "full_pose": out["full_pose"],
                   "dyn_row": out["dyn_row"]}
    x = {k: torch.tensor(p[k], dtype=dtype, requires_grad=grad) for k in ("betas", "global_orient", "body_pose")}
    out = O.smpl_forward(m, x["betas"], x["global_orient"], x["body_pose"])
    return x, {k: out[k] for k in ("vertices", "joints", "joints_ori")}


@functools.lru_cache(maxsize=None)
def forward_oracle(kind):
    """-> ({output: float64 [n, ...]}, {output: float32 run as float64}); SMPL-X: every frame's contour row is clear of a rounding
    boundary and the same in both, checked here"""
    with torch.no_grad():
        _, o64 = _forward(kind, torch.float64)
        _, o32 = _forward(kind, torch.float32)
    if kind == "smplx":
        m64 = O.to_torch_model(model(kind), torch.float64)
        n = len(frames(kind))
        R = O.batch_rodrigues(o64["full_pose"].reshape(-1, 3)).view(n, -1, 3, 3)
        rel = torch.eye(3, dtype=torch.float64).unsqueeze(0).expand(n, -1, -1)
        for j in m64["neck_kin_chain"]:
            rel = torch.bmm(R[:, int(j)], rel)
        deg = (-torch.atan2(-rel[:, 2, 0], torch.sqrt(rel[:, 0, 0] ** 2 + rel[:, 1, 0] ** 2)) * 180.0 / np.pi).numpy()
        margin = np.abs(deg - np.floor(deg) - 0.5)
        assert (margin >= ROW_MARGIN).all(), ("a frame sits on a rounding boundary of the contour row", int(margin.argmin()), margin.min())
        assert np.array_equal(o64["dyn_row"].numpy(), o32["dyn_row"].numpy())
    as64 = lambda o: {k: v.numpy().astype(np.int64 if k == "dyn_row" else np.float64) for k, v in o.items()}          # noqa: E731
    return as64(o64), as64(o32)


RESULTS = []               # (kind, what, frame, output / block, err, err32 or ref_err, band) of every comparison, for the report


def check_forward(kind, got, first=0, what="forward"):
    """got: {output: [k, ...]} of the frames first .. first + k - 1; every frame and output within max(3e-6, 8 * err32) of float64"""
    o64, o32 = forward_oracle(kind)
    failures = []
    for name, g in got.items():
        for i in range(len(g)):
            f = first + i
            err = float(np.abs(np.asarray(g[i], np.float64) - o64[name][f]).max())
            err32 = float(np.abs(o32[name][f] - o64[name][f]).max())
            band = max(FWD_BASE, 8.0 * err32)
            RESULTS.append((kind, what, f, name, err, err32, band))
            if not err <= band:
                failures.append(f"frame {f} ({frames(kind)[f].name}) {name}: err {err:.3e}, err32 {err32:.3e}, band {band:.3e}")
    assert not failures, f"{kind} {what}\n  " + "\n  ".join(failures)


def check_vjp(kind, case, inputs, got, g32, g64):
    """got / g32 / g64: one array per input of `inputs`, [n, width].  Per frame and block: 4 * ref_err + 1e-6 * max|f64| (the autograd
    files' _band_check); per swept joint's row the same with the row's own maximum and the row's own float32 error."""
    failures = []

    def one(what, f, name, a, b32, b64):
        err = float(np.abs(a.astype(np.float64) - b64).max())
        ref_err = float(np.abs(b32 - b64).max())
        band = 4 * ref_err + 1e-6 * float(np.abs(b64).max())
        RESULTS.append((kind, f"vjp {case} {what}", f, name, err, ref_err, band))
        if not err <= band:
            failures.append(f"{what} frame {f} ({frames(kind)[f].name}) d{name}: err {err:.3e}, ref_err {ref_err:.3e}, band {band:.3e}, "
                            f"max|f64| {np.abs(b64).max():.3e}")

    for i, name in enumerate(inputs):
        assert got[i].dtype == np.float32 and got[i].shape == g64[i].shape, name
        for f in range(len(frames(kind))):
            one("block", f, name, got[i][f], g32[i][f], g64[i][f])
    for f, j, name, sl in swept_rows(kind):
        i = inputs.index(name)
        one("row", f, f"{name}[joint {j}]", got[i][f, sl], g32[i][f, sl], g64[i][f, sl])
    assert not failures, f"{kind} vjp {case}\n  " + "\n  ".join(failures)


def report(kind):
    """per angle group: the worst err / band and err / err32 of the forward, the VJP's blocks and the VJP's rows"""
    print(f"\n{kind}: what | angle group | comparisons | worst frame : output | err | err32 | band | err / band | worst err / err32")
    fr = frames(kind)
    for what in sorted({r[1] for r in RESULTS if r[0] == kind}):
        for g in ("near zero", "rounding edges of n", "centres and wrap", "far"):
            rows = [r for r in RESULTS if r[0] == kind and r[1] == what and fr[r[2]].group == g]
            if not rows:
                continue
            w = max(rows, key=lambda r: r[4] / r[6] if r[6] > 0 else 0.0)
            ratio = max((r[4] / r[5] for r in rows if r[5] > 0), default=float("nan"))
            print(f"{what} | {g} | {len(rows)} | {fr[w[2]].name} : {w[3]} | {w[4]:.2e} | {w[5]:.2e} | {w[6]:.2e} | "
                  f"{w[4] / w[6] if w[6] > 0 else 0.0:.3f} | {ratio:.1f}")
