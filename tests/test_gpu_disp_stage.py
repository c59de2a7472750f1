"""The fused SMPL+D stage (bf_fit_displacement: the five kernels of csrc/disp_kernels.hip) where body templates do not take it - the
cases of tests/disp_stage_cases.py (tests/test_disp_stage_cases.py shows each on the CPU to be what it claims and well posed):

  a. the stage's gradient at step 1 and at step 4, read out of Adam's first moments, per case and per frame of a two-frame batch whose
     scans differ in height (one three-frame batch on hub17), held to float64 autograd of the oracle's objective: the whole [NV,3]
     block, and the hub's row, its rim's rows and the lonely vertex's row on their own
  b. Adam step by step, k = 1..4, with default hypers and with every hyper changed: the second moment, the first moment and the step,
     each re-evaluated in float64 from the float32 values read back, in bands derived from the count of float32 roundings; two runs
     agree bit for bit
  c. zero distance: every vertex exactly on its closest point - finite results and the oracle's gradient (torch's rule for the norm
     at zero: a zero gradient)
  d. the worst position inside a band

Bands: DESIGN.md 2.3's block rule max(5e-6 M, 8 err32) (scan_loss_cases.Band) plus the read-out's own rounding; nothing is
calibrated on what the kernels return.  Run with -s: every check prints its position inside its band."""
import numpy as np
import pytest

import dense_grad_cases as DC
import disp_stage_cases as D
import scan_loss_cases as SC
from bodyfitting_amd import native as N

pytestmark = pytest.mark.gpu
BAND = SC.Band()
TIES = {}                        # (case, frame, step) -> share of vertices whose closest face was taken from the device
U = D.U
DEFAULT = {"lr_displacement": 0.05, "adam_beta1": 0.9, "adam_beta2": 0.999, "adam_eps": 1e-8}
CHANGED = {"lr_displacement": 0.02, "adam_beta1": 0.8, "adam_beta2": 0.99, "adam_eps": 1e-3}      # every one moved; eps visible
STEPS = (1, 2, 3, 4)


@pytest.fixture(scope="module")
def devs():
    made = {}

    def get(case):
        if case not in made:
            made[case] = N.DeviceModel(D.model(case), DC.LC.gmm(), device=0)
        return made[case]
    yield get
    for m in made.values():
        m.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _batch(dev, problems):
    c2w, K, kp, ndiv, betas, pose = N.pack_problem(problems)
    b = N.FrameBatch(dev, len(problems), c2w.shape[1])
    b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose)
    return b


_RUNS = {}


def _run(dev, case, items, hypers=None):
    """fit(30), then bf_fit_displacement(k) for k = 1..4 from fresh calls (the stage restarts from zero on each) -> dict(base, and per k:
    disp, m, v; ids: the device's closest faces at base and at base + disp_3; again: a second fit_displacement(4)'s disp, m, v)"""
    key = (case, items, None if hypers is None else tuple(sorted(hypers.items())))
    if key in _RUNS:
        return _RUNS[key]
    scans = [N.Scan(*D.scan(f, sc)[1:]) for f, sc in items]
    b = _batch(dev, [D.scan(f, sc)[0] for f, sc in items])
    hp = None if hypers is None else N.make_hyper(**hypers)
    out = {"disp": {}, "m": {}, "v": {}}
    try:
        b.set_scans(scans)
        b.fit(30)
        out["base"] = b.get_result()[0].copy()
        for k in STEPS:
            b.fit_displacement(k, hp)
            out["disp"][k], out["m"][k], out["v"][k] = b.get_displacement().copy(), b.disp_moment().copy(), b.disp_moment2().copy()
        b.fit_displacement(STEPS[-1], hp)
        out["again"] = (b.get_displacement().copy(), b.disp_moment().copy(), b.disp_moment2().copy())
        out["ids"] = {1: [scans[i].nearest_points(out["base"][i])[1] for i in range(len(scans))],
                      4: [scans[i].nearest_points(out["base"][i] + out["disp"][3][i])[1] for i in range(len(scans))]}
    finally:
        b.close()
        for s in scans:
            s.close()
    _RUNS[key] = out
    return out


# ---- a. the gradient at step 1 and at step 4 -----------------------------------------------------------------------------------

GRADIENT_CASES = [(c, D.FRAMES) for c in D.CASES] + [(D.THREE_FRAME_CASE, D.FRAMES + (D.THIRD_FRAME,))]


@pytest.mark.parametrize("case,items", GRADIENT_CASES, ids=[f"{c}-F{len(i)}" for c, i in GRADIENT_CASES])
def test_gradient_at_step_1_and_step_4(devs, case, items):
    """g_1 = m_1 / (1 - beta1) at zero displacement and g_4 = m_3 + (m_4 - m_3) / (1 - beta1) at base + the device's displacement after
    three steps, every frame, against float64 autograd at those float32 vertices; closest points and faces from the reference's
    search there (ties settled as disp_stage_cases.settle_ties does).  The block, then the marked rows on their own."""
    r = _run(devs(case), case, items)
    topo = D.topology(case)
    assert np.abs(r["disp"][3]).max() > 0.01                                 # three steps of 5 cm: well away from zero
    failures = []
    for i, (f, sc) in enumerate(items):
        _, sv, sf = D.scan(f, sc)
        for step in (1, 4):
            m_prev = None if step == 1 else r["m"][3][i]
            m_now = r["m"][step][i]
            disp = np.zeros_like(r["base"][i]) if step == 1 else r["disp"][3][i]
            got = D.gradient_from_moments(m_prev, m_now)
            ref = D.reference(topo["faces"], sv, sf, r["base"][i], disp, r["ids"][step][i])
            TIES[(case, len(items), i, step)] = ref["share"]
            what = f"{case} F={len(items)} frame {i} step {step}"
            checks = [("block", None)] + ([] if case == D.REPEATED_CORNER else [(name + " row" + "s" * (len(rows) > 1), rows)
                                                                               for name, rows in topo["marked"].items()])
            for name, rows in checks:
                mp, mn = (None if m_prev is None else m_prev[rows], m_now[rows]) if rows is not None else (m_prev, m_now)
                try:
                    D.hold(BAND, f"{what} {name}", got, ref["g64"], ref["g32"], D.readout_rounding(mp, mn), rows=rows)
                except AssertionError as e:
                    worst = "" if rows is None else f" (vertices {np.asarray(rows).tolist()})"
                    failures.append(f"{what} {name}{worst}: {e}")
            M, err32 = float(np.abs(ref["g64"]).max()), float(np.abs(ref["g32"] - ref["g64"]).max())
            print(f"    {what}: M {M:.3e}, err32 {err32 / M:.2e} M; closest faces taken from the device at {ref['share']:.4f} of the vertices")
    assert not failures, "\n  ".join(failures)


# ---- b. Adam, step by step -------------------------------------------------------------------------------------------------------

def _host_constants(h, k):
    """step_size and bc2_sqrt as csrc/disp_api.hip forms them: a double expression of the float32 hypers, cast to float"""
    b1, b2, lr = (float(np.float32(h[n])) for n in ("adam_beta1", "adam_beta2", "lr_displacement"))
    return float(np.float32(lr / (1.0 - b1 ** k))), float(np.float32(np.sqrt(1.0 - b2 ** k)))


def _worst(ratio):
    """' (frame, vertex, coordinate)' of the largest entry, for the message"""
    return " at " + str(tuple(int(i) for i in np.unravel_index(np.argmax(ratio), ratio.shape)))


@pytest.mark.parametrize("hypers", [DEFAULT, CHANGED], ids=["default", "changed"])
@pytest.mark.parametrize("case", ["body", "hub17"])
def test_adam_step_by_step(devs, case, hypers):
    """disp_k, m_k, v_k for k = 1..4 from fresh calls; every relation of the kernel's Adam (csrc/disp_kernels.hip, bf_disp_adam_kernel)
    re-evaluated in float64 from the float32 values read back, element by element:
        m_k = m_{k-1} + (g_k - m_{k-1}) (1 - beta1)
        v_k = v_{k-1} beta2 + (1 - beta2) g_k g_k
        disp_k = disp_{k-1} - step_size (m_k / (sqrt(v_k) / bc2_sqrt + eps))
    u = 2^-24.  The build contracts a * b + c where the source writes it, which only removes roundings from the counts below."""
    r = _run(devs(case), case, D.FRAMES, None if hypers is DEFAULT else hypers)
    if hypers is DEFAULT:
        plain = _run(devs(case), case, D.FRAMES, DEFAULT)                      # the defaults given explicitly: the same bits as NULL
        for k in STEPS:
            for key in ("disp", "m", "v"):
                np.testing.assert_array_equal(_bits(plain[key][k]), _bits(r[key][k]), err_msg=f"{key}_{k}")
    for key, a in zip(("disp", "m", "v"), r["again"]):
        np.testing.assert_array_equal(_bits(a), _bits(r[key][STEPS[-1]]), err_msg=f"{key}: two runs of the same call differ")
    w1, w2 = D.one_minus(hypers["adam_beta1"]), D.one_minus(hypers["adam_beta2"])
    beta2, eps = float(np.float32(hypers["adam_beta2"])), float(np.float32(hypers["adam_eps"]))
    tiny = 4 * 2.0 ** -126                                                      # (a result below the normal range may be flushed)
    zero = np.zeros_like(r["m"][1], dtype=np.float64)
    for k in STEPS:
        what = f"Adam {case} {'default' if hypers is DEFAULT else 'changed'} step {k}"
        m0, v0, d0 = (zero if k == 1 else r[key][k - 1].astype(np.float64) for key in ("m", "v", "disp"))
        m1, v1, d1 = (r[key][k].astype(np.float64) for key in ("m", "v", "disp"))
        assert all(np.isfinite(a).all() for a in (m1, v1, d1)) and (v1 >= 0).all(), what
        # the gradient the kernel held, from the first moments.  m_k = fl(m0 + fl(fl(g - m0) w1)): the two inner roundings are each
        # u |g - m0| of g, the outer one u |m_k| / w1
        g = m0 + (m1 - m0) / w1
        dg = U * (2 * np.abs(g - m0) + np.abs(m1) / w1)
        # second moment: 4 float32 roundings - v0 beta2, (w2 g), (w2 g) g, the sum - each relative to a partial sum of positive
        # terms <= v_k: <= 3 u v_k to first order, 4 allowed; plus the read-out's rounding propagated, w2 (2 |g| dg + dg^2)
        want = v0 * beta2 + w2 * g * g
        allowed = w2 * (2 * np.abs(g) * dg + dg * dg) + 4 * U * np.maximum(v1, want) + tiny
        BAND._row(f"{what} second moment{_worst(np.abs(v1 - want) / allowed)}", float((np.abs(v1 - want) / allowed).max()), 1.0)
        # first moment, with |g| from the second moments (independent of the first): g^2 = (v_k - beta2 v0) / w2 inside
        # 4 u v_k / w2 (the same four roundings), |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(a), sqrt|a - b|); the sign from the
        # first moments.  Then 3 roundings: g - m0 and its product with w1 (u w1 |g - m0| each), the sum (u |m_k|); 2 u allowed for each
        x = (v1 - beta2 * v0) / w2
        dx = (4 * U * v1 + tiny) / w2
        gv = np.sqrt(np.maximum(x, 0.0))
        dgv = np.minimum(np.sqrt(dx + np.maximum(-x, 0.0)), dx / np.maximum(gv, 1e-300))
        gs = np.sign(g) * gv
        want = m0 + (gs - m0) * w1
        allowed = w1 * dgv + 2 * U * (w1 * (gv + np.abs(m0)) + np.abs(m1)) + tiny
        allowed += 2 * w1 * np.where(np.abs(g) <= dg, gv, 0.0)                  # (where the read-out cannot tell g's sign)
        BAND._row(f"{what} first moment{_worst(np.abs(m1 - want) / allowed)}", float((np.abs(m1 - want) / allowed).max()), 1.0)
        # the step: 5 float32 roundings relative to the step - sqrt, / bc2_sqrt, + eps, m / (.), step_size * (.) - 8 allowed, and the
        # subtraction's, one ulp (2^-23) of disp_k
        step_size, bc2 = _host_constants(hypers, k)
        want = -step_size * (m1 / (np.sqrt(v1) / bc2 + eps))
        allowed = 8 * U * np.abs(want) + 2.0 ** -23 * np.abs(d1) + tiny
        at = np.abs((d1 - d0) - want) / allowed
        BAND._row(f"{what} step{_worst(at)}", float(at.max()), 1.0)
    if hypers is CHANGED:                                                        # ... and the changed hypers are not ignored
        plain = _run(devs(case), case, D.FRAMES, None)
        assert np.abs(r["disp"][1]).max() < 0.021 < 0.049 < np.abs(plain["disp"][1]).max()


# ---- c. zero distance ---------------------------------------------------------------------------------------------------------------

def test_zero_distance_gives_finite_results_and_the_oracles_gradient(devs):
    """Every vertex exactly on its closest point: scans built from a fit's own float32 result vertices (bf_batch_set_scans keeps the
    result).  |P - C|_F = 0, and torch's rule for the norm at zero is a zero gradient (as bf_ml_pc_grad_kernel keeps it): the
    displacement and both moments are finite, and the step-1 gradient is the oracle's, which is the normal terms' alone.  Every
    vertex sits on a scan corner, so every closest face is tied by construction: the oracle takes the device's face wherever the
    reference's rule gives it the reference's own distance bit for bit, without the cap on how many."""
    case = "body"
    dev = devs(case)
    faces = D.topology(case)["faces"]
    b = _batch(dev, [D.scan(f, sc)[0] for f, sc in D.FRAMES])
    scans = []
    try:
        b.fit(30)
        V = b.get_result()[0].copy()
        assert V.dtype == np.float32
        scans = [N.Scan(V[i], faces) for i in range(len(V))]
        ids_dev = []
        for i, s in enumerate(scans):                                           # the precondition, on the device
            pts, ids, _ = s.nearest_points(V[i])
            off = np.nonzero((_bits(pts) != _bits(V[i])).any(1))[0]
            assert not len(off), f"frame {i}: {len(off)} vertices are not their own closest point, e.g. {off[:5].tolist()}: {pts[off[:5]]} for {V[i][off[:5]]}"
            ids_dev.append(ids)
        b.set_scans(scans)
        b.fit_displacement(1)
        d1, m1, v1 = b.get_displacement().copy(), b.disp_moment().copy(), b.disp_moment2().copy()
    finally:
        b.close()
        for s in scans:
            s.close()
    nan = {k: int((~np.isfinite(a)).sum()) for k, a in (("disp", d1), ("m", m1), ("v", v1))}
    assert not any(nan.values()), f"not finite at zero distance: {nan} of {d1.size} entries"
    for i in range(len(V)):
        ref = D.reference(faces, V[i], faces, V[i], np.zeros_like(V[i]), ids_dev[i], cap=None)
        np.testing.assert_array_equal(_bits(ref["closest"]), _bits(V[i]))      # (the reference's search agrees: zero distance)
        print(f"    zero distance frame {i}: closest faces taken from the device at {ref['share']:.4f} of the vertices")
        D.hold(BAND, f"zero distance frame {i} block", D.gradient_from_moments(None, m1[i]), ref["g64"], ref["g32"],
               D.readout_rounding(None, m1[i]))


# ---- d. the worst position -------------------------------------------------------------------------------------------------------------

def test_zz_the_worst_position_inside_a_band():
    worst = BAND.worst()
    assert worst is not None
    print(f"    {len(BAND.rows)} checks; the worst: {worst[0]}: error {worst[1]:.3e} of {worst[2]:.3e} allowed = {worst[3]:.3f} of the band")
    per_case = {}
    for what, err, allowed, at in BAND.rows:
        key = what.split(" F=")[0] if " F=" in what else " ".join(what.split()[:2])
        if key not in per_case or at > per_case[key][1]:
            per_case[key] = (what, at)
    for key, (what, at) in per_case.items():
        print(f"      {key}: worst {at:.3f} ({what})")
    if TIES:
        k = max(TIES, key=TIES.get)
        print(f"    closest faces taken from the device: at most {TIES[k]:.4f} of the vertices ({k}); cap {D.TIE_CAP}")
    assert worst[3] <= 1.0
