"""The gradient bf_fit descends in its dense iterations - keypoints + 5 x silhouette + 5 * imsize / scan_height x closest-point, through
the whole mesh back to the parameters - read with bf_dense_iter_grad and held to float64 torch autograd of
oracle.smplify_oracle.dense_loss_and_grad at the cases of tests/dense_grad_cases.py (tests/test_dense_grad_cases.py proves on the CPU
that every one is well posed, so nothing is skipped or filtered here).

  a. the reverse mesh pass alone: a seeded cotangent on every vertex (dverts_extra), each frame with its own parameters and cotangent,
     at batch sizes on both sides of every frames-per-workgroup instance of bf_mesh_bwd_multi_kernel; SMPL, kid, 8-wide and dense
     skinning rows, SMPL-X
  b. the same on the sub-models bf_fit runs its mesh passes on (one frame: the split tiles)
  c. the scan term, two frames with scans of different height; and at zero distance, every vertex on its closest point
  d. the silhouette term under both folds, with and without the sub-model, and together with a scan
  e. the call leaves the batch as it found it, and refuses what it cannot evaluate
  f. the fused SMPL+D stage's gradient away from zero displacement, read out of its first Adam moment

Bands (loss_grad_cases.band / term_band, nothing calibrated on the kernels): per parameter block max(5e-6 M, 8 err32) with M = max|g64|
and err32 the error of torch's float32 autograd of the same oracle; per term relative max(3e-6, 8 rel32).  Run with -s: every check
prints its position inside its band and test_report the worst one.
"""
import warnings

import numpy as np
import pytest
import torch

from bodyfitting_amd import _lib
from bodyfitting_amd import native as N
import dense_grad_cases as DC
from oracle import smplify_oracle as O

pytestmark = pytest.mark.gpu
RESULTS = []                # (check, block or term, err / band)


@pytest.fixture(scope="module")
def devs(dev_model):
    made = {"smpl6890": dev_model}

    def get(name):
        if name not in made:
            made[name] = N.DeviceModel(DC.model(name), DC.LC.gmm(), device=0)
        return made[name]
    yield get
    for key, m in made.items():
        if key != "smpl6890":
            m.close()


def _batch(dev, problems, params):
    c2w, K, kp, ndiv, betas, pose = N.pack_problem(problems)
    b = N.FrameBatch(dev, len(problems), c2w.shape[1])
    b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose)
    if params is not None:
        b.set_params(np.stack([N.pack_params(p) for p in params]))
    return b


def _hyper(prob, **kw):
    return N.make_hyper(**DC.hyper_keywords(prob, **kw))


def _hold(what, name, dev, terms, grads, ref64, ref32):
    """one frame's six terms and parameter blocks against the float64 oracle, inside the bands; -> list of failures"""
    t64, g64 = ref64[:2]
    t32, g32 = ref32[:2]
    failures, worst = [], 0.0
    for i, k in enumerate(O.DENSE_TERMS):
        if t64[k] == 0.0:
            if float(terms[i]) != 0.0:
                failures.append(f"term {k}: {float(terms[i])!r}, expected 0")
            continue
        rel, tb = abs(float(terms[i]) - t64[k]) / abs(t64[k]), DC.term_band(t64[k], t32[k])
        RESULTS.append((what, k, rel / tb))
        worst = max(worst, rel / tb)
        if not rel <= tb:
            failures.append(f"term {k}: {float(terms[i])!r} vs {t64[k]!r} (relative {rel:.2e}, band {tb:.2e})")
    got = N.split_params(grads, dev.n_joints, dev.n_betas)
    for k in DC.blocks(name):
        assert got[k].shape == g64[k].shape, k
        band, M, err32 = DC.band(g64[k], g32[k])
        err = float(np.abs(got[k].astype(np.float64) - g64[k]).max())
        RESULTS.append((what, k, err / band))
        worst = max(worst, err / band if np.isfinite(err) else np.inf)
        if not err <= band:                                   # (also catches a NaN)
            failures.append(f"{k}: err {err:.3e} = {err / M:.2e} M, band {band:.3e} = {band / M:.2e} M, err32 {err32:.3e}, err / band {err / band:.2f}")
    print(f"{what}: worst position inside its band {worst:.3f}")
    return [f"{what} {f}" for f in failures]


def _reverse(dev, name, frames, which=None, sub_model=False):
    """bf_dense_iter_grad with the cases' cotangents on a batch of the given frames -> (terms, grads)"""
    probs = [DC.problem(name, f) for f in frames]
    b = _batch(dev, probs, [DC.params(name, f) for f in frames])
    try:
        cot = np.stack([DC.cotangent(name, f, which) for f in frames]).astype(np.float32)
        return b.dense_iter_grad(_hyper(probs[0]), sub_model=sub_model, dverts_extra=cot)
    finally:
        b.close()


def _reverse_refs(name, f, which=None):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        r = DC.reverse_reference(name, f, which)
    return (r["terms64"], r["grads64"]), (r["terms32"], r["grads32"])


# ---- a. the reverse pass alone ---------------------------------------------------------------------------------------------

REVERSE = [(name, F) for name, Fs in DC.REVERSE_F.items() for F in Fs]


@pytest.mark.parametrize("name,F", REVERSE, ids=[f"{n}-F{F}" for n, F in REVERSE])
def test_reverse_pass_matches_fp64_autograd(devs, name, F):
    """keypoints + sum(cot * body_vertices): every frame of the batch, every block, against float64 autograd"""
    dev = devs(name)
    frames = DC.frames(name, F)
    terms, grads = _reverse(dev, name, frames)
    failures = []
    for i, f in enumerate(frames):
        failures += _hold(f"a {name} F={F} frame {i}", name, dev, terms[i], grads[i], *_reverse_refs(name, f))
    assert not failures, "\n  ".join(failures)


@pytest.mark.parametrize("F", [5, 9])
@pytest.mark.parametrize("name", ["smpl690", "smplx1200"])
def test_a_frame_of_a_batch_equals_its_single_frame_evaluation(devs, name, F):
    """bit for bit: the sums of the reverse pass do not depend on the frames-per-workgroup instance or the frame's place in it"""
    dev = devs(name)
    frames = DC.frames(name, F)
    terms, grads = _reverse(dev, name, frames)
    for i in (0, F // 2, F - 1):
        t1, g1 = _reverse(dev, name, frames[i:i + 1])
        np.testing.assert_array_equal(g1[0], grads[i], err_msg=f"frame {i}")
        np.testing.assert_array_equal(t1[0], terms[i], err_msg=f"frame {i}")


ZERO_MODELS = ["smpl690", "kid690", "nv690_BD", "smplx1200"]      # the sized and the table-driven fit instance, dense rows, SMPL-X


def _point_batch(dev, name, n=3):
    frames = DC.frames(name, n)
    probs = [DC.problem(name, f) for f in frames]
    cot = np.stack([DC.cotangent(name, f) for f in frames]).astype(np.float32)
    return _batch(dev, probs, [DC.params(name, f) for f in frames]), _hyper(probs[0]), cot


@pytest.mark.parametrize("name", ZERO_MODELS)
def test_second_call_and_no_cotangent(devs, name):
    """a second call gives equal bits; without "late" and without a cotangent the gradient is bf_loss_grad's bit for bit and terms 4
    and 5 are zero, with and without the sub-model flag"""
    b, hp, cot = _point_batch(devs(name), name)
    try:
        t1, g1 = b.dense_iter_grad(hp, dverts_extra=cot)
        t2, g2 = b.dense_iter_grad(hp, dverts_extra=cot)
        np.testing.assert_array_equal(g1, g2)
        np.testing.assert_array_equal(t1, t2)
        t0, g0 = b.loss_grad(hp)
        for sub in (False, True):
            tn, gn = b.dense_iter_grad(hp, sub_model=sub)
            assert not tn[:, 4:].any()
            if sub and DC.kind(name) == "smplx":               # (SMPL-X on its keypoint-only sub-model: other sums, held by part b)
                np.testing.assert_allclose(tn[:, :4], t0, rtol=1e-5)
                continue
            np.testing.assert_array_equal(tn[:, :4], t0)
            np.testing.assert_array_equal(gn, g0)
        assert np.abs(g1 - g0).max() > 1e-3 * np.abs(g0).max()          # ... and the cotangent is not ignored
    finally:
        b.close()


@pytest.mark.parametrize("name", ZERO_MODELS)
def test_zero_cotangent_gives_loss_grad_bits(devs, name):
    """A cotangent of zeros goes through the mesh passes and the fit kernel's instance with outside gradient blocks, and gives
    bf_loss_grad's bits: the instances of the fit kernel with and without outside blocks sum every parameter's gradient in one order.
    (smpl690 found that the sized SMPL instances did not: the plain one dealt the sums of dL/dbetas to 16 lanes per beta on waves 1-3,
    BETA_DEAL of csrc/fit_kernels.hip, the one with outside blocks summed them 6 lanes per beta on wave 3, and 7 of 10 betas per frame
    differed by up to 4.7e-7 relative.  Both take the deal now.)"""
    b, hp, cot = _point_batch(devs(name), name)
    try:
        t0, g0 = b.loss_grad(hp)
        tz, gz = b.dense_iter_grad(hp, dverts_extra=np.zeros_like(cot))
        assert not tz[:, 4:].any()
        np.testing.assert_array_equal(tz[:, :4], t0)
        differ = np.argwhere(gz != g0)
        if len(differ):
            rel = np.abs(gz - g0)[gz != g0] / np.abs(g0)[gz != g0]
            print(f"{name}: {len(differ)} of {g0.size} components differ, parameter indices {sorted(set(differ[:, 1].tolist()))}, max relative {rel.max():.2e}")
        np.testing.assert_array_equal(gz, g0)
    finally:
        b.close()


# ---- b. the sub-models -----------------------------------------------------------------------------------------------------

SUBS = [(name, w, F) for name in DC.MODELS for w in DC.sub_models(name) for F in DC.SUB_F]


@pytest.mark.parametrize("name,which,F", SUBS, ids=[f"{n}-{'kp' if w else 'sampled'}-F{F}" for n, w, F in SUBS])
def test_reverse_pass_on_the_sub_models(devs, name, which, F, monkeypatch):
    """the mesh passes on the sub-model bf_fit would choose, a cotangent that is zero off its vertices, the full model's float64 truth.
    SMPL-X's iterations before the switch-on run on the keypoint-only sub-model; BF_DENSE_SUBMODEL_KP=0 (the library's bring-up
    switch, read on every call) puts them on the sampled-first one, as bf_fit's later iterations are"""
    dev = devs(name)
    np.testing.assert_array_equal(dev.sub_vertices(which), DC.sub_vertices(name, which))
    if DC.kind(name) == "smplx" and which == DC.SUB_SAMPLED:
        monkeypatch.setenv("BF_DENSE_SUBMODEL_KP", "0")
    frames = DC.frames(name, F)
    terms, grads = _reverse(dev, name, frames, which, sub_model=True)
    failures = []
    for i, f in enumerate(frames):
        failures += _hold(f"b {name} sub {which} F={F} frame {i}", name, dev, terms[i], grads[i], *_reverse_refs(name, f, which))
    assert not failures, "\n  ".join(failures)
    # the same cotangent on the full model: the same truth, other sums
    t_full, g_full = _reverse(dev, name, frames, which, sub_model=False)
    for i, f in enumerate(frames):
        failures += _hold(f"b {name} sub {which} cotangent on the full model F={F} frame {i}", name, dev, t_full[i], g_full[i],
                          *_reverse_refs(name, f, which))
    assert not failures, "\n  ".join(failures)


# ---- c. scan term ----------------------------------------------------------------------------------------------------------

def _scan_batch(dev, name, items, at_point=True):
    probs = [DC.scan_problem(name, f, sc)[0] for f, sc in items]
    scans = [N.Scan(*DC.scan_problem(name, f, sc)[1:]) for f, sc in items]
    b = _batch(dev, probs, [DC.scan_params(name, f, sc) for f, sc in items] if at_point else None)
    b.set_scans(scans)
    return b, scans, _hyper(probs[0])


@pytest.mark.parametrize("F", [1, 2])
@pytest.mark.parametrize("name", DC.SCAN_MODELS)
def test_scan_term_matches_fp64_autograd(devs, name, F):
    """"late" on, scans attached (F = 2: of different height, so the per-frame constant scale and weight are both exercised): terms[5]
    and every block, without and with a cotangent.  The closest points are the reference's search (in its own float32 arithmetic) at
    the device's own float32 vertices, constant on the oracle's side as the reference detaches them"""
    dev = devs(name)
    items = DC.SCAN_FRAMES[:F]
    b, scans, hp = _scan_batch(dev, name, items)
    failures = []
    try:
        for with_cot in (False, True):
            cots = [DC.scan_cotangent(name, f, sc) if with_cot else None for f, sc in items]
            extra = np.stack(cots).astype(np.float32) if with_cot else None
            terms, grads = b.dense_iter_grad(hp, late=True, dverts_extra=extra)
            verts = b.debug_vertices()
            assert (terms[:, 5] > 0).all() and not terms[:, 4].any()
            for i, (f, sc) in enumerate(items):
                _, sv, sf = DC.scan_problem(name, f, sc)
                _, closest = DC.closest_points(sv, sf, verts[i])
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", UserWarning)
                    r64 = DC.scan_evaluate(name, f, sc, closest, cots[i])
                    r32 = DC.scan_evaluate(name, f, sc, closest, cots[i], dtype=torch.float32)
                np.testing.assert_allclose(verts[i], r64[2], rtol=0, atol=5e-6 * max(1.0, np.abs(r64[2]).max()))
                failures += _hold(f"c {name} F={F} frame {i}{' + cotangent' if with_cot else ''}", name, dev, terms[i], grads[i], r64, r32)
    finally:
        b.close()
        for s in scans:
            s.close()
    assert not failures, "\n  ".join(failures)


def test_scan_term_at_zero_distance(devs):
    """Every vertex exactly on its closest point: scans built from the batch's own float32 vertices at the parameter point.  The
    Frobenius norm is zero there and torch's rule for its gradient is zero (as bf_ml_pc_grad_kernel keeps it): terms[5] == 0, and the
    gradient is finite and the oracle's - DC.scan_evaluate's objective with closest = vertices - inside the band of every block.
    With a scan attached the constant scale is the scan's, height / 1.7, and the vertices carry it as a factor; so that attaching the
    scans leaves the vertices where they were, each scan gets two more vertices, in no face, that make its height h with
    float32(h / 1.7f) the constant scale c0 the vertices were formed with (the point's scale is 0.85 of the case's: the body fits inside)"""
    name = "smpl690"
    dev = devs(name)
    model = DC.model(name)
    items = DC.SCAN_FRAMES
    probs = [DC.scan_problem(name, f, sc)[0] for f, sc in items]
    params = [DC.scan_params(name, f, sc) for f, sc in items]
    for p in params:
        p["scale"] = p["scale"] * 0.85
    h = np.float32(probs[0]["constant_scale"]) * np.float32(1.7)
    c0 = h / np.float32(1.7)
    assert h.dtype == c0.dtype == np.float32
    b = _batch(dev, probs, params)
    hp = _hyper(probs[0], constant_scale=float(c0))
    scans, svs = [], []
    try:
        b.dense_iter_grad(hp, dverts_extra=np.zeros((len(items), dev.n_verts, 3), np.float32))       # (a full-model mesh pass at the point)
        verts = b.debug_vertices()
        for i in range(len(items)):
            lo, hi = verts[i][:, 1].min(), verts[i][:, 1].max()
            assert hi - lo < h
            y0 = np.float32(np.floor((lo - (h - (hi - lo)) / 2) * 1024) / 1024)                        # (a multiple of 2^-10: y0 + h is exact)
            y1 = np.float32(y0 + h)
            assert y0 <= lo and y1 >= hi and np.float32(y1 - y0) == h
            x, z = verts[i][:, 0].mean(), verts[i][:, 2].mean()
            svs.append(np.concatenate([verts[i], np.array([[x, y0, z], [x, y1, z]], np.float32)]))
            assert np.float32(DC.scan_cscale(svs[i])) == c0
            scans.append(N.Scan(svs[i], np.asarray(model["faces"]).reshape(-1, 3)))
        for i, s in enumerate(scans):                        # the precondition, on the device
            pts = s.nearest_points(verts[i])[0]
            np.testing.assert_array_equal(pts.view(np.uint32), verts[i].view(np.uint32), err_msg=f"frame {i}: a vertex is not its own closest point")
        b.set_scans(scans)
        terms, grads = b.dense_iter_grad(hp, late=True)
        np.testing.assert_array_equal(b.debug_vertices().view(np.uint32), verts.view(np.uint32), err_msg="attaching the scans moved the vertices")
    finally:
        b.close()
        for s in scans:
            s.close()
    assert np.isfinite(terms).all() and np.isfinite(grads).all(), f"{int((~np.isfinite(grads)).sum())} of {grads.size} gradient entries are not finite"
    assert not terms[:, 5].any() and not terms[:, 4].any()
    failures = []
    for i, (f, sc) in enumerate(items):
        # (closest = vertices on the oracle's side too: its own body vertices in each precision, so that its norm is exactly zero as the
        #  device's is; the constant scale and the height are those of the scan, the device's float32 vertices)
        kw = dict(scan_height=DC.scan_height(svs[i]), constant_scale=DC.scan_cscale(svs[i]))
        args = (model, DC.LC.gmm_bufs(), probs[i], params[i])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            r64 = O.dense_loss_and_grad(*args, closest=O.dense_loss_and_grad(*args, **kw)[2], **kw)
            r32 = O.dense_loss_and_grad(*args, dtype=torch.float32, closest=O.dense_loss_and_grad(*args, dtype=torch.float32, **kw)[2], **kw)
        assert r64[0]["scan_loss"] == 0.0 and r32[0]["scan_loss"] == 0.0
        np.testing.assert_allclose(verts[i], r64[2], rtol=0, atol=5e-6 * max(1.0, np.abs(r64[2]).max()))
        failures += _hold(f"c zero distance frame {i}", name, dev, terms[i], grads[i], r64, r32)
    assert not failures, "\n  ".join(failures)


# ---- d. silhouette term ----------------------------------------------------------------------------------------------------

def _mask_batch(dev):
    prob, mi = DC.mask_problem(), DC.mask_inputs()
    b = _batch(dev, [prob], [DC.mask_params()])
    b.set_masks(mi["masks_u8"][None], mi["views"], [mi["contours"]])
    return b, _hyper(prob)


@pytest.mark.parametrize("sub_model", [False, True], ids=["full", "sub-model"])
@pytest.mark.parametrize("fold", ["sums", "gather"])
def test_silhouette_term_matches_fp64_autograd(dev_model, fold, sub_model):
    """the well-posed silhouette case (dense_grad_cases.MASK_*: 64 x 64 image, two mask views), exact distances on both sides, under both
    folds of the contour gradients and with the mesh passes on the full model (samp_stride 4) and on the sampled-first sub-model
    (samp_stride 1): terms[4] and every block"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        r64, r32 = DC.mask_evaluate(), DC.mask_evaluate(torch.float32)
    before = N.set_mask_fold(fold)
    try:
        b, hp = _mask_batch(dev_model)
        try:
            terms, grads = b.dense_iter_grad(hp, late=True, sub_model=sub_model)
        finally:
            b.close()
    finally:
        N.set_mask_fold(before)
    assert terms[0, 4] > 0 and terms[0, 5] == 0
    failures = _hold(f"d silhouette {fold} {'sub-model' if sub_model else 'full model'}", DC.MASK_MODEL, dev_model, terms[0], grads[0], r64, r32)
    assert not failures, "\n  ".join(failures)


def test_silhouette_and_scan_together(dev_model):
    """keypoints + silhouette + scan in the order of additions dense_pass keeps (the scan's gradient adds onto keypoints +
    silhouette); the constant scale is the scan's"""
    sv, sf = DC.mask_scan()
    scan = N.Scan(sv, sf)
    b, hp = _mask_batch(dev_model)
    try:
        b.set_scans([scan])
        terms, grads = b.dense_iter_grad(hp, late=True)
        verts = b.debug_vertices()
    finally:
        b.close()
        scan.close()
    _, closest = DC.closest_points(sv, sf, verts[0])
    h, c = DC.scan_height(sv), DC.scan_cscale(sv)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        r64 = DC.mask_evaluate(closest=closest, height=h, cscale=c)
        r32 = DC.mask_evaluate(torch.float32, closest=closest, height=h, cscale=c)
    assert terms[0, 4] > 0 and terms[0, 5] > 0
    failures = _hold("d silhouette + scan", DC.MASK_MODEL, dev_model, terms[0], grads[0], r64, r32)
    assert not failures, "\n  ".join(failures)


# ---- e. state and refusals -------------------------------------------------------------------------------------------------

def test_the_call_leaves_a_keypoint_fit_as_it_found_it(devs):
    """fit(k), the call, fit(k) == fit(k), fit(k), bit for bit (parameters and the mesh of the result), for the sparse (SMPL) and the
    dense (SMPL-X) keypoint schedule"""
    for name in ("smpl690", "smplx1200"):
        dev = devs(name)
        frames = DC.frames(name, 2)
        probs = [DC.problem(name, f) for f in frames]
        cot = np.stack([DC.cotangent(name, f) for f in frames]).astype(np.float32)
        out = []
        for call in (False, True):
            b = _batch(dev, probs, None)
            try:
                b.fit(4)
                if call:
                    for sub in (False, True):
                        b.dense_iter_grad(_hyper(probs[0]), sub_model=sub, dverts_extra=cot)
                b.fit(4)
                out.append((b.get_params().copy(), b.get_result()[0].copy()))
            finally:
                b.close()
        np.testing.assert_array_equal(out[0][0], out[1][0], err_msg=name)
        np.testing.assert_array_equal(out[0][1], out[1][1], err_msg=name)


def test_the_call_leaves_a_scan_fit_as_it_found_it(devs):
    """with scans attached and dense_after = 5: calls before the switch-on (after 4 steps), across it and after it (after 8), late and
    not - the twelve steps give the bits of twelve steps without the calls (the closest-point search's warm start is put back)"""
    name = "smpl690"
    dev = devs(name)
    out = []
    for call in (False, True):
        b, scans, _ = _scan_batch(dev, name, DC.SCAN_FRAMES, at_point=False)          # (from the initial estimate, as a fit starts)
        hp = N.make_hyper(dense_after=5)
        try:
            for k in range(3):
                b.fit(4, hp)
                if call:
                    b.dense_iter_grad(hp, late=True)
                    b.dense_iter_grad(hp, late=False)
                    b.dense_iter_grad(hp, late=True, sub_model=True)
            out.append(b.get_params().copy())
        finally:
            b.close()
            for s in scans:
                s.close()
    np.testing.assert_array_equal(out[0], out[1])


def test_refusals(devs):
    """BF_ERR_INVALID (-1) for what cannot be evaluated: late with nothing attached, an unknown flag, a batch whose scan was destroyed"""
    name = "smpl690"
    dev = devs(name)
    prob = DC.problem(name, 0)
    b = _batch(dev, [prob], [DC.params(name, 0)])
    try:
        with pytest.raises(_lib.BodyfitError, match=r"\(-1\).*neither scans nor silhouettes"):
            b.dense_iter_grad(late=True)
        grads = np.empty((1, dev.n_params), np.float32)
        assert b._lib.bf_dense_iter_grad(b._h, None, 4, None, None, _lib.fptr(grads)) == -1
        assert b._lib.bf_dense_iter_grad(None, None, 0, None, None, None) == -1
        assert b._lib.bf_dense_iter_grad(b._h, None, 0, None, None, None) == 0          # every output may be NULL
    finally:
        b.close()
    b, scans, hp = _scan_batch(dev, name, DC.SCAN_FRAMES[:1])
    try:
        b.dense_iter_grad(hp, late=True)
        scans[0].close()
        with pytest.raises(_lib.BodyfitError, match=r"\(-1\).*was destroyed"):
            b.dense_iter_grad(hp, late=True)
        with pytest.raises(_lib.BodyfitError, match=r"\(-1\).*was destroyed"):
            b.dense_iter_grad(hp)
        b.set_scans(None)                                   # detached: late has nothing to evaluate, the keypoint gradient is back
        with pytest.raises(_lib.BodyfitError, match=r"\(-1\).*neither scans nor silhouettes"):
            b.dense_iter_grad(hp, late=True)
        assert np.isfinite(b.dense_iter_grad(hp)[1]).all()
    finally:
        b.close()


# ---- f. SMPL+D gradient away from zero ----------------------------------------------------------------------------------------

def test_displacement_gradient_after_three_steps(devs):
    """The stage's Adam keeps m_k = m_{k-1} + (g_k - m_{k-1}) (1 - beta1) with beta1 = 0.9 (csrc/disp_kernels.hip), so the gradient of
    step 4 is read from the first moments after three and four steps: g_4 = m_3 + (m_4 - m_3) / (1 - beta1), with the constants as
    the kernel holds them in float32.  It is held to float64 autograd of the oracle's SMPL+D objective (smplify.py:228-247) at
    base + the device's displacement after three steps, closest points and face ids from the reference's search at those float32
    vertices, on a two-frame batch whose scans differ in height (per-frame constant scale, block sums and face normals).
    Band: the block band of DESIGN.md 2.3, max(5e-6 M, 8 err32), plus the read-out's own rounding 19 * 2^-24 * max|m|."""
    import disp_stage_cases as D
    name = "smpl690"
    dev = devs(name)
    model = DC.model(name)
    b, scans, _ = _scan_batch(dev, name, DC.SCAN_FRAMES, at_point=False)
    try:
        b.fit(30)
        base = b.get_result()[0].copy()
        b.fit_displacement(3)
        d3, m3 = b.get_displacement().copy(), b.disp_moment().copy()
        b.fit_displacement(4)                              # (the stage restarts from zero: the same three steps, then the fourth)
        m4 = b.disp_moment().copy()
        ids_dev = [scans[i].nearest_points(base[i] + d3[i])[1] for i in range(len(scans))]
    finally:
        b.close()
        for s in scans:
            s.close()
    assert np.abs(d3).max() > 0.01                                        # three steps of 5 cm: well away from zero
    w = float(np.float32(1.0) - np.float32(0.9))
    grad = m3.astype(np.float64) + (m4.astype(np.float64) - m3) / w
    faces = np.asarray(model["faces"]).reshape(-1, 3)
    failures = []
    for i, (f, sc) in enumerate(DC.SCAN_FRAMES):
        _, sv, sf = DC.scan_problem(name, f, sc)
        # (the reference's search at the float32 base + d3, its ties with the device's search settled and capped, and the float64 and
        #  float32 autograd of the objective: disp_stage_cases.reference / settle_ties, shared with test_gpu_disp_stage.py)
        ref = D.reference(faces, sv, sf, base[i], d3[i], ids_dev[i])
        g = {torch.float64: ref["g64"], torch.float32: ref["g32"]}
        band, M, err32 = DC.band(g[torch.float64], g[torch.float32])
        readout = 19 * 2.0 ** -24 * float(max(np.abs(m3[i]).max(), np.abs(m4[i]).max()))
        err = float(np.abs(grad[i] - g[torch.float64]).max())
        RESULTS.append((f"f SMPL+D frame {i}", "displacement", err / (band + readout)))
        print(f"f SMPL+D frame {i}: err {err:.3e}, M {M:.3e}, err32 {err32:.3e}, band {band:.3e} + read-out {readout:.3e}; position {err / (band + readout):.3f}")
        if not err <= band + readout:
            failures.append(f"frame {i}: err {err:.3e} = {err / M:.2e} M, band {band + readout:.3e}")
    assert not failures, "\n  ".join(failures)


def test_report():
    """the worst position inside a band over every check of this file"""
    assert RESULTS
    w = max(RESULTS, key=lambda r: r[2] if np.isfinite(r[2]) else np.inf)
    print(f"\n{len(RESULTS)} terms and blocks compared; worst position inside its band {w[2]:.3f} ({w[0]}: {w[1]})")
    for part in "abcdf":
        rows = [r for r in RESULTS if r[0].startswith(part + " ")]
        if rows:
            wp = max(rows, key=lambda r: r[2])
            print(f"  {part}: {len(rows)} compared, worst {wp[2]:.3f} ({wp[0]}: {wp[1]})")
    assert all(np.isfinite(r[2]) for r in RESULTS)
