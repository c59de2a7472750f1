"""BASELINE configs 3 and 5 AT THEIR STATED SIZE through the C ABI (rounds 1-2 held them on reduced models / short loops only).

Config 3: SMPL-X (10,475 v, 55 joints, 135 output joints), 48 views + 8 silhouettes at 512 x 512, 200 iterations - against the
imported reference's run of exactly that (tests/golden/cfg3_smplx_48view_8mask_200it_base.npz) and its own drift under
perturbation (tests/ref_drift.py).  Config 5: 8 SMPL-X frames with a ~84k-triangle scan each, 300 iterations + 300 SMPL+D
iterations.  Frame 0 is held against the imported reference's run of exactly that (tests/golden/cfg5_smplx_48view_scan_300it_base.npz,
its closest-point search the grid walk of oracle/nearest_ref.c in the reference's float32 arithmetic) and its own drift under the
scan loops' eleven perturbations; the whole batch of eight by size-independent properties: batch == single frames, run == re-run,
resident launch == one launch per iteration (all bit for bit), and the objective / distance distribution improving by stated factors."""
import os

import numpy as np
import pytest

from conftest import load_golden
from bodyfitting_amd import _lib, native as N, synthetic as S
from oracle import smplify_oracle as O
import ref_drift as RD
from scan_metrics import disp_metrics

pytestmark = pytest.mark.gpu
MASK_FRAMES = list(range(0, 48, 6))


@pytest.fixture(scope="module")
def sx():
    model = S.make_model("smplx", seed=0)
    dev = N.DeviceModel(model, S.make_gmm(seed=0), device=0)
    yield model, dev
    dev.close()


def test_config3_as_stated_against_the_reference(sx):
    from oracle.contour_oracle import border_pixels_rowmajor_all as extract_contours      # (what the golden's cv2 stub returned)
    model, dev = sx
    g = load_golden("cfg3_smplx_48view_8mask_200it_base.npz")
    assert str(g["model_digest"]) == S.model_digest(model)
    prob = S.make_problem_smplx(model, frame=0, n_views=48, mask_frames=MASK_FRAMES)
    c2w, K, kp, ndiv, betas, pose = N.pack_problem([prob])
    b = N.FrameBatch(dev, 1, 48)
    b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose)
    b.set_masks(np.array(prob["masks"])[None], MASK_FRAMES, [extract_contours(np.array(prob["masks"]) > 128)])
    # the loss the loop computes in its first iteration (multiview_keypoint_loss's dict, loss.py:219-224)
    terms, _ = b.loss_grad()
    for i, n in enumerate(("reprojection_loss", "pose_prior_loss", "angle_prior_loss", "shape_prior_loss")):
        assert terms[0, i] == pytest.approx(float(g[f"it1_loss_{n}"]), rel=3e-5), n
    done, errs = 0, {}
    for k in (1, 66, 67, 68, 200):
        b.fit(k - done, N.make_hyper(dense_after=66))        # 200 // 3: ONE reference loop cut at the golden's snapshots
        done = k
        got = N.split_params(b.get_params()[0])
        errs[k] = max(float(np.abs(got[n] - g[f"it{k}_{n}"]).max()) for n in O.SMPLX_PARAMS)
    ref = {k: RD.cfg3_drift([f"it{k}_{n}" for n in O.SMPLX_PARAMS]) for k in (66, 67, 68, 200)}
    print("config 3 as stated: max |param - reference| per snapshot", errs, "| the reference's own largest drift under ten perturbations", ref)
    for k in (68, 200):
        print("  iteration", k, ":", RD.position(errs[k], RD.cfg3_drifts([f"it{k}_{n}" for n in O.SMPLX_PARAMS])))
    # iterations 1..67 are keypoint-only (the silhouette loss is active for loop index i > 200 // 3 = 66, i.e. from the 68th step on,
    # smplify.py:197): the north-star tolerance
    assert errs[1] < 1e-5 and errs[66] < 1e-4 and errs[67] < 1e-4
    # the first silhouette iteration: a tenth of one Adam step (lr 1e-2) - at most a near-tie flip of a nearest-vertex choice away
    # (the reference moves 1.3e-4 from itself in this step under a one-ulp nudge of the initial pose)
    assert errs[68] < max(1e-3, RD.K * ref[68]), (errs[68], ref[68])
    assert errs[200] < max(RD.FLOOR, RD.K * ref[200]), (errs[200], ref[200])
    verts, joints, full_pose, _ = b.get_result()
    # the 17 dynamic contour landmarks are picked by an integer look-up on the neck's yaw: between two runs of the REFERENCE they jump
    # by 25 cm; the other 118 joints are continuous in the parameters
    base, var = RD.cfg3_variants()
    jd = max(float(np.abs(var[v]["joints"][:118] - base["joints"][:118]).max()) for v in RD.VARIANTS)
    np.testing.assert_allclose(joints[0][:118], g["joints"][:118], atol=max(RD.FLOOR, RD.K * jd))
    np.testing.assert_allclose(verts[0][::53], g["vertices_sample"], atol=max(RD.FLOOR, RD.K * RD.cfg3_drift(["vertices_sample"])))
    # the silhouette term of the objective at the end state, evaluated by the same kernel at both parameter sets
    end_got = float(b.mask_loss()[0][0])
    names = O.SMPLX_PARAMS
    b.set_params(N.pack_params({n: g[f"it200_{n}"] for n in names})[None])
    end_ref = float(b.mask_loss()[0][0])
    ends = []
    for v in RD.VARIANTS:
        b.set_params(N.pack_params({n: var[v][f"it200_{n}"] for n in names})[None])
        ends.append(float(b.mask_loss()[0][0]))
    spread = max(abs(e - end_ref) for e in ends) / end_ref
    print("silhouette loss at the end state: HIP", end_got, "reference", end_ref, "reference variants", ends)
    print("  relative to the reference's:", RD.position(abs(end_got - end_ref) / end_ref, [abs(e - end_ref) / end_ref for e in ends]))
    assert abs(end_got - end_ref) / end_ref < max(0.01, RD.K * spread)
    b.close()


def test_config5_as_stated_against_the_reference(sx):
    """config 5 at its stated size for frame 0: SMPL-X, 48 views, the ~84k-triangle scan, 300 iterations (the closest-point loss
    active for loop index i > 300 // 3, smplify.py:205: steps 1..101 keypoint-only, 102 the first with the scan) + 300 SMPL+D
    iterations, against the imported reference's run of exactly that (oracle/gen_golden.py cfg5_goldens).  The fit is held
    snapshot by snapshot; the chaotic SMPL+D stage by its end state (as the reduced model's test in tests/test_gpu_scan.py); every
    band is K x the reference's own largest drift under the eleven SCAN_VARIANTS perturbations (tests/ref_drift.py)."""
    model, dev = sx
    base, var = RD.cfg5_variants()
    g = base
    prob, sv, sf = S.make_scan_problem_smplx(model, frame=0, n_views=48)
    assert str(g["model_digest"]) == S.model_digest(model)
    assert str(g["scan_digest"]) == S.scan_digest(sv, sf)
    names = O.SMPLX_PARAMS
    scan = N.Scan(sv, sf)
    c2w, K, kp, ndiv, betas, pose = N.pack_problem([prob])
    b = N.FrameBatch(dev, 1, 48)
    b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose); b.set_scans([scan])
    # the loss the loop computes in its first iteration (multiview_keypoint_loss's dict, loss.py:219-224; no scan term yet)
    terms, _ = b.loss_grad()
    for i, n in enumerate(("reprojection_loss", "pose_prior_loss", "angle_prior_loss", "shape_prior_loss")):
        assert terms[0, i] == pytest.approx(float(g[f"it1_loss_{n}"]), rel=3e-5), n
    snaps = (1, 100, 101, 102, 103, 300)
    done, errs = 0, {}
    for k in snaps:
        b.fit(k - done, N.make_hyper(dense_after=100))       # 300 // 3: ONE reference loop cut at the golden's snapshots
        done = k
        got = N.split_params(b.get_params()[0])
        errs[k] = max(float(np.abs(got[n] - g[f"it{k}_{n}"]).max()) for n in names)
    ref = {k: RD.cfg5_drift([f"it{k}_{n}" for n in names]) for k in snaps}
    print("config 5 as stated: max |param - reference| per snapshot", errs, "| the reference's own largest drift under eleven perturbations", ref)
    for k in (102, 103, 300):
        print("  iteration", k, ":", RD.position(errs[k], RD.cfg5_drifts([f"it{k}_{n}" for n in names])))
    # iterations 1..101 are keypoint-only: the north-star tolerance, and the reference is well conditioned there too
    assert errs[1] < 1e-5 and errs[100] < 1e-4 and errs[101] < 1e-4, errs
    assert max(RD.FLOOR, RD.K * ref[101]) < 2e-4, ref[101]
    # the first scan iteration: one Adam step past a closest-face choice decided by last bits
    assert errs[102] < max(1e-3, RD.K * ref[102]), (errs[102], ref[102])
    for k in (103, 300):
        assert errs[k] < max(RD.FLOOR, RD.K * ref[k]), (k, errs[k], ref[k])
    verts, joints, _, _ = b.get_result()
    np.testing.assert_allclose(verts[0], g["vertices"], atol=max(RD.FLOOR, RD.K * RD.cfg5_drift(["vertices"])))
    # (the 17 dynamic contour landmarks jump between runs of the reference, as in config 3; the other 118 joints are continuous)
    jd = max(float(np.abs(var[v]["joints"][:118] - g["joints"][:118]).max()) for v in RD.SCAN_VARIANTS)
    np.testing.assert_allclose(joints[0][:118], g["joints"][:118], atol=max(RD.FLOOR, RD.K * jd))

    def rel_band(metric_of, ref_value, floor=0.05):
        """K x how far the reference's perturbed runs end from the reference in this metric (relative), at least `floor`"""
        return max(floor, RD.K * max(abs(metric_of(v) - ref_value) for v in RD.SCAN_VARIANTS) / abs(ref_value))
    fit_ref = disp_metrics(model, sv, sf, g["vertices"], 0 * g["vertices"])
    fit_got = disp_metrics(model, sv, sf, verts[0], 0 * verts[0])
    fit_var = {v: disp_metrics(model, sv, sf, var[v]["vertices"], 0 * var[v]["vertices"]) for v in RD.SCAN_VARIANTS}
    print("fit end state  reference:", fit_ref, "\n               HIP:      ", fit_got, "\n               reference, perturbed:", fit_var)
    for key in ("mean", "median", "p95", "icp"):
        tol = rel_band(lambda v: fit_var[v][key], fit_ref[key])
        assert abs(fit_got[key] - fit_ref[key]) / fit_ref[key] < tol, (key, fit_got[key], fit_ref[key], tol)
    # the objective at the end of the fit: the keypoint terms by the same kernel at every parameter set + 5 * imsize / height * icp
    w_pc = 5.0 * 512.0 / float(sv[:, 1].max() - sv[:, 1].min())
    cases = [("reference", N.pack_params({n: g[f"it300_{n}"] for n in names})[None], fit_ref["icp"]), ("HIP", b.get_params().copy(), fit_got["icp"])]
    cases += [(v, N.pack_params({n: var[v][f"it300_{n}"] for n in names})[None], fit_var[v]["icp"]) for v in RD.SCAN_VARIANTS]
    obj = {}
    for name, pk, icp in cases:
        probe = N.FrameBatch(dev, 1, 48)
        probe.set_cameras(c2w, K); probe.set_keypoints(kp, ndiv); probe.set_init(betas, pose); probe.set_scans([scan])   # (constant scale = height / 1.7)
        probe.set_params(pk)
        obj[name] = float(probe.loss_grad()[0].sum()) + w_pc * icp
        probe.close()
    print("objective after 300 iterations:", obj)
    assert obj["HIP"] == pytest.approx(obj["reference"], rel=rel_band(lambda v: obj[v], obj["reference"], floor=0.02))
    # SMPL+D: chaotic under round-off, held by its end state
    b.fit_displacement(300)
    disp = b.get_displacement()[0]
    want = disp_metrics(model, sv, sf, g["vertices"], g["displacement"])
    before = disp_metrics(model, sv, sf, g["vertices"], 0 * g["displacement"])
    got = disp_metrics(model, sv, sf, verts[0], disp)
    disp_var = {v: disp_metrics(model, sv, sf, var[v]["vertices"], var[v]["displacement"]) for v in RD.SCAN_VARIANTS}
    print("SMPL+D end state  reference:", want, "\n                  HIP:      ", got, "\n                  before:   ", before,
          "\n                  reference, perturbed:", disp_var)
    for key in ("mean", "median", "p95", "icp", "normal", "laplacian"):
        tol = rel_band(lambda v: disp_var[v][key], want[key], floor=0.1)
        assert abs(got[key] - want[key]) / abs(want[key]) < tol, (key, got[key], want[key], tol)
    assert got["mean"] < 0.75 * before["mean"] and got["median"] < 0.4 * before["median"]
    print("max |displacement|: HIP", float(np.abs(disp).max()), "reference", float(np.abs(g["displacement"]).max()))
    assert np.abs(disp).max() < 2 * np.abs(g["displacement"]).max()
    b.close()
    scan.close()


def _cfg5_items(model, n):
    return [S.make_scan_problem_smplx(model, frame=f, n_views=48) for f in range(n)]


def _run_cfg5(dev, items, scans, frames, iters=300, disp=300):
    c2w, K, kp, ndiv, betas, pose = N.pack_problem([items[f][0] for f in frames])
    b = N.FrameBatch(dev, len(frames), 48)
    b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose); b.set_scans([scans[f] for f in frames])
    b.fit(iters, flags=_lib.FIT_FETCH)
    params = b.get_params().copy()
    verts = b.get_result()[0].copy()
    b.fit_displacement(disp)
    d = b.get_displacement().copy()
    b.close()
    return params, verts, d


def test_config5_as_stated_is_deterministic_and_improves(sx):
    """8 SMPL-X frames x 48 views, one ~84k-triangle scan per frame, 300 iterations (scan loss after 100) + 300 SMPL+D iterations"""
    model, dev = sx
    items = _cfg5_items(model, 8)
    assert 80_000 < len(items[0][2]) < 90_000
    scans = [N.Scan(sv, sf) for _, sv, sf in items]
    full = _run_cfg5(dev, items, scans, list(range(8)))
    # run == re-run, bit for bit (fixed-order reductions; the resident launch exchanges doorbells, not races)
    again = _run_cfg5(dev, items, scans, list(range(8)))
    for a, b_ in zip(full, again):
        np.testing.assert_array_equal(a, b_)
    # the resident fit launch == one fit launch per iteration, bit for bit
    os.environ["BF_DENSE_PERSISTENT"] = "0"
    try:
        plain = _run_cfg5(dev, items, scans, list(range(8)))
    finally:
        del os.environ["BF_DENSE_PERSISTENT"]
    for a, b_ in zip(full, plain):
        np.testing.assert_array_equal(a, b_)
    # the batch of 8 == eight single-frame fits, bit for bit (frames are independent)
    for f in (0, 3, 7):
        one = _run_cfg5(dev, items, scans, [f])
        np.testing.assert_array_equal(one[0][0], full[0][f])
        np.testing.assert_array_equal(one[1][0], full[1][f])
        np.testing.assert_array_equal(one[2][0], full[2][f])
    # what the loops achieve: point-to-scan distances of the fitted mesh against the keypoint-only fit, and of the SMPL+D mesh
    kp_only = N.FrameBatch(dev, 8, 48)
    c2w, K, kp, ndiv, betas, pose = N.pack_problem([it[0] for it in items])
    kp_only.set_cameras(c2w, K); kp_only.set_keypoints(kp, ndiv); kp_only.set_init(betas, pose); kp_only.set_scans(scans)
    kp_only.fit(100, N.make_hyper(dense_after=1000), flags=_lib.FIT_FETCH)          # the first third: no scan loss yet
    v100 = kp_only.get_result()[0]
    kp_only.close()
    ratios = []
    for f in range(8):
        dist = lambda v: np.linalg.norm(v - scans[f].nearest_points(v.astype(np.float32))[0], axis=1)      # noqa: E731
        d100, d300, dd = dist(v100[f]), dist(full[1][f]), dist(full[1][f] + full[2][f])
        print(f"frame {f}: mean distance to the scan after 100 keypoint-only iterations {d100.mean() * 1e3:.2f} mm, after the 300-iteration fit "
              f"{d300.mean() * 1e3:.2f} mm, after SMPL+D {dd.mean() * 1e3:.2f} mm (median {np.median(dd) * 1e3:.2f}, p95 {np.percentile(dd, 95) * 1e3:.2f})")
        ratios.append(float(d300.mean() / d100.mean()))
        assert d300.mean() < 1.2 * d100.mean()                       # the closest-point loss pulls the body onto the scan (below: on average) ...
        assert dd.mean() < 0.6 * d300.mean() and np.median(dd) < 0.4 * np.median(d300)     # ... and the displacement stage closes most of what is left
        assert np.isfinite(full[2][f]).all()
    # (the closest-point term is ~10 % of the objective and competes with the keypoints: frame 2 stays at 13 mm, the others halve)
    print("mean distance after the fit / after the keypoint-only third, per frame:", ratios)
    assert np.mean(ratios) < 0.8 and np.median(ratios) < 0.7
    for s in scans:
        s.close()
