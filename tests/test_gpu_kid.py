"""age='kid' on the MI355X: the 11-beta model (smplx's kid branch on a synthetic template) through the forward pass, the analytic
gradient, the keypoint / silhouette / scan + SMPL+D fits, the batched mesh kernels and the drop-in API - against the oracle run on
the CPU here (oracle/smplify_oracle.py takes any model dict and problem["init_betas"] of any width)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from bodyfitting_amd import assets, model_files, native as N, synthetic as S
from oracle import smplify_oracle as O
from oracle.contour_oracle import border_pixels_rowmajor_all as extract_contours
import ref_drift as RD

pytestmark = pytest.mark.gpu
PARAMS = ("global_transl", "scale", "pose", "betas", "global_orient")
KID_BETA = 0.4            # the ground truth's 11th beta: the fit has something to find along the kid direction
MASK_FRAMES = [1, 3, 5, 7]                 # (the adult mask tests' views)


@pytest.fixture(scope="module")
def kid(smpl_model):
    return model_files.kid_model(smpl_model, S.make_kid_template(smpl_model))


@pytest.fixture(scope="module")
def kid_dev(kid, gmm):
    m = N.DeviceModel(kid, gmm, device=0)
    yield m
    m.close()


def _problem(kid, frame=0, n_views=48, **kw):
    return S.as_kid_problem(S.make_problem(S.kid_problem_model(kid, KID_BETA), frame=frame, n_views=n_views, **kw), KID_BETA)


def _batch(dev, problems):
    c2w, K, kp, ndiv, betas, pose = N.pack_problem(problems)
    b = N.FrameBatch(dev, len(problems), c2w.shape[1])
    b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose)
    return b


def test_kid_model_sizes_and_instances(kid_dev, dev_model):
    """11 betas, 87 parameters, the table-driven fit instance; the adult model keeps the compile-time-sized one"""
    assert kid_dev.n_betas == 11 and kid_dev.n_params == 87
    assert kid_dev.fit_instance == "table-driven"
    assert dev_model.n_betas == 10 and dev_model.fit_instance == "sized"


@pytest.mark.parametrize("n", [1, 3, 32, 100])
def test_kid_forward_matches_oracle(kid_dev, kid, n):
    """vertices and the 49 joints at the adult bound, with a non-zero kid beta.  n = 1: the one-frame kernels; 3: the multi-frame
    kernel; 32: bf_mesh_batch32_kernel<12>; 100: the pose-blend GEMM + bf_mesh_epilogue_batch_kernel<12>"""
    rng = np.random.default_rng(11 + n)
    betas = rng.normal(0, 0.7, (n, 11)).astype(np.float32)
    betas[:, 10] = rng.uniform(0.2, 0.9, n)
    orient = rng.normal(0, 0.8, (n, 3)).astype(np.float32)
    pose = rng.normal(0, 0.3, (n, 69)).astype(np.float32)
    verts, joints, jori = kid_dev.forward(betas, orient, pose)
    m = O.to_torch_model(kid, torch.float64)
    ref = O.smpl_forward(m, torch.tensor(betas, dtype=torch.float64), torch.tensor(orient, dtype=torch.float64),
                         torch.tensor(pose, dtype=torch.float64))
    np.testing.assert_allclose(verts, ref["vertices"].numpy(), atol=3e-6)
    np.testing.assert_allclose(joints, ref["joints"].numpy(), atol=3e-6)
    np.testing.assert_allclose(jori, ref["joints_ori"].numpy(), atol=3e-6)


def test_kid_loss_grad_matches_fp64_autograd(kid_dev, kid, gmm_bufs):
    prob = _problem(kid, frame=1, n_views=6)
    b = _batch(kid_dev, [prob])
    rng = np.random.default_rng(5)
    params = {"global_transl": rng.normal(0, 0.03, 3), "scale": np.array([1.05]), "pose": rng.normal(0, 0.2, 69),
              "betas": np.concatenate([rng.normal(0, 0.5, 10), [0.3]]), "global_orient": np.array([0.1, 1.2, -0.05])}
    b.set_params(N.pack_params(params)[None])
    terms, grads = b.loss_grad()
    loss, _, g64, _, _ = O.loss_and_grad(kid, gmm_bufs, prob, params)
    assert float(terms.sum()) == pytest.approx(loss, rel=2e-6)
    got = N.split_params(grads[0], 24, 11)
    assert got["betas"].shape == (11,)
    for k in PARAMS:
        np.testing.assert_allclose(got[k], g64[k], atol=5e-6 * np.abs(g64[k]).max(), err_msg=k)
    b.close()


def test_kid_fit_matches_oracle_loop(kid_dev, kid, gmm_bufs):
    """1 frame x 48 views x 100 iterations (BASELINE config 2's size) against the oracle loop at iterations 1 / 2 / 10 / 50 / 100"""
    prob = _problem(kid, frame=0, n_views=48)
    want = O.fit(kid, gmm_bufs, prob, 100, snapshots=(1, 2, 10, 50, 100))
    b = _batch(kid_dev, [prob])
    done = 0
    for k in (1, 2, 10, 50, 100):
        b.fit(k - done)
        done = k
        got = N.split_params(b.get_params()[0], 24, 11)
        for n in PARAMS:
            np.testing.assert_allclose(got[n], want["snapshots"][k][n], rtol=0, atol=1e-4, err_msg=f"it{k} {n}")
    verts, joints, full_pose, _ = b.get_result()
    np.testing.assert_allclose(joints[0], want["joints"], atol=1e-4)
    np.testing.assert_allclose(verts[0], want["vertices"], atol=1e-4)
    assert abs(float(got["betas"][10])) > 0.05                   # the kid direction was used
    b.close()


def test_kid_mask_fit_against_oracle(kid_dev, kid, gmm_bufs):
    """use_mask=True, 30 iterations (19 with 5 x the silhouette loss).  Keypoint-only prefix at 1e-4; afterwards the discontinuous
    objective amplifies round-off, so the band is K x the larger of the adult reference's own drift (the adult mask test's band) and
    the kid oracle's own drift under two perturbations that change no mathematics"""
    prob = _problem(kid, frame=0, n_views=8, mask_frames=MASK_FRAMES)
    snaps = (11, 20, 30)
    want = O.fit(kid, gmm_bufs, prob, 30, snapshots=snaps)
    own = {k: [] for k in snaps}
    ulp = dict(prob, init_pose=np.nextafter(prob["init_pose"], np.float32(np.inf)).astype(np.float32))
    threads = torch.get_num_threads()
    for variant in ("ulp", "threads4"):
        try:
            if variant == "threads4":
                torch.set_num_threads(4)
            alt = O.fit(kid, gmm_bufs, ulp if variant == "ulp" else prob, 30, snapshots=snaps)
        finally:
            torch.set_num_threads(threads)
        for k in snaps:
            own[k].append(max(float(np.abs(alt["snapshots"][k][n] - want["snapshots"][k][n]).max()) for n in PARAMS))
    base, sens = load_golden("mask_fit_8view_30it.npz"), load_golden("sens_mask_fit_8view_30it.npz")
    adult_band = {k: RD.band(base, sens, [f"it{k}_{n}" for n in PARAMS]) for k in (20, 30)}
    b = _batch(kid_dev, [prob])
    b.set_masks(np.array(prob["masks"])[None], [prob["use_frames"].index(f) for f in prob["mask_frames"]],
                [extract_contours(np.array(prob["masks"]) > 128)])
    done = 0
    for k in snaps:
        b.fit(k - done, N.make_hyper(dense_after=10))
        done = k
        got = N.split_params(b.get_params()[0], 24, 11)
        err = max(float(np.abs(got[n] - want["snapshots"][k][n]).max()) for n in PARAMS)
        if k == 11:
            assert err < 1e-4, err
            continue
        band = max(adult_band[k], RD.K * max(own[k]))
        print(f"kid mask loop it{k}: max |param - oracle| {err:.3g}, band {band:.3g};", RD.position(err, own[k]))
        assert err < band, (k, err, band)
    verts, _, _, _ = b.get_result()
    assert np.isfinite(verts).all()
    b.close()


@pytest.fixture(scope="module")
def small_kid(gmm):
    model = S.make_model("smpl", seed=0, nv=690)
    k = model_files.kid_model(model, S.make_kid_template(model))
    dev = N.DeviceModel(k, gmm, device=0)
    yield k, dev
    dev.close()


def test_kid_scan_and_displacement_at_nv690(small_kid, gmm_bufs):
    """use_mesh=True on the reduced model: 11 keypoint-only iterations, 19 with the point-cloud loss, against the oracle's
    fit(scan=..., displacement=True) at the adult NV = 690 test's bounds (parameters, vertices, joints 1e-4; SMPL+D first step 2e-5,
    three steps: 97 % of the coordinates within 2e-4)"""
    model, dev = small_kid
    prob, sv, sf = S.make_scan_problem(S.kid_problem_model(model, KID_BETA), frame=0, n_views=8)
    prob = S.as_kid_problem(prob, KID_BETA)
    want = O.fit(model, gmm_bufs, prob, 30, scan=(sv, sf), displacement=True, disp_snapshots=(1, 3))
    scan = N.Scan(sv, sf)
    b = _batch(dev, [prob])
    b.set_scans([scan])
    b.fit(30)
    got = N.split_params(b.get_params()[0], 24, 11)
    for n in PARAMS:
        np.testing.assert_allclose(got[n], want[n] if n != "global_transl" else want["raw_transl"], rtol=0, atol=1e-4, err_msg=n)
    verts, joints, _, _ = b.get_result()
    np.testing.assert_allclose(verts[0], want["vertices"], atol=1e-4)
    np.testing.assert_allclose(joints[0], want["joints"], atol=1e-4)
    b.fit_displacement(1)
    np.testing.assert_allclose(b.get_displacement()[0], want["disp_snapshots"][1], atol=2e-5)
    b.fit_displacement(3)
    assert np.mean(np.abs(b.get_displacement()[0] - want["disp_snapshots"][3]) < 2e-4) > 0.97
    b.close()
    scan.close()


@pytest.mark.parametrize("n_frames", [32, 256])
def test_kid_batches_equal_single_frames_and_oracle(kid_dev, kid, n_frames):
    """F = 32 (bf_mesh_batch32_kernel<12>) and F = 256 (GEMM + bf_mesh_epilogue_batch_kernel<12>): parameters bit for bit those of
    the frame fitted alone, vertices / joints within 2e-6 of the single-frame mesh (these kernels against the oracle forward at 3e-6:
    test_kid_forward_matches_oracle, n = 32 and 100)"""
    problems = [_problem(kid, frame=f, n_views=48) for f in range(n_frames)]
    b = _batch(kid_dev, problems)
    b.fit(100)
    params = b.get_params()
    verts, joints, full_pose, terms = b.get_result()
    b.close()
    for f in (0, 1, 17, n_frames - 1):
        s = _batch(kid_dev, [problems[f]])
        s.fit(100)
        v1, j1, fp1, _ = s.get_result()
        np.testing.assert_array_equal(params[f], s.get_params()[0], err_msg=f"frame {f}")
        np.testing.assert_array_equal(full_pose[f], fp1[0], err_msg=f"frame {f}")
        s.close()
        np.testing.assert_allclose(verts[f], v1[0], atol=2e-6, err_msg=f"frame {f}")
        np.testing.assert_allclose(joints[f], j1[0], atol=2e-6, err_msg=f"frame {f}")
    assert np.isfinite(verts).all() and np.isfinite(terms).all()


@pytest.fixture
def kid_assets(kid, smpl_model, gmm, monkeypatch):
    monkeypatch.setattr(assets, "_MODELS", {("smpl", "male"): smpl_model, ("smpl", "neutral"): smpl_model})
    monkeypatch.setattr(assets, "_GMM", {"gmm": gmm})
    monkeypatch.setattr(assets, "_DEVICE_MODELS", {})
    monkeypatch.setattr(assets, "_KID_TEMPLATE", {})
    assets.register_kid_template(S.make_kid_template(smpl_model))
    yield
    for d in list(assets._DEVICE_MODELS.values()):
        d.close()


def test_dropin_kid_smpl_smplify_and_bodyfitting(kid_assets, kid, tmp_path):
    """SMPL(age='kid') forward, SMPLify(age='kid') - __call__, fit_frames and stream ignore init_betas of width 10 or 11 and
    start from zeros[11] - and BodyFitting(options.age='kid') writing betas (1, 11)"""
    from types import SimpleNamespace
    from bodyfitting_amd.smpl import SMPL
    from bodyfitting_amd.smplify import SMPLify
    from bodyfitting_amd.body_fitting import BodyFitting
    smpl = SMPL(age="kid", gender="neutral")
    out = smpl(global_orient=np.zeros((1, 3)), body_pose=np.zeros((1, 69)), betas=np.eye(11, dtype=np.float32)[10:11])
    t = S.make_kid_template(kid).astype(np.float64)        # (same synthetic template: it depends on the adult template only)
    np.testing.assert_allclose(out.vertices[0], (t - t.mean(0)).astype(np.float32), atol=3e-6)

    prob = _problem(kid, frame=2, n_views=8)
    fitter = SMPLify(age="kid", gender="male", num_iters=20)
    assert fitter._dev.n_betas == 11
    ref = _batch(fitter._dev, [prob])
    ref.fit(20)
    want = ref.get_params()[0]
    ref.close()
    kps = prob["keypoints"]
    for width in (10, 11):
        junk = np.full((1, width), 0.7, np.float32)                    # ignored: kid fits start from zeros (smplify.py:115)
        res = fitter((junk, prob["init_pose"]), prob["c2ws"], prob["Ks"], kps, use_frames=list(range(8)))
        assert res["betas"].shape == (11,)
        np.testing.assert_array_equal(res["betas"], want[73:84])
        fr = fitter.fit_frames(junk, prob["init_pose"], np.stack(prob["c2ws"])[None], np.stack(prob["Ks"])[None],
                               N.pack_problem([prob])[2], n_use_frames=[8], num_iters=20)[0]
        np.testing.assert_array_equal(fr["betas"], want[73:84])
    streamed = list(fitter.stream([((np.zeros((1, 10)), prob["init_pose"]), kps)] * 2, prob["c2ws"], prob["Ks"]))
    for r in streamed:
        np.testing.assert_array_equal(r["betas"], want[73:84])
    with pytest.raises(ValueError):
        fitter((np.zeros((1, 7)), prob["init_pose"]), prob["c2ws"], prob["Ks"], kps, use_frames=list(range(8)))
    fitter.close()

    opts = SimpleNamespace(age="kid", smpl_type="smpl", num_iters=20)
    bf = BodyFitting(opts)
    res = bf(None, prob["c2ws"], prob["Ks"], kps, gender="male", use_frames=list(range(8)), output_folder=str(tmp_path),
             net_output=(np.zeros((1, 10), np.float32), prob["init_pose"]))
    saved = np.load(tmp_path / "smpl_parameter.npy", allow_pickle=True).item()
    assert np.asarray(saved["betas"]).reshape(1, -1).shape == (1, 11)
    np.testing.assert_array_equal(np.asarray(saved["betas"]).reshape(-1), want[73:84])
    assert res["betas"].shape == (11,)
