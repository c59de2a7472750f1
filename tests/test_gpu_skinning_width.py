"""Models with more than four bones per vertex on the MI355X, against the oracle run on the CPU here.

derive_tables (csrc/model_api.hip) sorts a model by its widest skinning row: MeshTab::v_nnz = 4 / 8, or 0 (dense: more than 8), and
FitTab::sel_nnz by the selector rows the keypoint loss reads (1..8, 0 = dense or none).  The default synthetic model has at most 4
bones per vertex, so every other test runs the 4-wide side of each branch; these run the others:

  variant        model                                          v_nnz  sel_nnz  fit instance
  smpl B8        SMPL, 5..8 bones per vertex                    8      8        table-driven
  smpl BD        SMPL, 9..12                                    0      0        table-driven
  smpl 4+1       SMPL, one non-selector vertex with 9           0      4        sized
  smpl 4+S       SMPL, one loss selector vertex with 6          8      6        table-driven
  kid B8         kid model (11 betas) of smpl B8                8      8        table-driven
  smplx 4/B8/BD  SMPL-X, default / 5..8 / 9..12                 4/8/0  0        (dense keypoint schedule)
  nv690 B8/BD    SMPL at 690 vertices, 5..8 / 9..12             8/0    5..8/0   table-driven

Each model fixture asserts its class (`width_class`, the host-side mirror of derive_tables) and its fit instance, so no variant
falls back to the 4-bone path unnoticed."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from bodyfitting_amd import native as N, synthetic as S
from oracle import smplify_oracle as O
from oracle.contour_oracle import border_pixels_rowmajor_all as extract_contours
import ref_drift as RD
from width_variants import Variants, quiet_vertex, smpl_problem as _smpl_problem          # (the table of variants, their class check and problems)

pytestmark = pytest.mark.gpu
PARAMS = ("global_transl", "scale", "pose", "betas", "global_orient")
MASK_FRAMES = [1, 3, 5, 7]
# the forward's dispatch boundaries (api.hip bf_launch_mesh): 1 frame (bf_mesh_kernel or the one-frame multi kernel, `pre` rows for
# v_nnz 4 / 8 and nb <= 10 / 12), 2..15 (bf_mesh_multi_kernel, 2 / 4 / 8 frames per workgroup), 16..64 (bf_mesh_batch32_kernel - v_nnz 4
# only - else the pose-blend GEMM), > 64 (GEMM + bf_mesh_epilogue_batch_kernel for v_nnz 4, bf_mesh_epilogue_kernel otherwise)
FORWARD_N = (1, 2, 8, 9, 15, 16, 17, 32, 33, 64, 65, 128, 129)


@pytest.fixture(scope="module")
def variants(gmm):
    v = Variants(gmm)
    yield v
    v.close()


def _batch(dev, problems):
    c2w, K, kp, ndiv, betas, pose = N.pack_problem(problems)
    b = N.FrameBatch(dev, len(problems), c2w.shape[1])
    b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose)
    return b


# ---- a. forward at every dispatch boundary ------------------------------------------------------------------------------------

def _smpl_inputs(nb, n=max(FORWARD_N)):
    rng = np.random.default_rng(29)
    betas = rng.normal(0, 0.7, (n, nb)).astype(np.float32)
    orient = rng.normal(0, 0.8, (n, 3)).astype(np.float32)
    pose = rng.normal(0, 0.3, (n, 69)).astype(np.float32)
    return betas, orient, pose


def _smpl_oracle(variants, name):
    key = ("fwd", name)
    if key not in variants.cache:
        model, dev = variants.get(name)
        betas, orient, pose = _smpl_inputs(dev.n_betas)
        t = lambda a: torch.tensor(a, dtype=torch.float64)          # noqa: E731
        ref = O.smpl_forward(O.to_torch_model(model, torch.float64), t(betas), t(orient), t(pose))
        variants.cache[key] = ((betas, orient, pose), {k: ref[k].numpy() for k in ("vertices", "joints", "joints_ori")})
    return variants.cache[key]


@pytest.mark.parametrize("n", FORWARD_N)
@pytest.mark.parametrize("name", ["smpl_B8", "smpl_BD", "smpl_4+1", "smpl_4+S", "kid_B8"])
def test_smpl_forward_every_frame_at_each_dispatch(variants, name, n):
    """bf_smpl_forward, every frame against the fp64 oracle at 3e-6.  B8 / 4+S (v_nnz 8): n = 1 the multi kernel's `pre` rows with 8
    entries (kid, nb = 11: the 12-direction `pre` instance), 2..15 the generic sparse loop over v_nzw, >= 16 the pose-blend GEMM +
    per-frame bf_mesh_epilogue_kernel (bf_mesh_batch32_kernel and the batched epilogue take v_nnz 4 only).  BD / 4+1 (v_nnz 0): the dense
    loop over MeshTab::lbs_weights below 16 frames, bf_mesh_epilogue_kernel's dense loop from 16 on"""
    model, dev = variants.get(name)
    (betas, orient, pose), ref = _smpl_oracle(variants, name)
    verts, joints, jori = dev.forward(betas[:n], orient[:n], pose[:n])
    np.testing.assert_allclose(verts, ref["vertices"][:n], rtol=0, atol=3e-6)
    np.testing.assert_allclose(joints, ref["joints"][:n], rtol=0, atol=3e-6)
    np.testing.assert_allclose(jori, ref["joints_ori"][:n], rtol=0, atol=3e-6)


def test_one_wide_vertex_leaves_the_others_as_they_were(variants, dev_model):
    """4+1: one vertex with 9 bones takes the whole mesh to the dense skinning loop; the other 6889 vertices are those of the 4-bone
    model within 2e-6 at every dispatch (their zero weights add exact zeros)"""
    _, dev = variants.get("smpl_4+1")
    (betas, orient, pose), _ = _smpl_oracle(variants, "smpl_4+1")
    v9 = quiet_vertex(S.make_model("smpl"))
    keep = np.arange(6890) != v9
    for n in FORWARD_N:
        a = dev.forward(betas[:n], orient[:n], pose[:n])[0][:, keep]
        b = dev_model.forward(betas[:n], orient[:n], pose[:n])[0][:, keep]
        print(f"4+1, {n} frames: the 6889 unchanged vertices {'are bit-equal to' if np.array_equal(a, b) else 'differ from'} the 4-bone model's"
              f" (max {float(np.abs(a - b).max()):.3g})")
        np.testing.assert_allclose(a, b, rtol=0, atol=2e-6, err_msg=f"n={n}")


def _smplx_params(n):
    rng = np.random.default_rng(31)
    p = {"global_transl": rng.normal(0, 0.03, (n, 3)), "scale": rng.uniform(0.9, 1.1, (n, 1)), "pose": rng.normal(0, 0.25, (n, 63)),
         "betas": rng.normal(0, 0.7, (n, 10)), "global_orient": rng.normal(0, 0.8, (n, 3)), "leye_pose": rng.normal(0, 0.1, (n, 3)),
         "reye_pose": rng.normal(0, 0.1, (n, 3)), "left_hand_pose": rng.normal(0, 0.5, (n, 6)), "right_hand_pose": rng.normal(0, 0.5, (n, 6))}
    return {k: v.astype(np.float32) for k, v in p.items()}


@pytest.mark.parametrize("n", FORWARD_N)
@pytest.mark.parametrize("name", ["smplx_4", "smplx_B8", "smplx_BD"])
def test_smplx_forward_every_frame_at_each_dispatch(variants, name, n):
    """bf_model_forward for SMPL-X (486 pose features: the multi kernel from one frame on; >= 16 frames the fp32-MFMA pose-blend GEMM
    with kpad = 520, then - 4 bones - bf_mesh_epilogue_batch_kernel with 55 joints, or - 8 / dense - bf_mesh_epilogue_kernel), every
    frame's vertices and 135 joints (landmarks included) against the fp64 oracle at 3e-6"""
    model, dev = variants.get(name)
    key = ("fwd", name)
    if key not in variants.cache:
        P = _smplx_params(max(FORWARD_N))
        t = lambda k: torch.tensor(P[k], dtype=torch.float64)          # noqa: E731
        ref = O.smplx_forward(O.to_torch_model(model, torch.float64), t("betas"), t("global_orient"), t("pose"), t("leye_pose"),
                              t("reye_pose"), t("left_hand_pose"), t("right_hand_pose"))
        packed = np.concatenate([P[k] for k in O.SMPLX_PARAMS], 1)          # (pack_params' order, one row per frame)
        variants.cache[key] = (packed, ref["vertices"].numpy(), ref["joints"].numpy())
    packed, rv, rj = variants.cache[key]
    verts, joints = dev.forward_packed(packed[:n])
    np.testing.assert_allclose(verts, rv[:n], rtol=0, atol=3e-6)
    np.testing.assert_allclose(joints, rj[:n], rtol=0, atol=3e-6)


# ---- b. loss and gradient ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["smpl_B8", "smpl_BD", "smpl_4+1", "smpl_4+S", "kid_B8"])
def test_smpl_loss_grad_matches_fp64_autograd(variants, name, gmm_bufs):
    """bf_loss_grad against O.loss_and_grad (fp64 autograd) at test_kid_loss_grad_matches_fp64_autograd's bands, at a non-trivial
    pose / betas / translation: the fit kernel's selector skinning and its reverse - the sized instance's 4-entry rows (4+1), the
    table-driven instance's sel_nzw rows of 5..8 (B8, 4+S) and its dense S.sel_w loop (BD)"""
    model, dev = variants.get(name)
    prob = _smpl_problem(name, model, frame=1, n_views=6)
    b = _batch(dev, [prob])
    rng = np.random.default_rng(5)
    nb = dev.n_betas
    params = {"global_transl": rng.normal(0, 0.03, 3), "scale": np.array([1.05]), "pose": rng.normal(0, 0.2, 69),
              "betas": rng.normal(0, 0.5, nb), "global_orient": np.array([0.1, 1.2, -0.05])}
    b.set_params(N.pack_params(params)[None])
    terms, grads = b.loss_grad()
    b.close()
    loss, _, g64, _, _ = O.loss_and_grad(model, gmm_bufs, prob, params)
    assert float(terms.sum()) == pytest.approx(loss, rel=2e-6)
    got = N.split_params(grads[0], 24, nb)
    for k in PARAMS:
        np.testing.assert_allclose(got[k], g64[k], atol=5e-6 * np.abs(g64[k]).max(), err_msg=k)


def _smplx_batch(dev, prob):
    c2w, K, kp, ndiv, betas, pose = N.pack_problem([prob])
    b = N.FrameBatch(dev, 1, c2w.shape[1])
    b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose)
    return b


@pytest.mark.parametrize("name", ["smplx_B8", "smplx_BD"])
def test_smplx_loss_grad_matches_fp64_autograd(variants, name, gmm_bufs):
    """SMPL-X's keypoint loss is the dense kernel: the forward keeps v_posed and the dense reverse pass (scan_kernels.hip) carries
    dL/dvertices back through the skinning - its sparse v_nzw rows with 8 entries (B8) and its dense s_w loop (BD, v_nnz 0).  Against
    O.smplx_loss_and_grad at test_loss_and_gradient_match_autograd's bands"""
    model, dev = variants.get(name)
    prob = S.make_problem_smplx(model, 0, 8)
    P = {"global_transl": np.array([0.01, -0.02, 0.015]), "scale": np.array([1.05]), "pose": prob["init_pose"][0, 3:66] + 0.1,
         "betas": np.linspace(-0.4, 0.4, 10), "global_orient": prob["init_pose"][0, :3], "leye_pose": np.array([0.02, -0.01, 0.03]),
         "reye_pose": np.array([-0.02, 0.01, 0.0]), "left_hand_pose": np.linspace(-0.3, 0.3, 6), "right_hand_pose": np.linspace(0.2, -0.2, 6)}
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    b = _smplx_batch(dev, prob)
    b.set_params(N.pack_params(P)[None])
    terms, grads = b.loss_grad()
    b.close()
    _, t64, g64, _, _, _ = O.smplx_loss_and_grad(model, gmm_bufs, prob, P)
    for i, n in enumerate(("reprojection_loss", "pose_prior_loss", "angle_prior_loss", "shape_prior_loss")):
        assert terms[0, i] == pytest.approx(t64[n], rel=3e-6), n
    got = N.split_params(grads[0])
    for k in O.SMPLX_PARAMS:
        np.testing.assert_allclose(got[k], g64[k], atol=1e-5 * np.abs(g64[k]).max(), err_msg=k)


# ---- c. fit loops ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["smpl_B8", "smpl_BD", "smpl_4+S", "smpl_4+1"])
def test_smpl_fit_matches_oracle_loop(variants, name, gmm_bufs):
    """1 frame x 48 views x 100 iterations against O.fit at iterations 1 / 2 / 10 / 50 / 100 and the final mesh, at 1e-4 (as
    test_kid_fit_matches_oracle_loop): the table-driven fit kernel with sel_nnz 5..8 (B8, 4+S) and 0 (BD: the dense S.sel_w loop),
    the sized instance beside a dense mesh (4+1); the final mesh through the 8-wide / dense single-frame forward"""
    model, dev = variants.get(name)
    prob = _smpl_problem(name, model, frame=0, n_views=48)
    want = O.fit(model, gmm_bufs, prob, 100, snapshots=(1, 2, 10, 50, 100))
    b = _batch(dev, [prob])
    done = 0
    for k in (1, 2, 10, 50, 100):
        b.fit(k - done)
        done = k
        got = N.split_params(b.get_params()[0], 24, dev.n_betas)
        for n in PARAMS:
            np.testing.assert_allclose(got[n], want["snapshots"][k][n], rtol=0, atol=1e-4, err_msg=f"it{k} {n}")
    verts, joints, _, _ = b.get_result()
    np.testing.assert_allclose(joints[0], want["joints"], atol=1e-4)
    np.testing.assert_allclose(verts[0], want["vertices"], atol=1e-4)
    b.close()


@pytest.mark.parametrize("name", ["smplx_B8", "smplx_BD"])
def test_smplx_fit_matches_oracle_loop(variants, name, gmm_bufs):
    """SMPL-X, 8 views x 40 iterations against O.fit_smplx at iterations 1 / 2 / 10 / 40, final joints and vertices at 1e-4 (as
    test_fit_matches_reference_golden): the dense keypoint schedule - mesh forward with v_posed, dense reverse pass, sub-models -
    on 8-wide and dense skinning"""
    model, dev = variants.get(name)
    prob = S.make_problem_smplx(model, frame=0, n_views=8)
    snaps = (1, 2, 10, 40)
    want = O.fit_smplx(model, gmm_bufs, prob, 40, snapshots=snaps)
    b = _smplx_batch(dev, prob)
    done = 0
    for k in snaps:
        b.fit(k - done)
        done = k
        got = N.split_params(b.get_params()[0])
        for n in O.SMPLX_PARAMS:
            np.testing.assert_allclose(got[n], want["snapshots"][k][n], rtol=0, atol=1e-4, err_msg=f"it{k} {n}")
    verts, joints, _, _ = b.get_result()
    np.testing.assert_allclose(joints[0], want["joints"], atol=1e-4)
    np.testing.assert_allclose(verts[0], want["vertices"], atol=1e-4)
    b.close()


# ---- d. dense losses ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["nv690_B8", "nv690_BD"])
def test_scan_and_displacement_at_nv690(variants, name, gmm_bufs):
    """use_mesh=True at 690 vertices, built and banded as test_kid_scan_and_displacement_at_nv690: 11 keypoint-only iterations and 19
    with the point-cloud loss against O.fit(scan=..., displacement=True) - parameters, vertices, joints 1e-4; SMPL+D first step 2e-5,
    three steps 97 % within 2e-4.  The scan iterations' reverse pass runs the dense skinning's sparse 8-wide rows / dense s_w loop"""
    model, dev = variants.get(name)
    prob, sv, sf = S.make_scan_problem(model, frame=0, n_views=8)
    want = O.fit(model, gmm_bufs, prob, 30, scan=(sv, sf), displacement=True, disp_snapshots=(1, 3))
    scan = N.Scan(sv, sf)
    b = _batch(dev, [prob])
    b.set_scans([scan])
    b.fit(30)
    got = N.split_params(b.get_params()[0])
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


def test_mask_fit_dense_skinning_against_oracle(variants, gmm_bufs):
    """SMPL BD with use_mask=True, 30 iterations, built and banded as test_kid_mask_fit_against_oracle: the keypoint-only prefix at
    1e-4, then K x the larger of the adult reference's own drift and this model's oracle drift under a one-ulp nudge of the initial
    pose and 4 intra-op threads (the discontinuous silhouette objective amplifies round-off).  The dense iterations run the v_posed
    forward and the reverse pass over dense skinning rows"""
    model, dev = variants.get("smpl_BD")
    prob = S.make_problem(model, frame=0, n_views=8, mask_frames=MASK_FRAMES)
    snaps = (11, 20, 30)
    want = O.fit(model, gmm_bufs, prob, 30, snapshots=snaps)
    own = {k: [] for k in snaps}
    ulp = dict(prob, init_pose=np.nextafter(prob["init_pose"], np.float32(np.inf)).astype(np.float32))
    threads = torch.get_num_threads()
    for variant in ("ulp", "threads4"):
        try:
            if variant == "threads4":
                torch.set_num_threads(4)
            alt = O.fit(model, gmm_bufs, ulp if variant == "ulp" else prob, 30, snapshots=snaps)
        finally:
            torch.set_num_threads(threads)
        for k in snaps:
            own[k].append(max(float(np.abs(alt["snapshots"][k][n] - want["snapshots"][k][n]).max()) for n in PARAMS))
    base, sens = load_golden("mask_fit_8view_30it.npz"), load_golden("sens_mask_fit_8view_30it.npz")
    adult_band = {k: RD.band(base, sens, [f"it{k}_{n}" for n in PARAMS]) for k in (20, 30)}
    b = _batch(dev, [prob])
    b.set_masks(np.array(prob["masks"])[None], [prob["use_frames"].index(f) for f in prob["mask_frames"]],
                [extract_contours(np.array(prob["masks"]) > 128)])
    done = 0
    for k in snaps:
        b.fit(k - done, N.make_hyper(dense_after=10))
        done = k
        got = N.split_params(b.get_params()[0])
        err = max(float(np.abs(got[n] - want["snapshots"][k][n]).max()) for n in PARAMS)
        if k == 11:
            assert err < 1e-4, err
            continue
        band = max(adult_band[k], RD.K * max(own[k]))
        print(f"BD mask loop it{k}: max |param - oracle| {err:.3g}, band {band:.3g};", RD.position(err, own[k]))
        assert err < band, (k, err, band)
    verts, _, _, _ = b.get_result()
    assert np.isfinite(verts).all()
    b.close()


def test_smplx_sub_model_loop_matches_the_full_model_loop(variants):
    """SMPL-X B8: the dense schedule's sub-models (derive_sub with nnz 8: the sampled-first and the keypoint-only one) against the full
    model, keypoint-only loop of 12 iterations at 2e-5 (as test_sub_model_loop_matches_the_full_model_loop)"""
    import os
    model, dev = variants.get("smplx_B8")
    prob = S.make_problem_smplx(model, frame=0, n_views=8)
    out = {}
    for flag, env in (("1", {"BF_DENSE_SUBMODEL": "1"}), ("kp0", {"BF_DENSE_SUBMODEL": "1", "BF_DENSE_SUBMODEL_KP": "0"}),
                      ("0", {"BF_DENSE_SUBMODEL": "0"})):
        os.environ.update(env)
        try:
            b = _smplx_batch(dev, prob)
            b.fit(12)
            out[flag] = b.get_params().copy()
            b.close()
        finally:
            for k in env:
                del os.environ[k]
    assert np.isfinite(out["0"]).all() and np.abs(out["0"]).sum() > 1
    np.testing.assert_allclose(out["1"], out["0"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(out["kp0"], out["0"], rtol=0, atol=2e-5)
    assert np.abs(out["1"] - out["kp0"]).max() > 0          # (another summation order: the switch really selects another sub-model)


# ---- e. batches --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_frames", [32, 129])
@pytest.mark.parametrize("name", ["smpl_B8", "smpl_BD"])
def test_batches_equal_single_frames(variants, name, n_frames):
    """F = 32 and F = 129 frames fitted together: the final mesh is the pose-blend GEMM + per-frame bf_mesh_epilogue_kernel (v_nnz 8 /
    0 never take bf_mesh_batch32_kernel or the batched epilogue).  Parameters bit for bit those of the frame fitted alone, vertices /
    joints within 2e-6 of the single-frame mesh (as test_cfg4_shard_equals_single_frames_and_goldens)"""
    model, dev = variants.get(name)
    problems = [_smpl_problem(name, model, frame=f, n_views=48) for f in range(n_frames)]
    b = _batch(dev, problems)
    b.fit(100)
    params = b.get_params()
    verts, joints, full_pose, terms = b.get_result()
    b.close()
    for f in (0, 1, 17, n_frames - 1):
        s = _batch(dev, [problems[f]])
        s.fit(100)
        v1, j1, fp1, _ = s.get_result()
        np.testing.assert_array_equal(params[f], s.get_params()[0], err_msg=f"frame {f}")
        np.testing.assert_array_equal(full_pose[f], fp1[0], err_msg=f"frame {f}")
        s.close()
        np.testing.assert_allclose(verts[f], v1[0], atol=2e-6, err_msg=f"frame {f}")
        np.testing.assert_allclose(joints[f], j1[0], atol=2e-6, err_msg=f"frame {f}")
    assert np.isfinite(verts).all() and np.isfinite(terms).all()


def test_seventeen_frames_with_masks_on_dense_skinning(variants):
    """SMPL BD, 17 frames with silhouettes: the dense iterations' v_posed forward always takes the GEMM + per-frame
    bf_mesh_epilogue_kernel, here with the dense skinning loop, and the dense reverse pass over it.  As
    test_sixteen_frames_with_masks_take_the_batched_mesh_path: the first silhouette iteration of a frame agrees with the frame fitted
    alone (2e-3: one step of a discontinuous loss on 2e-6-different meshes), the same frame twice in a batch gives the same bits"""
    model, dev = variants.get("smpl_BD")
    probs = [S.make_problem(model, frame=f % 2, n_views=8, mask_frames=MASK_FRAMES) for f in range(17)]
    c2w, K, kp, ndiv, betas, pose = N.pack_problem(probs)
    masks = np.stack([np.array(p["masks"]) for p in probs])
    view_index = [probs[0]["use_frames"].index(f) for f in MASK_FRAMES]
    b = N.FrameBatch(dev, 17, 8)
    b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose); b.set_masks(masks, view_index, None)
    b.fit(12, N.make_hyper(dense_after=10))
    together = b.get_params()
    b.close()
    assert np.isfinite(together).all()
    for i in (0, 1, 16):
        b1 = N.FrameBatch(dev, 1, 8)
        b1.set_cameras(c2w[i:i + 1], K[i:i + 1]); b1.set_keypoints(kp[i:i + 1], ndiv[i:i + 1]); b1.set_init(betas[i:i + 1], pose[i:i + 1])
        b1.set_masks(masks[i:i + 1], view_index, None)
        b1.fit(12, N.make_hyper(dense_after=10))
        np.testing.assert_allclose(together[i], b1.get_params()[0], atol=2e-3)
        b1.close()
    np.testing.assert_array_equal(together[0], together[16])
