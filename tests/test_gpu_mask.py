"""HIP silhouette loss (loss.py:85-130) through the C ABI."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from bodyfitting_amd import native as N
from bodyfitting_amd import synthetic as S
from oracle.contour_oracle import border_pixels_rowmajor_all as extract_contours      # what the goldens were made with
from oracle import smplify_oracle as O
from test_mask_oracle import MASK_FRAMES, mask_inputs

pytestmark = pytest.mark.gpu
PARAMS = ("global_transl", "scale", "pose", "betas", "global_orient")
# The silhouette loss is discontinuous (nearest-vertex choices, 1 <-> 10 weights, the inside filter) and ~10x the keypoint loss, so the
# loop amplifies round-off.  How much is MEASURED on the reference itself (tests/golden/sens_mask_fit_8view_30it.npz: the imported
# reference with 8 intra-op threads instead of 1, and with the initial pose moved by one float32 ulp): it ends 3.9e-4 from itself after
# the first silhouette iteration and 4.9e-2 after 30.  The bands below are K x the largest drift under ten such perturbations (tests/ref_drift.py), never below 1e-4.
import ref_drift as RD


def _bands():
    base, sens = load_golden("mask_fit_8view_30it.npz"), load_golden("sens_mask_fit_8view_30it.npz")
    per_it = {k: RD.band(base, sens, [f"it{k}_{n}" for n in PARAMS]) for k in (12, 20, 30)}
    return base, sens, per_it, RD.band(base, sens, ["joints"])


def _batch(dev_model, prob):
    c2w, K, kp, ndiv, betas, pose = N.pack_problem([prob])
    b = N.FrameBatch(dev_model, 1, c2w.shape[1])
    b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose)
    masks = np.array(prob["masks"])[None]
    contours = [extract_contours(np.array(prob["masks"]) > 128)]
    b.set_masks(masks, [prob["use_frames"].index(f) for f in prob["mask_frames"]], contours)
    return b


def test_mask_loss_value_and_gradient(dev_model, smpl_model):
    """bf_batch_mask_loss in both distance forms: mask_cdist_form = 0 (exact (a-b)^2) vs the fp64 oracle, and the default
    (torch.cdist's expanded fp32 form, loss.py:108) vs the fp32 oracle evaluating torch.cdist literally and vs the
    golden of the imported reference"""
    g = load_golden("mask_loss_f0.npz")
    prob, contours, masks, w2cs, Ks = mask_inputs(smpl_model, torch.float64)
    b = _batch(dev_model, prob)
    params = {"global_transl": g["transl"], "scale": np.array([float(g["scale"])]), "pose": prob["init_pose"][0, 3:],
              "betas": prob["init_betas"][0], "global_orient": prob["init_pose"][0, :3]}
    b.set_params(N.pack_params(params)[None])
    loss, dv = b.mask_loss(N.make_hyper(mask_cdist_form=0))
    # same vertices on the oracle side (fp64 forward of the same parameters)
    m = O.to_torch_model(smpl_model, torch.float64)
    out = O.smpl_forward(m, torch.tensor(prob["init_betas"], dtype=torch.float64), torch.tensor(prob["init_pose"][:, :3], dtype=torch.float64),
                         torch.tensor(prob["init_pose"][:, 3:], dtype=torch.float64))
    verts = ((out["vertices"][0] + torch.tensor(g["transl"], dtype=torch.float64)) * float(g["scale"]) * 0.3).detach().requires_grad_(True)
    want = O.multview_mask_loss(contours, masks, verts, w2cs, Ks, imsize=512)
    want.backward()
    assert float(loss[0]) == pytest.approx(float(want), rel=2e-5)
    gw = verts.grad.numpy()
    assert np.all(dv[0].reshape(-1, 3)[np.arange(6890) % 4 != 0] == 0)          # only every 4th vertex (loss.py:99)
    err = np.abs(dv[0] - gw)
    assert np.mean(err < 1e-4 * np.abs(gw).max()) > 0.998                        # (an argmin tie may flip a few)
    # the reference's own form (default): the golden of the imported reference, value and gradient
    # (the golden was evaluated on torch's fp32 vertices, these on the HIP forward's: ~1e-4 px apart, which moves a few of the
    #  nearest-vertex choices and 1 <-> 10 weights - each flipped weight is ~10 units of the loss = 5e-5 of it)
    loss_c, dv_c = b.mask_loss()
    assert float(loss_c[0]) == pytest.approx(float(g["loss"]), rel=2e-4)
    assert np.mean(np.abs(dv_c[0][::4] - g["grad_sampled"]) < 1e-4 * np.abs(gw).max()) > 0.985
    # and it is closer to the reference than the exact form is (that is the point of the option)
    assert np.abs(dv_c[0][::4] - g["grad_sampled"]).sum() < np.abs(dv[0][::4] - g["grad_sampled"]).sum()
    b.close()


def _end_state(dev_model, prob, params):
    """size-independent end-state metrics of a silhouette fit: the (unweighted) mask loss and the keypoint loss terms at
    `params`, evaluated by the HIP path with exact distances"""
    b = _batch(dev_model, prob)
    b.set_params(params[None])
    mask = float(b.mask_loss(N.make_hyper(mask_cdist_form=0))[0][0])
    terms, _ = b.loss_grad()
    b.close()
    return mask, terms[0]


def test_mask_fit_loop_against_the_reference(dev_model, smpl_model, gmm_bufs):
    """The use_mask=True loop (smplify.py:138-144,197-199), 30 iterations of which 19 carry 5 x the silhouette loss.
    Keypoint-only prefix: exact.  With the distances in the reference's own fp32 form the trajectory follows the golden of
    the imported reference far more closely than with exact distances; the objective stays discontinuous (nearest-vertex
    choice, 1 <-> 10 weights), so beyond the per-parameter tolerance the END STATE is asserted: silhouette loss, keypoint
    terms and joints after the 30 steps within a stated percentage of the reference's."""
    g = load_golden("mask_fit_8view_30it.npz")
    prob = S.make_problem(smpl_model, frame=0, n_views=8, mask_frames=MASK_FRAMES)
    b = _batch(dev_model, prob)
    l0 = b.mask_loss()[0][0]
    # the reference loop cut at the golden's snapshots: dense_after = 10 = 30 // 3 keeps the switch-on iteration of ONE call
    done, drift = 0, {}
    for k in (1, 11, 12, 20, 30):
        b.fit(k - done, N.make_hyper(dense_after=10))
        done = k
        got = N.split_params(b.get_params()[0])
        drift[k] = max(float(np.abs(got[n] - g[f"it{k}_{n}"]).max()) for n in PARAMS)
    print("mask loop, distances in the reference's fp32 form: max |param - reference| per snapshot =", drift)
    _, sens, bands, joints_band = _bands()
    print("bands = K x the reference's largest drift under ten perturbations (tests/ref_drift.py):", bands, "joints", joints_band)
    assert drift[1] < 1e-6 and drift[11] < 1e-5                 # keypoint-only prefix
    assert drift[12] < bands[12]                                # the first silhouette iteration: at most a near-tie flip away
    assert drift[20] < bands[20] and drift[30] < bands[30]      # afterwards the discontinuous objective amplifies single flips
    verts, joints, _, _ = b.get_result()
    np.testing.assert_allclose(joints[0], g["joints"], atol=joints_band)
    assert b.mask_loss()[0][0] < 0.7 * l0                    # the silhouette term really went down
    b.close()
    b = _batch(dev_model, prob)                              # one call of 30 == the five calls above, bit for bit
    b.fit(30)
    np.testing.assert_array_equal(N.pack_params(N.split_params(b.get_params()[0])), N.pack_params(got))
    b.close()
    # end state vs the reference's end state (parameters of the golden, evaluated by the same HIP kernels)
    ref_params = N.pack_params({n: g[f"it30_{n}"] for n in PARAMS})
    mask_ref, terms_ref = _end_state(dev_model, prob, ref_params)
    mask_got, terms_got = _end_state(dev_model, prob, N.pack_params(got))
    print("silhouette loss: initial", float(l0), "reference end state", mask_ref, "HIP end state", mask_got,
          "| keypoint terms: reference", terms_ref.tolist(), "HIP", terms_got.tolist())
    # 30 Adam steps do not converge this objective, so the end states are compared as what they are: both far below the initial loss,
    # and as far from each other as the reference's own perturbed runs end from the reference (K x that spread)
    ends = [_end_state(dev_model, prob, N.pack_params({n: sens[f"{v}_it30_{n}"] for n in PARAMS})) for v in RD.VARIANTS]
    mask_spread = max(abs(e[0] - mask_ref) for e in ends) / mask_ref
    terms_spread = max(abs(float(e[1].sum()) - float(terms_ref.sum())) for e in ends) / float(terms_ref.sum())
    print("the reference's own end states:", [(e[0], e[1].tolist()) for e in ends], "relative spread", mask_spread, terms_spread)
    assert mask_ref < 0.7 * float(l0) and mask_got < 0.7 * float(l0)
    assert mask_got == pytest.approx(mask_ref, rel=max(0.02, RD.K * mask_spread))
    assert float(terms_got.sum()) == pytest.approx(float(terms_ref.sum()), rel=max(0.02, RD.K * terms_spread))
    mask_band, terms_band = max(0.02, RD.K * mask_spread), max(0.02, RD.K * terms_spread)
    # exact distances: a chosen deviation that drifts from the reference (documented in DESIGN.md), same quality of fit
    b = _batch(dev_model, prob)
    b.fit(30, N.make_hyper(mask_cdist_form=0))
    got_x = N.split_params(b.get_params()[0])
    b.close()
    mask_x, terms_x = _end_state(dev_model, prob, N.pack_params(got_x))
    print("exact distances: end state", mask_x, terms_x.tolist())
    assert mask_x == pytest.approx(mask_ref, rel=mask_band) and float(terms_x.sum()) == pytest.approx(float(terms_ref.sum()), rel=terms_band)
    # keypoint-only prefix is exact: 11 steps == golden
    c2w, K, kp, ndiv, betas, pose = N.pack_problem([prob])
    p = N.FrameBatch(dev_model, 1, 8)
    p.set_cameras(c2w, K); p.set_keypoints(kp, ndiv); p.set_init(betas, pose)
    p.fit(11)
    got = N.split_params(p.get_params()[0])
    for n in PARAMS:
        np.testing.assert_allclose(got[n], g[f"it11_{n}"], rtol=0, atol=1e-4)
    p.close()


def _blobs(seed, shape):
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    m = ndimage.gaussian_filter(rng.normal(size=shape), 2.5) > 0.02
    m[shape[0] // 2:shape[0] // 2 + 3, 5:shape[1] - 9] = True        # a bar and a one-pixel-wide spur
    m[5, 10:30] = True
    return m


@pytest.mark.parametrize("shape", [(48, 64), (100, 37), (512, 512), (700, 1100)])
def test_device_contours_equal_border_following_oracle(shape):
    """bf_extract_contours (one wave per mask, bit planes in LDS; global planes for the 700 x 1100 case) returns the
    points of oracle/contour_oracle.extract_contour - Suzuki-Abe border following, longest external border -
    in the same order, repeated pixels included"""
    from bodyfitting_amd.contours import extract_contours as device_contours
    from oracle import contour_oracle as CO
    masks = np.stack([_blobs(s, shape) for s in range(3)] + [np.zeros(shape, bool)])
    masks[2, :, :] = False
    masks[2, 3:9, 4:12] = True; masks[2, 5:7, 6:10] = False; masks[2, 5, 7] = True     # box with a hole and an island in it
    masks[2, 0, 0] = masks[2, -1, -1] = True                                            # single pixels in the corners
    from bodyfitting_amd import _lib
    for select, name in ((_lib.CONTOUR_OPENCV_FIRST, "opencv_first"), (_lib.CONTOUR_RASTER_FIRST, "raster_first"), (_lib.CONTOUR_LONGEST, "longest")):
        got = device_contours(masks, select=select)
        for m, c in zip(masks, got):
            np.testing.assert_array_equal(c, CO.extract_contour(m, name), err_msg=name)
        assert len(got[3]) == 0 and len(got[0]) > 0
        # mask 2 = single pixels in two corners + a box with a hole and an island: three external borders
        want_len = {"opencv_first": 1, "raster_first": 1, "longest": 2 * (6 + 8) - 4}[name]
        assert len(got[2]) == want_len
        if name != "longest":
            assert got[2][0].tolist() == ([shape[1] - 1, shape[0] - 1] if name == "opencv_first" else [0, 0])


def test_two_component_mask_feeds_the_loss_the_border_the_reference_keeps(dev_model, smpl_model):
    """a silhouette with a second, smaller component further down the image: loss.py:80 keeps OpenCV's first listed contour,
    which is the border met LAST by the raster scan - here the small blob, not the body.  bf_batch_set_masks(contour_select)
    follows that by default and offers the other two readings; each equals passing that contour explicitly."""
    from bodyfitting_amd import _lib
    from bodyfitting_amd.contours import extract_contours as device_contours
    prob = S.make_problem(smpl_model, frame=0, n_views=8, mask_frames=MASK_FRAMES)
    c2w, K, kp, ndiv, betas, pose = N.pack_problem([prob])
    masks = np.array(prob["masks"])[None].copy()
    masks[:, :, 500:506, 20:30] = 255                                          # a 6 x 10 blob near the bottom-left corner
    view_index = [prob["use_frames"].index(f) for f in prob["mask_frames"]]
    losses = {}
    for select in (_lib.CONTOUR_OPENCV_FIRST, _lib.CONTOUR_RASTER_FIRST, _lib.CONTOUR_LONGEST):
        out = []
        for contours in (None, [device_contours(masks[0] > 128, select=select)]):
            b = N.FrameBatch(dev_model, 1, c2w.shape[1])
            b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose)
            b.set_masks(masks, view_index, contours, contour_select=select)
            out.append(b.mask_loss())
            b.close()
        np.testing.assert_array_equal(out[0][0], out[1][0])
        np.testing.assert_array_equal(out[0][1], out[1][1])
        losses[select] = float(out[0][0][0])
    first = device_contours(masks[0] > 128, select=_lib.CONTOUR_OPENCV_FIRST)
    assert all(len(c) == 2 * (6 + 10) - 4 for c in first)                       # the blob's rim: that is what the reference would fit to
    assert losses[_lib.CONTOUR_RASTER_FIRST] == losses[_lib.CONTOUR_LONGEST] != losses[_lib.CONTOUR_OPENCV_FIRST]


def test_set_masks_extracts_the_contours_itself(dev_model, smpl_model):
    """bf_batch_set_masks with contour_count == NULL: same loss and gradient, bit for bit, as with the contours
    of bf_extract_contours passed in explicitly"""
    from bodyfitting_amd.contours import extract_contours as device_contours
    prob = S.make_problem(smpl_model, frame=0, n_views=8, mask_frames=MASK_FRAMES)
    c2w, K, kp, ndiv, betas, pose = N.pack_problem([prob])
    masks = np.array(prob["masks"])[None]
    view_index = [prob["use_frames"].index(f) for f in prob["mask_frames"]]
    out = []
    for contours in (None, [device_contours(masks[0] > 128)]):
        b = N.FrameBatch(dev_model, 1, c2w.shape[1])
        b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose)
        b.set_masks(masks, view_index, contours)
        out.append(b.mask_loss())
        b.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert np.isfinite(out[0][0]).all() and out[0][0][0] > 0


def test_border_longer_than_the_first_slab_inside_a_fit(dev_model, smpl_model):
    """A comb: its outer border has far more than 4 (H + W) points, so the contour kernel's first slab is too short and the
    deferred second half of bf_batch_set_masks (which runs in the MIDDLE of the fit, under the resident fit launch, where nothing
    may be freed) has to follow the border again with room for it.  Same loss, gradient and fitted parameters, bit for bit, as
    with the contours handed over by the caller."""
    from bodyfitting_amd import _lib
    from bodyfitting_amd.contours import extract_contours as device_contours
    prob = S.make_problem(smpl_model, frame=0, n_views=8, mask_frames=MASK_FRAMES)
    c2w, K, kp, ndiv, betas, pose = N.pack_problem([prob])
    masks = np.array(prob["masks"])[None].copy()
    H, W = masks.shape[-2:]
    comb = np.zeros((H, W), np.uint8)
    comb[H // 8: 7 * H // 8, W // 8: 7 * W // 8: 2] = 255          # teeth, one pixel wide, every other column
    comb[7 * H // 8 - 2: 7 * H // 8, W // 8: 7 * W // 8] = 255      # the back of the comb joins them: one component
    masks[0, 1] = comb
    view_index = [prob["use_frames"].index(f) for f in prob["mask_frames"]]
    given = [device_contours(masks[0] > 128)]
    assert len(given[0][1]) > 4 * (H + W)
    out = []
    for contours in (None, given, None):
        b = N.FrameBatch(dev_model, 1, c2w.shape[1])
        b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose)
        b.set_masks(masks, view_index, contours)
        if len(out) < 2:
            loss, dv = b.mask_loss()
        b.fit(9, N.make_hyper(dense_after=3))                         # (the border is read from iteration 5 on)
        out.append((loss, dv, b.get_params().copy()))
        # a second frame's masks on the same batch: the outgrown buffers are retired, not leaked or reused
        b.set_masks(np.array(prob["masks"])[None], view_index, None)
        b.fit(9, N.make_hyper(dense_after=3), flags=_lib.FIT_RESET | _lib.FIT_FETCH)
        assert np.isfinite(b.get_params()).all()
        b.close()
    for k in range(3):
        np.testing.assert_array_equal(out[0][k], out[1][k])
    np.testing.assert_array_equal(out[0][2], out[2][2])


def test_two_frames_device_contours_match_single_frames(dev_model, smpl_model):
    """F = 2 with different silhouettes, contours extracted on the device for all F x M masks in one launch:
    each frame's loss and gradient are bit for bit those of the frame alone"""
    probs = [S.make_problem(smpl_model, frame=f, n_views=8, mask_frames=MASK_FRAMES) for f in (0, 1)]
    c2w, K, kp, ndiv, betas, pose = N.pack_problem(probs)
    masks = np.stack([np.array(p["masks"]) for p in probs])
    view_index = [probs[0]["use_frames"].index(f) for f in MASK_FRAMES]
    b = N.FrameBatch(dev_model, 2, 8)
    b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose); b.set_masks(masks, view_index, None)
    loss2, dv2 = b.mask_loss()
    b.close()
    for i in range(2):
        b1 = N.FrameBatch(dev_model, 1, 8)
        b1.set_cameras(c2w[i:i + 1], K[i:i + 1]); b1.set_keypoints(kp[i:i + 1], ndiv[i:i + 1]); b1.set_init(betas[i:i + 1], pose[i:i + 1])
        b1.set_masks(masks[i:i + 1], view_index, None)
        loss1, dv1 = b1.mask_loss()
        b1.close()
        np.testing.assert_array_equal(loss2[i], loss1[0])
        np.testing.assert_array_equal(dv2[i], dv1[0])
    assert loss2[0] != loss2[1]


def test_sixteen_frames_with_masks_take_the_batched_mesh_path(dev_model, smpl_model):
    """>= 16 frames: the dense schedule's forward mesh is the fp32-MFMA pose-blend GEMM + batched epilogue (the sampled vertices are
    then projected by bf_mask_project_kernel, not inside the mesh pass) - the first silhouette iteration of every frame agrees
    with the frame fitted alone"""
    probs = [S.make_problem(smpl_model, frame=f % 2, n_views=8, mask_frames=MASK_FRAMES) for f in range(17)]
    c2w, K, kp, ndiv, betas, pose = N.pack_problem(probs)
    masks = np.stack([np.array(p["masks"]) for p in probs])
    view_index = [probs[0]["use_frames"].index(f) for f in MASK_FRAMES]
    b = N.FrameBatch(dev_model, 17, 8)
    b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose); b.set_masks(masks, view_index, None)
    b.fit(12, N.make_hyper(dense_after=10))
    together = b.get_params()
    b.close()
    for i in (0, 1, 16):
        b1 = N.FrameBatch(dev_model, 1, 8)
        b1.set_cameras(c2w[i:i + 1], K[i:i + 1]); b1.set_keypoints(kp[i:i + 1], ndiv[i:i + 1]); b1.set_init(betas[i:i + 1], pose[i:i + 1])
        b1.set_masks(masks[i:i + 1], view_index, None)
        b1.fit(12, N.make_hyper(dense_after=10))
        np.testing.assert_allclose(together[i], b1.get_params()[0], atol=2e-3)      # (one iteration of a discontinuous loss on 2e-6-different meshes)
        b1.close()
    np.testing.assert_array_equal(together[0], together[16])                        # same frame, same batch: same bits


def test_staged_masks_equal_masks_set_between_the_fits(dev_model, smpl_model):
    """bf_batch_stage_masks: the next frame's silhouettes go up and are border-followed while the previous frame's fit is still in
    flight (no wait for the device in between), two arenas changing places - every frame's fit equals, bit for bit, the one with
    bf_batch_set_masks called after the previous result was read.  One of the frames is the comb whose border outgrows the slab
    (the arena is regrown inside that fit and the other arena catches up when it is next staged into)."""
    from bodyfitting_amd import _lib
    probs = [S.make_problem(smpl_model, frame=f, n_views=8, mask_frames=MASK_FRAMES) for f in (0, 1, 2, 0, 1)]
    view_index = [probs[0]["use_frames"].index(f) for f in MASK_FRAMES]
    frames = []
    for i, p in enumerate(probs):
        c2w, K, kp, ndiv, betas, pose = N.pack_problem([p])
        masks = np.array(p["masks"])[None].copy()
        if i == 2:
            H, W = masks.shape[-2:]
            comb = np.zeros((H, W), np.uint8)
            comb[H // 8: 7 * H // 8, W // 8: 7 * W // 8: 2] = 255
            comb[7 * H // 8 - 2: 7 * H // 8, W // 8: 7 * W // 8] = 255
            masks[0, 1] = comb
        frames.append((kp, ndiv, betas, pose, masks))
    hyper = N.make_hyper(dense_after=3)
    flags = _lib.FIT_RESET | _lib.FIT_FETCH

    def run(staged):
        b = N.FrameBatch(dev_model, 1, 8)
        b.set_cameras(c2w, K)
        out = []
        for i, (kp, ndiv, betas, pose, masks) in enumerate(frames):
            if i == 0 or not staged:
                if i:
                    out.append(b.get_params().copy())
                b.set_masks(masks, view_index, None)
            else:
                b.stage_masks(masks, view_index)                 # (frame i - 1's fit is in flight)
                out.append(b.get_params().copy())
            b.stage_inputs(kp, ndiv, betas, pose)
            b.fit(9, hyper, flags)
        out.append(b.get_params().copy())
        b.close()
        return out
    plain, staged = run(False), run(True)
    for a, c in zip(plain, staged):
        np.testing.assert_array_equal(a, c)
    assert not np.array_equal(plain[0], plain[1])


def test_contour_gradient_sums_equal_the_ordered_walk(dev_model, smpl_model):
    """Round 5: inside a fit the contour scan adds every contour point's pull onto its nearest vertex as a 64-bit fixed-point number
    (atomic adds, exact sums) and the reverse mesh pass maps the sums back through the projection - no gather launch
    (bodyfit.h: bf_mask_fold_set).  The sums are exact, the ordered float32 walk of rounds 2-4 rounds after every addition: after a
    few iterations with the silhouette loss on the two paths agree to float32 round-off, the fixed-point path is reproducible bit for
    bit (an atomic's arrival order must not show), whatever else is in the batch."""
    from bodyfitting_amd import _lib
    probs = [S.make_problem(smpl_model, frame=f, n_views=8, mask_frames=MASK_FRAMES) for f in (0, 1, 2)]
    view_index = [probs[0]["use_frames"].index(f) for f in MASK_FRAMES]
    hyper = N.make_hyper(dense_after=2)

    def run(which, mode, iters=8, masks=True):
        before = N.set_mask_fold(mode)
        try:
            c2w, K, kp, ndiv, betas, pose = N.pack_problem([probs[i] for i in which])
            b = N.FrameBatch(dev_model, len(which), 8)
            b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose)
            if masks:
                b.set_masks(np.array([probs[i]["masks"] for i in which]), view_index, None)
            b.fit(iters, hyper)
            out = b.get_params().copy()
            b.close()
            return out
        finally:
            N.set_mask_fold(before)
    assert N.set_mask_fold("sums") in ("sums", "gather")
    # the first step that sees the silhouette gradient (Adam then turns round-off on a near-zero gradient into +-lr steps: later
    # iterations of the two paths drift apart the way the reference drifts from itself, tests/ref_drift.py)
    first = hyper.dense_after + 2 if hasattr(hyper, "dense_after") else 4
    a, w, none = run([0, 1, 2], "sums", first), run([0, 1, 2], "gather", first), run([0, 1, 2], "sums", first, masks=False)
    assert np.abs(a - none).max() > 1e-3                    # the silhouette term moves the step ...
    np.testing.assert_allclose(a, w, rtol=0, atol=2e-6)     # ... and both paths make the same one
    sums, again = run([0, 1, 2], "sums"), run([0, 1, 2], "sums")
    np.testing.assert_array_equal(sums, again)
    twice = run([0, 1, 0], "sums")
    np.testing.assert_array_equal(twice[0], twice[2])      # the same frame twice in a batch: the same bits
    np.testing.assert_array_equal(twice[:2], sums[:2])     # ... and a frame's bits do not depend on its neighbours
    with pytest.raises(ValueError):
        N.set_mask_fold(7)


def test_stage_masks_refuses_what_it_cannot_take(dev_model, smpl_model):
    from bodyfitting_amd._lib import BodyfitError
    prob = S.make_problem(smpl_model, frame=0, n_views=8, mask_frames=MASK_FRAMES)
    c2w, K, kp, ndiv, betas, pose = N.pack_problem([prob])
    masks = np.array(prob["masks"])[None]
    view_index = [prob["use_frames"].index(f) for f in MASK_FRAMES]
    b = N.FrameBatch(dev_model, 1, 8)
    b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose)
    with pytest.raises(BodyfitError, match="first frame"):
        b.stage_masks(masks, view_index)                          # nothing attached yet
    b.set_masks(masks, view_index, None)
    with pytest.raises(BodyfitError, match="keep its views and shape"):
        b.stage_masks(masks[:, :, :-2], view_index)
    with pytest.raises(BodyfitError, match="keep its views and shape"):
        b.stage_masks(masks, view_index[::-1])
    b.stage_masks(masks, view_index)
    b.set_masks(masks, view_index, None)                          # (supersedes the staged set)
    b.fit(6, N.make_hyper(dense_after=3))
    assert np.isfinite(b.get_params()).all()
    b.close()


TWO_VIEWS = MASK_FRAMES[:2]


def _attached(dev_model, prob, masks, contours=None):
    """a one-frame, 8-view batch on `prob` with `masks` [1, 2, H, W] attached -> the batch, its view indices and its inputs"""
    c2w, K, kp, ndiv, betas, pose = N.pack_problem([prob])
    view_index = [prob["use_frames"].index(f) for f in TWO_VIEWS]
    b = N.FrameBatch(dev_model, 1, c2w.shape[1])
    b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose)
    b.set_masks(masks, view_index, contours)
    return b, view_index, (kp, ndiv, betas, pose)


def _fresh_fit(b, inputs, n_iters=6):
    from bodyfitting_amd import _lib
    b.stage_inputs(*inputs)
    b.fit(n_iters, N.make_hyper(dense_after=3), _lib.FIT_RESET | _lib.FIT_FETCH)
    return b.get_params().copy()


def test_global_planes_inside_a_batch(dev_model, smpl_model):
    """400 x 1056 masks: their bit planes take 3 * 400 * 33 * 4 = 158,400 bytes, past the 153,600 the contour kernel keeps in LDS, so
    the batch's own border following (attach and staging) runs on planes in global memory.  Loss and gradient equal, bit for bit,
    those with the contours of bf_extract_contours handed in; a second set staged under way gives the fit the bits it has with
    that set attached by bf_batch_set_masks."""
    from bodyfitting_amd.contours import extract_contours as device_contours
    shape = (400, 1056)
    first, second = ((np.stack([_blobs(s, shape) for s in seeds])[None] * 255).astype(np.uint8) for seeds in ((0, 1), (2, 3)))
    prob = S.make_problem(smpl_model, frame=0, n_views=8)
    out = []
    for contours in (None, [device_contours(first[0] > 128)]):
        b, _, _ = _attached(dev_model, prob, first, contours)
        out.append(b.mask_loss())
        b.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert np.isfinite(out[0][0]).all() and out[0][0][0] > 0
    fits = []
    for staged in (True, False):
        b, view_index, inputs = _attached(dev_model, prob, first)
        if staged:
            b.stage_masks(second, view_index)
        else:
            b.set_masks(second, view_index, None)
        fits.append(_fresh_fit(b, inputs))
        b.close()
    np.testing.assert_array_equal(fits[0], fits[1])
    b, _, inputs = _attached(dev_model, prob, first)
    assert not np.array_equal(_fresh_fit(b, inputs), fits[0])             # (the second set is what that fit saw)
    b.close()


def test_two_stagings_before_one_fit(dev_model, smpl_model):
    """stage A, stage B, fit: the second staging overwrites the arena that is not the active one, and the fit sees B - the bits of the
    run that attaches B with bf_batch_set_masks"""
    probs = [S.make_problem(smpl_model, frame=f, n_views=8, mask_frames=TWO_VIEWS) for f in (0, 1, 2)]
    m0, mA, mB = (np.array(p["masks"])[None] for p in probs)
    fits = []
    for staged in (True, False):
        b, view_index, inputs = _attached(dev_model, probs[0], m0)
        if staged:
            b.stage_masks(mA, view_index)
            b.stage_masks(mB, view_index)
        else:
            b.set_masks(mB, view_index, None)
        fits.append(_fresh_fit(b, inputs))
        b.close()
    np.testing.assert_array_equal(fits[0], fits[1])
    b, view_index, inputs = _attached(dev_model, probs[0], m0)
    b.stage_masks(mA, view_index)
    assert not np.array_equal(_fresh_fit(b, inputs), fits[0])             # (A alone gives another fit: B really replaced it)
    b.close()


def test_destroy_with_a_staged_arena_and_retired_blocks(dev_model, smpl_model):
    """the comb's border outgrows the slab inside the fit (outgrown blocks retired, not freed), then another set is staged and never
    fitted: closing the batch returns, and a fresh batch on the same model repeats the first one's bits"""
    prob = S.make_problem(smpl_model, frame=0, n_views=8, mask_frames=TWO_VIEWS)
    plain = np.array(prob["masks"])[None]
    masks = plain.copy()
    H, W = masks.shape[-2:]
    masks[0, 1] = 0
    masks[0, 1, H // 8: 7 * H // 8, W // 8: 7 * W // 8: 2] = 255          # the comb of the tests above
    masks[0, 1, 7 * H // 8 - 2: 7 * H // 8, W // 8: 7 * W // 8] = 255
    fits = []
    for leave_staged in (True, False):
        b, view_index, inputs = _attached(dev_model, prob, masks)
        fits.append(_fresh_fit(b, inputs, 9))                   # (the border is read from iteration 5 on)
        if leave_staged:
            b.stage_masks(plain, view_index)
        b.close()
    np.testing.assert_array_equal(fits[0], fits[1])
    assert np.isfinite(fits[0]).all()
