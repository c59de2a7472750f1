"""Parity of the HIP path (through the C ABI) against the oracle and the reference goldens.

Tolerances: the north star asks for fitted beta / theta / transl within 1e-4 abs of the reference
PyTorch CPU path after 100 iterations; stage-level quantities are held tighter (fp32 round-off).
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from bodyfitting_amd import synthetic as S
from bodyfitting_amd import native as N
from oracle import analytic as A
from oracle import smplify_oracle as O

pytestmark = pytest.mark.gpu
PARAMS = ("global_transl", "scale", "pose", "betas", "global_orient")
FIT_TOL = 1e-4


def _batch(dev_model, problems):
    c2w, K, kp, ndiv, betas, pose = N.pack_problem(problems)
    b = N.FrameBatch(dev_model, len(problems), c2w.shape[1])
    b.set_cameras(c2w, K)
    b.set_keypoints(kp, ndiv)
    b.set_init(betas, pose)
    return b


def test_smpl_forward_matches_oracle(dev_model, smpl_model):
    """models.smpl.SMPL.forward: vertices[6890,3], joints[49,3], joints_ori[45,3] (fp32 round-off)."""
    rng = np.random.default_rng(3)
    n = 3
    betas = rng.normal(0, 0.7, (n, 10)).astype(np.float32)
    orient = rng.normal(0, 0.8, (n, 3)).astype(np.float32)
    pose = rng.normal(0, 0.3, (n, 69)).astype(np.float32)
    pose[1] = 0.0
    orient[1] = 0.0                      # identity pose: the Rodrigues singular point
    verts, joints, jori = dev_model.forward(betas, orient, pose)
    m = O.to_torch_model(smpl_model, torch.float64)
    ref = O.smpl_forward(m, torch.tensor(betas, dtype=torch.float64), torch.tensor(orient, dtype=torch.float64),
                         torch.tensor(pose, dtype=torch.float64))
    np.testing.assert_allclose(verts, ref["vertices"].numpy(), atol=3e-6)
    np.testing.assert_allclose(joints, ref["joints"].numpy(), atol=3e-6)
    np.testing.assert_allclose(jori, ref["joints_ori"].numpy(), atol=3e-6)
    # known answer: identity pose => v_template + S beta
    shaped = smpl_model["v_template"] + smpl_model["shapedirs"] @ betas[1]
    np.testing.assert_allclose(verts[1], shaped, atol=2e-6)


def test_loss_terms_and_gradient(dev_model, smpl_model, gmm_bufs):
    """bf_loss_grad vs the reference's loss dict / autograd gradient (golden) and the fp64 oracle."""
    g = load_golden("loss_terms_f0.npz")
    prob = S.make_problem(smpl_model, frame=0, n_views=48)
    b = _batch(dev_model, [prob])
    params = {k: g[f"param_{k}"] for k in PARAMS}
    b.set_params(N.pack_params(params)[None])
    terms, grads = b.loss_grad()
    names = ("reprojection_loss", "pose_prior_loss", "angle_prior_loss", "shape_prior_loss")
    for i, n in enumerate(names):
        assert terms[0, i] == pytest.approx(float(g[f"term_{n}"]), rel=2e-6)
    got = N.split_params(grads[0])
    _, _, g64, _, _ = O.loss_and_grad(smpl_model, gmm_bufs, prob, {k: v.astype(np.float64) for k, v in params.items()})
    for k in PARAMS:
        scale = np.abs(g64[k]).max()
        np.testing.assert_allclose(got[k], g64[k], atol=5e-6 * scale, err_msg=k)
        np.testing.assert_allclose(got[k], g[f"grad_{k}"], atol=5e-6 * scale, err_msg=k)
    b.close()


def test_gradient_at_zero_pose(dev_model, smpl_model, gmm_bufs):
    """theta = 0 sits on the Rodrigues singular point (angle = ||1e-8||)."""
    prob = S.make_problem(smpl_model, frame=2, n_views=5, missing_views=(1, 3))
    b = _batch(dev_model, [prob])
    params = {"global_transl": np.array([0.02, -0.01, 0.03]), "scale": np.array([1.1]), "pose": np.zeros(69),
              "betas": np.linspace(-0.5, 0.5, 10), "global_orient": np.zeros(3)}
    b.set_params(N.pack_params(params)[None])
    terms, grads = b.loss_grad()
    loss, t64, g64, _, _ = O.loss_and_grad(smpl_model, gmm_bufs, prob, params)
    assert float(terms.sum()) == pytest.approx(loss, rel=2e-6)
    got = N.split_params(grads[0])
    for k in PARAMS:
        np.testing.assert_allclose(got[k], g64[k], atol=1e-5 * np.abs(g64[k]).max(), err_msg=k)
    b.close()


@pytest.mark.parametrize("frame", [0, 1, 2, 3])
def test_cfg2_fit_matches_reference(dev_model, smpl_model, frame):
    """BASELINE config 2 (1 frame, 48 views, 100 iters): fitted parameters vs the reference goldens."""
    g = load_golden(f"cfg2_48view_100it_f{frame}.npz")
    prob = S.make_problem(smpl_model, frame=frame, n_views=48)
    b = _batch(dev_model, [prob])
    done = 0
    for k in (1, 2, 10, 50, 100):
        b.fit(k - done)
        done = k
        got = N.split_params(b.get_params()[0])
        for n in PARAMS:
            np.testing.assert_allclose(got[n], g[f"it{k}_{n}"], rtol=0, atol=FIT_TOL, err_msg=f"it{k} {n}")
    verts, joints, full_pose, terms = b.get_result()
    np.testing.assert_allclose(joints[0], g["joints"], atol=FIT_TOL)
    np.testing.assert_allclose(verts[0][::53], g["vertices_sample"], atol=FIT_TOL)
    np.testing.assert_allclose(full_pose[0], g["full_pose"], atol=FIT_TOL)
    p = N.split_params(b.get_params()[0])
    # rtn_dict's global_transl = t * s (smplify.py:223), a field of the result: 1e-4 like everything else on the well-conditioned
    # frames.  Frame 3's translation is the ill-conditioned one of the four: the imported reference itself ends between 1.6e-5 and
    # 1.9e-4 from its own answer in this field under the ten perturbations of tests/ref_drift.py (2 / 4 / 8 threads, one-ulp nudges of
    # the initial pose, the keypoints, the cameras; at most 1.5e-5 / 3.7e-5 / 1.1e-6 on frames 0 / 1 / 2) -
    # tests/golden/sens_cfg2_48view_100it.npz, oracle/gen_golden.py: sensitivity_cfg2_goldens - and the band for that frame is the
    # one of the other round-off-amplifying loops: K x the reference's own largest drift
    band = FIT_TOL
    if frame == 3:
        import ref_drift as RD
        sens = load_golden("sens_cfg2_48view_100it.npz")
        owns = [float(np.abs(sens[f"{v}_f3_final_global_transl"] - g["final_global_transl"]).max()) for v in RD.VARIANTS]
        own = max(owns)
        assert 1e-4 < own < 3e-4, own
        band = max(FIT_TOL, RD.K * own)
        print("cfg2 frame 3 global_transl:", RD.position(float(np.abs(p["global_transl"] * p["scale"] - g["final_global_transl"]).max()), owns))
    np.testing.assert_allclose(p["global_transl"] * p["scale"], g["final_global_transl"], atol=band)
    b.close()


def test_cfg1_one_view(dev_model, smpl_model):
    g = load_golden("cfg1_1view_50it.npz")
    prob = S.make_problem(smpl_model, frame=0, n_views=1)
    b = _batch(dev_model, [prob])
    b.fit(50)
    got = N.split_params(b.get_params()[0])
    for n in PARAMS:
        np.testing.assert_allclose(got[n], g[f"it50_{n}"], rtol=0, atol=FIT_TOL, err_msg=n)
    b.close()


def test_ragged_views(dev_model, smpl_model):
    """None keypoint views: skipped, but still counted in the divisor (loss.py:157,197)."""
    g = load_golden("ragged_8view_20it.npz")
    prob = S.make_problem(smpl_model, frame=5, n_views=8, missing_views=tuple(g["missing_views"]))
    b = _batch(dev_model, [prob])
    b.fit(20)
    got = N.split_params(b.get_params()[0])
    for n in PARAMS:
        np.testing.assert_allclose(got[n], g[f"it20_{n}"], rtol=0, atol=FIT_TOL, err_msg=n)
    b.close()


def test_batch_frames_are_independent(dev_model, smpl_model):
    """config 4 in miniature: a batch gives exactly what each frame gives alone, in any order."""
    probs = [S.make_problem(smpl_model, frame=f, n_views=48) for f in (0, 1, 2, 3)]
    b = _batch(dev_model, probs)
    b.fit(100)
    together = b.get_params()
    b.close()
    for i, f in enumerate((0, 1, 2, 3)):
        g = load_golden(f"cfg2_48view_100it_f{f}.npz")
        got = N.split_params(together[i])
        for n in PARAMS:
            np.testing.assert_allclose(got[n], g[f"it100_{n}"], rtol=0, atol=FIT_TOL)
    b2 = _batch(dev_model, probs[::-1])
    b2.fit(100)
    np.testing.assert_array_equal(b2.get_params()[::-1], together)   # bit-identical: deterministic reductions
    b2.close()


def test_dense_schedule_gives_same_fit(dev_model, smpl_model):
    """BF_FIT_DENSE evaluates the full mesh every iteration like the reference; same parameters."""
    from bodyfitting_amd import _lib
    prob = S.make_problem(smpl_model, frame=1, n_views=48)
    a, b = _batch(dev_model, [prob]), _batch(dev_model, [prob])
    a.fit(30)
    b.fit(30, flags=_lib.FIT_DENSE)
    np.testing.assert_array_equal(a.get_params(), b.get_params())
    va, ja, _, _ = a.get_result()
    vb, jb, _, _ = b.get_result()
    np.testing.assert_array_equal(va, vb)
    np.testing.assert_array_equal(ja, jb)
    a.close()
    b.close()


def test_fit_is_resumable(dev_model, smpl_model):
    """100 steps in one launch == 37 + 63 steps in two launches (Adam state carried in HBM)."""
    prob = S.make_problem(smpl_model, frame=2, n_views=48)
    a, b = _batch(dev_model, [prob]), _batch(dev_model, [prob])
    a.fit(100)
    b.fit(37)
    b.fit(63)
    np.testing.assert_array_equal(a.get_params(), b.get_params())
    a.close()
    b.close()


def test_python_mirror_end_to_end(smpl_model, gmm, tmp_path):
    """bodyfitting_amd.body_fitting.BodyFitting called the way apps/genebody_fitting.py:165-170 calls the
    reference: same arguments, same files written, same result dict as the reference golden."""
    import types
    from bodyfitting_amd import assets
    from bodyfitting_amd.body_fitting import BodyFitting
    assets.register_model(smpl_model, "smpl", "neutral")
    assets.register_gmm(gmm)
    g = load_golden("cfg2_48view_100it_f0.npz")
    prob = S.make_problem(smpl_model, frame=0, n_views=48)
    opts = types.SimpleNamespace(debug=False, load_size=512, use_mask=False, smpl_type="smpl", age="adult", num_iters=100)
    fitter = BodyFitting(opts)
    images = [np.zeros((512, 512, 3), np.uint8)] * 48
    out = tmp_path / "smplify"
    res = fitter(images, prob["c2ws"], prob["Ks"], prob["keypoints"], gender="neutral", keyframe=25,
                 use_frames=prob["use_frames"], output_folder=str(out),
                 net_output=(prob["init_betas"], prob["init_pose"]))
    for key, want in (("pose", "it100_pose"), ("betas", "it100_betas"), ("global_orient", "it100_global_orient"),
                      ("global_transl", "final_global_transl"), ("scale", "it100_scale"), ("joints", "joints"),
                      ("full_pose", "full_pose")):
        np.testing.assert_allclose(res[key], g[want], atol=FIT_TOL, err_msg=key)
    assert res["vertices"].shape == (6890, 3) and res["faces"].dtype == np.int32
    saved = np.load(out / "smpl_parameter.npy", allow_pickle=True).item()        # body_fitting.py:96
    assert set(saved) == {"vertices", "joints", "pose", "betas", "global_orient", "faces", "global_transl", "scale", "full_pose"}
    first = (out / "smpl.obj").read_text().splitlines()[0]
    assert first == "v %.4f %.4f %.4f" % tuple(res["vertices"][0])


def test_smplify_mirror_reuses_its_batch_between_frames(smpl_model, gmm):
    """one SMPLify instance, frame after frame (apps/genebody_fitting.py:183-192): the device batch is kept and re-armed,
    results are those of the goldens for each frame, whatever was fitted before"""
    from bodyfitting_amd import assets
    from bodyfitting_amd.smplify import SMPLify
    assets.register_model(smpl_model, "smpl", "neutral")
    assets.register_gmm(gmm)
    fitter = SMPLify(smpl_type="smpl", num_iters=100, gender="neutral", device=0, debug=False)
    for frame in (1, 0, 1):
        g = load_golden(f"cfg2_48view_100it_f{frame}.npz")
        p = S.make_problem(smpl_model, frame=frame, n_views=48)
        res = fitter((p["init_betas"], p["init_pose"]), p["c2ws"], p["Ks"], p["keypoints"], use_frames=p["use_frames"], imsize=512)
        for key, want in (("pose", "it100_pose"), ("betas", "it100_betas"), ("global_orient", "it100_global_orient"),
                          ("scale", "it100_scale"), ("joints", "joints")):
            np.testing.assert_allclose(res[key], g[want], atol=FIT_TOL, err_msg=f"frame {frame} {key}")
    assert len(fitter._batches) == 1
    fitter.close()


@pytest.mark.parametrize("n", [17, 32, 37, 64, 70])
def test_batched_mfma_pose_blend_matches_per_frame_path(dev_model, smpl_model, n):
    """>= 16 frames: the pose blend runs on the matrix cores over the batch; same vertices as frame by frame.  Up to 64 frames it is
    ONE launch with the epilogue behind the accumulators (bf_mesh_batch32_kernel: 17 = a ragged block, 32 = config 4's shard,
    37 = a second, ragged block, 64 = two full blocks), beyond that pack_feat -> GEMM -> batched epilogue (70)"""
    rng = np.random.default_rng(11)
    betas = rng.normal(0, 0.7, (n, 10)).astype(np.float32)
    orient = rng.normal(0, 0.8, (n, 3)).astype(np.float32)
    pose = rng.normal(0, 0.3, (n, 69)).astype(np.float32)
    verts, joints, _ = dev_model.forward(betas, orient, pose)
    for i in sorted({0, 5, 16, min(31, n - 1), n - 1}):
        v1, j1, _ = dev_model.forward(betas[i:i + 1], orient[i:i + 1], pose[i:i + 1])
        np.testing.assert_allclose(verts[i], v1[0], atol=2e-6)
        np.testing.assert_allclose(joints[i], j1[0], atol=2e-6)
    m = O.to_torch_model(smpl_model, torch.float64)
    ref = O.smpl_forward(m, torch.tensor(betas[:3], dtype=torch.float64), torch.tensor(orient[:3], dtype=torch.float64),
                         torch.tensor(pose[:3], dtype=torch.float64))
    np.testing.assert_allclose(verts[:3], ref["vertices"].numpy(), atol=3e-6)


@pytest.mark.parametrize("n", [2, 3, 8, 13])
def test_small_batch_forward_is_bitwise_the_single_frame_forward(dev_model, n):
    """2..15 frames: one workgroup streams a tile's posedirs slice once for up to 8 frames (bf_mesh_multi_kernel);
    per frame the same arithmetic in the same order as the single-frame kernel"""
    rng = np.random.default_rng(100 + n)
    betas = rng.normal(0, 0.7, (n, 10)).astype(np.float32)
    orient = rng.normal(0, 0.8, (n, 3)).astype(np.float32)
    pose = rng.normal(0, 0.3, (n, 69)).astype(np.float32)
    verts, joints, jori = dev_model.forward(betas, orient, pose)
    for i in range(n):
        v1, j1, o1 = dev_model.forward(betas[i:i + 1], orient[i:i + 1], pose[i:i + 1])
        np.testing.assert_array_equal(verts[i], v1[0])
        np.testing.assert_array_equal(joints[i], j1[0])
        np.testing.assert_array_equal(jori[i], o1[0])


def test_graph_replay_equals_host_issued_commands(dev_model, smpl_model):
    """BF_FIT_RESET | BF_FIT_GRAPH: the captured command sequence gives bit-identical results, call after call"""
    from bodyfitting_amd import _lib
    probs = [S.make_problem(smpl_model, frame=f, n_views=48) for f in (0, 1)]
    a, b = _batch(dev_model, probs), _batch(dev_model, probs)
    a.fit(25, flags=_lib.FIT_FETCH)
    want_p, want_r = a.get_params(), a.get_result()
    for _ in range(3):
        b.fit(25, flags=_lib.FIT_FETCH | _lib.FIT_RESET | _lib.FIT_GRAPH)
        np.testing.assert_array_equal(b.get_params(), want_p)
        got = b.get_result()
        for x, y in zip(got, want_r):
            np.testing.assert_array_equal(x, y)
    b.fit(10, flags=_lib.FIT_RESET | _lib.FIT_GRAPH)                       # a different call shape re-captures
    a.reset(); a.fit(10)
    np.testing.assert_array_equal(b.get_params(), a.get_params())
    a.close()
    b.close()


def test_pipelined_fetch_alternates_result_arenas(dev_model, smpl_model):
    """A fetch of >= 512 KB leaves the graph: fresh fits alternate between two result arenas and the device-to-host
    copy of one runs under the kernels of the next.  Results must not depend on it, including when a host-issued
    (non-graph) call follows immediately and writes the arena a copy may still be reading."""
    from bodyfitting_amd import _lib
    probs = [S.make_problem(smpl_model, frame=f % 4, n_views=12) for f in range(8)]     # 8 x 82 KB of vertices
    a, b = _batch(dev_model, probs), _batch(dev_model, probs)
    a.fit(12, flags=_lib.FIT_FETCH)
    want_p, want_r = a.get_params(), a.get_result()
    for _ in range(4):                                                      # back to back, no sync in between
        b.fit(12, flags=_lib.FIT_FETCH | _lib.FIT_RESET | _lib.FIT_GRAPH)
    np.testing.assert_array_equal(b.get_params(), want_p)
    for x, y in zip(b.get_result(), want_r):
        np.testing.assert_array_equal(x, y)
    # pipelined call, then straight away a continuing host-issued call on the same arena
    b.fit(12, flags=_lib.FIT_FETCH | _lib.FIT_RESET | _lib.FIT_GRAPH)
    b.fit(5, flags=_lib.FIT_FETCH)
    a.fit(5, flags=_lib.FIT_FETCH)
    np.testing.assert_array_equal(b.get_params(), a.get_params())
    for x, y in zip(b.get_result(), a.get_result()):
        np.testing.assert_array_equal(x, y)
    a.close()
    b.close()


def test_back_to_back_fits_hand_their_tail_to_the_second_stream(dev_model, smpl_model):
    """Frame after frame without timing records (RESET | FETCH | NOTIME, small batch): the mesh / joints / result hand-over of a call
    runs on the second stream under the next call's fit kernel and the two result arenas alternate.  The results are those of the
    plain call, whichever call is read back, also when the inputs change between calls and when a continuing call follows."""
    from bodyfitting_amd import _lib
    pa, pb = S.make_problem(smpl_model, frame=0, n_views=12), S.make_problem(smpl_model, frame=1, n_views=12)
    ref = {}
    for name, pr in (("a", pa), ("b", pb)):
        r = _batch(dev_model, [pr])
        r.fit(12, flags=_lib.FIT_FETCH)
        ref[name] = (r.get_params(), r.get_result())
        r.fit(5, flags=_lib.FIT_FETCH)
        ref[name + "+5"] = (r.get_params(), r.get_result())
        r.close()
    fast = _lib.FIT_FETCH | _lib.FIT_RESET | _lib.FIT_NOTIME
    b = _batch(dev_model, [pa])
    c2w, K, kp, ndiv, betas, pose = N.pack_problem([pb])
    for rep in range(3):
        for _ in range(3):                                                   # back to back, no sync in between
            b.fit(12, flags=fast)
        np.testing.assert_array_equal(b.get_params(), ref["a"][0])
        for x, y in zip(b.get_result(), ref["a"][1]):
            np.testing.assert_array_equal(x, y)
    # other inputs, then a continuing (non-reset) call straight behind a hand-over that may still be running
    b.set_cameras(c2w, K); b.set_keypoints(kp, ndiv); b.set_init(betas, pose)
    b.fit(12, flags=fast)
    b.fit(12, flags=fast)
    np.testing.assert_array_equal(b.get_params(), ref["b"][0])
    b.fit(5, flags=_lib.FIT_FETCH)
    np.testing.assert_array_equal(b.get_params(), ref["b+5"][0])
    for x, y in zip(b.get_result(), ref["b+5"][1]):
        np.testing.assert_array_equal(x, y)
    b.close()
    # the same with a batch on the MFMA mesh path and a result above the 512 KB that leave the publish kernel for a copy
    probs = [S.make_problem(smpl_model, frame=f % 4, n_views=12) for f in range(20)]
    r, b = _batch(dev_model, probs), _batch(dev_model, probs)
    r.fit(12, flags=_lib.FIT_FETCH)
    for _ in range(3):
        b.fit(12, flags=fast)
    np.testing.assert_array_equal(b.get_params(), r.get_params())
    for x, y in zip(b.get_result(), r.get_result()):
        np.testing.assert_array_equal(x, y)
    r.close(); b.close()


@pytest.mark.parametrize("route", ["crowded", "one_lane_by_frame_count"])
def test_back_to_back_fits_of_a_batch_too_large_for_lanes(dev_model, smpl_model, route):
    """A batch gets fit lanes unless compute units / frames < 2, so only a batch of more than half the machine's CUs reaches the
    single-stream tail-aside routes in process: with a frame per CU ("crowded") the mesh stays on the batch stream and only the copy
    goes aside; with CUs // 2 + 1 frames the whole tail is deferred to the second stream, on the >= 128-frame GEMM mesh path.  Whichever
    call is read back, and through whichever getter, the results are those of one plain call."""
    from bodyfitting_amd import _lib
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_frames = cus if route == "crowded" else cus // 2 + 1
    probs = [S.make_problem(smpl_model, frame=f, n_views=2) for f in range(4)]
    probs = [probs[f % 4] for f in range(n_frames)]
    r, b = _batch(dev_model, probs), _batch(dev_model, probs)
    r.fit(4, flags=_lib.FIT_FETCH)
    want_p, want_r = r.get_params(), r.get_result()
    fast = _lib.FIT_FETCH | _lib.FIT_RESET | _lib.FIT_NOTIME
    b.fit(4, flags=fast)
    b.fit(4, flags=fast)
    prev = b.get_previous()                                                  # the first fit's, under the second
    b.fit(4, flags=fast)
    np.testing.assert_array_equal(prev[0], want_p)
    for x, y in zip(prev[1:], want_r):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(b.get_params(), want_p)
    for x, y in zip(b.get_result(), want_r):
        np.testing.assert_array_equal(x, y)
    r.close(); b.close()


def test_more_than_48_views_streams_the_rest(dev_model, smpl_model, gmm_bufs):
    """Views past the 48 staged in LDS are streamed from global memory by the projection phase: 60 views against the
    fp64 oracle (gradient) and the fp64 analytic loop (a short fit)."""
    from oracle import analytic as A
    prob = S.make_problem(smpl_model, frame=2, n_views=60)
    b = _batch(dev_model, [prob])
    terms, grads = b.loss_grad()
    P0 = {k: np.asarray(v, np.float64) for k, v in N.split_params(b.get_params()[0]).items()}
    _, _, g64, _, _ = O.loss_and_grad(smpl_model, gmm_bufs, prob, P0)
    got = N.split_params(grads[0])
    for k in PARAMS:
        np.testing.assert_allclose(got[k], g64[k], atol=2e-5 * np.abs(g64[k]).max(), err_msg=k)
    b.fit(10)
    want, _, _ = A.fit(smpl_model, gmm_bufs, prob, 10, dtype=np.float64)
    got = N.split_params(b.get_params()[0])
    for k, v in want.items():
        np.testing.assert_allclose(got[k], v, atol=1e-4, err_msg=k)
    b.close()


def test_untimed_submission_gives_the_same_fit(dev_model, smpl_model):
    """BF_FIT_NOTIME (what bench.py steps with): no event records, same commands, same bits"""
    from bodyfitting_amd import _lib
    prob = S.make_problem(smpl_model, frame=1, n_views=48)
    a, b = _batch(dev_model, [prob]), _batch(dev_model, [prob])
    a.fit(20, flags=_lib.FIT_FETCH | _lib.FIT_RESET)
    for _ in range(2):
        b.fit(20, flags=_lib.FIT_FETCH | _lib.FIT_RESET | _lib.FIT_NOTIME)
    np.testing.assert_array_equal(b.get_params(), a.get_params())
    for x, y in zip(b.get_result(), a.get_result()):
        np.testing.assert_array_equal(x, y)
    a.close()
    b.close()


def _stream_case(dev_model, smpl_model, frames):
    probs = [S.make_problem(smpl_model, frame=f, n_views=48) for f in frames]
    packed = [N.pack_problem([p]) for p in probs]
    return probs, packed


def test_frames_streamed_back_to_back_hold_their_goldens(dev_model, smpl_model):
    """The frame loop of apps/genebody_fitting.py:183-192 as the library runs it: frames 0..3 go through ONE batch back to back,
    each frame's keypoints + initial estimate staged (bf_batch_stage_inputs) while the previous frame is still being fitted,
    each result read (bf_batch_get_previous) while the next frame is being fitted.  Every frame lands on the reference's golden
    (1e-4, the north-star tolerance) and on the bits of the same frame fitted alone."""
    from bodyfitting_amd import _lib
    flags = _lib.FIT_RESET | _lib.FIT_FETCH | _lib.FIT_NOTIME
    frames = (0, 1, 2, 3)
    probs, packed = _stream_case(dev_model, smpl_model, frames)
    b = N.FrameBatch(dev_model, 1, 48)
    b.set_cameras(packed[0][0], packed[0][1])               # the capture's cameras: shared by its frames
    got = []
    for i, (c2w, K, kp, ndiv, betas, pose) in enumerate(packed):
        assert np.array_equal(c2w, packed[0][0])
        b.stage_inputs(kp, ndiv, betas, pose)
        b.fit(100, flags=flags)
        if i > 0:
            got.append(b.get_previous())
    b.sync()
    got.append((b.get_params(),) + b.get_result())
    for f, (params, verts, joints, full_pose, terms) in zip(frames, got):
        g = load_golden(f"cfg2_48view_100it_f{f}.npz")
        p = N.split_params(params[0])
        for k in PARAMS:
            np.testing.assert_allclose(p[k], g[f"it100_{k}"], atol=FIT_TOL, err_msg=f"frame {f} {k}")
        np.testing.assert_allclose(joints[0], g["joints"], atol=FIT_TOL)
        np.testing.assert_allclose(verts[0][::53], g["vertices_sample"], atol=FIT_TOL)
        np.testing.assert_allclose(full_pose[0], g["full_pose"], atol=FIT_TOL)
        alone = _batch(dev_model, [probs[frames.index(f)]])
        alone.fit(100)
        assert np.array_equal(alone.get_params(), params), f"frame {f}: streamed fit differs from the frame fitted alone"
        av, aj, _, _ = alone.get_result()
        assert np.array_equal(av, verts) and np.array_equal(aj, joints)
        alone.close()
    b.close()


@pytest.mark.parametrize("n_frames", [3, 32])
def test_staging_while_a_fit_is_in_flight_never_touches_its_inputs(dev_model, smpl_model, n_frames):
    """stage_inputs returns without draining the stream; the fit in flight must still see ITS frames (two input arenas), also for
    a batch, and after eight alternations"""
    from bodyfitting_amd import _lib
    flags = _lib.FIT_RESET | _lib.FIT_FETCH | _lib.FIT_NOTIME
    sets = [N.pack_problem([S.make_problem(smpl_model, frame=10 * s + f, n_views=48) for f in range(n_frames)]) for s in range(3)]
    want = []
    for c2w, K, kp, ndiv, betas, pose in sets:
        ref = N.FrameBatch(dev_model, n_frames, 48)
        ref.set_cameras(sets[0][0], sets[0][1]); ref.set_keypoints(kp, ndiv); ref.set_init(betas, pose)
        ref.fit(100)
        want.append(ref.get_params())
        ref.close()
    b = N.FrameBatch(dev_model, n_frames, 48)
    b.set_cameras(sets[0][0], sets[0][1])
    order = [0, 1, 2, 1, 0, 2, 2, 1]
    seen = []
    for i, s in enumerate(order):
        _, _, kp, ndiv, betas, pose = sets[s]
        b.stage_inputs(kp, ndiv, betas, pose)           # (issued while fit i-1 is running)
        b.fit(100, flags=flags)
        if i > 0:
            seen.append(b.get_previous(vertices=False)[0])
    seen.append(b.get_params())
    for i, (s, p) in enumerate(zip(order, seen)):
        bad = np.argwhere(np.any(p != want[s], axis=1)).ravel()
        assert bad.size == 0, (f"fit {i} (frame set {s}): frames {bad.tolist()} differ, max |diff| {np.abs(p - want[s]).max():.3g}; "
                               f"equal to another set's result: {[int(np.array_equal(p[bad], w[bad])) for w in want]}")
    # a staged frame needs a fresh start: continuing the previous frame's optimiser on new inputs is refused
    b.stage_inputs(sets[0][2], sets[0][3], sets[0][4], sets[0][5])
    with pytest.raises(_lib.BodyfitError, match="BF_FIT_RESET"):
        b.fit(10, flags=_lib.FIT_FETCH)
    b.fit(10, flags=flags)
    # and the synchronous setters keep working on whichever arena is current
    b.set_keypoints(sets[1][2], sets[1][3]); b.set_init(sets[1][4], sets[1][5])
    b.fit(100)
    assert np.array_equal(b.get_params(), want[1])
    b.close()


def test_staging_aside_in_irregular_call_orders(dev_model, smpl_model):
    """Round 5: in the frame loop the input transfer rides on the second stream ahead of the deferred mesh / hand-over tail of the fit
    in flight (api.hip: bf_batch_stage_inputs, bf_flush_tail).  Call orders a frame loop does not produce must give the same bits:
    two stagings before one fit (the second goes into the arena the fit in flight reads from: it has to be ordered behind that fit),
    a result read straight after a fit whose tail is still deferred, a plain fit in between, and a batch destroyed with a tail
    pending."""
    from bodyfitting_amd import _lib
    flags = _lib.FIT_RESET | _lib.FIT_FETCH | _lib.FIT_NOTIME
    sets = [N.pack_problem([S.make_problem(smpl_model, frame=20 * s + 3, n_views=48)]) for s in range(3)]
    want = []
    for c2w, K, kp, ndiv, betas, pose in sets:
        ref = N.FrameBatch(dev_model, 1, 48)
        ref.set_cameras(sets[0][0], sets[0][1]); ref.set_keypoints(kp, ndiv); ref.set_init(betas, pose)
        ref.fit(100)
        want.append((ref.get_params(), ref.get_result()[0]))
        ref.close()
    b = N.FrameBatch(dev_model, 1, 48)
    b.set_cameras(sets[0][0], sets[0][1])
    stage = lambda s: b.stage_inputs(sets[s][2], sets[s][3], sets[s][4], sets[s][5])
    stage(0); b.fit(100, flags=flags)
    stage(1); b.fit(100, flags=flags)                   # (fit of set 1 in flight, its tail deferred)
    stage(2); stage(0)                                  # the second staging overwrites the arena fit 1 reads from ... behind it
    b.fit(100, flags=flags)
    p1 = b.get_previous()                               # fit of set 1
    assert np.array_equal(p1[0], want[1][0]) and np.array_equal(p1[1], want[1][1])
    verts = b.get_result()[0]                           # fit of set 0 (staged last), read with its tail still deferred
    assert np.array_equal(b.get_params(), want[0][0]) and np.array_equal(verts, want[0][1])
    stage(2); b.fit(100, flags=flags)
    b.set_keypoints(sets[1][2], sets[1][3]); b.set_init(sets[1][4], sets[1][5])       # synchronous setters drain everything
    b.fit(100)                                          # a plain fit
    assert np.array_equal(b.get_params(), want[1][0])
    stage(2); b.fit(100, flags=flags)
    stage(0); b.fit(100, flags=flags)
    p2 = b.get_previous()
    assert np.array_equal(p2[0], want[2][0]) and np.array_equal(p2[1], want[2][1])
    b.close()                                           # (a tail pending: nobody reads it)
    c = N.FrameBatch(dev_model, 1, 48)                  # the device is fine afterwards
    c.set_cameras(sets[0][0], sets[0][1]); c.set_keypoints(sets[2][2], sets[2][3]); c.set_init(sets[2][4], sets[2][5])
    c.fit(100)
    assert np.array_equal(c.get_params(), want[2][0])
    c.close()


def test_smplify_stream_yields_the_frames_of_the_call_path(smpl_model, gmm):
    """SMPLify.stream: the capture's frame loop as a generator (two-deep pipeline) == __call__ frame by frame, bit for bit"""
    from bodyfitting_amd import assets
    from bodyfitting_amd.smplify import SMPLify
    assets.register_model(smpl_model, "smpl", "neutral")
    assets.register_gmm(gmm)
    fitter = SMPLify(smpl_type="smpl", num_iters=100, gender="neutral", device=0, debug=False)
    probs = [S.make_problem(smpl_model, frame=f, n_views=48) for f in (2, 0, 3)]
    streamed = list(fitter.stream((((p["init_betas"], p["init_pose"]), p["keypoints"]) for p in probs), probs[0]["c2ws"], probs[0]["Ks"]))
    assert len(streamed) == 3
    for p, res in zip(probs, streamed):
        one = fitter((p["init_betas"], p["init_pose"]), p["c2ws"], p["Ks"], p["keypoints"], use_frames=p["use_frames"], imsize=512)
        for key in ("vertices", "joints", "pose", "betas", "global_orient", "global_transl", "scale", "full_pose"):
            assert np.array_equal(res[key], one[key]), key
        # ... and both equal the synchronous setters' path (the call stages its frame like the stream does)
        V = len(p["use_frames"])
        kp = np.stack([np.zeros((25, 3), np.float32) if k is None else np.asarray(k["pose"], np.float32)[:25] for k in p["keypoints"][:V]])
        c2w = np.stack([np.asarray(c, np.float32) for c in p["c2ws"][:V]])
        K = np.stack([np.asarray(k, np.float32) for k in p["Ks"][:V]])
        sync = fitter.fit_frames(np.asarray(p["init_betas"], np.float32)[:1], np.asarray(p["init_pose"], np.float32)[:1], c2w[None], K[None],
                                 kp[None], n_use_frames=[V], imsize=512)[0]
        for key in ("vertices", "joints", "pose", "betas", "global_orient", "global_transl", "scale", "full_pose"):
            assert np.array_equal(sync[key], one[key]), key
    # a call after the cameras changed must not reuse the cached ones
    p = probs[0]
    moved = [np.asarray(c, np.float32).copy() for c in p["c2ws"]]
    for c in moved:
        c[:3, 3] += 0.05
    a = fitter((p["init_betas"], p["init_pose"]), moved, p["Ks"], p["keypoints"], use_frames=p["use_frames"], imsize=512)
    b = fitter((p["init_betas"], p["init_pose"]), p["c2ws"], p["Ks"], p["keypoints"], use_frames=p["use_frames"], imsize=512)
    assert not np.array_equal(a["pose"], b["pose"])
    assert np.array_equal(b["pose"], streamed[0]["pose"])
    # a keypoint-only stream never looks its mask views up (smplify.py:141 does so only under use_mask): use_frames without view 0, and
    # mask_frames None / [] as older callers pass them, are fine; a frame WITH masks and no mask_frames is the error
    sub = [1, 7, 13]
    p = probs[1]
    args = ([p["c2ws"][i] for i in sub], [p["Ks"][i] for i in sub])
    kps = [p["keypoints"][i] for i in sub]
    for mf in ((0,), None, []):
        got = list(fitter.stream([((p["init_betas"], p["init_pose"]), kps)], *args, use_frames=sub, mask_frames=mf))
        one = fitter((p["init_betas"], p["init_pose"]), *args, kps, use_frames=sub, imsize=512)
        assert len(got) == 1 and np.array_equal(got[0]["pose"], one["pose"])
    with pytest.raises(ValueError):
        list(fitter.stream([((p["init_betas"], p["init_pose"]), kps, [np.zeros((64, 64), np.uint8)] * 1)], *args, use_frames=sub, mask_frames=None))
    fitter.close()


# --------------------------------------------------------------------------------------------------------------------------------
# the joint-angle sweep through the pose-state forward (tests/model_sweep_cases.py): m_rodrigues from 1e-6 rad to beyond 4 pi
# --------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["smpl", "kid"])
def sweep_dev(request):
    import model_sweep_cases as MS
    dev = N.DeviceModel(MS.model(request.param), S.make_gmm(seed=0), device=0)
    yield request.param, dev
    dev.close()


def _sweep_forward(dev, p, lo, hi):
    verts, joints, jori = dev.forward(p["betas"][lo:hi], p["global_orient"][lo:hi], p["body_pose"][lo:hi])
    return {"vertices": verts, "joints": joints, "joints_ori": jori}


def test_angle_sweep_forward_matches_the_oracle_frame_by_frame(sweep_dev):
    """every angle, axis and joint set of axis R as one batch (>= 16 frames: the matrix-core mesh pass behind the pose state), in
    calls of five frames (the multi-frame kernel) and frame by frame: vertices, joints and joints_ori of EVERY frame within
    max(3e-6, 8 * err32) of the float64 oracle; below 16 frames a frame's bits do not depend on its neighbours"""
    import model_sweep_cases as MS
    kind, dev = sweep_dev
    p, n = MS.params(kind), len(MS.frames(kind))
    assert dev.n_verts == 690 and dev.n_betas == p["betas"].shape[1]
    MS.check_forward(kind, _sweep_forward(dev, p, 0, n), what="forward, one batch")
    alone = [_sweep_forward(dev, p, f, f + 1) for f in range(n)]
    MS.check_forward(kind, {k: np.concatenate([a[k] for a in alone]) for k in alone[0]}, what="forward, frame alone")
    for lo in range(0, n, 5):
        got = _sweep_forward(dev, p, lo, min(lo + 5, n))
        MS.check_forward(kind, got, first=lo, what="forward, five frames")
        for k, v in got.items():
            for i in range(len(v)):
                assert np.array_equal(v[i], alone[lo + i][k][0]), (kind, k, lo + i, MS.frames(kind)[lo + i].name)
    MS.report(kind)
