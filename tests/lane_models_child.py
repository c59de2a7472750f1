"""The frame-loop routes on models other than the adult 4-bone SMPL, in FRESH processes (tests/test_gpu_lane_models.py): the lane
settings are read once per process, so every setting gets a child of its own, and each child runs every variant of LANE_VARIANTS
(tests/width_variants.py: the kid model with its 87 parameters and 12-direction mesh instance, 8-wide and dense skinning, the sized
fit instance beside a dense mesh tail, the 690-vertex models).  Every streamed result - every slot of a group, with a loss divisor
(n_use_frames) that differs from slot to slot, groups split by iterations and hyper-parameters, per-call mesh tails of 4- and
16-frame batches, a continuing fit behind a held group - is held bit for bit against the same frame fitted alone by a plain (timed,
lane-free) call in the same process.  The streamed parameters, and frame 0's mesh, go to the parent, which compares them across
settings and holds frame 0 to the fp64 oracle."""
import os
import sys

import numpy as np

from lanes_child import _run

VIEWS, ITERS, ITERS16 = 5, 20, 10          # 5 views: 375 keypoint floats per frame and slot, no 16-byte multiple
NDIV = (5, 3, 4, 5, 2)                     # n_use_frames by frame index: the loss's divisor only - neighbouring slots never share one
LANE_VARIANTS = ("kid", "smpl_4+S", "smpl_4+1", "nv690_B8", "nv690_BD")
ORDER4 = (0, 1, 2, 3, 4, 2, 0, 3, 1, 4)
ORDER16 = (0, 1, 2, 1, 0)


def ndiv_of(first, n_frames):
    return np.array([NDIV[(first + f) % len(NDIV)] for f in range(n_frames)], np.int32)


def same(got, want, what):
    """(params, vertices, joints, full_pose, loss terms) of a streamed fit are the bits of the frame fitted alone"""
    for x, y, name in zip(got, want, ("params", "vertices", "joints", "full_pose", "loss_terms")):
        assert np.array_equal(x, y), f"{what}: {name} differs from the frame fitted alone (max |diff| {np.abs(x - y).max():.3g})"


def models(out_path, width, fill, lanes=None):
    """lanes None: lane groups of BF_FIT_LANE_WIDTH = width, BF_FIT_LANE_FILL = fill; lanes = 1: no lanes, the single-stream route"""
    for k in ("BF_FIT_LANE_WIDTH", "BF_FIT_LANE_FILL", "BF_FIT_LANES"):
        os.environ.pop(k, None)
    if lanes is None:                                    # (before libbodyfit is loaded: the library reads them once)
        os.environ["BF_FIT_LANE_WIDTH"] = str(width)
        os.environ["BF_FIT_LANE_FILL"] = str(fill)
    else:
        os.environ["BF_FIT_LANES"] = str(lanes)
        width, fill = 1, 0

    def body():
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        if repo not in sys.path:
            sys.path.insert(0, repo)
        from bodyfitting_amd import _lib, native as N, synthetic as S
        from width_variants import Variants, smpl_problem
        import loss_grad_cases as LC
        fast = _lib.FIT_RESET | _lib.FIT_FETCH | _lib.FIT_NOTIME
        variants = Variants(S.make_gmm(seed=0))
        out = {}
        last = lambda q: (q.get_params(),) + q.get_result()          # noqa: E731
        ceil_div = lambda a, b: -(-a // b)                           # noqa: E731

        def one(name):
            model, dev = variants.get(name)

            def sets(n_frames, n_sets, base):
                """n_sets frame sets (cameras, keypoints, divisors, initial estimate); set s, frame f divides by NDIV[s + f]"""
                got = []
                for s in range(n_sets):
                    c2w, K, kp, _, betas, pose = N.pack_problem([smpl_problem(name, model, frame=base + 10 * s + f, n_views=VIEWS) for f in range(n_frames)])
                    if (n_frames, base, s) == (1, 0, 1):
                        # the second streamed frame starts with its root at 2 pi + 1e-3 and a leaf of the chain (joint 20) at 4.7 rad
                        # (axis R of tests/loss_grad_cases.py): past the wrap and in quadrant 3 of the fit kernel's sine / cosine
                        assert pose.shape == (1, 72)
                        pose = pose.copy()
                        pose[0, 0:3] = LC.Sweep(2 * LC.PI + 1e-3, "general", "root").theta
                        pose[0, 60:63] = LC.Sweep(4.7, "-y", "leaf").theta
                    got.append((c2w, K, kp, ndiv_of(s, n_frames), betas, pose))
                return got

            def alone(packed, cams, iters=ITERS, hyper=None, more=0):
                _, _, kp, ndiv, betas, pose = packed
                r = N.FrameBatch(dev, kp.shape[0], VIEWS)
                r.set_cameras(*cams); r.set_keypoints(kp, ndiv); r.set_init(betas, pose)
                r.fit(iters, hyper)
                res = [last(r)]
                if more:
                    r.fit(more, hyper, flags=_lib.FIT_FETCH)
                    res.append(last(r))
                r.close()
                return res

            def streamer(batch, frame_sets):
                def stage(s):
                    _, _, kp, ndiv, betas, pose = frame_sets[s]
                    batch.stage_inputs(kp, ndiv, betas, pose)
                return stage

            # the references, once: W + 2 distinct frames (eight at least) fitted alone, each with its own divisor
            frames = sets(1, max(width, 6) + 2, 0)
            cams = (frames[0][0], frames[0][1])
            want = [alone(p, cams)[0] for p in frames]
            assert not np.array_equal(want[0][0], alone(frames[0][:3] + (ndiv_of(1, 1),) + frames[0][4:], cams)[0][0]), \
                f"{name}: the divisor does not reach the fit"

            # 1. every slot, ragged divisor: n staged fits with no reads, then the last two - every slot of a full group, of a partial one
            #    and of the group after it, read as the previous fit and as the last one
            b = N.FrameBatch(dev, 1, VIEWS)
            b.set_cameras(*cams)
            stage = streamer(b, frames)
            W = b.lane_stats()["width"]
            assert W == width, f"{name}: W = {W} with BF_FIT_LANE_WIDTH={width}, lanes {lanes}"
            calls = launches = 0
            for n in range(1, W + 3):
                for i in range(n):
                    stage(i); b.fit(ITERS, flags=fast)
                calls += n
                launches += ceil_div(n, W)
                b.sync()
                if n >= 2:
                    same(b.get_previous(), want[n - 2], f"{name}, {n} frames: previous")
                same(last(b), want[n - 1], f"{name}, {n} frames: last")
            st = b.lane_stats()
            if lanes is None:
                assert st["calls"] == calls, (name, st, calls)
                if fill or W == 1:
                    assert (st["launches"], st["max_group"]) == (launches, W), (name, st, launches)
            # ... and the capture's loop: stage, fit, read the frame before
            got = []
            for i in range(8):
                stage(i); b.fit(ITERS, flags=fast)
                if i > 0:
                    got.append(b.get_previous())
            b.sync()
            got.append(last(b))
            for i, g in enumerate(got):
                same(g, want[i], f"{name}: streamed frame {i}")
            out[f"streamed_{name}"] = np.concatenate([g[0] for g in got])
            out[f"frame0_vertices_{name}"], out[f"frame0_joints_{name}"], out[f"frame0_full_pose_{name}"] = got[0][1][0], got[0][2][0], got[0][3][0]

            # 3. groups split by n_iters and by hyper-parameters, on a batch of their own (its lane_stats count these calls alone)
            h512, h256 = N.make_hyper(), N.make_hyper(imsize=256, constant_scale=0.3)
            split = [(0, ITERS, h512), (1, 12, h512), (2, ITERS, h256), (3, ITERS, h256)]
            wsplit = [alone(frames[s], cams, iters, h)[0] for s, iters, h in split]
            assert not np.array_equal(wsplit[2][0], want[2][0]), f"{name}: the hyper-parameters do not reach the fit"
            c = N.FrameBatch(dev, 1, VIEWS)
            c.set_cameras(*cams)
            cstage = streamer(c, frames)
            for s, iters, h in split:
                cstage(s); c.fit(iters, h, flags=fast)
            c.sync()
            st = c.lane_stats()
            if lanes is None:
                assert st["calls"] == 4, (name, st)
                if fill:            # three launches - each differing call sends the open group off - and the last two calls as one group
                    assert (st["launches"], st["max_group"]) == (3, 2), (name, st)
                elif W == 1:
                    assert (st["launches"], st["max_group"]) == (4, 1), (name, st)
            same(c.get_previous(), wsplit[2], f"{name}: first call with the other hyper-parameters")
            same(last(c), wsplit[3], f"{name}: second call with the other hyper-parameters")
            for s, iters, h in split[:2]:
                cstage(s); c.fit(iters, h, flags=fast)
            same(c.get_previous(), wsplit[0], f"{name}: call ahead of one with fewer iterations")
            same(last(c), wsplit[1], f"{name}: call with fewer iterations")
            c.close()

            # 4. a continuing (non-reset) fit straight behind a held group continues the last slot's optimiser: the drain's copy of
            #    that slot's Adam moments and result slices
            cont = alone(frames[5], cams, more=7)
            stage(4); b.fit(ITERS, flags=fast)
            stage(5); b.fit(ITERS, flags=fast)
            b.fit(7, flags=_lib.FIT_FETCH)
            same(last(b), cont[1], f"{name}: continuing fit behind a held group")

            # 5. destroyed with a group held and a slot staged past it; the device is fine afterwards
            stage(0); b.fit(ITERS, flags=fast)
            stage(3); b.fit(ITERS, flags=fast)
            stage(4)
            b.close()
            c = N.FrameBatch(dev, 1, VIEWS)
            c.set_cameras(*cams); c.set_keypoints(frames[2][2], frames[2][3]); c.set_init(frames[2][4], frames[2][5])
            c.fit(ITERS)
            same(last(c), want[2], f"{name}: a batch after a destroy with a group held")
            c.close()

            # 2. per-call mesh tails: a group's tail gives every call a pass of its own at the call's offset into the state, vertex and
            #    extra-joint partial arrays.  4 frames: bf_mesh_multi_kernel (the sparse 8-wide and the dense skinning loops); 16 frames:
            #    bf_mesh_batch32_kernel<12> (kid) or the pose-blend GEMM into the lane's one scratch, pass after pass (8-wide, dense)
            for n_frames, order, iters, n_sets, base, w_cus, key in ((4, ORDER4, ITERS, 5, 300, 16, "batch4"), (16, ORDER16, ITERS16, 3, 500, 4, "batch16")):
                group = sets(n_frames, n_sets, base)
                gcams = (group[0][0], group[0][1])
                wgroup = [alone(p, gcams, iters)[0] for p in group]
                b = N.FrameBatch(dev, n_frames, VIEWS)
                b.set_cameras(*gcams)
                gstage = streamer(b, group)
                Wg = b.lane_stats()["width"]
                assert Wg == min(width, w_cus), (name, n_frames, b.lane_stats())      # (a frame per CU at most: 256 CUs, four lanes)
                for s in order:                                  # no reads: groups as large as the setting lets them grow
                    gstage(s); b.fit(iters, flags=fast)
                b.sync()
                same(b.get_previous(), wgroup[order[-2]], f"{name}: {n_frames}-frame set before the last")
                same(last(b), wgroup[order[-1]], f"{name}: last {n_frames}-frame set")
                st = b.lane_stats()
                if lanes is None:
                    assert st["calls"] == len(order), (name, st)
                    if fill or Wg == 1:
                        assert (st["launches"], st["max_group"]) == (ceil_div(len(order), Wg), min(Wg, len(order))), (name, n_frames, st)
                got = []
                for i, s in enumerate(order):                    # ... and reading the set before at every step
                    gstage(s); b.fit(iters, flags=fast)
                    if i > 0:
                        got.append(b.get_previous())
                got.append(last(b))
                for g, s in zip(got, order):
                    same(g, wgroup[s], f"{name}: {n_frames}-frame set {s}")
                out[f"{key}_{name}"] = np.concatenate([g[0] for g in got])
                b.close()

        for name in LANE_VARIANTS:
            one(name)
        variants.close()
        return out

    _run(out_path, body)
