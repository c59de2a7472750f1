"""Frame-after-frame fits under BF_FIT_LANES in FRESH processes (tests/test_gpu_fit_lanes.py): the lane count is read once per process,
so every count gets a child of its own.  Each child streams frames through one batch in the call orders a capture produces and in
irregular ones, checks every result against the same frame fitted alone by a plain (timed, lane-free) call in the same process, and
stores the streamed parameters for the parent to hold against the other lane counts."""
import os
import sys
import traceback

import numpy as np

VIEWS, ITERS = 12, 30


def _run(out_path, body):
    try:
        np.savez(out_path, **body())
    except BaseException:
        with open(out_path + ".err", "w") as f:
            f.write(traceback.format_exc())
        raise


def lanes(out_path, n_lanes):
    os.environ["BF_FIT_LANES"] = str(n_lanes)          # (before libbodyfit is loaded: the library reads it once)

    def body():
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        if repo not in sys.path:
            sys.path.insert(0, repo)
        from bodyfitting_amd import _lib, native as N, synthetic as S
        fast = _lib.FIT_RESET | _lib.FIT_FETCH | _lib.FIT_NOTIME
        model = S.make_model("smpl", seed=0)
        dev = N.DeviceModel(model, S.make_gmm(seed=0), device=0)
        out = {}

        def sets(n_frames, n_sets, base):
            return [N.pack_problem([S.make_problem(model, frame=base + 10 * s + f, n_views=VIEWS) for f in range(n_frames)]) for s in range(n_sets)]

        def alone(packed, cams, iters=ITERS, more=0):
            _, _, kp, ndiv, betas, pose = packed
            r = N.FrameBatch(dev, kp.shape[0], VIEWS)
            r.set_cameras(*cams); r.set_keypoints(kp, ndiv); r.set_init(betas, pose)
            r.fit(iters)
            res = [(r.get_params(),) + r.get_result()]
            if more:
                r.fit(more, flags=_lib.FIT_FETCH)
                res.append((r.get_params(),) + r.get_result())
            r.close()
            return res

        def same(got, want, what):
            for x, y, name in zip(got, want, ("params", "vertices", "joints", "full_pose", "loss_terms")):
                assert np.array_equal(x, y), f"{what}: {name} differs from the frame fitted alone (max |diff| {np.abs(x - y).max():.3g})"

        # 1. the capture's loop: stage, fit, read the frame before - eight frames, more than any lane count cycles through
        frames = sets(1, 8, 0)
        cams = (frames[0][0], frames[0][1])
        want = [alone(p, cams)[0] for p in frames]
        b = N.FrameBatch(dev, 1, VIEWS)
        b.set_cameras(*cams)
        got = []
        for i, (_, _, kp, ndiv, betas, pose) in enumerate(frames):
            b.stage_inputs(kp, ndiv, betas, pose)
            b.fit(ITERS, flags=fast)
            if i > 0:
                got.append(b.get_previous())
        b.sync()
        got.append((b.get_params(),) + b.get_result())
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, f"streamed frame {i}")
        out["streamed_params"] = np.concatenate([g[0] for g in got])

        # 2. irregular orders (tests/test_gpu_parity.py::test_staging_aside_in_irregular_call_orders, here with lanes)
        stage = lambda s: b.stage_inputs(frames[s][2], frames[s][3], frames[s][4], frames[s][5])
        stage(0); b.fit(ITERS, flags=fast)
        stage(1); b.fit(ITERS, flags=fast)
        stage(2); stage(3)                                   # two stagings before one fit
        b.fit(ITERS, flags=fast)
        same(b.get_previous(), want[1], "previous after a double staging")
        same((b.get_params(),) + b.get_result(), want[3], "result straight after a fit")
        stage(4); b.fit(ITERS, flags=fast)
        stage(5); b.fit(ITERS, flags=fast)
        same(b.get_previous(), want[4], "previous after a drained read")
        # fits that re-use the staged inputs on every lane, then a staging into the arena they all read
        for _ in range(5):
            b.fit(ITERS, flags=fast)
        stage(6); b.fit(ITERS, flags=fast)
        stage(5); b.fit(ITERS, flags=fast)
        same(b.get_previous(), want[6], "previous after re-used inputs")
        same((b.get_params(),) + b.get_result(), want[5], "re-staged arena")
        # a continuing (non-reset) fit straight behind a lane fit continues that fit's optimiser
        cont = alone(frames[7], cams, more=7)
        stage(7); b.fit(ITERS, flags=fast)
        b.fit(7, flags=_lib.FIT_FETCH)
        same((b.get_params(),) + b.get_result(), cont[1], "continuing fit behind a lane fit")
        # synchronous setters in between, then lane fits from the setters' inputs and a plain fit
        stage(2); b.fit(ITERS, flags=fast)
        b.set_keypoints(frames[1][2], frames[1][3]); b.set_init(frames[1][4], frames[1][5])
        b.fit(ITERS, flags=fast); b.fit(ITERS, flags=fast)
        same((b.get_params(),) + b.get_result(), want[1], "lane fits from the setters' inputs")
        b.fit(ITERS, flags=_lib.FIT_RESET)
        same((b.get_params(),) + b.get_result(), want[1], "plain (timed) fit after lane fits")
        # destroyed with lane work pending; the device is fine afterwards
        stage(0); b.fit(ITERS, flags=fast)
        stage(3); b.fit(ITERS, flags=fast)
        stage(4)
        b.close()
        c = N.FrameBatch(dev, 1, VIEWS)
        c.set_cameras(*cams); c.set_keypoints(frames[2][2], frames[2][3]); c.set_init(frames[2][4], frames[2][5])
        c.fit(ITERS)
        same((c.get_params(),) + c.get_result(), want[2], "a batch after a destroy with lanes pending")
        c.close()

        # 3. a 32-frame batch (config 4's shard) streamed through the lanes, staging and reading the frame set before
        big = sets(32, 4, 100)
        cams32 = (big[0][0], big[0][1])
        wbig = [alone(p, cams32)[0] for p in big]
        b = N.FrameBatch(dev, 32, VIEWS)
        b.set_cameras(*cams32)
        got = []
        for i, s in enumerate((0, 1, 2, 3, 1, 0)):
            _, _, kp, ndiv, betas, pose = big[s]
            b.stage_inputs(kp, ndiv, betas, pose)
            b.fit(ITERS, flags=fast)
            if i > 0:
                got.append(b.get_previous())
        got.append((b.get_params(),) + b.get_result())
        for g, s in zip(got, (0, 1, 2, 3, 1, 0)):
            same(g, wbig[s], f"32-frame set {s}")
        out["batch32_params"] = np.concatenate([g[0] for g in got])
        b.close()
        dev.close()
        return out

    _run(out_path, body)
