"""Fit-lane groups under BF_FIT_LANE_WIDTH / BF_FIT_LANE_FILL in FRESH processes (tests/test_gpu_lane_groups.py): both are read once
per process, so every (width, fill) gets a child of its own.  Each child streams frames through one batch so that every slot of a full
group, of a partial one and of the group after it is read back both ways, forces the group shapes (fill = 1) and checks them through
lane_stats, runs the irregular call orders with a group held open, and holds every result against the same frame fitted alone by a
plain (timed, lane-free) call in the same process.  The streamed parameters go to the parent, which compares them across settings."""
import os
import sys

import numpy as np

from lanes_child import _run

VIEWS, ITERS = 12, 30


def groups(out_path, width, fill):
    os.environ["BF_FIT_LANE_WIDTH"] = str(width)        # (before libbodyfit is loaded: the library reads them once)
    os.environ["BF_FIT_LANE_FILL"] = str(fill)
    os.environ.pop("BF_FIT_LANES", None)

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

        # the references, once: W + 2 distinct frames fitted alone
        frames = sets(1, max(width, 8) + 2, 0)
        cams = (frames[0][0], frames[0][1])
        want = [alone(p, cams)[0] for p in frames]
        last = lambda q: (q.get_params(),) + q.get_result()

        # 1. group shapes: eight calls and a sync on a fresh batch
        b = N.FrameBatch(dev, 1, VIEWS)
        b.set_cameras(*cams)
        stage = lambda s: b.stage_inputs(frames[s][2], frames[s][3], frames[s][4], frames[s][5])
        got = []
        for i in range(8):                                   # (the capture's loop: stage, fit, no reads)
            stage(i); b.fit(ITERS, flags=fast)
        b.sync()
        st = b.lane_stats()
        W = st["width"]
        assert W == width, f"W = {W} with BF_FIT_LANE_WIDTH={width}"
        assert st["calls"] == 8, st
        if fill:
            assert (st["launches"], st["max_group"]) == {3: (3, 3), 8: (1, 8)}[width], st
        elif width == 1:
            assert (st["launches"], st["max_group"]) == (8, 1), st
        same(b.get_previous(), want[6], "frame 6 of eight, read as the previous one")
        same(last(b), want[7], "frame 7 of eight")

        # 2. every slot position: n frames with no reads, then the last two - every slot of a full group, a partial group and the
        #    first slot of the group after it, read as the previous fit and as the last one
        calls = 8
        for n in range(1, W + 3):
            for i in range(n):
                stage(i); b.fit(ITERS, flags=fast)
            calls += n
            b.sync()
            if n >= 2:
                same(b.get_previous(), want[n - 2], f"{n} frames: previous")
            same(last(b), want[n - 1], f"{n} frames: last")
        assert b.lane_stats()["calls"] == calls, (b.lane_stats(), calls)

        # 3. the capture's loop with a read of the frame before at every step
        got = []
        for i in range(8):
            stage(i); b.fit(ITERS, flags=fast)
            if i > 0:
                got.append(b.get_previous())
        b.sync()
        got.append(last(b))
        for i, g in enumerate(got):
            same(g, want[i], f"streamed frame {i}")
        out["streamed_params"] = np.concatenate([g[0] for g in got])

        # 4. irregular orders, with a group held open wherever the width allows one
        stage(0); b.fit(ITERS, flags=fast)
        stage(1); b.fit(ITERS, flags=fast)
        same(b.get_previous(), want[0], "previous and last in one group")
        stage(2); b.fit(ITERS, flags=fast)
        same(b.get_previous(), want[1], "previous in the group before the last fit's")
        stage(2); stage(3)                                   # two stagings before one fit
        b.fit(ITERS, flags=fast)
        same(b.get_previous(), want[2], "previous after a double staging")
        same(last(b), want[3], "result straight after a fit")
        stage(4); b.fit(ITERS, flags=fast)
        stage(5); b.fit(ITERS, flags=fast)
        same(b.get_previous(), want[4], "previous after a drained read")
        for _ in range(5):                                   # un-staged re-fits, then a staging into the arena they read
            b.fit(ITERS, flags=fast)
        same(b.get_previous(), want[5], "previous among re-fits")
        stage(6); b.fit(ITERS, flags=fast)
        stage(5); b.fit(ITERS, flags=fast)
        same(b.get_previous(), want[6], "previous after re-used inputs")
        same(last(b), want[5], "re-staged arena")
        # a continuing (non-reset) fit straight behind a held lane fit continues that fit's optimiser
        cont = alone(frames[7], cams, more=7)
        stage(6); b.fit(ITERS, flags=fast)
        stage(7); b.fit(ITERS, flags=fast)
        b.fit(7, flags=_lib.FIT_FETCH)
        same(last(b), cont[1], "continuing fit behind a held lane fit")
        # synchronous setters in between, then lane fits from the setters' inputs and a plain fit
        stage(2); b.fit(ITERS, flags=fast)
        b.set_keypoints(frames[1][2], frames[1][3]); b.set_init(frames[1][4], frames[1][5])
        b.fit(ITERS, flags=fast); b.fit(ITERS, flags=fast)
        same(b.get_previous(), want[1], "previous of lane fits from the setters' inputs")
        same(last(b), want[1], "lane fits from the setters' inputs")
        b.fit(ITERS, flags=_lib.FIT_RESET)
        same(last(b), want[1], "plain (timed) fit after lane fits")
        # destroyed with a group held and a slot staged past it; the device is fine afterwards
        stage(0); b.fit(ITERS, flags=fast)
        stage(3); b.fit(ITERS, flags=fast)
        stage(4)
        b.close()
        c = N.FrameBatch(dev, 1, VIEWS)
        c.set_cameras(*cams); c.set_keypoints(frames[2][2], frames[2][3]); c.set_init(frames[2][4], frames[2][5])
        c.fit(ITERS)
        same(last(c), want[2], "a batch after a destroy with a group held")
        c.close()

        # 5. a 32-frame batch streamed through the lanes: two calls per launch at most
        big = sets(32, 4, 100)
        cams32 = (big[0][0], big[0][1])
        wbig = [alone(p, cams32)[0] for p in big]
        b = N.FrameBatch(dev, 32, VIEWS)
        b.set_cameras(*cams32)
        assert b.lane_stats()["width"] == min(width, 2), b.lane_stats()
        got = []
        order = (0, 1, 2, 3, 1, 0)
        for i, s in enumerate(order):
            _, _, kp, ndiv, betas, pose = big[s]
            b.stage_inputs(kp, ndiv, betas, pose)
            b.fit(ITERS, flags=fast)
            if i > 0:
                got.append(b.get_previous())
        got.append(last(b))
        for g, s in zip(got, order):
            same(g, wbig[s], f"32-frame set {s}")
        assert b.lane_stats()["calls"] == len(order)
        out["batch32_params"] = np.concatenate([g[0] for g in got])
        b.close()

        # 6. a 4-frame batch: its result mesh is bf_mesh_multi_kernel, which tiles over frames - a group's tail gives every call a pass
        #    of its own at the call's offset into the state, vertex and extra-joint partial arrays.  Groups of up to `width` calls
        small = sets(4, 5, 300)
        cams4 = (small[0][0], small[0][1])
        wsmall = [alone(p, cams4)[0] for p in small]
        b = N.FrameBatch(dev, 4, VIEWS)
        b.set_cameras(*cams4)
        assert b.lane_stats()["width"] == width, b.lane_stats()
        order = (0, 1, 2, 3, 4, 2, 0, 3, 1, 4)
        for s in order:                                      # no reads: groups as large as the setting lets them grow
            _, _, kp, ndiv, betas, pose = small[s]
            b.stage_inputs(kp, ndiv, betas, pose)
            b.fit(ITERS, flags=fast)
        b.sync()
        same(b.get_previous(), wsmall[order[-2]], "4-frame set before the last")
        same(last(b), wsmall[order[-1]], "last 4-frame set")
        st = b.lane_stats()
        assert st["calls"] == len(order), st
        if fill:
            assert (st["launches"], st["max_group"]) == {3: (4, 3), 8: (2, 8)}[width], st
        got = []
        for i, s in enumerate(order):
            _, _, kp, ndiv, betas, pose = small[s]
            b.stage_inputs(kp, ndiv, betas, pose)
            b.fit(ITERS, flags=fast)
            if i > 0:
                got.append(b.get_previous())
        got.append(last(b))
        for g, s in zip(got, order):
            same(g, wsmall[s], f"4-frame set {s}")
        out["batch4_params"] = np.concatenate([g[0] for g in got])
        b.close()
        dev.close()
        return out

    _run(out_path, body)
