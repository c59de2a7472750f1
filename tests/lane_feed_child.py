"""How the fit lanes are fed (bf_batch_lane_feed_stats), under BF_FIT_LANE_WIDTH / BF_FIT_LANE_FILL in FRESH processes
(tests/test_gpu_lane_feed.py): both are read once per process, so every (width, fill) gets a child of its own.  With W > 1 a staging
packs into a pinned slot and issues nothing, a group's launch carries ONE input transfer, a call without a staging of its own copies
its inputs on the host while their pinned copy is valid and on the device after a drain, and a group is fed one way only.  Every
result is held against the same frame fitted alone by a plain (timed, lane-free) call in the same process; the counts that a forced
group shape fixes are asserted at (3, 1).  The streamed parameters go to the parent, which compares them across settings."""
import os
import sys

import numpy as np

from lanes_child import _run

VIEWS, ITERS = 12, 30


def feed(out_path, width, fill):
    os.environ["BF_FIT_LANE_WIDTH"] = str(width)        # (before libbodyfit is loaded: the library reads them once)
    os.environ["BF_FIT_LANE_FILL"] = str(fill)
    os.environ.pop("BF_FIT_LANES", None)

    def body():
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        if repo not in sys.path:
            sys.path.insert(0, repo)
        from bodyfitting_amd import _lib, native as N, synthetic as S
        fast = _lib.FIT_RESET | _lib.FIT_FETCH | _lib.FIT_NOTIME
        forced3 = (width, fill) == (3, 1)
        model = S.make_model("smpl", seed=0)
        dev = N.DeviceModel(model, S.make_gmm(seed=0), device=0)
        out = {}

        def sets(n_frames, n_sets, base, views=VIEWS):
            return [N.pack_problem([S.make_problem(model, frame=base + 10 * s + f, n_views=views) for f in range(n_frames)]) for s in range(n_sets)]

        def alone(packed, cams, iters=ITERS):
            _, _, kp, ndiv, betas, pose = packed
            r = N.FrameBatch(dev, kp.shape[0], kp.shape[1])
            r.set_cameras(*cams); r.set_keypoints(kp, ndiv); r.set_init(betas, pose)
            r.fit(iters)
            res = (r.get_params(),) + r.get_result()
            r.close()
            return res

        def same(got, want, what):
            for x, y, name in zip(got, want, ("params", "vertices", "joints", "full_pose", "loss_terms")):
                assert np.array_equal(x, y), f"{what}: {name} differs from the frame fitted alone (max |diff| {np.abs(x - y).max():.3g})"

        last = lambda q: (q.get_params(),) + q.get_result()
        stats = lambda q: {**q.lane_stats(), **q.lane_feed_stats()}

        # the references, once: ten distinct frames fitted alone
        frames = sets(1, 10, 0)
        cams = (frames[0][0], frames[0][1])
        want = [alone(p, cams) for p in frames]

        def fresh():
            q = N.FrameBatch(dev, 1, VIEWS)
            q.set_cameras(*cams)
            return q, (lambda s: q.stage_inputs(frames[s][2], frames[s][3], frames[s][4], frames[s][5]))

        # 1. transfers: seven stage + fit pairs and a sync - one transfer per launch (W = 1: per staged call), no copies
        b, stage = fresh()
        for i in range(7):
            stage(i); b.fit(ITERS, flags=fast)
        b.sync()
        st = stats(b)
        assert st["width"] == width and st["calls"] == 7, st
        assert (st["host_copies"], st["device_copies"]) == (0, 0), st
        if width == 1:
            assert (st["launches"], st["transfers"]) == (7, 7), st
        else:
            assert st["transfers"] == st["launches"], st
        if forced3:
            assert (st["launches"], st["transfers"], st["max_group"]) == (3, 3, 3), st
        same(b.get_previous(), want[5], "transfers: frame 5 of seven")
        same(last(b), want[6], "transfers: frame 6 of seven")
        # ... and the capture's loop with a read of the frame before at every step: what the parent compares across settings
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
        b.close()

        # 2. re-fits by host copy: a staged fit, four calls without a staging of their own, a staged fit
        b, stage = fresh()
        stage(0); b.fit(ITERS, flags=fast)
        for k in range(4):
            b.fit(ITERS, flags=fast)
            same(b.get_previous(), want[0], f"re-fit {k}: the fit before it")
        stage(1); b.fit(ITERS, flags=fast)
        same(b.get_previous(), want[0], "the last re-fit")
        same(last(b), want[1], "the staged fit behind the re-fits")
        st = stats(b)
        assert st["device_copies"] == 0 and st["host_copies"] == (4 if width > 1 else 0), st
        # ... the same without reads in between, so that re-fits share a group with the call they copy from
        for _ in range(2):
            stage(2); b.fit(ITERS, flags=fast)
            b.fit(ITERS, flags=fast); b.fit(ITERS, flags=fast); b.fit(ITERS, flags=fast)
            b.sync()
            same(b.get_previous(), want[2], "re-fits in one group: the one before the last")
            same(last(b), want[2], "re-fits in one group: the last")
        st = stats(b)
        assert st["device_copies"] == 0 and st["host_copies"] == (10 if width > 1 else 0), st
        b.close()

        # 3. kind switch: a host-fed group held open, setters (they drain), two device-fed calls, then a staged one
        b, stage = fresh()
        stage(0); b.fit(ITERS, flags=fast)
        stage(1); b.fit(ITERS, flags=fast)
        b.set_keypoints(frames[2][2], frames[2][3]); b.set_init(frames[2][4], frames[2][5])
        b.fit(ITERS, flags=fast); b.fit(ITERS, flags=fast)
        stage(3); b.fit(ITERS, flags=fast)
        st = stats(b)
        assert st["calls"] == 5, st
        if width > 1:
            assert st["device_copies"] >= 1 and st["host_copies"] == 0, st
        b.sync()
        st = stats(b)
        if forced3:         # [0, 1] by the drain | the two device-fed calls, sent out by the staged call | the staged call, by the sync
            assert (st["launches"], st["max_group"], st["transfers"], st["device_copies"]) == (3, 2, 2, 2), st
        same(b.get_previous(), want[2], "the second device-fed call")
        same(last(b), want[3], "the host-fed call behind the device-fed group")
        # ... and device-fed re-fits of a frame that was staged, after a read drained the lanes
        b.fit(ITERS, flags=fast); b.fit(ITERS, flags=fast)
        same(b.get_previous(), want[3], "device-fed re-fit of a staged frame")
        same(last(b), want[3], "device-fed re-fit of a staged frame, the last")
        b.close()

        # 4. staged past the group: the open group goes out by a drain with a slot staged past it, and a plain fit reads that slot on
        #    the device; then a slot staged with no call joined at all
        b, stage = fresh()
        stage(0); b.fit(ITERS, flags=fast)
        stage(1)
        b.fit(ITERS, flags=_lib.FIT_RESET)
        same(last(b), want[1], "plain fit of a frame staged past the open group")
        stage(2)
        b.fit(ITERS, flags=_lib.FIT_RESET)
        same(last(b), want[2], "plain fit of a frame staged with no call joined")
        st = stats(b)
        # (forced shape: the group of one and the slot past it share a transfer; otherwise the first fit found its lane idle and went out alone)
        assert st["calls"] == 1 and st["transfers"] == (2 if forced3 else 3), st
        b.close()

        # 5. double staging before one fit; destroyed with a group held and a slot staged past it; the device is fine afterwards
        b, stage = fresh()
        stage(2); stage(3)
        b.fit(ITERS, flags=fast)
        stage(4); b.fit(ITERS, flags=fast)
        same(b.get_previous(), want[3], "the fit behind a double staging")
        stage(5); stage(6)
        b.fit(ITERS, flags=fast)
        stage(7)
        b.close()
        c = N.FrameBatch(dev, 1, VIEWS)
        c.set_cameras(*cams); c.set_keypoints(frames[2][2], frames[2][3]); c.set_init(frames[2][4], frames[2][5])
        c.fit(ITERS)
        same(last(c), want[2], "a batch after a destroy with a group held")
        c.close()

        # 6. arena re-use under back-pressure: every pinned arena of every lane is filled again (2 arenas x 4 lanes x 3 slots + 6 at
        #    W = 3) with no read in between
        b, stage = fresh()
        for i in range(30):
            stage(i % 10); b.fit(ITERS, flags=fast)
        same(b.get_previous(), want[8], "back-pressure: frame 28 of thirty")
        same(last(b), want[9], "back-pressure: frame 29 of thirty")
        st = stats(b)
        assert st["calls"] == 30 and st["waits"] >= 0, st
        if forced3:
            assert (st["launches"], st["transfers"]) == (10, 10), st
        b.close()

        # 7. 50 views: more than the fit kernel keeps in registers - it reads the keypoints inside the loop, from the device arena
        wide = sets(1, 3, 50, views=50)
        cams50 = (wide[0][0], wide[0][1])
        wwide = [alone(p, cams50, iters=10) for p in wide]
        b = N.FrameBatch(dev, 1, 50)
        b.set_cameras(*cams50)
        for order in ((0, 1, 2), (2, 0, 1)):
            for s in order:
                b.stage_inputs(wide[s][2], wide[s][3], wide[s][4], wide[s][5]); b.fit(10, flags=fast)
            b.sync()
            same(b.get_previous(), wwide[order[1]], "50 views: slot 1")
            same(last(b), wwide[order[2]], "50 views: slot 2")
        for s in (1, 2):
            b.stage_inputs(wide[s][2], wide[s][3], wide[s][4], wide[s][5]); b.fit(10, flags=fast)
        same(b.get_previous(), wwide[1], "50 views: slot 0")
        st = stats(b)
        if forced3:
            assert (st["launches"], st["transfers"], st["max_group"]) == (3, 3, 3), st
        b.close()

        # 8. a 4-frame batch: ten calls cycling five frame sets
        small = sets(4, 5, 300)
        cams4 = (small[0][0], small[0][1])
        wsmall = [alone(p, cams4) for p in small]
        b = N.FrameBatch(dev, 4, VIEWS)
        b.set_cameras(*cams4)
        order = (0, 1, 2, 3, 4, 2, 0, 3, 1, 4)
        for s in order:                                      # no reads: groups as large as the setting lets them grow
            b.stage_inputs(small[s][2], small[s][3], small[s][4], small[s][5]); b.fit(ITERS, flags=fast)
        b.sync()
        same(b.get_previous(), wsmall[order[-2]], "4-frame set before the last")
        same(last(b), wsmall[order[-1]], "last 4-frame set")
        st = stats(b)
        if forced3:
            assert (st["launches"], st["transfers"], st["max_group"]) == (4, 4, 3), st
        got = []
        for i, s in enumerate(order):
            b.stage_inputs(small[s][2], small[s][3], small[s][4], small[s][5]); b.fit(ITERS, flags=fast)
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
