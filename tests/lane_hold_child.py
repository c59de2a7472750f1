"""The idle rule's hold (BF_FIT_LANE_HOLD_US) and the one-launch group tail, in FRESH processes (tests/test_gpu_lane_hold.py): the
library reads its BF_* settings once, so every setting gets a child of its own.  Small shapes: 5 views, 20 iterations, the synthetic
adult SMPL and the dense-skinning and kid models of tests/width_variants.py.  Every streamed result is held bit for bit against the
same frames fitted alone by a plain (timed, lane-free) call in the same process; a batch's results are read through get_previous and
get_result, which expose the last two calls, so a group's slots are read as the last two calls of groups of every size up to it."""
import os
import sys
import time

import numpy as np

from lanes_child import _run

VIEWS, ITERS = 5, 20
NAMES = ("params", "vertices", "joints", "full_pose", "loss_terms")


def _env(width, fill, hold_us):
    for k in ("BF_FIT_LANE_WIDTH", "BF_FIT_LANE_FILL", "BF_FIT_LANES", "BF_FIT_LANE_HOLD_US"):
        os.environ.pop(k, None)
    os.environ["BF_FIT_LANE_WIDTH"] = str(width)         # (before libbodyfit is loaded: the library reads them once)
    os.environ["BF_FIT_LANE_FILL"] = str(fill)
    if hold_us is not None:
        os.environ["BF_FIT_LANE_HOLD_US"] = str(hold_us)


def _tools():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if repo not in sys.path:
        sys.path.insert(0, repo)
    from bodyfitting_amd import _lib, native as N, synthetic as S
    return _lib, N, S


def same(got, want, what):
    for x, y, name in zip(got, want, NAMES):
        assert np.array_equal(x, y), f"{what}: {name} differs from the frames fitted alone (max |diff| {np.abs(x - y).max():.3g})"


def last(q):
    return (q.get_params(),) + q.get_result()


def alone(N, dev, packed, cams):
    _, _, kp, ndiv, betas, pose = packed
    r = N.FrameBatch(dev, kp.shape[0], VIEWS)
    r.set_cameras(*cams); r.set_keypoints(kp, ndiv); r.set_init(betas, pose)
    r.fit(ITERS)
    res = last(r)
    r.close()
    return res


def hold(out_path, width, hold_us, mode):
    """mode "fast": eight pairs back to back; "slow": six pairs 5 ms apart; "off": both loops, only the bits and W = 1's launch per call"""
    _env(width, 0, hold_us)

    def body():
        _lib, N, S = _tools()
        fast = _lib.FIT_RESET | _lib.FIT_FETCH | _lib.FIT_NOTIME
        model = S.make_model("smpl", seed=0)
        dev = N.DeviceModel(model, S.make_gmm(seed=0), device=0)
        frames = [N.pack_problem([S.make_problem(model, frame=s, n_views=VIEWS)]) for s in range(8)]
        cams = (frames[0][0], frames[0][1])
        want = [alone(N, dev, p, cams) for p in frames]

        def fresh():
            q = N.FrameBatch(dev, 1, VIEWS)
            q.set_cameras(*cams)
            return q, (lambda s: q.stage_inputs(frames[s][2], frames[s][3], frames[s][4], frames[s][5]))

        out = {}
        if mode in ("fast", "off"):
            b, stage = fresh()
            for i in range(8):                               # a burst: nothing between the pairs
                stage(i); b.fit(ITERS, flags=fast)
            b.sync()
            st = b.lane_stats()
            assert st["width"] == width and st["calls"] == 8, st
            if mode == "fast":                               # the first call goes out alone; seven are held and sent by the sync
                assert (st["launches"], st["max_group"]) == (2, 7), st
            if width == 1:
                assert (st["launches"], st["max_group"]) == (8, 1), st
            same(b.get_previous(), want[6], "burst: frame 6 of eight")
            same(last(b), want[7], "burst: frame 7 of eight")
            b.close()
            # ... every frame of the burst: the same loop with a read of the frame before at every step
            b, stage = fresh()
            got = []
            for i in range(8):
                stage(i); b.fit(ITERS, flags=fast)
                if i > 0:
                    got.append(b.get_previous())
            b.sync()
            got.append(last(b))
            for i, g in enumerate(got):
                same(g, want[i], f"burst with reads: frame {i}")
            out["burst_params"] = np.concatenate([g[0] for g in got])
            # ... and without reads, every frame as the last two of a burst of its length
            for n in range(1, 9):
                for i in range(n):
                    stage(i); b.fit(ITERS, flags=fast)
                b.sync()
                if n >= 2:
                    same(b.get_previous(), want[n - 2], f"burst of {n}: previous")
                same(last(b), want[n - 1], f"burst of {n}: last")
            b.close()
        if mode in ("slow", "off"):
            b, stage = fresh()
            got = []
            for i in range(6):
                if i:
                    time.sleep(0.005)                        # a feeder slower than a call per H: every call finds its lane idle and goes out alone
                stage(i); b.fit(ITERS, flags=fast)
                if i > 0:
                    got.append(b.get_previous())
            b.sync()
            got.append(last(b))
            st = b.lane_stats()
            assert st["calls"] == 6, st
            if mode == "slow" or width == 1:
                assert (st["launches"], st["max_group"]) == (6, 1), st
            for i, g in enumerate(got):
                same(g, want[i], f"slow feeder: frame {i}")
            out["slow_params"] = np.concatenate([g[0] for g in got])
            b.close()
        dev.close()
        return out

    _run(out_path, body)


def tail(out_path, name):
    """W = 16, forced shapes: the group tail of one-frame calls (a full group: two 8-frame blocks; nine calls: a one-frame last block) and
    of two-frame calls (five calls: the call boundaries off the 8-frame blocks), on model `name` ("smpl": the synthetic adult)"""
    _env(16, 1, None)

    def body():
        _lib, N, S = _tools()
        from width_variants import Variants, smpl_problem
        fast = _lib.FIT_RESET | _lib.FIT_FETCH | _lib.FIT_NOTIME
        variants = None
        if name == "smpl":
            model = S.make_model("smpl", seed=0)
            dev = N.DeviceModel(model, S.make_gmm(seed=0), device=0)
            problem = lambda f: S.make_problem(model, frame=f, n_views=VIEWS)          # noqa: E731
        else:
            variants = Variants(S.make_gmm(seed=0))
            model, dev = variants.get(name)
            problem = lambda f: smpl_problem(name, model, frame=f, n_views=VIEWS)      # noqa: E731
        out = {}

        def run(n_frames, sizes, full):
            """groups of every size in `sizes` (a sync ends each), the last two calls of each read; `full`: the size that fills a group itself"""
            frames = [N.pack_problem([problem(10 * s + f) for f in range(n_frames)]) for s in range(max(sizes))]
            cams = (frames[0][0], frames[0][1])
            want = [alone(N, dev, p, cams) for p in frames]
            b = N.FrameBatch(dev, n_frames, VIEWS)
            b.set_cameras(*cams)
            assert b.lane_stats()["width"] == 16, b.lane_stats()
            calls = 0
            for n in sizes:
                before = b.lane_stats()["launches"]
                for i in range(n):
                    b.stage_inputs(frames[i][2], frames[i][3], frames[i][4], frames[i][5]); b.fit(ITERS, flags=fast)
                calls += n
                if n == full:
                    assert b.lane_stats()["launches"] == before + 1, "a full group goes out with its last call"
                b.sync()
                st = b.lane_stats()
                assert st["launches"] == before + 1 and st["calls"] == calls, (n, st)          # ONE group of n calls
                if n >= 2:
                    same(b.get_previous(), want[n - 2], f"{name}, {n_frames}-frame calls, group of {n}: previous")
                same(last(b), want[n - 1], f"{name}, {n_frames}-frame calls, group of {n}: last")
            assert b.lane_stats()["max_group"] == max(sizes), b.lane_stats()
            key = f"params_{n_frames}"
            out[key] = np.concatenate([w[0] for w in want])
            b.close()

        # one-frame calls: the full group and the group of nine first, then every other size - every slot of both blocks is read
        run(1, (16, 9) + tuple(n for n in range(1, 16) if n != 9), 16)
        if name == "smpl":
            run(2, (5, 1, 2, 3, 4), 0)                        # two-frame calls: 10, 2, 4, 6 and 8 frames
        dev.close()
        if variants is not None:
            variants.close()
        return out

    _run(out_path, body)
