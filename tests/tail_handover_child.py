"""The tail that hands its results over itself (BF_TAIL_HANDOVER=store: the mesh and joints kernels store into the pinned mirror) against
the copy behind the tail (=copy) and the library's own choice by size (unset), and the one-kernel drain, in FRESH processes
(tests/test_gpu_tail_handover.py): the library reads its BF_* settings once, so every setting gets a child of its own.  Small shapes: 5 views, at most 10 iterations.  Every streamed result is
held bit for bit against the same frames fitted alone by a plain (timed, lane-free) call in the same process - a route that hands over
by a copy command in either setting - and stored for the parent to hold the settings against each other.  A batch's results are read
through get_previous and get_result, which expose the last two calls of a burst."""
import os
import sys

import numpy as np

from lanes_child import _run

VIEWS, ITERS = 5, 10
NAMES = ("params", "vertices", "joints", "full_pose", "loss_terms")


def _env(mode, lanes=None):
    for k in ("BF_FIT_LANE_WIDTH", "BF_FIT_LANE_FILL", "BF_FIT_LANES", "BF_FIT_LANE_HOLD_US", "BF_TAIL_HANDOVER"):
        os.environ.pop(k, None)
    if mode != "by-size":                                # (unset: the library chooses by the tail's size)
        os.environ["BF_TAIL_HANDOVER"] = mode            # (before libbodyfit is loaded: the library reads them once)
    os.environ["BF_FIT_LANE_WIDTH"] = "16"
    os.environ["BF_FIT_LANE_FILL"] = "1"
    if lanes is not None:
        os.environ["BF_FIT_LANES"] = str(lanes)


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


class Alone:
    """frame sets fitted alone by plain timed calls on a batch of their own: computed once per frame set and iteration count"""

    def __init__(self, _lib, N, dev, cams):
        self._lib, self.N, self.dev, self.cams, self.cache = _lib, N, dev, cams, {}

    def __call__(self, key, packed, iters=ITERS, more=0, grad=False):
        k = (key, iters, more, grad)
        if k not in self.cache:
            _, _, kp, ndiv, betas, pose = packed
            r = self.N.FrameBatch(self.dev, kp.shape[0], VIEWS)
            r.set_cameras(*self.cams); r.set_keypoints(kp, ndiv); r.set_init(betas, pose)
            r.fit(iters)
            if more:
                r.fit(more, flags=self._lib.FIT_FETCH)
            res = last(r)
            if grad:
                res = res + r.loss_grad()
            r.close()
            self.cache[k] = res
        return self.cache[k]


def _model(S, N, name):
    """("smpl690": the synthetic adult at 690 vertices; "smpl": at full size; else a variant of tests/width_variants.py) -> model, device
    model, problem(frame), closer"""
    if name in ("smpl", "smpl690"):
        model = S.make_model("smpl", seed=0, nv=690 if name == "smpl690" else None)
        dev = N.DeviceModel(model, S.make_gmm(seed=0), device=0)
        return model, dev, (lambda f: S.make_problem(model, frame=f, n_views=VIEWS)), dev.close
    from width_variants import Variants, smpl_problem
    variants = Variants(S.make_gmm(seed=0))
    model, dev = variants.get(name)
    return model, dev, (lambda f: smpl_problem(name, model, frame=f, n_views=VIEWS)), variants.close


def groups(out_path, mode, name, sizes, sizes2=()):
    """Forced shapes at W = 16: bursts of one-frame calls, one group each (`sizes`, then the same sizes again with every frame moved one
    slot on: each lane arena is used again and a mirror left from its first use would show), then bursts of two-frame calls (`sizes2`);
    then what a drain leaves in the batch's own buffers: the device arena against the mirror, a continuing fit, parameters and gradient."""
    _env(mode)

    def body():
        _lib, N, S = _tools()
        fast = _lib.FIT_RESET | _lib.FIT_FETCH | _lib.FIT_NOTIME
        model, dev, problem, close = _model(S, N, name)
        out = {n: [] for n in NAMES}

        def keep(res):
            for n, x in zip(NAMES, res):
                out[n].append(np.asarray(x).ravel())

        def run(n_frames, sizes, shifts):
            most = max(sizes) + max(shifts)
            frames = [N.pack_problem([problem(10 * s + f) for f in range(n_frames)]) for s in range(most)]
            cams = (frames[0][0], frames[0][1])
            alone = Alone(_lib, N, dev, cams)
            b = N.FrameBatch(dev, n_frames, VIEWS)
            b.set_cameras(*cams)
            assert b.lane_stats()["width"] == 16, b.lane_stats()
            stage = lambda s: b.stage_inputs(frames[s][2], frames[s][3], frames[s][4], frames[s][5])      # noqa: E731
            for shift in shifts:
                for n in sizes:
                    before = b.lane_stats()["launches"]
                    for i in range(n):
                        stage(i + shift); b.fit(ITERS, flags=fast)
                    b.sync()
                    assert b.lane_stats()["launches"] == before + 1, (n, b.lane_stats())      # ONE group of n calls
                    what = f"{name} [{mode}], {n_frames}-frame calls, group of {n}, frames from {shift}"
                    if n >= 2:
                        prev = b.get_previous()
                        same(prev, alone(n - 2 + shift, frames[n - 2 + shift]), what + ": previous")
                        keep(prev)
                    res = last(b)
                    same(res, alone(n - 1 + shift, frames[n - 1 + shift]), what + ": last")
                    keep(res)
                    # after the drain the batch's device arena holds what its mirror holds
                    assert np.array_equal(b.debug_vertices(), res[1]), what + ": the device arena's vertices differ from the mirror's"
            # a group of three (the drain hands back slot 2), then a continuing fit: the drain's parameters and Adam moments
            for i in range(3):
                stage(i); b.fit(7, flags=fast)
            b.fit(3, flags=_lib.FIT_FETCH)
            res = last(b)
            same(res, alone(2, frames[2], iters=7, more=3), f"{name} [{mode}]: fit(3) behind a streamed fit(7) against the same two calls alone")
            same(res, alone(2, frames[2], iters=10), f"{name} [{mode}]: fit(3) behind a streamed fit(7) against fit(10) alone")
            keep(res)
            # ... and parameters and gradient read straight after a drain: the drain's slices under the batch's views
            for i in range(3):
                stage(i); b.fit(ITERS, flags=fast)
            want = alone(2, frames[2], grad=True)
            assert np.array_equal(b.get_params(), want[0]), f"{name} [{mode}]: get_params after a drain"
            terms, grads = b.loss_grad()
            assert np.array_equal(terms, want[5]) and np.array_equal(grads, want[6]), f"{name} [{mode}]: loss_grad after a drain"
            out["params"].append(grads.ravel())
            b.close()

        run(1, sizes, (0, 1))
        if sizes2:
            run(2, sizes2, (0,))
        close()
        return {n: np.concatenate(v) for n, v in out.items()}

    _run(out_path, body)


def aside(out_path, mode, name):
    """BF_FIT_LANES=1: frame after frame on the single-stream path, each call's tail on the second stream (enqueue_tail), G = 1"""
    _env(mode, lanes=1)

    def body():
        _lib, N, S = _tools()
        fast = _lib.FIT_RESET | _lib.FIT_FETCH | _lib.FIT_NOTIME
        model, dev, problem, close = _model(S, N, name)
        out = {n: [] for n in NAMES}
        frames = [N.pack_problem([problem(10 * s)]) for s in range(4)]
        cams = (frames[0][0], frames[0][1])
        alone = Alone(_lib, N, dev, cams)
        b = N.FrameBatch(dev, 1, VIEWS)
        b.set_cameras(*cams)
        assert b.lane_stats()["width"] == 1, b.lane_stats()
        got = []
        for rnd in range(2):                                  # (twice: both arenas are used again, with other frames in them)
            order = (0, 1, 2, 3) if rnd == 0 else (3, 2, 1, 0, 2)
            for i, s in enumerate(order):
                b.stage_inputs(frames[s][2], frames[s][3], frames[s][4], frames[s][5]); b.fit(ITERS, flags=fast)
                if i > 0:
                    got.append((order[i - 1], b.get_previous()))
            b.sync()
            res = last(b)
            got.append((order[-1], res))
            assert np.array_equal(b.debug_vertices(), res[1]), f"{name} [{mode}]: the device arena's vertices differ from the mirror's"
        assert b.lane_stats()["calls"] == 0, b.lane_stats()
        for s, g in got:
            same(g, alone(s, frames[s]), f"{name} [{mode}], tail aside: frame {s}")
            for n, x in zip(NAMES, g):
                out[n].append(np.asarray(x).ravel())
        b.close()
        close()
        return {n: np.concatenate(v) for n, v in out.items()}

    _run(out_path, body)
