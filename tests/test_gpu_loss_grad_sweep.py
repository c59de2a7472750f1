"""The hand-derived gradient of the multi-view keypoint objective, swept: bf_loss_grad (fit_kernels.hip's sized SMPL instance and
its table-driven instance; for SMPL-X bf_kp_loss_body + joints_body.h) against float64 torch autograd of oracle/smplify_oracle.py
at every case of tests/loss_grad_cases.py - view counts across every staging edge of both kernels, all 79 face-contour rows, every
GMM component, non-default hyper-parameters, prior / pose extremes, keypoint edges and one joint angle swept from 1e-6 rad to beyond
4 pi (axis R: every quadrant, wrap and rounding edge of sincos_small, either side of rodrigues_fwd's Taylor switch;
profiles/rodrigues_sweep.md) - and, for a subset, ten Adam steps from the
case's point against the oracle's loop (the loop consumes the same gradient).  tests/test_loss_grad_cases.py proves on the CPU
that every case is well posed, so nothing is skipped or filtered here: every case, every term, every component of every block.

Bands (loss_grad_cases.band, nothing calibrated against the kernels): per parameter block, with g64 the float64 oracle, g32 torch's
float32 autograd of the same oracle at the same point and M = max|g64|,

    err = max|hip - g64|      err32 = max|g32 - g64|      band = max(5e-6 * M, 8 * err32)

5e-6 * M is what test_gpu_parity.py::test_loss_terms_and_gradient holds at the baseline point; 2e-5 * M replaces it for SMPL-kind
cases with more than 48 views (test_more_than_48_views_streams_the_rest's existing band); the second term follows the reference's
own float32 error where the arithmetic is harder.  Terms: relative, max(3e-6, 8 * rel32).  Blocks a case declares zero (the
priors-only variants) must be exactly zero.

The dense kernel keeps the views' projection matrices in LDS while V * 12 + 3 <= 1024 + nl * 3; with SMPL-X's nl = 135 loss joints
that is V * 12 <= 1426, V <= 118, and from V = 119 on it reads them from global memory: axis B straddles that switch.

Run with -s to see, per axis, the worst err / band and err / err32 (profiles/loss_grad_sweep.md holds one run's table).
"""
import warnings

import numpy as np
import pytest
import torch

from bodyfitting_amd import _lib
from bodyfitting_amd import native as N
import loss_grad_cases as LC

pytestmark = pytest.mark.gpu
CASES = LC.all_cases()
LOOPS = LC.loop_cases()
FIT_TOL = 1e-4             # the project's band on fitted parameters
JOINT_TOL = 3e-6           # the existing band of forward_packed's joints (test_gpu_smplx.py)
RESULTS = []               # (axis, case id, block, err, M, err32, band) of every compared block, for the report
FIRST = {}                 # (kind, size) -> (terms, grads) of the default-hyper case's first evaluation


@pytest.fixture(scope="module")
def devs(dev_model):
    """device models by (kind, size), created on first use; the full-size SMPL model is the suite's shared one"""
    made = {("smpl", "full"): dev_model}

    def get(kind, size):
        if (kind, size) not in made:
            made[(kind, size)] = N.DeviceModel(LC.model(kind, size), LC.gmm(), device=0)
        return made[(kind, size)]
    yield get
    for key, m in made.items():
        if key != ("smpl", "full"):
            m.close()


def _batch(dev, prob):
    c2w, K, kp, ndiv, betas, pose = N.pack_problem([prob])
    b = N.FrameBatch(dev, 1, c2w.shape[1])
    b.set_cameras(c2w, K)
    b.set_keypoints(kp, ndiv)
    b.set_init(betas, pose)
    return b


def _split(dev, packed):
    return N.split_params(packed, dev.n_joints, dev.n_betas)


def _hyper(case):
    kw = case.library_hyper()
    default = N.make_hyper()
    if all(getattr(default, k) == float(v) for k, v in kw.items()):
        return None                                           # (the library's own defaults: the NULL hyper of every other test)
    return N.make_hyper(**kw)


def _loss_grad(dev, case):
    b = _batch(dev, case.problem)
    try:
        b.set_params(N.pack_params(case.params)[None])
        terms, grads = b.loss_grad(_hyper(case))
    finally:
        b.close()
    return terms[0].copy(), grads[0].copy()


def _oracles(case):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return LC.oracle(case, torch.float64), LC.oracle(case, torch.float32)


@pytest.mark.parametrize("kind", ["smpl", "kid", "smplx"])
def test_largest_view_count_is_what_the_library_accepts(devs, kind):
    """bf_batch_create takes loss_grad_cases.V_MAX views and refuses one more with BF_ERR_UNSUPPORTED, launching nothing"""
    dev = devs(kind, "small")
    N.FrameBatch(dev, 1, LC.V_MAX[kind]).close()
    with pytest.raises(_lib.BodyfitError, match=r"\(-3\).*too many views"):
        N.FrameBatch(dev, 1, LC.V_MAX[kind] + 1)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_terms_and_gradient_match_fp64_autograd(devs, case):
    dev = devs(case.kind, case.size)
    assert dev.fit_instance == ("sized" if case.kind == "smpl" else "table-driven") or case.kind == "smplx"
    terms, grads = _loss_grad(dev, case)
    if case.axis == "E" and case.name == "default-hyper":
        FIRST[(case.kind, case.size)] = (terms, grads)
        # a fit with the default hypers BEFORE the other hypers come: the model's cached LDS image (bf_ensure_fit_image) is built now
        b = _batch(dev, case.problem)
        b.fit(2)
        b.close()
    o64, o32 = _oracles(case)
    got = _split(dev, grads)
    failures = []
    for i, n in enumerate(LC.TERMS):
        t64, t32 = o64["terms"][n], o32["terms"][n]
        if t64 == 0.0:
            ok, rel = float(terms[i]) == 0.0, float(abs(terms[i]))
        else:
            rel = abs(float(terms[i]) - t64) / abs(t64)
            ok = rel <= LC.term_band(t64, t32)
        if not ok:
            failures.append(f"term {n}: {float(terms[i])!r} vs {t64!r} (relative {rel:.2e}, band {LC.term_band(t64, t32):.2e})")
    for k in case.blocks:
        g64 = o64["grads"][k]
        assert got[k].shape == g64.shape, k
        band, M, err32 = LC.band(g64, o32["grads"][k], case.base)
        err = float(np.abs(got[k].astype(np.float64) - g64).max())
        if k in case.zero_blocks:
            np.testing.assert_array_equal(got[k], np.zeros_like(got[k]), err_msg=f"{case.id} {k}")
            continue
        RESULTS.append((case.axis, case.id, k, err, M, err32, band))
        if not err <= band:                                   # (also catches a NaN)
            failures.append(f"{k}: err {err:.3e} = {err / M:.2e} M, band {band:.3e} = {band / M:.2e} M, err32 {err32:.3e}, err / band {err / band:.2f}")
    if case.axis == "C":
        # the 135 joints of the forward pass: the 17 contour landmarks come from the row the neck's yaw selects
        s, c, t = float(case.params["scale"][0]), float(case.problem["constant_scale"]), case.params["global_transl"]
        want = o64["joints"] / (s * c) - t
        _, joints = dev.forward_packed(N.pack_params(case.params)[None])
        jerr = float(np.abs(joints[0] - want).max())
        if not jerr <= JOINT_TOL:
            failures.append(f"joints of the forward pass (oracle row {o64['row']}): max error {jerr:.3e}")
    assert not failures, case.id + "\n  " + "\n  ".join(failures)


@pytest.mark.parametrize("case", LOOPS, ids=[c.id for c in LOOPS])
def test_ten_adam_steps_from_the_case_match_the_oracle_loop(devs, case):
    """bf_batch_set_params resets Adam's moments, so a fit without BF_FIT_RESET after it is the reference loop started at that point"""
    dev = devs(case.kind, case.size)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        want = LC.oracle_loop(case, 10, double=True)
    b = _batch(dev, case.problem)
    try:
        b.set_params(N.pack_params(case.params)[None])
        b.fit(10, _hyper(case))
        got = _split(dev, b.get_params()[0])
    finally:
        b.close()
    worst = {k: float(np.abs(got[k] - np.asarray(want[k], np.float64).reshape(got[k].shape)).max()) for k in case.blocks}
    print(f"\nH {case.id}: max |param - oracle| after 10 steps = {max(worst.values()):.2e}")
    assert max(worst.values()) <= FIT_TOL, worst


@pytest.mark.parametrize("kind,size", LC.HYPER_MODELS, ids=["-".join(x) for x in LC.HYPER_MODELS])
def test_default_hyper_case_is_bit_identical_after_the_other_hypers(devs, kind, size):
    """the first default-hyper evaluation on a device model, then every other hyper (loss_grad and a fit) on the same model, then the
    first case again: same bits.  Nothing a call's hypers decide may outlive the call (the model keeps an LDS image made with the
    hypers of its first fit)."""
    dev = devs(kind, size)
    first = LC.hyper_default_case(kind, size)
    before = FIRST.get((kind, size)) or _loss_grad(dev, first)
    for c in CASES:
        if c.axis == "E" and (c.kind, c.size) == (kind, size) and c.hyper:
            b = _batch(dev, c.problem)
            b.set_params(N.pack_params(c.params)[None])
            t, g = b.loss_grad(_hyper(c))
            assert np.isfinite(t).all() and np.isfinite(g).all()
            b.fit(2, _hyper(c))
            b.close()
    after = _loss_grad(dev, first)
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])


def test_report():
    """per axis: the number of compared blocks, the worst err / band with its case, and the worst err / err32"""
    print("\naxis | cases | blocks | worst case : block | err / M | err32 / M | err / band | worst err / err32")
    for axis, _ in LC.AXES:
        rows = [r for r in RESULTS if r[0] == axis]
        if not rows:
            continue
        w = max(rows, key=lambda r: r[3] / r[6])
        ratio = max((r[3] / r[5] for r in rows if r[5] > 0), default=float("nan"))
        print(f"{axis} | {len({r[1] for r in rows})} | {len(rows)} | {w[1]} : {w[2]} | {w[3] / w[4]:.2e} | {w[5] / w[4]:.2e} | {w[3] / w[6]:.3f} | {ratio:.1f}")
    # axis R by angle group and parameter block (profiles/rodrigues_sweep.md)
    group = {c.id: c.group for c in CASES if c.axis == "R"}
    print("\nR: angle group | block | blocks | worst case | err / M | err32 / M | err / band | worst err / err32")
    for g in ("near zero", "rounding edges of n", "centres and wrap", "far"):
        for k in LC.O.SMPLX_PARAMS:
            rows = [r for r in RESULTS if r[0] == "R" and group[r[1]] == g and r[2] == k]
            if not rows:
                continue
            w = max(rows, key=lambda r: r[3] / r[6])
            ratio = max((r[3] / r[5] for r in rows if r[5] > 0), default=float("nan"))
            print(f"{g} | {k} | {len(rows)} | {w[1]} | {w[3] / w[4]:.2e} | {w[5] / w[4]:.2e} | {w[3] / w[6]:.3f} | {ratio:.1f}")
    assert all(np.isfinite(r[3]) for r in RESULTS)
