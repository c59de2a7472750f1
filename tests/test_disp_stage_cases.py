"""CPU: the cases of tests/disp_stage_cases.py are what they claim to be, with the oracle alone - the valences and face counts, a finite
gradient, well posed (torch's float32 gradient within 1e-5 M of the float64 one, so the band never degenerates; repeated_corner, whose
gradient is 1e8 times the others', excepted) and the share of vertices whose closest scan face is tied under its cap.  The base mesh is
the frame's ground-truth body plus 2 mm of noise (as near its scan as a fit leaves it), at zero displacement: where the stage starts.
The tie share is measured with the reference alone - the vertices at which some other scan face returns the winner's float32 distance
bit for bit, the only ones where a device's search may answer with another face - and bounds what the GPU file may take from the device.
Run with -s for the figures."""
import numpy as np
import pytest

import disp_stage_cases as D
import scan_loss_cases as SC

CASE_FRAMES = [(c, fr) for c in D.CASES for fr in D.FRAMES] + [(D.THREE_FRAME_CASE, D.THIRD_FRAME)]


def test_the_claimed_valences_and_face_counts():
    body = D.body_faces()
    val = D.valence(body)
    assert body.shape == (1376, 3) and val.min() == 3 and val.max() == 11 and (val > D.ADJ_BATCH).sum() == 5     # the issue's histogram
    for k in D.HUBS:
        t = D.topology(f"hub{k}")
        (hub,) = t["marked"]["hub"]
        v = D.valence(t["faces"])
        assert v[hub] == k == t["valence"][hub] and t["nf"] == 1376 + k - 3
        assert val[hub] == 3 and (k <= 11 or v.max() == k)
        np.testing.assert_array_equal(t["faces"][:1376], body)
        assert hub not in t["marked"]["rim"] and len(t["marked"]["rim"]) >= k - 3 + 1
        assert -(-k // D.ADJ_BATCH) == {8: 1, 9: 2, 16: 2, 17: 3, 25: 4}[k]                # batches the walks take at the hub
    t = D.topology("lonely")
    (v0,) = t["marked"]["lonely"]
    v = D.valence(t["faces"])
    assert val[v0] == 11 and v[v0] == 0 and (v == 0).sum() == 1 and t["nf"] == 1376 - 11
    for n in D.FACE_COUNTS:
        t = D.topology(f"nf{n}")
        assert t["nf"] == n and -(-n // SC.BLOCK) == (5 if n <= D.FACE_BLOCK_EDGE else 6)
        np.testing.assert_array_equal(t["faces"], body[:n])
    t = D.topology(D.REPEATED_CORNER)
    assert t["nf"] == 1377 and t["faces"][-1, 0] == t["faces"][-1, 1] != t["faces"][-1, 2]
    for case in D.CASES:
        f = np.asarray(D.model(case)["faces"])
        assert f.dtype == np.asarray(D.base_model()["faces"]).dtype and f.min() >= 0 and f.max() < D.NV
        assert set(D.model(case)) == set(D.base_model())


@pytest.mark.parametrize("case,fr", CASE_FRAMES, ids=[f"{c}-frame{fr[0]}" for c, fr in CASE_FRAMES])
def test_every_case_is_finite_well_posed_and_under_the_tie_cap(case, fr):
    frame, scale = fr
    _, sv, sf = D.scan(frame, scale)
    base = D.cpu_base(frame, scale)
    faces = D.topology(case)["faces"]
    r = D.reference(faces, sv, sf, base, np.zeros_like(base))
    M, err32 = float(np.abs(r["g64"]).max()), float(np.abs(r["g32"] - r["g64"]).max())
    share = D.tie_share(sv, sf, base)
    print(f"    {case} frame {frame}: M {M:.3e}, err32 {err32:.3e} = {err32 / M:.2e} M, tied vertices {share:.4f}")
    assert np.isfinite(r["g64"]).all() and np.isfinite(r["g32"]).all() and M > 0
    assert share < D.TIE_CAP
    if case != D.REPEATED_CORNER:
        SC.well_posed(f"{case} frame {frame}", r["g64"], r["g32"])


def test_the_read_out_of_a_gradient_from_the_moments():
    """float32 Adam moments of a known gradient sequence give it back inside the stated rounding"""
    rng = np.random.default_rng(1)
    for beta1 in (0.9, 0.8):
        w = np.float32(1.0) - np.float32(beta1)
        m = np.zeros((50, 3), np.float32)
        for k in range(1, 5):
            g = rng.normal(size=m.shape).astype(np.float32)
            m_new = (m + (g - m) * w).astype(np.float32)
            got = D.gradient_from_moments(None if k == 1 else m, m_new, beta1)
            assert np.abs(got - g).max() <= D.readout_rounding(None if k == 1 else m, m_new, beta1) + 2 * D.U * np.abs(g - m).max()
            m = m_new
    assert abs(D.readout_rounding(np.ones(3), np.ones(3), 0.9) - 19 * D.U) < 1e-6 * D.U * 19
