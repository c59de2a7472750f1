"""The frame loop's idle rule with a hold (BF_FIT_LANE_HOLD_US, csrc/lanes.hip bf_lanes_fit, csrc/lane_policy.h) and the one-launch mesh tail of a lane group
(bf_launch_mesh, csrc/mesh_choice.h).  Each setting runs in a child of its own (tests/lane_hold_child.py), which holds every
streamed frame bit for bit against the frame fitted alone.

Hold: on a fast feed (eight stage + fit pairs back to back, H = 1 s, W = 8) the first call goes out alone and seven are held until
the sync - 2 launches, largest group 7; a feeder that sleeps 5 ms between pairs at H = 2 ms gets a launch per call; H = 0 and W = 1
give the same bits, W = 1 a launch per call at any H.
Tail: with W = 16 and forced shapes a full group of one-frame calls (two 8-frame blocks), a group of nine (a one-frame last block)
and five two-frame calls (call boundaries off the blocks) give every call the bits of the call fitted alone - also on the
dense-skinning and kid models."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _child(tmp_path, target, *args):
    import conftest
    import lane_hold_child
    if conftest.FRESH is None:
        pytest.skip("no fork server")
    out = str(tmp_path / "out.npz")
    p = conftest.FRESH.Process(target=getattr(lane_hold_child, target), args=(out,) + args)
    p.start()
    p.join(600)
    if p.is_alive():
        p.terminate()
        pytest.fail("the child hung")
    err = tmp_path / "out.npz.err"
    assert p.exitcode == 0, "exit code %s\n%s" % (p.exitcode, err.read_text() if err.exists() else "")
    return np.load(out)


@pytest.fixture(scope="module")
def hold_off(tmp_path_factory):
    """H = 0 at W = 8: the idle rule alone"""
    return _child(tmp_path_factory.mktemp("hold_0"), "hold", 8, 0, "off")


def test_hold_off_gives_the_frames_fitted_alone(hold_off):
    assert hold_off["burst_params"].shape[0] == 8 and hold_off["slow_params"].shape[0] == 6
    assert np.isfinite(hold_off["burst_params"]).all()


def test_fast_feed_holds_seven_behind_the_first_call(tmp_path, hold_off):
    got = _child(tmp_path, "hold", 8, 1000000, "fast")
    np.testing.assert_array_equal(got["burst_params"], hold_off["burst_params"])


def test_slow_feeder_gets_a_launch_per_call(tmp_path, hold_off):
    got = _child(tmp_path, "hold", 8, 2000, "slow")
    np.testing.assert_array_equal(got["slow_params"], hold_off["slow_params"])


def test_width_one_is_a_launch_per_call_at_any_hold(tmp_path, hold_off):
    got = _child(tmp_path, "hold", 1, 1000000, "off")
    np.testing.assert_array_equal(got["burst_params"], hold_off["burst_params"])
    np.testing.assert_array_equal(got["slow_params"], hold_off["slow_params"])


@pytest.mark.parametrize("name", ["smpl", "smpl_4+1", "kid"])
def test_group_tail_gives_every_call_the_bits_of_the_call_alone(tmp_path, name):
    got = _child(tmp_path, "tail", name)
    assert got["params_1"].shape[0] == 16 and np.isfinite(got["params_1"]).all()
    if name == "smpl":
        assert got["params_2"].shape[0] == 5 * 2
