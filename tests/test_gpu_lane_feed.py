"""Host-fed lane groups (lanes.hip): with W > 1 a staging packs the call's inputs into a pinned slot and issues no GPU work, a group's
launch carries one input transfer for all its slots, a re-fit copies its inputs on the host, and a group is fed from the host or on the
device, never both.  For forced groups of 3 (BF_FIT_LANE_FILL=1), the adaptive default and a launch per call (W = 1, the call sequence
before groups), every result - seven streamed frames, re-fits, a switch of kind, a slot staged past its group, a double staging, a
destroy with a group held, every pinned arena re-used, 50 views, a 4-frame batch - must be the bits of the same frame fitted alone, the
counts of bf_batch_lane_feed_stats must be the ones the forced shape fixes (tests/lane_feed_child.py), and the streamed parameters
must not depend on the setting."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SETTINGS = [(3, 1), (8, 0), (1, 0)]          # (BF_FIT_LANE_WIDTH, BF_FIT_LANE_FILL)


def _child(tmp_path, width, fill):
    import conftest
    import lane_feed_child
    if conftest.FRESH is None:
        pytest.skip("no fork server")
    out = str(tmp_path / "out.npz")
    p = conftest.FRESH.Process(target=lane_feed_child.feed, args=(out, width, fill))
    p.start()
    p.join(600)
    if p.is_alive():
        p.terminate()
        pytest.fail("the child hung")
    err = tmp_path / "out.npz.err"
    assert p.exitcode == 0, "exit code %s\n%s" % (p.exitcode, err.read_text() if err.exists() else "")
    return np.load(out)


@pytest.fixture(scope="module")
def forced_three(tmp_path_factory):
    return _child(tmp_path_factory.mktemp("feed_3_1"), 3, 1)


def test_forced_groups_of_three_are_fed_by_one_transfer_each(forced_three):
    assert forced_three["streamed_params"].shape[0] == 8 and np.isfinite(forced_three["streamed_params"]).all()
    assert forced_three["batch4_params"].shape[0] == 10 * 4


@pytest.mark.parametrize("width,fill", SETTINGS[1:])
def test_the_feed_does_not_change_the_fits(tmp_path, forced_three, width, fill):
    got = _child(tmp_path, width, fill)
    for key in ("streamed_params", "batch4_params"):
        np.testing.assert_array_equal(got[key], forced_three[key], err_msg=key)
