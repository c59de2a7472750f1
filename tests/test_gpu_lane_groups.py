"""Fit-lane groups (BF_FIT_LANE_WIDTH, lanes.hip): a lane launch carries up to W consecutive frame-after-frame calls.  For a launch per
call (W = 1), forced groups of 3 and of 8 (BF_FIT_LANE_FILL=1) and the adaptive default, every streamed frame - in every slot of a full
group, of a partial one and of the group after it, read back as the frame before the last or as the last one, in the capture's call
order and in irregular ones, for one frame and for a 32-frame batch - must be the bits of the same frame fitted alone, the forced
shapes must be the ones lane_stats reports (tests/lane_groups_child.py), and the streamed parameters must not depend on the setting."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SETTINGS = [(1, 0), (3, 1), (8, 1), (8, 0)]          # (BF_FIT_LANE_WIDTH, BF_FIT_LANE_FILL)


def _child(tmp_path, width, fill):
    import conftest
    import lane_groups_child
    if conftest.FRESH is None:
        pytest.skip("no fork server")
    out = str(tmp_path / "out.npz")
    p = conftest.FRESH.Process(target=lane_groups_child.groups, args=(out, width, fill))
    p.start()
    p.join(600)
    if p.is_alive():
        p.terminate()
        pytest.fail("the child hung")
    err = tmp_path / "out.npz.err"
    assert p.exitcode == 0, "exit code %s\n%s" % (p.exitcode, err.read_text() if err.exists() else "")
    return np.load(out)


@pytest.fixture(scope="module")
def width_one(tmp_path_factory):
    return _child(tmp_path_factory.mktemp("groups_1_0"), 1, 0)


def test_a_launch_per_call_gives_the_frames_fitted_alone(width_one):
    assert width_one["streamed_params"].shape[0] == 8 and np.isfinite(width_one["streamed_params"]).all()
    assert width_one["batch32_params"].shape[0] == 6 * 32
    assert width_one["batch4_params"].shape[0] == 10 * 4


@pytest.mark.parametrize("width,fill", SETTINGS[1:])
def test_grouped_frames_are_the_frames_fitted_alone(tmp_path, width_one, width, fill):
    got = _child(tmp_path, width, fill)
    for key in ("streamed_params", "batch32_params", "batch4_params"):
        np.testing.assert_array_equal(got[key], width_one[key], err_msg=key)
