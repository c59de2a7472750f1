"""Fit lanes (BF_FIT_LANES, lanes.hip): frame-after-frame fits of one batch run side by side on streams of their own.  For one lane (the
single-stream path), two, three and more lanes than the process has hardware queues (4 on the GPU hosts: lanes then share queues
and run in turn), every streamed frame - read back as the frame before the last or as the last one, in the capture's call order and
in irregular ones, for one frame and for a 32-frame batch - must be the bits of the same frame fitted alone (tests/lanes_child.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _child(tmp_path, n_lanes):
    import conftest
    import lanes_child
    if conftest.FRESH is None:
        pytest.skip("no fork server")
    out = str(tmp_path / "out.npz")
    p = conftest.FRESH.Process(target=lanes_child.lanes, args=(out, n_lanes))
    p.start()
    p.join(600)
    if p.is_alive():
        p.terminate()
        pytest.fail("the child hung")
    err = tmp_path / "out.npz.err"
    assert p.exitcode == 0, "exit code %s\n%s" % (p.exitcode, err.read_text() if err.exists() else "")
    return np.load(out)


@pytest.fixture(scope="module")
def one_lane(tmp_path_factory):
    return _child(tmp_path_factory.mktemp("lanes1"), 1)


@pytest.mark.parametrize("n_lanes", [2, 3, 8])
def test_streamed_frames_under_lanes_are_the_frames_fitted_alone(tmp_path, one_lane, n_lanes):
    got = _child(tmp_path, n_lanes)
    for key in ("streamed_params", "batch32_params"):
        np.testing.assert_array_equal(got[key], one_lane[key], err_msg=key)


def test_one_lane_is_the_single_stream_path(one_lane):
    assert one_lane["streamed_params"].shape[0] == 8 and np.isfinite(one_lane["streamed_params"]).all()
    assert one_lane["batch32_params"].shape[0] == 6 * 32
