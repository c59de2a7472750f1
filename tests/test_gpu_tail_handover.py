"""The frame loop's tail hands its results over itself (csrc/api.hip bf_enqueue_tail, csrc/lanes.hip lane_launch, MeshPass::mirror): bf_mesh_kernel and
bf_mesh_multi_kernel store every vertex into the arena's pinned mirror as well, bf_joints_kernel its joints and the arena's params /
terms / state rows; and a drain hands the last slot of a lane's group back to the batch by one kernel on that lane's stream
(bf_lanes_drain).  BF_TAIL_HANDOVER=store has every tail that can do so, =copy keeps the launch or copy command behind the tail, and
unset the library chooses by the tail's size.

Each case runs once per setting in a child of its own (tests/tail_handover_child.py), which holds every call it reads bit for bit
against the call fitted alone, the device arena against the mirror after a sync, a second use of every lane arena with other frames, a
continuing fit behind a drain and the parameters and gradient read after one; here the settings' results are held against each
other.  Shapes: 690 vertices (22 tiles, the last of 18 vertices) in groups of 1, 2, 3, 8, 9 and 16 one-frame calls and five two-frame
calls; the full-size model (216 tiles, the last of 10) in groups of 5, 6 and 7 - six frames are 522,000-odd bytes, just under the
512 KiB at which the hand-over becomes a copy command and the default starts to store, seven are over it - and frame after frame
without lanes; the kid model and a dense-skinning variant in groups of 1 and 9."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ("params", "vertices", "joints", "full_pose", "loss_terms")


def _child(tmp_path, target, *args):
    import conftest
    import tail_handover_child
    if conftest.FRESH is None:
        pytest.skip("no fork server")
    out = str(tmp_path / "out.npz")
    p = conftest.FRESH.Process(target=getattr(tail_handover_child, target), args=(out,) + args)
    p.start()
    p.join(300)
    if p.is_alive():
        p.terminate()
        pytest.fail("the child hung")
    err = tmp_path / "out.npz.err"
    assert p.exitcode == 0, "exit code %s\n%s" % (p.exitcode, err.read_text() if err.exists() else "")
    return np.load(out)


def _both(tmp_path, target, *args):
    got = {}
    for mode in ("store", "copy", "by-size"):
        d = tmp_path / mode
        d.mkdir()
        got[mode] = _child(d, target, mode, *args)
    for n in NAMES:
        assert got["store"][n].size > 0 and np.isfinite(got["store"][n]).all(), n
        assert np.array_equal(got["store"][n], got["copy"][n]), f"{n}: BF_TAIL_HANDOVER=store and =copy give different bits"
        assert np.array_equal(got["by-size"][n], got["copy"][n]), f"{n}: BF_TAIL_HANDOVER unset and =copy give different bits"


CASES = {
    "smpl690": ("smpl690", (16, 9, 8, 3, 2, 1), (5,)),
    "smpl_5_6_7": ("smpl", (5, 6, 7), ()),
    "kid": ("kid", (1, 9), ()),
    "dense_skinning": ("nv690_BD", (1, 9), ()),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_groups_hand_over_the_bits_of_the_call_alone(tmp_path, case):
    _both(tmp_path, "groups", *CASES[case])


def test_tail_aside_without_lanes_hands_over_the_bits_of_the_call_alone(tmp_path):
    _both(tmp_path, "aside", "smpl")
