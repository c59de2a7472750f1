"""The device route of the torch drop-ins on the MI355X (bf_*_dev, bodyfitting_amd/_autograd.py): float32 tensors on the model's GPU
go into the kernels where they lie, on torch's current stream.  Every test body runs in a FRESH process that imports torch before the
library (tests/device_route_child.py), one child per test, children one after another; a child's assertions are the test.

The yardstick is the host route on the same build - the numpy paths and DeviceModel.vjp / vjp_smplx, held to the float64 oracle by
the existing suites: the device route issues the same launches and must give the same BITS, for every output and every gradient
block, at 1, 2, 9, 17 and 65 frames (the plain kernel, the multi-frame kernel with a tail, the 32-frame matrix-core kernel, and the
GEMM path the forward takes above 64 frames and the reverse's forward from 16 on)."""
import pytest

pytestmark = pytest.mark.gpu


def _child(tmp_path, target, *args):
    import conftest
    import device_route_child
    if conftest.FRESH is None:
        pytest.skip("no fork server")
    out = str(tmp_path / "out.npz")
    p = conftest.FRESH.Process(target=getattr(device_route_child, target), args=(out,) + args)
    p.start()
    p.join(300)
    if p.is_alive():
        p.terminate()
        pytest.fail("the child hung")
    err = tmp_path / "out.npz.err"
    assert p.exitcode == 0, "exit code %s\n%s" % (p.exitcode, err.read_text() if err.exists() else "")


@pytest.mark.parametrize("which", ["smpl", "smplx", "smplx_expr", "smpl_full"])
def test_gpu_tensors_give_the_host_routes_bits(tmp_path, which):
    """SMPL.forward / SMPLX.forward (without and with expression) on GPU tensors against the numpy path, .backward() of a seeded
    cotangent sum against DeviceModel.vjp / vjp_smplx, for every single-output case and all outputs together; smpl_full: the
    6890-vertex model at 1 and 17 frames"""
    _child(tmp_path, "same_bits", which)


def test_gradients_sit_in_the_oracles_band(tmp_path):
    """independent of the host route: n = 9 on the small SMPL against float64 autograd of the oracle, in the band of
    tests/test_gpu_smpl_autograd.py (4 x torch float32's own error + 1e-6 of the largest value)"""
    _child(tmp_path, "oracle_band")


def test_keypoint_loss_and_prior_give_the_cpu_tensor_calls_bits(tmp_path):
    """multiview_keypoint_loss (1 and 3 views, a view without keypoints, without and with hands and face) and MaxMixturePrior: total,
    the four terms and the three gradients; the same cameras again are neither packed nor sent again"""
    _child(tmp_path, "keypoint_loss")


def test_optional_outputs_of_the_dev_entries(tmp_path):
    """bf_keypoint_loss_dev with the 16 subsets of its outputs (n = 1, two views, one row), bf_smpl_vjp_dev and bf_smplx_vjp_dev with
    expression at n = 1 and 3 with one gradient asked for (dbetas, dglobal_orient, one hand, dexpression): the host route's
    all-outputs bits, 64 floats behind every output untouched, no allocation on a second identical call, no stream switch"""
    _child(tmp_path, "optional_outputs")


def test_a_keypoint_stage_loop_stays_on_the_device(tmp_path):
    """ten Adam steps with everything on cuda:0: only *_dev calls (four per step: the loss is entered for its terms and again for
    its gradient), no allocation after the first step, no stream switch"""
    _child(tmp_path, "stays_on_the_device")


def test_work_is_ordered_on_torchs_current_stream(tmp_path):
    """inputs produced on a side stream behind a long chain, model and backward queued with no synchronisation: the same bits; two
    streams alternating on one model: waits inserted, the same bits"""
    _child(tmp_path, "stream_order")


@pytest.mark.parametrize("switched_off", [True, False])
def test_fallbacks_and_refusals(tmp_path, switched_off):
    """BF_TORCH_DEVICE_ROUTE=0: GPU tensors give the same bits through the host entry points alone.  Else: CPU tensors take the host
    route, the pointer check refuses NULL and host memory without leaving an error, and the *_dev calls refuse an SMPL-X model in
    bf_smpl_forward_dev, coefficients without directions, a NULL workspace and n = 0 before anything is queued"""
    _child(tmp_path, "fallbacks", switched_off)


def test_smpl_forward_optional_outputs_on_both_routes(tmp_path):
    """bf_smpl_forward / bf_smpl_forward_dev on the 690-vertex model at n = 1, 3, 15, 16 with each non-empty subset of (vertices,
    joints, joints_ori): the bits of the host all-outputs call on both routes, the guard behind each device output whole, no
    allocation on a second identical call; the host entry counts one host call, runs with all three outputs NULL and does not look
    at the model's kind; both entries refuse NULL arguments, n = 0, a NULL workspace and (the device entry) an SMPL-X model with
    their own messages and count nothing"""
    _child(tmp_path, "smpl_forward_outputs")
