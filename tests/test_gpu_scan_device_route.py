"""The device route of the SMPL+D loop's functions on the MI355X (bf_vertex_normals_dev, bf_vertex_normals_vjp_dev,
bf_normal_laplacian_dev, bf_scan_point_loss_dev, bf_scan_nearest_dev, bf_normal_loss_dev, bf_scale_gradient_dev): float32 tensors on
the topology's / the scan's GPU go into the kernels where they lie, on torch's current stream, and the losses stay there.  Like
tests/test_gpu_device_route.py: every test body runs in a FRESH process that imports torch before the library
(tests/scan_route_child.py), one child per test, children one after another; a child's assertions are the test.

The yardstick is the host route of the same build, which tests/test_gpu_scan_losses.py holds to the float64 oracle: the device route
issues the same launches and must give the same BITS."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _child(tmp_path, target, *args, name="out"):
    import conftest
    import scan_route_child
    if conftest.FRESH is None:
        pytest.skip("no fork server")
    out = str(tmp_path / f"{name}.npz")
    p = conftest.FRESH.Process(target=getattr(scan_route_child, target), args=(out,) + args)
    p.start()
    p.join(300)
    if p.is_alive():
        p.terminate()
        pytest.fail("the child hung")
    err = tmp_path / f"{name}.npz.err"
    assert p.exitcode == 0, "exit code %s\n%s" % (p.exitcode, err.read_text() if err.exists() else "")
    return out


@pytest.mark.parametrize("which", ["normals", "laplacian", "point", "point_large", "normal"])
def test_gpu_tensors_give_the_host_routes_bits(tmp_path, which):
    """value and every gradient, for cotangents 1, 2.5 and -1.5.  normals / laplacian: the 690-vertex body, fans of 255, 256 and 257
    vertices around one hub with a vertex in no face, strips of 255, 256 and 257 faces.  point: 1, 3, 4, 5, 255, 256 and 257 points,
    and points on the scan (loss 0, gradient exactly 0).  point_large: 65,537 points, more than 256 block sums.  normal: an
    un-normalised face_norm_mesh at 1, 256 and 257 points"""
    _child(tmp_path, "same_bits", which)


def test_results_sit_in_the_oracles_band(tmp_path):
    """independent of the host route: one case per function against float64 autograd of the oracle, in tests/scan_loss_cases.py's band"""
    _child(tmp_path, "oracle_band")


def test_the_gather_kernel_and_the_scaling_kernel_alone(tmp_path):
    """bf_normal_loss_dev against table[ids] in numpy followed by the host bf_normal_loss (face 0, face NF - 1, repeated ids, n no
    multiple of 256, an id outside the table); bf_scale_gradient_dev against numpy's float32 g * c and g * c + 0.0"""
    _child(tmp_path, "gather_alone")


def test_optional_outputs_of_the_dev_entries(tmp_path):
    """bf_scan_point_loss_dev at 1, 5 and 257 points with all 16 NULL / non-NULL choices of its outputs, bf_normal_laplacian_dev on
    the 257-vertex fan and bf_normal_loss_dev at 257 points with loss only, gradient only, both and neither: the host route's
    all-outputs bits, 64 floats behind every output untouched, no allocation on a second identical call, no stream switch"""
    _child(tmp_path, "optional_outputs")


def test_nearest_points_on_gpu_tensors(tmp_path):
    """points, ids (int32) and coefficients: the numpy call's bits, on the tensors' device"""
    _child(tmp_path, "nearest_tensors")


def test_an_smpl_d_loop_stays_on_the_device(tmp_path):
    """ten iterations of smplify.py:236-245 as written with everything on cuda:0: only *_dev calls, eight per step (one search: the
    memo's hit), no workspace allocation after the first step, no stream switch; the displacement is bit-equal to the same loop with
    BF_TORCH_DEVICE_ROUTE=0 in another child"""
    dev = np.load(_child(tmp_path, "smpld_loop", False, name="device"))["disp"]
    host = np.load(_child(tmp_path, "smpld_loop", True, name="host"))["disp"]
    assert dev.shape == host.shape == (1, 690, 3)
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32)), \
        f"{int((dev.view(np.uint32) != host.view(np.uint32)).sum())} words differ (max |diff| {np.abs(dev - host).max():.3g})"


def test_the_query_memo_is_sound(tmp_path):
    """an in-place edit, a fresh tensor with equal contents, a new tensor after the old one was deleted, set_mesh with another scan:
    a second search and the right answer each time"""
    _child(tmp_path, "memo")


def test_work_is_ordered_on_torchs_current_stream(tmp_path):
    """vertices produced on a side stream behind a long chain, the four functions and their backward queued with no synchronisation:
    the same bits; two streams alternating on one searcher and one topology: waits inserted, the same bits"""
    _child(tmp_path, "stream_order")


@pytest.mark.parametrize("switched_off", [True, False])
def test_fallbacks_and_refusals(tmp_path, switched_off):
    """BF_TORCH_DEVICE_ROUTE=0: GPU tensors give the same bits through the host entry points alone.  Else: CPU tensors and float64
    take the host route, and the *_dev entries refuse a NULL workspace, n = 0 and n beyond the limit before anything is queued and
    leave no HIP error behind"""
    _child(tmp_path, "fallbacks", switched_off)


def test_nearest_optional_outputs_on_both_routes(tmp_path):
    """bf_scan_nearest / bf_scan_nearest_dev at 1, 3, 4, 5 and 257 points with each non-empty subset of (face_ids, nearest, bary): the
    all-outputs call's words, host and device route agreeing word for word, the guard behind each device output whole; the host
    entry counts one host call; both entries refuse NULL arguments, n = 0, n beyond the limit and a NULL workspace with their own
    messages and count nothing"""
    _child(tmp_path, "nearest_outputs")
