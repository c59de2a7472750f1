"""The device route of the silhouette term on the MI355X (bf_silhouette_create_dev, bf_silhouette_contours_dev,
bf_silhouette_rows_dev, bf_silhouette_loss_dev; extract_countours and multview_mask_loss on GPU tensors): masks, vertices and cameras
go into the kernels where they lie, on torch's current stream, and contours and loss stay there.  Like
tests/test_gpu_scan_device_route.py: every test body runs in a FRESH process that imports torch before the library
(tests/mask_route_child.py), one child per test, children one after another; a child's assertions are the test.

The yardstick of the equality tests is the host route of the same build, which tests/test_gpu_mask_loss.py holds to the float64
oracle: the device route issues the same launches and must give the same BITS.  One test is held to the oracle directly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _child(tmp_path, target, *args, name="out"):
    import conftest
    import mask_route_child
    if conftest.FRESH is None:
        pytest.skip("no fork server")
    out = str(tmp_path / f"{name}.npz")
    p = conftest.FRESH.Process(target=getattr(mask_route_child, target), args=(out,) + args)
    p.start()
    p.join(300)
    if p.is_alive():
        p.terminate()
        pytest.fail("the child hung")
    err = tmp_path / f"{name}.npz.err"
    assert p.exitcode == 0, "exit code %s\n%s" % (p.exitcode, err.read_text() if err.exists() else "")
    return out


def test_dev_entries_give_the_host_routes_bits(tmp_path):
    """every case of mask_loss_cases.CASE_NAMES in both distance forms: terms[1 + 2M] and dverts of bf_silhouette_loss_dev are
    bf_silhouette_loss's bytes - 1 to 690 sampled vertices across the 255 / 256 / 257 block edges, contours of 1, 15 / 16 / 17 and
    about 1,050 points, 1 to 8 views, a view with no inside vertex, 48 x 80, epsilon 1, 10 and 37.5 - and so is
    multview_mask_loss(...).backward() on GPU tensors for cotangents 1, -2.5 and 0, with +0 at unsampled vertices"""
    _child(tmp_path, "same_bits")


def test_results_sit_in_the_oracles_band(tmp_path):
    """independent of the host route: one case per distance form, and eps1 and ns32 in both, against float64 autograd of
    oracle.smplify_oracle.multview_mask_loss inside scan_loss_cases.Band"""
    _child(tmp_path, "oracle_band")


def test_the_rows_kernel_alone(tmp_path):
    """bf_sil_rows_kernel against the numpy float64 expression, byte for byte: M = 1, 3 and 65, entries from 1e-3 to 1e4"""
    _child(tmp_path, "rows_alone")


def test_the_ingest_kernel_alone(tmp_path):
    """bf_sil_ingest_kernel on float32, uint8 and bool masks of 1, 255 (W = 17), 256, 257 and 3 x 48 x 80 pixels and on a slice at
    an odd address: bf_silhouette_create's contours and loss bits, the contour oracle's points; a 0.5, a 2 and a NaN give the
    "0 / 1 only" ValueError, an all-zero view the "no foreground" one that names it"""
    _child(tmp_path, "ingest_alone")


def test_optional_outputs_and_the_workspace(tmp_path):
    """the three choices of terms and dverts that write give the all-outputs bits with 64 guard words behind every output whole, and
    both NULL launches nothing; a
    small case behind a large one on one workspace gives a fresh workspace's bits; a second identical call allocates nothing and
    switches no stream; the same call under torch.cuda.stream(s) gives the same bits"""
    _child(tmp_path, "optional_outputs")


def test_a_mask_loop_stays_on_the_device(tmp_path):
    """ten Adam steps of smplify.py:177-213 with use_mask=True, everything on cuda:0: from extract_countours on no host call
    (bf_silhouette_loss counts as one), six *_dev calls per step, no workspace allocation after the first step, no stream switch,
    the cameras stacked once.  The parent commit has no device route for the silhouette term: this cannot pass there"""
    _child(tmp_path, "mask_loop")


def test_step_one_of_the_loop_sits_in_the_oracles_band(tmp_path):
    """step one of that loop: the total and the gradient of every block of LOOP_BLOCKS inside scan_loss_cases.Band around float64
    autograd of the oracle's same expression (mask_loss_cases.loop_evaluate).

    The cameras come from torch.inverse, as in smplify.py:131-135: column-major tensors.  This step is what found that
    multiview_keypoint_loss's device route handed such cameras to its kernel transposed (loss.py: _views_on, fixed with this route;
    tests/test_mask_device_route.py pins it without a GPU): the total was 299734.2 against the oracle's 142323.87 then."""
    import mask_loss_cases as MC
    import torch
    got = np.load(_child(tmp_path, "mask_loop"))
    _, params, _ = MC.loop_case()
    t64, g64, _ = MC.loop_evaluate(params, torch.float64)
    t32, g32, _ = MC.loop_evaluate(params, torch.float32)
    print(f"    step one: total {float(got['first_total']):.4f} (body {float(got['first_body']):.4f}, mask {float(got['first_mask']):.4f}), "
          f"oracle float64 {t64:.4f}, float32 {t32:.4f}")
    band = MC.Band()
    band.value("step one: total", float(got["first_total"]), t64, t32)
    for k in MC.LOOP_BLOCKS:
        band.block(f"step one: d{k}", got["first_" + k], g64[k], g32[k])
    worst = band.worst()
    print(f"    worst position inside the band: {worst[0]} at {worst[3]:.3f}")
    assert worst[3] <= 1.0


@pytest.mark.parametrize("switched_off", [True, False])
def test_fallbacks_and_refusals(tmp_path, switched_off):
    """BF_TORCH_DEVICE_ROUTE=0: GPU tensors give the same bits through the host entry points alone.  Else: CPU tensors, numpy and
    float64 do what they did, contours of another identity are served by the object of equal ones, and the *_dev entries make
    their host twins' refusals - and refuse a NULL workspace - before anything is queued or counted, leaving no HIP error behind"""
    _child(tmp_path, "fallbacks", switched_off)
