"""The device route of neural_renderer.Renderer on the MI355X (bf_nr_render_dev, bf_nr_tape_texture_grad_dev,
bf_nr_tape_vertex_grad_dev; the drop-in on GPU tensors): vertices, textures, cameras and cotangents go into the kernels where they
lie, on torch's current stream, and images and gradients stay there.  Like tests/test_gpu_mask_device_route.py: every test body runs
in a FRESH process that imports torch before the library (tests/nr_route_child.py), one child per test, children one after another;
a child's assertions are the test.

The yardstick of the equality tests is the host route of the same build, which tests/test_gpu_nr.py and tests/test_gpu_nr_vertex.py
hold to the oracles: the device route issues the same kernels and must give the same BITS.  One test is held to the oracles directly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _child(tmp_path, target, *args, name="out"):
    import conftest
    import nr_route_child
    if conftest.FRESH is None:
        pytest.skip("no fork server")
    out = str(tmp_path / f"{name}.npz")
    p = conftest.FRESH.Process(target=getattr(nr_route_child, target), args=(out,) + args)
    p.start()
    p.join(300)
    if p.is_alive():
        p.terminate()
        pytest.fail("the child hung")
    err = tmp_path / f"{name}.npz.err"
    assert p.exitcode == 0, "exit code %s\n%s" % (p.exitcode, err.read_text() if err.exists() else "")
    return out


def test_dev_entries_give_the_host_routes_bits(tmp_path):
    """rgb, depth, alpha, grad_textures, grad_verts, grad_R and grad_t byte for byte: one triangle at 8 without anti-aliasing, also
    partly outside the image; the 33- and 70-face fans at 20; the open shell seen from inside; the big face at output 40 with
    anti-aliasing; the vertex of valence 70; the degenerate face; ts 2, 3 and 4; lit and lightoff; fill_back on and off; each
    cotangent alone and all together; single-output renders; an ndc render without textures; every combination of K, R, t by value
    and by address; 64 guard words behind every output and gradient whole.

    One place has no "host route's bytes" to equal: the texture cube of the big face itself.  Its pixel box is above
    BF_TEX_GATHER_MAX, so bf_nr_backward_large_kernel adds its pixels with float atomics on global memory in no fixed order, on both
    routes.  Measured on the MI355X: with every grad_textures word compared, 56 of the big face case's 6,561 words differed from the
    host route, all of them in that one cube of 81; over this test's three such comparisons (243 words) two calls of the HOST
    route differed from each other in 156 words and the device route from the host route in 170, the worst error 0.005 of the
    bound.  There the device route, the host route and a second call of the host route are
    each held to tests/nr_oracle.py within (n + 3) 2^-23 S - the bound tests/test_gpu_nr.py holds this kernel to - every other cube
    of the case stays byte for byte, and the child reports how many of those words the host route changes against itself"""
    got = np.load(_child(tmp_path, "same_bits"))
    print(f"    the atomic kernel's cubes: {int(got['atomic_words'])} words, host route against itself {int(got['atomic_host_against_itself'])} differ, "
          f"device against host {int(got['atomic_device_against_host'])} differ, worst err / bound {float(got['atomic_worst']):.3f}")
    assert int(got["atomic_words"]) > 0


def test_batches_shared_cameras_and_two_tapes_in_one_graph(tmp_path):
    """the drop-in with geometry_grad on, GPU tensors against CPU tensors: a [1,3,3] camera shared by B = 2 (its gradient the items'
    sum in item order) and a [2,3,3] one; two taped renders of one mesh from two views in one graph, one backward, and a second
    backward that raises"""
    _child(tmp_path, "batches_and_graphs")


def test_the_pointer_view_kernels_alone(tmp_path):
    """the projection and the fold reading the TexView through a pointer, at 1, 255, 256 and 257 vertices, valence 1 and 70, the view
    at a 4-byte-aligned address that is not 16-byte-aligned: their by-value forms' bytes"""
    _child(tmp_path, "view_kernels_alone")


def test_results_sit_in_the_oracles_bounds(tmp_path):
    """independent of the host route: a lit fill-back case and a lightoff front-only one - renders bit-equal to tests/nr_oracle.py,
    the texture VJP within (n + 3) 2^-23 S with exact zeros where the oracle has no term, grad_verts, grad_R, grad_t within
    tests/nr_vertex_oracle.py's (n + 72) 2^-23 S"""
    _child(tmp_path, "oracle_independent")


def test_tile_lists_grow_before_the_fill_pass(tmp_path):
    """the render that overflows its first tile lists: one growth and no repeated render, the host route's bits; a smaller render
    behind it on the same renderer gives a fresh renderer's bits; 4 bytes read back per render and nothing else"""
    got = np.load(_child(tmp_path, "tile_lists"))
    assert int(got["growths"]) == 1


def test_outputs_workspace_and_streams(tmp_path):
    """a second identical call allocates nothing and switches no stream; the same call under torch.cuda.stream(s) gives the same
    bits; host, device and host calls alternate on one renderer, each with its route's usual bits; every new refusal returns
    BF_ERR_INVALID before anything is queued or counted"""
    _child(tmp_path, "outputs_workspace_streams")


def test_the_references_texture_loop_stays_on_the_device(tmp_path):
    """eight iterations of texture_fitting.py:257-276 as written (torch.optim.Adam, K numpy in the constructor, fresh cuda R / t
    each step), everything on cuda:0: from the first render on no host-route call, exactly three *_dev calls per step, no workspace
    allocation and no tile-list growth after step one, no stream switch, 8 bytes read back per step - and the losses and final
    texels of a second child with BF_TORCH_DEVICE_ROUTE=0, byte for byte.  The parent commit has no bf_nr_render_dev: this cannot
    pass there"""
    dev = np.load(_child(tmp_path, "texture_loop", False, name="dev"))
    host = np.load(_child(tmp_path, "texture_loop", True, name="host"))
    for k in ("losses", "texels"):
        assert dev[k].dtype == np.float32 and dev[k].tobytes() == host[k].tobytes(), k


def test_the_vertex_loop_stays_on_the_device(tmp_path):
    """geometry_grad on: five Adam steps of a sphere toward a shifted silhouette with vertices, R and t on the GPU - no host call, no
    set_vertices - end in the bits of the BF_TORCH_DEVICE_ROUTE=0 run"""
    dev = np.load(_child(tmp_path, "vertex_loop", False, name="dev"))
    host = np.load(_child(tmp_path, "vertex_loop", True, name="host"))
    for k in ("losses", "verts"):
        assert dev[k].dtype == np.float32 and dev[k].tobytes() == host[k].tobytes(), k
