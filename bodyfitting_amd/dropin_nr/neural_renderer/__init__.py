"""`import neural_renderer as nr` for callers of the reference (smplify/texture_fitting.py:8, utils/renderer.py:4, utils/io_utils.py,
test/correspondence.py): the HIP-backed `Renderer`, `load_obj`, `save_obj` and `__version__` of bodyfitting_amd/neural_renderer.py.
This package lives in a directory of its own, beside `dropin/` and `dropin_smplx/`: put `bodyfitting_amd/dropin_nr` on `sys.path`
only where the real neural_renderer is to be replaced.  The other names of the reference package raise NotImplementedError."""
from bodyfitting_amd import neural_renderer as _impl
from bodyfitting_amd.neural_renderer import Renderer, load_obj, save_obj, __version__, name  # noqa: F401


def __getattr__(attr):
    return _impl.__getattr__(attr)
