"""`utils.io_utils` of the reference, as far as a user's own SMPL+D loop needs it (smplify/smplify.py:14): `compute_normal_torch`
on the HIP path and `load_obj_mesh`.  Every other name (`load_openpose`, `image_cropping`, `save_obj_mesh`, ... -
apps/genebody_fitting.py:14, smplify/body_fitting.py:15) is looked up, on first use, in the `io_utils.py` of a `utils` package
further down sys.path - the caller's own - so that importing this module pulls in none of that file's dependencies."""
import importlib.util
import os
import sys

from bodyfitting_amd.io import load_obj_mesh  # noqa: F401
from bodyfitting_amd.normals import compute_normal_torch  # noqa: F401

_here = os.path.abspath(os.path.dirname(__file__))
_NEXT = []


def _callers_module():
    if _NEXT:
        return _NEXT[0]
    found = None
    for d in sys.modules[__package__].__path__:
        path = os.path.join(os.path.abspath(d), "io_utils.py")
        if os.path.abspath(d) != _here and os.path.isfile(path):
            spec = importlib.util.spec_from_file_location(__package__ + "._callers_io_utils", path)
            found = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(found)
            break
    _NEXT.append(found)
    return found


def __getattr__(name):
    if name.startswith("__"):
        raise AttributeError(name)
    mod = _callers_module()
    if mod is None or not hasattr(mod, name):
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    return getattr(mod, name)
