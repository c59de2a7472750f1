"""`utils.mesh_grid_searcher` and `utils.io_utils` of the reference resolve here (smplify/smplify.py:14-15); every other `utils.*`
module still resolves to a `utils` package further down sys.path - the reference's own - and so does every name of `utils.io_utils`
but `compute_normal_torch` and `load_obj_mesh` (apps/genebody_fitting.py:14; io_utils.py here hands them on)."""
import os
import sys

_here = os.path.abspath(os.path.dirname(__file__))
for _d in list(sys.path):
    _p = os.path.abspath(os.path.join(_d or ".", "utils"))
    if _p != _here and _p not in __path__ and os.path.isfile(os.path.join(_p, "__init__.py")):
        __path__.append(_p)
