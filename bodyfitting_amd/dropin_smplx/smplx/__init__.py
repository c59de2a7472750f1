"""`import smplx` for callers of the reference (smplify/smplify.py:7,80; models/smpl.py:2-6): the HIP-backed `create`, `SMPLX`
and `SMPL`.  This package lives in a directory of its own, beside `dropin/`: put `bodyfitting_amd/dropin_smplx` on `sys.path`
only where the real smplx is to be replaced."""
from bodyfitting_amd.smplx import create, SMPLX  # noqa: F401
from bodyfitting_amd.smpl import SMPL, ModelOutput  # noqa: F401
from . import lbs  # noqa: F401
