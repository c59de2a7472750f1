"""`from smplx.lbs import vertices2joints` (models/smpl.py:6)"""
from bodyfitting_amd.smplx import vertices2joints  # noqa: F401
