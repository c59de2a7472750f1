from .smpl import SMPL  # noqa: F401
from .inpaint import Inpainter  # noqa: F401
