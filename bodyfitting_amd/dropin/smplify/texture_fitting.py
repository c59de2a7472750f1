"""`from smplify.texture_fitting import TextureFitting` (apps/rp_fitting.py:11) resolves here."""
from bodyfitting_amd.texture_dropin import (TextureFitting, create_smpld_uv, gen_cam_views, load_obj_uv, render_texture_map,  # noqa: F401
                                            sphere2rot, to8b)
