"""`from utils.renderer import render_texture_mesh, gen_cam_views` (apps/rp_fitting.py:17, smplify/texture_fitting.py:12) resolves here."""
from bodyfitting_amd.texture_dropin import gen_cam_views, render_texture_mesh  # noqa: F401
