"""The part of the reference's ``sim/`` package that draws: ``render_mesh`` (pictures of grippers, silhouettes of objects) on the
library's own rasteriser (csrc/render.hip).  Running MuJoCo stays with the user's simulator setup."""
from . import render_mesh  # noqa: F401
