"""The part of the reference's ``sim/`` package that draws: ``render_mesh`` (pictures of grippers, silhouettes of objects) on the
library's own rasteriser (csrc/render.hip), and a model-free stand-in for the part that simulates: ``squeeze`` (a
frictionless, quasi-static parallel-jaw squeeze, csrc/squeeze.hip; for 3-D fingers a sliced one) and ``sim_2d`` /
``sim_3d``, which write the dynamics datasets with it.  Running MuJoCo stays with the user's simulator setup."""
from . import render_mesh, sim_2d, sim_3d, squeeze  # noqa: F401
