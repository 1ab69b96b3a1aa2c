"""Import-path shim: ``sim.render_mesh`` / ``sim.sim_2d`` / ``sim.sim_3d`` of the reference map onto ``dgdm_amd.sim.*`` (``sim_2d`` and
``sim_3d`` make their data with the squeeze simulator of ``dgdm_amd.sim.squeeze`` instead of MuJoCo)."""
import sys as _sys
from dgdm_amd.sim import render_mesh, sim_2d, sim_3d, squeeze  # noqa: F401
for _n in ("render_mesh", "sim_2d", "sim_3d", "squeeze"):
    _sys.modules.setdefault(__name__ + "." + _n, getattr(_sys.modules[__name__], _n))
