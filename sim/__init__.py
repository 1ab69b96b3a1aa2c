"""Import-path shim: ``sim.render_mesh`` of the reference maps onto ``dgdm_amd.sim.render_mesh`` (gripper pictures and object
silhouettes on the library's rasteriser, see dgdm_amd/sim/__init__.py)."""
import sys as _sys
from dgdm_amd.sim import render_mesh  # noqa: F401
_sys.modules[__name__ + ".render_mesh"] = render_mesh
