"""Import-path shim: ``assets.finger_sampler`` / ``assets.finger_3d`` / ``assets.icon_process`` of the reference map onto
``dgdm_amd.assets.*`` (the sampler-adjacent decode, the mesh / XML export and the contour extraction, see dgdm_amd/assets/__init__.py)."""
import sys as _sys
from dgdm_amd.assets import FingerMesh, finger_3d, finger_sampler, icon_process, save_grippers  # noqa: F401
for _n in ("finger_3d", "finger_sampler", "icon_process"):
    _sys.modules[__name__ + "." + _n] = getattr(_sys.modules[__name__], _n)
