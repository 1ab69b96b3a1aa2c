"""Import-path shim: ``assets.finger_sampler`` / ``assets.finger_3d`` / ``assets.icon_process`` / ``assets.object_sampler`` /
``assets.scan_object_process`` of the reference map onto ``dgdm_amd.assets.*`` (the sampler-adjacent decode, the mesh / XML export,
the contour extraction and the icon objects, see dgdm_amd/assets/__init__.py)."""
import sys as _sys
from dgdm_amd.assets import (FingerMesh, finger_3d, finger_sampler, generate_icon_mesh, generate_object_3d_xml,  # noqa: F401
                             generate_object_xml, icon_process, object_sampler, read_object_names, save_grippers, save_icon_mesh,
                             save_icon_objects, scan_object_process)
for _n in ("finger_3d", "finger_sampler", "icon_process", "object_sampler", "scan_object_process"):
    _sys.modules[__name__ + "." + _n] = getattr(_sys.modules[__name__], _n)
