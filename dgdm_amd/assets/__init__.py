"""The part of the reference's ``assets/`` package that sits behind the sampler, on the device: finger-geometry decode (SURVEY.md §8(f)
rank 3), the contour extraction of the 2-D test objects (icon_process), and the export of designed fingers as watertight meshes, convex
collision pieces and MuJoCo gripper files (finger_mesh, gripper_xml), and of the icon objects as meshes, convex pieces and MuJoCo object
files (icon_process, object_sampler, scan_object_process).  Running MuJoCo stays with the user's simulator setup."""
from .finger_mesh import FingerMesh, save_grippers  # noqa: F401
from .icon_process import generate_icon_mesh, save_icon_mesh, save_icon_objects  # noqa: F401
from .object_sampler import generate_object_xml  # noqa: F401
from .scan_object_process import generate_object_3d_xml, read_object_names  # noqa: F401
