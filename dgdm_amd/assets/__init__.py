"""The part of the reference's ``assets/`` package that sits behind the sampler, on the device: finger-geometry decode (SURVEY.md §8(f)
rank 3), the contour extraction of the 2-D test objects (icon_process), and the export of designed fingers as watertight meshes, convex
collision pieces and MuJoCo gripper files (finger_mesh, gripper_xml).  Running MuJoCo stays with the user's simulator setup."""
from .finger_mesh import FingerMesh, save_grippers  # noqa: F401
