"""Finger-geometry decode on the device: the part of the reference's ``assets/`` package that sits directly behind the sampler
(SURVEY.md §8(f) rank 3), and the contour extraction of the 2-D test objects (icon_process).  Mesh extrusion, convex decomposition and
MuJoCo XML generation stay with the user's simulator setup."""
