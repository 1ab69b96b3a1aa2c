#!/usr/bin/env python3
"""`python sim/sim_3d.py MODEL_ROOT GRIPPER_IDX OBJECT_IDX NUM_GRIPPERS NUM_OBJECTS SAVE_DIR NUM_CPUS` as the reference's
sim/run_sim_3d.sh calls it: writes the 3-D dynamics dataset with the sliced squeeze simulator (dgdm_amd/sim/sim_3d.py)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from dgdm_amd.sim.sim_3d import generate, main  # noqa: E402,F401

if __name__ == "__main__":
    main(sys.argv[1:])
