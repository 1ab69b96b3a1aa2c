"""Writes tests/golden/g16_grad_shapes.npz: the float64 side of the 3-D cases of tests/test_gpu_grad_shapes.py, from the oracle alone
(oracle/dgdm_oracle.py on the synthetic inputs of tests/grad_shapes_cases.py; PointNet++ in float64 costs about 40 ms per row on a CPU,
too much for a GPU test).

    python -m tests.golden.make_golden_grad_shapes            # the fixture (about a minute)
    python -m tests.golden.make_golden_grad_shapes --search   # prints the x seeds the cases hard-code, 2-D and 3-D (minutes)

Per case <name>/: x (distinct, B, L, 1) float32 and starts (distinct, 2 R) int64, the inputs; g64, g32 (distinct, B, L) and l64, l32
(distinct, R, 3), the oracle's gradients and logits in float64 and float32 (the float32 run is the tolerance's yardstick); g16 for the cases
that also run in bf16 (the oracle under contraction('bf16')); margin (distinct,), the float64 run's smallest relative ReLU margin; and the
yardsticks as plain numbers: e32 / e16 (distinct,) = rel_l2(g32 | g16, g64 | g32), d32 (distinct,) = max |l32 - l64|."""
import os
import sys

import numpy as np
import torch

from tests import grad_shapes_cases as gc
from tests import util


def case_arrays(case):
    ref = gc.reference(case)
    out = {k: v.numpy() for k, v in ref.items()}
    out["x"] = gc.x_all(case).numpy()
    D = case["distinct"]
    out["e32"] = np.array([util.rel_l2(ref["g32"][c], ref["g64"][c]) for c in range(D)])
    out["d32"] = np.array([float((ref["l32"][c] - ref["l64"][c]).abs().max()) for c in range(D)])
    if "g16" in ref:
        out["e16"] = np.array([util.rel_l2(ref["g16"][c], ref["g32"][c]) for c in range(D)])
    return out


def main():
    if "--search" in sys.argv:
        for case in gc.CASES_2D + gc.CASES_3D:
            print(case["dim"], case["name"], gc.search_xseeds(case), flush=True)
        return
    out = {}
    for case in gc.CASES_3D:
        a = case_arrays(case)
        assert float(a["margin"].min()) >= gc.MARGIN, (case["name"], a["margin"])
        print(f"{case['name']:12s} margin {a['margin'].min():.2e} | oracle32 vs f64: gradient {a['e32'].max():.2e}, logits {a['d32'].max():.2e}"
              + (f" | oracle bf16 vs oracle32 {a['e16'].max():.2e}" if "e16" in a else ""), flush=True)
        out.update({f"{case['name']}/{k}": v for k, v in a.items()})
    path = os.path.join(util.GOLDEN, gc.GOLDEN_3D)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    torch.manual_seed(0)
    main()
