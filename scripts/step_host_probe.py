#!/usr/bin/env python3
"""Host time per step at a launch-bound size: 64^3, all solid, Robin, no extras, state resident in HBM.  500 steps, one
synchronise at the end, wall-clock per step; five repeats and their median, for StagedStepper.step and adi_step_hip_coeff.

    python scripts/step_host_probe.py [TREE]      TREE: a checkout to import the package from (default: this one)

Prints one JSON line.  Run one process per measurement and alternate the trees to compare: the medians of one tree differ by
several per cent from process to process (profiles/step_forms_ab.txt)."""
import json
import os
import sys
import time

TREE = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TREE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import adi_thermal_fields_amd.adi3d_hip_coeff as hip  # noqa: E402

assert os.path.abspath(hip.__file__).startswith(TREE), hip.__file__
N, STEPS, REPEATS = 64, 500, 5
grid = hip.Grid3D(N, N, N, 5e-4, np.ones((N, N, N), bool))
mat, prm = hip.Material(7800.0, 490.0, 54.0), hip.Params(0.05, 0.5)
packs = hip.precompute_coeff_packs_unified(grid, mat, robin_h=500.0)
st = hip.StagedStepper(grid, mat, prm, packs, 20.0)
T0 = hip.to_device(np.random.default_rng(1).uniform(20.0, 1000.0, (N, N, N)))


def measure(step):
    T = T0
    for _ in range(100):
        T = step(T)
    torch.cuda.synchronize()
    reps = []
    for _ in range(REPEATS):
        T = T0
        t0 = time.perf_counter()
        for _ in range(STEPS):
            T = step(T)
        torch.cuda.synchronize()
        reps.append((time.perf_counter() - t0) / STEPS * 1e6)
    return dict(median_us=round(float(np.median(reps)), 3), repeats_us=[round(r, 3) for r in reps])


print(json.dumps(dict(stepper_step=measure(lambda T: st.step(T)),
                      adi_step_hip_coeff=measure(lambda T: hip.adi_step_hip_coeff(T, grid, mat, prm, packs, Tinf=20.0)))))
