"""Cost of the moving heat source at 512^3 (DESIGN.md section "Heat source"), alternated in one process with device events.

    python scripts/source_probe.py [--n 512] [--rounds 6] [--steps 20] [--out profiles/source_probe.json]

All-solid box, steel, Robin h = 500 on all faces, dx = 0.2 mm, dt = dx^2 / (2 kappa); Goldak source a = b = c_f = 2 mm, c_r = 4 mm
travelling along axis 1 (depth axis 2, centre on the top surface).  Timed, round-robin so that drift hits every form alike:
  plain      StagedStepper.run, no source (the headline step, fused)
  moving     the same stepper with source= (fused step + adi_source_lines0 + tick per step)
  unfused    StagedStepper(fused=False).run, no source
  field      adi_step_numba_coeff(S=<DeviceField>): adi_explicit_rhs_src + the three unfused sweeps, per call
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (--rounds 1)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import adi_thermal_fields_amd.adi3d_hip_coeff as hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n, dx = a.n, 2e-4
    rho, cp, k = 7800.0, 500.0, 30.0
    dt = 0.5 * dx * dx / (k / (rho * cp))
    g = hip.Grid3D(n, n, n, dx, np.ones((n, n, n), dtype=bool))
    mat, prm = hip.Material(rho, cp, k), hip.Params(dt, 0.5)
    packs = hip.precompute_coeff_packs_unified(g, mat, robin_h=500.0)
    src = hip.GoldakSource(2000.0, 0.8, 2e-3, 2e-3, 2e-3, 4e-3, origin=(0.5 * n * dx, 0.3 * n * dx, n * dx),
                           velocity=0.01)
    T = hip.to_device(np.full((n, n, n), 300.0))
    st_plain = hip.StagedStepper(g, mat, prm, packs, 300.0)
    st_src = hip.StagedStepper(g, mat, prm, packs, 300.0, source=src)
    st_unf = hip.StagedStepper(g, mat, prm, packs, 300.0, fused=False)
    S = src.sample_device(g, 0.0)

    def field():
        X = T
        for i in range(a.steps):
            X = hip.adi_step_numba_coeff(X, g, mat, prm, packs, 300.0, S=S)
        return X
    forms = dict(plain=lambda: st_plain.run(T, a.steps), moving=lambda: st_src.run(T, a.steps, t0=0.0),
                 unfused=lambda: st_unf.run(T, a.steps), field=field)
    for f in forms.values():                         # warm-up: graphs captured, modules loaded
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(a.rounds):
        for name, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.steps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = dict(n=n, steps=a.steps, rounds=a.rounds, ms_per_step_median=med, ms_per_step_all=ms,
               source_cost_ms=med['moving'] - med['plain'], source_cost_fraction=(med['moving'] - med['plain']) / med['plain'],
               field_vs_unfused_ms=med['field'] - med['unfused'],
               note='plain / moving / unfused: graph-replayed runs of %d steps (incl. one copy in and out); field: per-call '
                    'steps' % a.steps)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
