"""Cost of the moving heat source on the cylindrical loop ("Cylindrical step"), alternated in one process
with device events.

    python scripts/cyl_source_probe.py [--rounds 8] [--steps 50] [--out profiles/cyl_source_probe.json]

BASELINE configs[3]: 128 x 256 x 512 cells, dr = dz = 0.25 mm, steel, dt = 0.05 s, Robin on the outer wall and the top.  Goldak
source a = b = c_f = 2 mm, c_r = 4 mm on the outer wall (r_c = 32 mm, depth along r: cladding), turning at 2 pi / 10 s and
rising at 1 mm/s.  Timed, round-robin so that drift hits both forms alike:
  plain    StagedCylStepper.run, no source (the graph-replayed loop of bench.py --config cyl)
  moving   the same loop with source= (k_cyl_r_fast_src<8> + phi + k_cyl_z_fast_tick<16> per step)
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (--rounds 1)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import adi_thermal_fields_amd.adi3d_hip_cyl as cyl  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    nr, nphi, nz = 128, 256, 512
    g = cyl.GridCyl(nr, nphi, nz, 2.5e-4, 2 * np.pi / nphi, 2.5e-4, 0.032)
    mat, prm = cyl.Material(7800.0, 490.0, 54.0), cyl.Params(0.05, 1.0, "be")
    rr, zbc = cyl.RobinR(400.0, 20.0), cyl.ZBC('neumann0', 'robin', h_top=500.0, T_inf_top=20.0)
    T0 = np.full((nr, nphi, nz), 20.0)
    T0[:, :, -16:] = 1000.0
    T = cyl.to_device(T0)
    src = cyl.CylGoldakSource(3000.0, 0.8, 2e-3, 2e-3, 2e-3, 4e-3, r_c=0.032, phi0=0.0, omega=2 * math.pi / 10.0,
                              z0=0.06, v_z=1e-3, depth='r')
    st_plain = cyl.StagedCylStepper(g, mat, prm, rr, zbc)
    st_src = cyl.StagedCylStepper(g, mat, prm, rr, zbc, source=src)
    forms = dict(plain=lambda: st_plain.run(T, a.steps), moving=lambda: st_src.run(T, a.steps, t0=0.0))
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
    hot = float(st_src.run(T, a.steps, t0=0.0).t.max())
    res = dict(shape=[nr, nphi, nz], steps=a.steps, rounds=a.rounds, ms_per_step_median=med, ms_per_step_all=ms,
               source_cost_ms=med['moving'] - med['plain'], source_cost_fraction=(med['moving'] - med['plain']) / med['plain'],
               T_max_with_source=hot, T_max_plain=float(st_plain.run(T, a.steps).t.max()),
               note='graph-replayed runs of %d steps (incl. one copy in and out), alternated' % a.steps)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
