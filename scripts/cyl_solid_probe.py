"""Cost of the solidification record on the cylindrical loop, alternated in one process with device
events.

    python scripts/cyl_solid_probe.py [--samples 5] [--steps 200] [--out profiles/cyl_solid_probe.json]
                                      [--parent-lines FILE ...] [--head-lines FILE ...]

BASELINE configs[3]: 128 x 256 x 512 cells, dr = dz = 0.25 mm, steel, dt = 0.05 s, Robin on the outer wall and the top; the
graph-replayed StagedCylStepper.run, medians of `samples` runs of `steps` steps, round-robin so that drift hits every case alike:
  a  plain            no keyword (the in-place loop of bench.py --config cyl)
  b  history_cold     history= alone on a cold field: the yardstick of the two-field loop
  c  solid_cold       solidification= on a cold field, with the hot words: every tile's word clear
  d  solid_cold_null  the same with use_hot_words = False: every tile runs the full path
  e  solid_front      solidification= on a field hot in 13 of the 256 phi columns (5 % of the tiles), cooling through T_freeze
  f  all_front        solidification= next to phase= and history= on the field of (e)
Expectation by bytes, stated before the measurement and not a pass bar: a step moves 48 B/cell; the cold pass reads 8 B/cell
with the hot words (B alone; there is no mask) and 16 B/cell without them (B and A), the cold history= pass 16 (B and T_peak).
So (c) should cost less than (b), and less than (d).
--parent-lines / --head-lines: result lines of `bench.py --config cyl --gpus 1 --steps 200 --warmup 20` of the parent commit and
of this one, taken in the same session on the same GPU (cyl_extras_probe.parent_check)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adi_thermal_fields_amd.adi3d_hip_cyl as cyl  # noqa: E402
from cyl_extras_probe import parent_check  # noqa: E402

T_FREEZE = 1425.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=5)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--out', default=None)
    ap.add_argument('--parent-lines', nargs='*', default=[])
    ap.add_argument('--head-lines', nargs='*', default=[])
    a = ap.parse_args()
    nr, nphi, nz = 128, 256, 512
    g = cyl.GridCyl(nr, nphi, nz, 2.5e-4, 2 * np.pi / nphi, 2.5e-4, 0.032)
    mat, prm = cyl.Material(7800.0, 490.0, 54.0), cyl.Params(0.05, 1.0, "be")
    rr, zbc = cyl.RobinR(400.0, 20.0), cyl.ZBC('neumann0', 'robin', h_top=500.0, T_inf_top=20.0)
    law, levels = cyl.PhaseChange(2.7e5, 1400.0, 1450.0), cyl.HistoryLevels(800.0, 500.0, 1450.0)
    cold = np.full((nr, nphi, nz), 20.0)
    front = cold.copy()
    front[:, :13, :] = 1500.0                           # 5 % of the tiles (a tile is one z line here): above T_freeze
    Tc, Tf = cyl.to_device(cold), cyl.to_device(front)
    cap = a.steps * (a.samples + 2)

    def stepper(T, phase, history, solid, words=True):
        ph = cyl.CylPhaseField(g, mat, law, T=T) if phase else None
        hi = cyl.CylThermalHistory(g, levels, capacity=cap, T=T) if history else None
        so = cyl.CylSolidificationRecord(g, T_FREEZE, capacity=cap) if solid else None
        if so is not None:
            so.use_hot_words = words
        return cyl.StagedCylStepper(g, mat, prm, rr, zbc, phase=ph, history=hi, solidification=so), ph, hi, so

    cases = dict(a_plain=(Tc, False, False, False), b_history_cold=(Tc, False, True, False),
                 c_solid_cold=(Tc, False, False, True), d_solid_cold_null=(Tc, False, False, True, False),
                 e_solid_front=(Tf, False, False, True), f_all_front=(Tf, True, True, True))
    built = {k: (v[0],) + stepper(*v) for k, v in cases.items()}

    def prepare(name):
        """every sample starts from the same state; outside the timed region"""
        T, st, ph, hi, so = built[name]
        if ph is not None:
            ph.seed(T)
        if hi is not None:
            hi.reset(T)
        if so is not None:
            so.reset()

    def run(name):
        T, st = built[name][:2]
        return st.run(T, a.steps)

    for name in cases:                                  # warm-up: graphs captured, modules loaded
        prepare(name)
        run(name)
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(a.samples):
        for name in cases:
            prepare(name)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(name)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.steps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    base = med['a_plain']
    so_e = built['e_solid_front'][4]
    words = so_e.d_hot.cpu().numpy()
    fr = so_e.front()
    res = dict(shape=[nr, nphi, nz], steps=a.steps, samples=a.samples, ms_per_step_median=med, ms_per_step_all=ms,
               ratio_to_plain={k: med[k] / base for k in med},
               ratio_solid_cold_to_history_cold=med['c_solid_cold'] / med['b_history_cold'],
               ratio_solid_cold_words_to_null=med['c_solid_cold'] / med['d_solid_cold_null'],
               expected_by_bytes=dict(c_solid_cold=1.0 + 8.0 / 48.0, d_solid_cold_null=1.0 + 16.0 / 48.0,
                                      b_history_cold=1.0 + 16.0 / 48.0),
               e_hot_tile_fraction_at_end=float(words.mean()), e_cells_frozen=int(fr['cells'].sum()),
               e_steps_with_a_front=int((fr['cells'] > 0).sum()),
               scatter={k: (max(v) - min(v)) / med[k] for k, v in ms.items()},
               parent_check=parent_check(a.parent_lines, a.head_lines),
               note='graph-replayed runs of %d steps (incl. one copy in and out and, with solidification=, the seeding of the '
                    'hot words; the recorders are reset before each sample, outside the timed region), alternated' % a.steps)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
