"""Cost of the field monitor on the cylindrical loop, alternated in one process with device events.

    python scripts/cyl_monitor_probe.py [--samples 5] [--steps 200] [--out profiles/cyl_monitor_probe.json]
                                        [--parent-lines FILE ...] [--head-lines FILE ...]

BASELINE configs[3]: 128 x 256 x 512 cells, dr = dz = 0.25 mm, steel, dt = 0.05 s, Robin on the outer wall and the top; the
graph-replayed StagedCylStepper.run, medians of `samples` runs of `steps` steps, round-robin so that drift hits every case alike:
  a  plain            no keyword (the in-place loop of bench.py --config cyl)
  b  monitor_whole    monitor= with the whole grid as its one region and 4 probes
  c  monitor_box      monitor= with one region of 16 radii x 32 phi cells x 64 z cells (astride the seam) and 4 probes
  d  monitor_all      monitor= (the whole grid, extra = f) next to phase= and history=, on a field with 5 % of the cells mushy
  e  phase_history    (d) without the monitor: what (d) is held against
Expectation by bytes, stated before the measurement and not a pass bar: a step moves 48 B/cell, the monitor reads 8 more, so
about +17 % for (b); (c) reads 1/512 of the grid and costs its three launches and the tick.
The check of (a) against the parent commit: --parent-lines are result lines of the PARENT commit's `bench.py --config cyl --gpus 1
--steps 200 --warmup 20`, --head-lines the same of this commit, all taken in the same session on the same GPU.  The JSON records
both sets in ms per step, each set's scatter (max - min over its median), the ratio of the medians, and `agrees`: the medians
differ by no more than the two scatters together.  Without the files the check is recorded as not measured."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import adi_thermal_fields_amd.adi3d_hip_cyl as cyl  # noqa: E402
from cyl_extras_probe import parent_check  # noqa: E402


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
    hot = cold.copy()
    hot[:, :, -26:] = 1425.0                            # 5 % of the cells (the top 26 planes): mushy, and above T_lo
    Tc, Th = cyl.to_device(cold), cyl.to_device(hot)
    cap = a.steps * (a.samples + 2)
    probes = [(0, 0, 0), (nr - 1, nphi - 1, nz - 1), (64, 0, 500), (64, nphi - 1, 500)]
    box = ((56, 72), (nphi - 16, nphi + 16), (nz - 64, nz))

    def stepper(T, phase, history, regions):
        ph = cyl.CylPhaseField(g, mat, law, T=T) if phase else None
        hi = cyl.CylThermalHistory(g, levels, capacity=cap, T=T) if history else None
        mon = None
        if regions is not None:
            mon = cyl.CylFieldMonitor(g, probes=probes, regions=regions, capacity=cap, extra=None if ph is None else ph.f)
        return cyl.StagedCylStepper(g, mat, prm, rr, zbc, phase=ph, history=hi, monitor=mon), ph, hi, mon

    cases = dict(a_plain=(Tc, False, False, None), b_monitor_whole=(Tc, False, False, [None]),
                 c_monitor_box=(Tc, False, False, [box]), d_monitor_all=(Th, True, True, [None]),
                 e_phase_history=(Th, True, True, None))
    built = {k: (v[0],) + stepper(*v) for k, v in cases.items()}

    def prepare(name):
        """every sample starts from the same state; outside the timed region"""
        T, st, ph, hi, mon = built[name]
        if ph is not None:
            ph.seed(T)
        if hi is not None:
            hi.reset(T)
        if mon is not None:
            mon.reset()

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
    whole = built['b_monitor_whole'][4].region_log(mat)
    ratio = {k: med[k] / base for k in med}
    ratio['d_monitor_all_to_e_phase_history'] = med['d_monitor_all'] / med['e_phase_history']
    res = dict(shape=[nr, nphi, nz], steps=a.steps, samples=a.samples, ms_per_step_median=med, ms_per_step_all=ms,
               ratio_to_plain=ratio, expected_by_bytes=dict(b_monitor_whole=1.0 + 8.0 / 48.0),
               meets_expectation=dict(b_monitor_whole=bool(ratio['b_monitor_whole'] <= 1.0 + 8.0 / 48.0)),
               monitor_ms_per_step=dict(whole=med['b_monitor_whole'] - base, box=med['c_monitor_box'] - base,
                                        next_to_phase_and_history=med['d_monitor_all'] - med['e_phase_history']),
               rows_b=int(built['b_monitor_whole'][4].slot), T_mean_b_last=float(whole['T_mean'][0, -1]),
               scatter={k: (max(v) - min(v)) / med[k] for k, v in ms.items()},
               parent_check=parent_check(a.parent_lines, a.head_lines),
               note='graph-replayed runs of %d steps (incl. one copy in and out; f, the history and the log are reset before '
                    'each sample, outside the timed region), alternated' % a.steps)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
