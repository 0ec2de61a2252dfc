"""Cost of material transitions inside the step of a MaterialMap: the graph-replayed step with
`material_map=` alone against the same step with `transitions=`, cold and with a pool that consolidates, without and with a
MapPhaseField, on the same shape in the same process.

    python scripts/transitions_probe.py [--rounds 5] [--steps 100] [--grids box,ellipsoid,head]
                                        [--out profiles/transitions_probe.json]

Shapes, dx, theta and dt: those of scripts/matmap_extras_probe.py with loose powder for the second material -- the 512^3
two-layer box with the upper layer as powder, the 512^3 ellipsoid with a powder shell, the 256 x 256 x 320 head of powder on a
dense base plate.  Rule: powder -> dense at 1450.  Every shape runs in a fresh child process; inside it the forms are timed
round-robin with device events, `rounds` samples of `steps` steps each, medians reported:
  matmap          StagedStepper.run with material_map= alone
  tr_cold         + transitions=, the field below the threshold everywhere: powder bricks read flags and T and return
  tr_pool         + transitions=, the field 300 K hotter: the powder above 1450 consolidates in the first step of every sample
                  (ids, words and packs are put back between samples, outside the timing)
  phase_cold      + phase=MapPhaseField alone, cold: the yardstick of DESIGN.md 6l2 (it reads the same bytes)
  phase_tr_pool   + phase= and transitions=, with the pool
There is no pass bar.  The byte estimate: a brick with powder reads flags and T, 9 B/cell, next to the map step's 72; every
other brick costs one word."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from matmap_probe import make_case, STEEL  # noqa: E402

POWDER = (4000.0, 490.0, 0.3)
FORMS = ('matmap', 'tr_cold', 'tr_pool', 'phase_cold', 'phase_tr_pool')
TAG = 'TRANSITIONS_PROBE '


def child(a):
    import torch
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from adi_thermal_fields_amd import waam
    shape, mask, ids, T0 = make_case(a.grid, waam)
    if a.grid == 'head':
        ids = (1 - ids).astype(np.uint8)                    # the head is the powder, the plate dense
    dx, Tinf = 2e-4, 25.0
    rho, cp, k = STEEL
    dt = 0.5 * dx * dx * rho * cp / k
    g = hip.Grid3D(*shape, dx, mask)
    prm = hip.Params(dt, 0.5)
    rules = (None, (0, 1450.0))
    laws = (hip.PhaseChange(2.7e5, 1400.0, 1450.0),) * 2
    T_cold = hip.to_device(0.5 * np.asarray(T0))            # 10 .. 650
    T_pool = hip.to_device(np.asarray(T0) + 300.0)          # 320 .. 1600
    # one map per form that changes ids, so that no form sees another's consolidated cells
    maps = {n: hip.MaterialMap(g, (STEEL, POWDER), ids, robin_h=15.0) for n in ('matmap', 'tr_pool', 'phase_tr_pool')}
    mm, mm_p, mm_pp = maps['matmap'], maps['tr_pool'], maps['phase_tr_pool']
    tr_cold, tr_pool = hip.MaterialTransitions(mm, rules), hip.MaterialTransitions(mm_p, rules)
    ph_cold, ph_pool = hip.MapPhaseField(mm, laws, T=T_cold), hip.MapPhaseField(mm_pp, laws, T=T_pool)
    tr_pp = hip.MaterialTransitions(mm_pp, rules, phase=ph_pool)
    mk = lambda m, **kw: hip.StagedStepper(g, m.mat, prm, m.packs, Tinf, material_map=m, **kw)      # noqa: E731
    st = dict(matmap=(mk(mm), T_pool, None), tr_cold=(mk(mm, transitions=tr_cold), T_cold, tr_cold),
              tr_pool=(mk(mm_p, transitions=tr_pool), T_pool, tr_pool), phase_cold=(mk(mm, phase=ph_cold), T_cold, None),
              phase_tr_pool=(mk(mm_pp, phase=ph_pool, transitions=tr_pp), T_pool, tr_pp))
    start = {n: (st[n][2].snapshot(), ph_pool.snapshot() if n == 'phase_tr_pool' else None)
             for n in ('tr_pool', 'phase_tr_pool')}
    changed = {}

    def timed(name):
        s, T, tr = st[name]
        if name in start:                                   # the pool consolidates anew in every sample
            tr.restore(start[name][0])
            if start[name][1] is not None:
                ph_pool.restore(start[name][1])
        if tr is not None:
            tr.reset_count()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        s.run(T, a.steps)
        e1.record()
        torch.cuda.synchronize()
        if tr is not None:
            changed[name] = tr.changed
        return e0.elapsed_time(e1) / a.steps
    for n in FORMS:                                        # warm-up: graphs captured, modules loaded, allocator filled
        timed(n)
        print('%s %s: warm-up %.3f ms per step' % (a.grid, n, timed(n)), file=sys.stderr, flush=True)
    ms = {n: [] for n in FORMS}
    for _ in range(a.rounds):
        for n in FORMS:
            ms[n].append(timed(n))
    in_mask = int(mask.sum())
    powder = int((mask & (ids == 1)).sum())
    info = dict(grid=a.grid, shape=shape, physical=g.layout.pd, steps=a.steps, rounds=a.rounds, ms_per_step=ms,
                cells=int(np.prod(shape)), in_mask=in_mask, powder_cells=powder, changed_per_sample=changed,
                matmap_bytes_per_cell=mm.bytes_per_cell, captures={n: st[n][0].captures for n in FORMS})
    print(TAG + json.dumps(info), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--grids', default='box,ellipsoid,head')
    ap.add_argument('--out', default=None)
    ap.add_argument('--timeout', type=float, default=400.0, help='seconds a child process may take')
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--grid', default='box')
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.child:
        return child(a)
    summary = []
    for grid in a.grids.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--child', '--grid', grid, '--rounds', str(a.rounds), '--steps', str(a.steps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)    # (its progress lines go to our stderr)
        if p.returncode != 0:                           # a child that failed ends the probe: nothing more is started
            sys.stderr.write(p.stdout[-2000:])
            raise SystemExit('transitions_probe: %s failed with status %d' % (grid, p.returncode))
        line = [ln for ln in p.stdout.splitlines() if ln.startswith(TAG)][-1]
        r = json.loads(line[len(TAG):])
        med = {n: float(np.median(v)) for n, v in r['ms_per_step'].items()}
        r['ms'] = med
        r['over_matmap'] = {n: med[n] / med['matmap'] for n in FORMS}
        r['phase_tr_pool_over_phase_cold'] = med['phase_tr_pool'] / med['phase_cold']
        # the estimate by bytes: 9 B per powder cell (flags and T) next to the map step's bytes per cell of the box
        r['tr_cold_byte_estimate'] = 1.0 + 9.0 * r['powder_cells'] / (r['matmap_bytes_per_cell'] * r['cells'])
        summary.append(r)
        print(grid, {n: round(v, 4) for n, v in med.items()}, file=sys.stderr, flush=True)
    out = dict(note='ms per step, medians over `rounds` samples of `steps` graph-replayed steps (StagedStepper.run, incl. one copy '
                    'in and out) in one process per shape; over_matmap: each form over material_map= alone; '
                    'tr_cold_byte_estimate: 1 + 9 B x powder cells / (map bytes per cell x cells of the box); changed_per_sample: '
                    'cells that changed their material in the last sample of the form',
               summary=summary)
    print(json.dumps(dict(summary=[{k: v for k, v in r.items() if k != 'ms_per_step'} for r in summary])))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
