"""Cost of latent heat and surface loss on a grid of several materials: the graph-replayed step with
`material_map=` alone -- the yardstick, what the step could do before -- against the same step with a MapLossPacks, with a
MapPhaseField (cold, and with a melt pool), and with both, on the same shape in the same process.

    python scripts/matmap_extras_probe.py [--rounds 2] [--steps 100] [--grids box,ellipsoid,head]
                                          [--out profiles/matmap_extras_probe.json]

Shapes, dx, theta and dt: those of scripts/matmap_probe.py (the 512^3 two-layer box, the 512^3 ellipsoid with a shell, the
256 x 256 x 320 head on a base plate; steel and copper).  The map is built with robin_h=None (a MapLossPacks needs that); the
sweeps read the coefficient arrays at exposed cells whatever they hold, so the yardstick's traffic is that of a map with h.
Every shape runs in a fresh child process; inside it the forms are timed round-robin with device events, `rounds` samples of
`steps` steps each, medians reported:
  matmap       StagedStepper.run with material_map= alone
  loss         + surface_loss=MapLossPacks (h = 15 W/m^2/K, emissivity 0.8 / 0.05, a 4-knot table on steel)
  phase_cold   + phase=MapPhaseField, the field below every solidus: f = 0 everywhere, the pass reads T once
  phase_pool   + phase=MapPhaseField, the field 300 K hotter: both materials melt in places
  both         + both, with the pool
There is no pass bar.  The byte estimate: the cold phase pass reads 8 B/cell of in-mask bricks next to the map step's 72; the
loss pass reads the flags (1 B/cell) outside set inner bricks and touches exposed cells only."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from matmap_probe import make_case, STEEL, COPPER  # noqa: E402

FORMS = ('matmap', 'loss', 'phase_cold', 'phase_pool', 'both')


def child(a):
    import torch
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from adi_thermal_fields_amd import waam
    shape, mask, ids, T0 = make_case(a.grid, waam)
    dx, Tinf = 2e-4, 25.0
    rho, cp, k = STEEL
    dt = 0.5 * dx * dx * rho * cp / k
    g = hip.Grid3D(*shape, dx, mask)
    prm = hip.Params(dt, 0.5)
    mm = hip.MaterialMap(g, (STEEL, COPPER), ids)
    losses = (hip.SurfaceLoss(h=15.0, emissivity=0.8, table=([300.0, 800.0, 1200.0, 1600.0], [2.0, 9.0, 30.0, 55.0])),
              hip.SurfaceLoss(h=15.0, emissivity=0.05))
    laws = (hip.PhaseChange(2.7e5, 1400.0, 1450.0), hip.PhaseChange(2.05e5, 1083.0, 1085.0))
    T_cold = hip.to_device(0.5 * np.asarray(T0))            # 10 .. 650: below both solidus temperatures
    T_pool = hip.to_device(np.asarray(T0) + 300.0)          # 320 .. 1600: pools in both materials
    lp = hip.MapLossPacks(mm, losses, Tinf)
    ph_cold = hip.MapPhaseField(mm, laws, T=T_cold)
    ph_pool = hip.MapPhaseField(mm, laws, T=T_pool)
    liquid = float((ph_pool.f > 0).sum().item()) / float(mask.sum())
    mk = lambda **kw: hip.StagedStepper(g, mm.mat, prm, mm.packs, Tinf, material_map=mm, **kw)     # noqa: E731
    st = dict(matmap=(mk(), T_pool), loss=(mk(surface_loss=lp), T_pool), phase_cold=(mk(phase=ph_cold), T_cold),
              phase_pool=(mk(phase=ph_pool), T_pool), both=(mk(surface_loss=lp, phase=ph_pool), T_pool))

    def timed(name):
        s, T = st[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        s.run(T, a.steps)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps
    for n in FORMS:                                        # warm-up: graphs captured, modules loaded, allocator filled
        timed(n)
        print('%s %s: warm-up %.3f ms per step' % (a.grid, n, timed(n)), file=sys.stderr, flush=True)
    ms = {n: [] for n in FORMS}
    for _ in range(a.rounds):
        for n in FORMS:
            ms[n].append(timed(n))
    exposed = float(((g.d_flags & 1) != 0).logical_and((g.d_flags & 0x7e) != 0x7e).sum().item())
    info = dict(grid=a.grid, shape=shape, physical=g.layout.pd, steps=a.steps, rounds=a.rounds, ms_per_step=ms,
                cells=int(np.prod(shape)), in_mask=int(mask.sum()), exposed_cells=int(exposed), liquid_share_at_start=liquid,
                matmap_bytes_per_cell=mm.bytes_per_cell, captures={n: st[n][0].captures for n in FORMS})
    print('MATMAP_EXTRAS_PROBE ' + json.dumps(info), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--grids', default='box,ellipsoid,head')
    ap.add_argument('--out', default=None)
    ap.add_argument('--timeout', type=float, default=240.0, help='seconds a child process may take')
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
            raise SystemExit('matmap_extras_probe: %s failed with status %d' % (grid, p.returncode))
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('MATMAP_EXTRAS_PROBE ')][-1]
        r = json.loads(line[len('MATMAP_EXTRAS_PROBE '):])
        med = {n: float(np.median(v)) for n, v in r['ms_per_step'].items()}
        r['ms'] = med
        r['over_matmap'] = {n: med[n] / med['matmap'] for n in FORMS}
        # the estimate by bytes: 8 B per cell of the box for the cold pass (an upper bound where bricks are empty) next to the
        # map step's bytes per cell
        r['phase_cold_byte_estimate'] = (r['matmap_bytes_per_cell'] + 8.0) / r['matmap_bytes_per_cell']
        summary.append(r)
        print(grid, {n: round(v, 4) for n, v in med.items()}, file=sys.stderr, flush=True)
    out = dict(note='ms per step, medians over `rounds` samples of `steps` graph-replayed steps (StagedStepper.run, incl. one copy '
                    'in and out) in one process per shape; over_matmap: each form over material_map= alone; '
                    'phase_cold_byte_estimate: (map bytes per cell + 8) / map bytes per cell',
               summary=summary)
    print(json.dumps(dict(summary=[{k: v for k, v in r.items() if k != 'ms_per_step'} for r in summary])))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
