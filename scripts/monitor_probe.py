"""Cost of the field monitor: the graph-replayed step with and without `monitor=`, with a plain device
read of one field as the floor.

    python scripts/monitor_probe.py [--repeats 2] [--rounds 5] [--steps 20] [--grids box,ellipsoid,head]
                                    [--out profiles/monitor_probe.json]

Three grids: the 512^3 all-solid box, the 512^3 ellipsoid and the 256 x 256 x 320 synthetic head (scripts/history_probe.py).
Steel, dx = 0.2 mm, dt = dx^2 / (2 kappa), theta = 0.5, h = 15 W/m^2/K.  Every grid is measured in a fresh child process,
`repeats` times; inside a child the forms are timed round-robin with device events, `rounds` samples of `steps`
graph-replayed steps each:
  plain          StagedStepper.run without monitor= (what the parent commit runs)
  monitor_whole  the same stepper with monitor=, one region: the whole grid, and 8 probes
  monitor_pool   (head only) one region of 64^3 cells under the crown, 8 probes: the launch box is 4 x 4 x 4 bricks (5 along an
                 axis the box is not aligned on)
  read8          one torch sum over a field's storage, 8 B/cell read: the floor of a pass over T
There is no pass bar.  The expectation is byte-derived: the monitor adds 8 B/cell to the step's bytes
(StagedStepper.stage_bytes_per_cell), plus 1 B/cell of flags in the bricks that hold a surface."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from history_probe import make_case, RHO, CP, K  # noqa: E402  (the same three grids)

FORMS = ('plain', 'monitor_whole', 'monitor_pool', 'read8')


def child(a):
    sys.path.insert(0, a.tree)
    import torch
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from adi_thermal_fields_amd import waam
    shape, mask, u = make_case(a.grid, waam)
    dx = 2e-4
    dt = 0.5 * dx * dx / (K / (RHO * CP))
    Tinf = 25.0
    g = hip.Grid3D(*shape, dx, mask)
    mat, prm = hip.Material(RHO, CP, K), hip.Params(dt, 0.5)
    packs = hip.precompute_coeff_packs_unified(g, mat, robin_h=15.0)
    T = hip.to_device(900.0 + 700.0 * u)
    cap = 64 * a.steps * (a.rounds + 4)
    inside = np.argwhere(mask)
    probes = [tuple(int(v) for v in inside[i]) for i in np.linspace(0, len(inside) - 1, 8).astype(int)]
    steppers = {'plain': hip.StagedStepper(g, mat, prm, packs, Tinf)}
    mons = {'monitor_whole': hip.FieldMonitor(g, probes=probes, regions=(None,), capacity=cap)}
    if a.grid == 'head':                                # 64^3 under the crown: the top in-mask cell of the centre line
        ci, cj = shape[0] // 2, shape[1] // 2
        top = int(np.flatnonzero(mask[ci, cj])[-1]) + 1
        box = ((ci - 32, ci + 32), (cj - 32, cj + 32), (top - 64, top))
        mons['monitor_pool'] = hip.FieldMonitor(g, probes=probes, regions=(box,), capacity=cap)
    for n, m in mons.items():
        steppers[n] = hip.StagedStepper(g, mat, prm, packs, Tinf, monitor=m)
    flat = T.t.as_strided((T.t.untyped_storage().nbytes() // 8,), (1,))

    def read8():
        for _ in range(a.steps):
            flat.sum()
    forms = {n: (lambda s=s: s.run(T, a.steps)) for n, s in steppers.items()}
    forms['read8'] = read8
    info = dict(tree=a.tree, grid=a.grid, shape=shape, physical=g.layout.pd, steps=a.steps, rounds=a.rounds,
                step_bytes_per_cell=float(sum(steppers['plain'].stage_bytes_per_cell)))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps
    for fn in forms.values():                           # warm-up: graphs captured, modules loaded, allocator filled
        timed(fn)
        timed(fn)
    torch.cuda.synchronize()
    ms = {n: [] for n in forms}
    for _ in range(a.rounds):
        for n, fn in forms.items():
            ms[n].append(timed(fn))
    info['ms_per_step'] = ms
    nb = [(n + 15) // 16 for n in g.layout.pd[:3]]
    words = g.d_bricks.cpu().numpy().view(np.uint32)
    log = mons['monitor_whole'].region_log(mat=mat)
    info.update(cells_in_mask=int(mask.sum()), cells_logged=int(log['cells'][0, -1]), rows_logged=int(log['cells'].shape[1]),
                bricks=int(nb[0] * nb[1] * nb[2]),
                launch_bricks={n: [b for _, b in hip.FieldMonitor.brick_box(m.regions[0])] for n, m in mons.items()},
                flag_bricks_all_solid_fraction=sum(bin(int(w)).count('1') for w in words) / float(nb[0] * nb[1] * nb[2]))
    print('MONITOR_PROBE ' + json.dumps(info), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--grids', default='box,ellipsoid,head')
    ap.add_argument('--out', default=None)
    ap.add_argument('--timeout', type=float, default=400.0, help='seconds a child process may take')
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--tree', default=ROOT)
    ap.add_argument('--grid', default='box')
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for grid in a.grids.split(','):
        for rep in range(a.repeats):
            cmd = [sys.executable, os.path.abspath(__file__), '--child', '--tree', ROOT, '--grid', grid, '--rounds',
                   str(a.rounds), '--steps', str(a.steps)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.timeout)
            if p.returncode != 0:                       # a child that failed ends the probe: nothing more is started
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit('monitor_probe: %s failed with status %d' % (grid, p.returncode))
            line = [ln for ln in p.stdout.splitlines() if ln.startswith('MONITOR_PROBE ')][-1]
            r = json.loads(line[len('MONITOR_PROBE '):])
            r.update(repeat=rep)
            r.pop('tree')
            runs.append(r)
            print(grid, rep, {n: round(float(np.median(v)), 4) for n, v in r['ms_per_step'].items()}, file=sys.stderr, flush=True)
    summary = []
    for grid in a.grids.split(','):
        mine = [r for r in runs if r['grid'] == grid]
        this = mine[0]

        def med(form):
            v = [float(np.median(r['ms_per_step'][form])) for r in mine]
            return float(np.median(v)), [round(x, 5) for x in v]
        plain, plain_all = med('plain')
        read, _ = med('read8')
        s = dict(grid=grid, shape=this['shape'], physical=this['physical'], ms_plain=plain, ms_read8=read,
                 ms_plain_per_process=plain_all, read_GBps=8.0 * this['physical'][0] * this['physical'][3] / read / 1e6,
                 step_bytes_per_cell=this['step_bytes_per_cell'], byte_estimate_fraction=8.0 / this['step_bytes_per_cell'])
        for form in ('monitor_whole', 'monitor_pool'):
            if form in this['ms_per_step']:
                m, m_all = med(form)
                s.update({'ms_' + form: m, 'ms_%s_per_process' % form: m_all, 'overhead_%s_ms' % form: m - plain,
                          'overhead_%s_fraction' % form: (m - plain) / plain, 'overhead_%s_over_read8' % form: (m - plain) / read})
        for k in ('cells_in_mask', 'cells_logged', 'rows_logged', 'bricks', 'launch_bricks', 'flag_bricks_all_solid_fraction'):
            s[k] = this[k]
        summary.append(s)
    out = dict(note='ms per step of graph-replayed runs of `steps` steps (incl. one copy in and out); medians over `rounds` samples '
                    'per process, then over `repeats` fresh processes; read8: one torch sum over a field\'s storage per step; '
                    'byte_estimate_fraction: 8 B/cell over the step\'s bytes per cell',
               summary=summary, runs=runs)
    print(json.dumps(dict(summary=summary)))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
