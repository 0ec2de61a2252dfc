"""Cost of the solidification recorder: the graph-replayed step with and without `solidification=`, with a
plain device read of one field as the floor.

    python scripts/solidification_probe.py [--repeats 2] [--rounds 5] [--steps 20] [--grids box,ellipsoid,head]
                                           [--out profiles/solidification_probe.json]

Three grids: the 512^3 all-solid box, the 512^3 ellipsoid and the 256 x 256 x 320 synthetic head.  Steel, dx = 0.2 mm,
dt = dx^2 / (2 kappa), theta = 0.5, h = 15 W/m^2/K, T_freeze = 1450 degrees.  Two states of the metal:
  cold   the field between 20 and 480 degrees: no brick word is set, the pass reads B (and flags in surface bricks)
  hot    the field between 200 and 1600 degrees: the bricks that hold a cell above T_freeze load A too, and the cells that
         cool through it in a step take the divergent part; on the head a Goldak source on the crown has made a pool first and
         stays on, so a front exists in every step
Every grid is measured in a fresh child process, `repeats` times; inside a child the forms are timed round-robin with device
events, `rounds` samples of `steps` graph-replayed steps each:
  plain        StagedStepper.run without solidification=
  solid_cold   the same stepper with solidification=, the recorder reset to the cold field before every sample (untimed)
  solid_hot    ... to the hot field
  read8        one torch sum over a field's storage, 8 B/cell read: the floor of a pass over B
There is no pass bar.  The expectation is byte-derived: cold metal adds 8 B/cell to the step's bytes
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

T_FREEZE = 1450.0
FORMS = ('plain', 'solid_cold', 'solid_hot', 'read8')


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
    T_cold, T_hot = hip.to_device(250.0 + 230.0 * u), hip.to_device(900.0 + 700.0 * u)
    src = None
    if a.grid == 'head':                                # the crown of the head: the top in-mask cell of the centre line
        top = int(np.flatnonzero(mask[shape[0] // 2, shape[1] // 2])[-1]) + 1
        src = hip.GoldakSource(power=2500.0, eta=0.8, a=1.5e-3, b=1.5e-3, c_f=1.5e-3, c_r=3e-3, f_f=0.6,
                               origin=(shape[0] // 2 * dx, (shape[1] // 2 - 20) * dx, top * dx), velocity=0.01, travel_axis=1,
                               travel_sign=1, depth_axis=2)
    rec = hip.SolidificationRecord(g, T_FREEZE, T=T_cold)
    st_plain = hip.StagedStepper(g, mat, prm, packs, Tinf, source=src)
    st_rec = hip.StagedStepper(g, mat, prm, packs, Tinf, source=src, solidification=rec)
    if src is not None:                                 # make the pool: 60 steps under the source, then time from that state
        T_hot = st_plain.run(T_hot, 60, t0=0.0)
    flat = T_cold.t.as_strided((T_cold.t.untyped_storage().nbytes() // 8,), (1,))

    def read8():
        for _ in range(a.steps):
            flat.sum()
    forms = {'plain': (None, lambda: st_plain.run(T_hot, a.steps, t0=0.0)),          # (untimed preparation, timed work)
             'solid_cold': (lambda: rec.reset(T_cold), lambda: st_rec.run(T_cold, a.steps, t0=0.0)),
             'solid_hot': (lambda: rec.reset(T_hot), lambda: st_rec.run(T_hot, a.steps, t0=0.0)),
             'read8': (None, read8)}
    info = dict(tree=a.tree, grid=a.grid, shape=shape, physical=g.layout.pd, steps=a.steps, rounds=a.rounds,
                step_bytes_per_cell=float(sum(st_plain.stage_bytes_per_cell)))

    def timed(prep, fn):
        if prep is not None:
            prep()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps
    for prep, fn in forms.values():                     # warm-up: graphs captured, modules loaded, allocator filled
        timed(prep, fn)
        timed(prep, fn)
    torch.cuda.synchronize()
    ms = {n: [] for n in forms}
    for _ in range(a.rounds):
        for n, (prep, fn) in forms.items():
            ms[n].append(timed(prep, fn))
    info['ms_per_step'] = ms
    nb = [(n + 15) // 16 for n in g.layout.pd[:3]]
    words = g.d_bricks.cpu().numpy().view(np.uint32)
    info.update(cells_in_mask=int(mask.sum()),                                       # (of the last sample: the hot state)
                cells_frozen_in_last_sample=int(np.isfinite(np.asarray(rec.t_solid)).sum()),
                bricks=int(nb[0] * nb[1] * nb[2]), bricks_hot_after_last_sample=int(rec.d_hot.sum().item()),
                flag_bricks_all_solid_fraction=sum(bin(int(w)).count('1') for w in words) / float(nb[0] * nb[1] * nb[2]))
    print('SOLIDIFICATION_PROBE ' + json.dumps(info), flush=True)


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
                raise SystemExit('solidification_probe: %s failed with status %d' % (grid, p.returncode))
            line = [ln for ln in p.stdout.splitlines() if ln.startswith('SOLIDIFICATION_PROBE ')][-1]
            r = json.loads(line[len('SOLIDIFICATION_PROBE '):])
            r.update(repeat=rep)
            r.pop('tree')
            runs.append(r)
            print(grid, rep, {n: round(float(np.median(v)), 4) for n, v in r['ms_per_step'].items()}, file=sys.stderr, flush=True)
    summary = []
    for grid in a.grids.split(','):
        mine = [r for r in runs if r['grid'] == grid]

        def med(form):
            v = [float(np.median(r['ms_per_step'][form])) for r in mine]
            return float(np.median(v)), [round(x, 5) for x in v]
        (plain, plain_all), (cold, cold_all), (hot, hot_all), (read, _) = (med(f) for f in FORMS)
        this = mine[0]
        s = dict(grid=grid, shape=this['shape'], physical=this['physical'], ms_plain=plain, ms_solid_cold=cold,
                 ms_solid_hot=hot, ms_read8=read, ms_plain_per_process=plain_all, ms_solid_cold_per_process=cold_all,
                 ms_solid_hot_per_process=hot_all, overhead_cold_ms=cold - plain, overhead_cold_fraction=(cold - plain) / plain,
                 overhead_hot_ms=hot - plain, overhead_hot_fraction=(hot - plain) / plain,
                 overhead_cold_over_read8=(cold - plain) / read,
                 read_GBps=8.0 * this['physical'][0] * this['physical'][3] / read / 1e6,
                 step_bytes_per_cell=this['step_bytes_per_cell'], byte_estimate_fraction=8.0 / this['step_bytes_per_cell'])
        for k in ('cells_in_mask', 'cells_frozen_in_last_sample', 'bricks', 'bricks_hot_after_last_sample',
                  'flag_bricks_all_solid_fraction'):
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
