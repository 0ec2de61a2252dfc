"""Cost of the latent-heat correction: the graph-replayed step with and without `phase=`, against the
same step on the parent commit's library, with a plain device read of the field as the floor.

    python scripts/phase_probe.py --parent-tree <checkout of the parent commit, its library built>
                                  [--repeats 2] [--rounds 5] [--steps 20] [--grids box,ellipsoid,head] [--out profiles/phase_probe.json]

Three grids: the 512^3 all-solid box and the 512^3 ellipsoid with nothing molten (field between 20 and 1300 degrees), and the
256 x 256 x 320 synthetic head with a pool that a Goldak source on its crown has made (the source stays on while timing).  Steel,
dx = 0.2 mm, dt = dx^2 / (2 kappa), theta = 0.5, h = 15 W/m^2/K, melting between 1400 and 1450 degrees, L = 2.7e5 J/kg.
Every (tree, grid) pair is measured in a fresh child process, the two trees alternated `repeats` times, because the fused
kernel's time differs from process to process by more than it does inside one; inside a child the forms are timed round-robin
with device events, `rounds` samples of `steps` graph-replayed steps each:
  plain    StagedStepper.run without phase=                     (both trees: the parent's is the reference point)
  phase    the same stepper with phase=                         (this tree)
  read     a torch sum over the field's storage, 8 B/cell read  (this tree: the floor of one more pass over T)
There is no pass bar.  The expectation is byte-derived: where nothing is molten the pass reads T once, 8 B/cell on top of the
step's bytes (StagedStepper.stage_bytes_per_cell), plus 1 B/cell of flags in the bricks that hold a surface."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO, CP, K = 7800.0, 490.0, 54.0


def make_case(name, waam):
    """(shape, mask, T0): nothing above 1300 degrees"""
    if name == 'box':
        shape = (512, 512, 512)
        mask = np.ones(shape, dtype=bool)
    elif name == 'ellipsoid':
        shape = (512, 512, 512)
        x = (np.arange(512, dtype=np.float32) + 0.5) / 512 - 0.5
        mask = (x[:, None, None] / 0.48) ** 2 + (x[None, :, None] / 0.45) ** 2 + (x[None, None, :] / 0.47) ** 2 <= 1.0
    elif name == 'head':
        shape = (256, 256, 320)
        mask = waam.synthetic_head_mask(*shape)
    else:
        raise ValueError(name)
    i = np.arange(shape[0], dtype=np.float64)[:, None, None]
    k = np.arange(shape[2], dtype=np.float64)[None, None, :]
    return shape, mask, np.broadcast_to(660.0 + 640.0 * np.sin(0.02 * i) * np.cos(0.015 * k), shape)


def child(a):
    sys.path.insert(0, a.tree)
    import torch
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from adi_thermal_fields_amd import waam
    with_phase = hasattr(hip, 'PhaseField')
    shape, mask, T0 = make_case(a.grid, waam)
    dx = 2e-4
    dt = 0.5 * dx * dx / (K / (RHO * CP))
    Tinf = 25.0
    g = hip.Grid3D(*shape, dx, mask)
    mat, prm = hip.Material(RHO, CP, K), hip.Params(dt, 0.5)
    packs = hip.precompute_coeff_packs_unified(g, mat, robin_h=15.0)
    T = hip.to_device(T0)
    src = None
    if a.grid == 'head':                                # the crown of the head: the top in-mask cell of the centre line
        top = int(np.flatnonzero(mask[shape[0] // 2, shape[1] // 2])[-1]) + 1
        src = hip.GoldakSource(power=2500.0, eta=0.8, a=1.5e-3, b=1.5e-3, c_f=1.5e-3, c_r=3e-3, f_f=0.6,
                               origin=(shape[0] // 2 * dx, (shape[1] // 2 - 20) * dx, top * dx), velocity=0.01, travel_axis=1,
                               travel_sign=1, depth_axis=2)
    forms = {}
    st_plain = hip.StagedStepper(g, mat, prm, packs, Tinf, source=src)
    forms['plain'] = (None, lambda: st_plain.run(T, a.steps, t0=0.0))       # (untimed preparation, timed work)
    info = dict(tree=a.tree, grid=a.grid, shape=shape, physical=g.layout.pd, steps=a.steps, rounds=a.rounds,
                step_bytes_per_cell=float(sum(st_plain.stage_bytes_per_cell)))
    if with_phase:
        law = hip.PhaseChange(2.7e5, 1400.0, 1450.0)
        ph = hip.PhaseField(g, mat, law, T=T)
        st_phase = hip.StagedStepper(g, mat, prm, packs, Tinf, source=src, phase=ph)
        if src is not None:                             # make the pool: 60 steps under the source, then time from that state
            T = st_phase.run(T, 60, t0=0.0)
        held = ph.snapshot()
        forms['phase'] = (lambda: ph.restore(held), lambda: st_phase.run(T, a.steps, t0=0.0))
        flat = T.t.as_strided((T.t.untyped_storage().nbytes() // 8,), (1,))

        def read():
            for _ in range(a.steps):
                flat.sum()
        forms['read'] = (None, read)
        f = np.asarray(ph.liquid_fraction)
        info.update(cells_with_liquid=int((f > 0).sum()), cells_fully_liquid=int((f == 1).sum()),
                    summary_entries=int(ph.summary.numel()), summary_entries_set=int((ph.summary != 0).sum().item()))
        nb = [(n + 15) // 16 for n in g.layout.pd[:3]]
        words = g.d_bricks.cpu().numpy().view(np.uint32)
        nset = int(sum(bin(int(w)).count('1') for w in words))
        info['flag_bricks_all_solid_fraction'] = nset / float(nb[0] * nb[1] * nb[2])
    elif src is not None:
        T = st_plain.run(T, 60, t0=0.0)

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
    print('PHASE_PROBE ' + json.dumps(info), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-tree', default=None, help='a checkout of the parent commit with its library built')
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
    trees = [('this', ROOT)] + ([('parent', os.path.abspath(a.parent_tree))] if a.parent_tree else [])
    runs = []
    for grid in a.grids.split(','):
        for rep in range(a.repeats):
            for label, tree in trees:
                env = dict(os.environ)
                env.pop('ADI_HIP_LIB', None)
                cmd = [sys.executable, os.path.abspath(__file__), '--child', '--tree', tree, '--grid', grid, '--rounds',
                       str(a.rounds), '--steps', str(a.steps)]
                p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.timeout)
                if p.returncode != 0:                   # a child that failed ends the probe: nothing more is started
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit('phase_probe: the %s tree failed on %s with status %d' % (label, grid, p.returncode))
                line = [ln for ln in p.stdout.splitlines() if ln.startswith('PHASE_PROBE ')][-1]
                r = json.loads(line[len('PHASE_PROBE '):])
                r.update(label=label, repeat=rep)
                runs.append(r)
                print(grid, label, rep, {n: round(float(np.median(v)), 4) for n, v in r['ms_per_step'].items()}, file=sys.stderr,
                      flush=True)
    summary = []
    for grid in a.grids.split(','):
        def med(label, form):
            v = [float(np.median(r['ms_per_step'][form])) for r in runs if r['grid'] == grid and r['label'] == label
                 and form in r['ms_per_step']]
            return (float(np.median(v)), [round(x, 5) for x in v]) if v else (None, [])
        this = [r for r in runs if r['grid'] == grid and r['label'] == 'this'][0]
        plain, plain_all = med('this', 'plain')
        phase, phase_all = med('this', 'phase')
        read, _ = med('this', 'read')
        parent, parent_all = med('parent', 'plain')
        ncell = float(np.prod(this['physical'][:3]))
        s = dict(grid=grid, shape=this['shape'], physical=this['physical'], ms_plain=plain, ms_phase=phase, ms_read=read,
                 ms_parent_plain=parent, ms_plain_per_process=plain_all, ms_phase_per_process=phase_all,
                 ms_parent_plain_per_process=parent_all, overhead_ms=phase - plain, overhead_fraction=(phase - plain) / plain,
                 overhead_over_read=(phase - plain) / read, read_GBps=8.0 * this['physical'][0] * this['physical'][3] / read / 1e6,
                 step_bytes_per_cell=this['step_bytes_per_cell'], byte_estimate_fraction=8.0 / this['step_bytes_per_cell'],
                 plain_over_parent=None if parent is None else plain / parent,
                 phase_over_parent=None if parent is None else phase / parent, cells=ncell,
                 cells_with_liquid=this['cells_with_liquid'], summary_entries=this['summary_entries'],
                 summary_entries_set=this['summary_entries_set'],
                 flag_bricks_all_solid_fraction=this['flag_bricks_all_solid_fraction'])
        summary.append(s)
    out = dict(note='ms per step of graph-replayed runs of `steps` steps (incl. one copy in and out); medians over `rounds` samples '
                    'per process, then over `repeats` fresh processes per tree; read: one torch sum over the field storage per '
                    'step; byte_estimate_fraction: 8 B/cell over the step\'s bytes per cell',
               summary=summary, runs=runs)
    print(json.dumps(dict(summary=summary)))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
