"""Cost of temperature-dependent k(T) and cp(T): the graph-replayed step with and without `material=`,
against the plain step on the parent commit's library.

    python scripts/matlaw_probe.py --parent-tree <checkout of the parent commit, its library built>
                                   [--repeats 2] [--rounds 5] [--steps 20] [--grids box,head] [--out profiles/matlaw_probe.json]

Two grids: the 512^3 all-solid box and the 256 x 256 x 320 synthetic head, the field between 20 and 1300 degrees.  Steel-like
tables (k 52 -> 28 -> 60 W/m/K, cp 450 -> 800 J/kg/K, 2.7e5 J/kg between 1450 and 1500 degrees), dx = 0.2 mm,
dt = dx^2 rho cp_ref / (2 k_ref), theta = 0.5, h = 15 W/m^2/K: a constant-h pack for the plain step, SurfaceLoss(h=15) under the law.
Every (tree, grid) pair is measured in a fresh child process, the two trees alternated `repeats` times, because the fused
kernel's time differs from process to process by more than it does inside one; inside a child the forms are timed round-robin
with device events, `rounds` samples of `steps` graph-replayed steps each:
  plain     StagedStepper.run with Material(rho, cp_ref, k_ref)     (both trees: the parent's is the reference point)
  material  the same stepper with material=, loss included          (this tree)
  bare      ... with material= and no surface loss                  (this tree: the two passes alone)
There is no pass bar.  The expectation is byte-derived: the Kirchhoff pass reads T and the flags and writes theta (17 B/cell), the
recovery reads T, theta* and the flags and writes T (25 B/cell), less the flags of all-solid bricks: 40 B/cell next to the step's
bytes (StagedStepper.stage_bytes_per_cell)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO = 7800.0
STEEL = dict(T=[20.0, 400.0, 800.0, 1200.0, 1450.0, 1500.0, 2500.0], k=[52.0, 44.0, 30.0, 28.0, 32.0, 60.0, 60.0],
             cp=[450.0, 560.0, 800.0, 650.0, 700.0, 800.0, 800.0], latent_heat=2.7e5, T_solidus=1450.0, T_liquidus=1500.0)
K_REF, CP_REF = 52.0, 450.0          # the law's defaults: k[0] and min(cp k_ref / k)


def make_case(name, waam):
    if name == 'box':
        shape = (512, 512, 512)
        mask = np.ones(shape, dtype=bool)
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
    with_law = hasattr(hip, 'MaterialLaw')
    shape, mask, T0 = make_case(a.grid, waam)
    dx, Tinf = 2e-4, 25.0
    dt = 0.5 * dx * dx * RHO * CP_REF / K_REF
    g = hip.Grid3D(*shape, dx, mask)
    mat, prm = hip.Material(RHO, CP_REF, K_REF), hip.Params(dt, 0.5)
    packs = hip.precompute_coeff_packs_unified(g, mat, robin_h=15.0)
    T = hip.to_device(T0)
    forms = {}
    st_plain = hip.StagedStepper(g, mat, prm, packs, Tinf)
    forms['plain'] = lambda: st_plain.run(T, a.steps)
    info = dict(tree=a.tree, grid=a.grid, shape=shape, physical=g.layout.pd, steps=a.steps, rounds=a.rounds,
                step_bytes_per_cell=float(sum(st_plain.stage_bytes_per_cell)))
    if with_law:
        law = hip.MaterialLaw(**STEEL)
        assert (law.k_ref, law.cp_ref) == (K_REF, CP_REF)
        nm = hip.NonlinearPacks(g, RHO, law, Tinf, loss=hip.SurfaceLoss(h=15.0), T=T)
        st_mat = hip.StagedStepper(g, nm.mat, prm, nm.packs, material=nm)
        forms['material'] = lambda: st_mat.run(T, a.steps)
        bare = hip.NonlinearPacks(g, RHO, law, Tinf)
        st_bare = hip.StagedStepper(g, bare.mat, prm, bare.packs, material=bare)
        forms['bare'] = lambda: st_bare.run(T, a.steps)

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
    print('MATLAW_PROBE ' + json.dumps(info), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-tree', default=None, help='a checkout of the parent commit with its library built')
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--grids', default='box,head')
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
                    raise SystemExit('matlaw_probe: the %s tree failed on %s with status %d' % (label, grid, p.returncode))
                line = [ln for ln in p.stdout.splitlines() if ln.startswith('MATLAW_PROBE ')][-1]
                r = json.loads(line[len('MATLAW_PROBE '):])
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
        full, full_all = med('this', 'material')
        bare, bare_all = med('this', 'bare')
        parent, parent_all = med('parent', 'plain')
        summary.append(dict(grid=grid, shape=this['shape'], physical=this['physical'], ms_plain=plain, ms_material=full, ms_bare=bare,
                            ms_parent_plain=parent, ms_plain_per_process=plain_all, ms_material_per_process=full_all,
                            ms_bare_per_process=bare_all, ms_parent_plain_per_process=parent_all,
                            material_over_plain=full / plain, bare_over_plain=bare / plain,
                            step_bytes_per_cell=this['step_bytes_per_cell'],
                            byte_estimate_ratio=1.0 + 40.0 / this['step_bytes_per_cell'],
                            plain_over_parent=None if parent is None else plain / parent,
                            material_over_parent=None if parent is None else full / parent))
    out = dict(note='ms per step of graph-replayed runs of `steps` steps (incl. one copy in and out); medians over `rounds` samples '
                    'per process, then over `repeats` fresh processes per tree; byte_estimate_ratio: 1 + 40 B/cell over the '
                    'step\'s bytes per cell',
               summary=summary, runs=runs)
    print(json.dumps(dict(summary=summary)))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
