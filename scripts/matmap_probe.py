"""Cost of several materials in one grid: the graph-replayed step with `material_map=` against the plain
step on the same shape, in the same process.  No existing kernel differs from the parent commit's, so the plain step here IS the
parent's.

    python scripts/matmap_probe.py [--rounds 5] [--steps 100] [--grids box,ellipsoid,head] [--out profiles/matmap_probe.json]

Shapes: the 512^3 all-solid box split into two layers (steel under copper), the 512^3 ellipsoid with a shell of a second
material, and the 256 x 256 x 320 synthetic head on a base plate of a second material.  dx = 0.2 mm, theta = 0.5, dt at cfl 0.5 of
steel, h = 15 W/m^2/K.  Every shape runs in a fresh child process; inside it the forms are timed round-robin with device events,
`rounds` samples of `steps` steps each (30 ms to 0.6 s per sample), medians reported:
  plain     StagedStepper.run with the first material everywhere (fused FAST kernels)
  general   the plain step forced onto its GENERAL dense kernels: explicit stage + three sweeps, variant GENERAL, dense reads
  matmap    StagedStepper.run with material_map=
There is no pass bar.  The byte estimate: MaterialMap.bytes_per_cell next to the plain stepper's stage_bytes_per_cell."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEEL, COPPER = (7800.0, 490.0, 54.0), (8900.0, 385.0, 390.0)


def make_case(name, waam):
    if name == 'box':
        shape = (512, 512, 512)
        mask = np.ones(shape, dtype=bool)
        ids = np.zeros(shape, np.uint8)
        ids[:, :, 256:] = 1
    elif name == 'ellipsoid':
        shape = (512, 512, 512)
        g = np.meshgrid(*[((np.arange(n) + 0.5) / n - 0.5).astype(np.float32) for n in shape], indexing='ij', sparse=True)
        r2 = (g[0] / 0.47) ** 2 + (g[1] / 0.49) ** 2 + (g[2] / 0.48) ** 2
        mask = r2 <= 1.0
        ids = (r2 > 0.8 ** 2).astype(np.uint8)
    elif name == 'head':
        shape = (256, 256, 320)
        mask = waam.synthetic_head_mask(*shape)
        ids = np.zeros(shape, np.uint8)
        ids[:, :, :48] = 1                                 # the base plate
    else:
        raise ValueError(name)
    i = np.arange(shape[0], dtype=np.float64)[:, None, None]
    k = np.arange(shape[2], dtype=np.float64)[None, None, :]
    return shape, mask, ids, np.broadcast_to(660.0 + 640.0 * np.sin(0.02 * i) * np.cos(0.015 * k), shape)


def child(a):
    import torch
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from adi_thermal_fields_amd import waam, _lib
    shape, mask, ids, T0 = make_case(a.grid, waam)
    dx, Tinf = 2e-4, 25.0
    rho, cp, k = STEEL
    dt = 0.5 * dx * dx * rho * cp / k
    g = hip.Grid3D(*shape, dx, mask)
    mat, prm = hip.Material(*STEEL), hip.Params(dt, 0.5)
    packs = hip.precompute_coeff_packs_unified(g, mat, robin_h=15.0)
    T = hip.to_device(T0)
    st_plain = hip.StagedStepper(g, mat, prm, packs, Tinf)
    mm = hip.MaterialMap(g, (STEEL, COPPER), ids, robin_h=15.0)
    st_map = hip.StagedStepper(g, mm.mat, prm, mm.packs, Tinf, material_map=mm)
    (ta, tb), _, _ = g.scratch(2)
    X = g.layout.to_layout(T, torch.float64)          # the state itself, read only (a clone() would drop the padded plane pitch)
    assert g.layout.is_native(X)

    def general():
        cur = X
        for _ in range(a.steps):
            hip.check(hip.lib.adi_explicit_rhs(hip._p(cur), hip._p(g.d_flags), *g.layout.pd, g.dx, prm.dt, k / (rho * cp), prm.theta,
                                               hip._p(ta), hip._stream()))
            st_plain.sweep_into(0, ta, tb, variant=_lib.SWEEP_GENERAL, dense=True)
            st_plain.sweep_into(1, tb, ta, variant=_lib.SWEEP_GENERAL, dense=True)
            st_plain.sweep_into(2, ta, tb, variant=_lib.SWEEP_GENERAL, dense=True)
            cur = tb
    forms = {'plain': lambda: st_plain.run(T, a.steps), 'general': general, 'matmap': lambda: st_map.run(T, a.steps)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps
    for n, fn in forms.items():                         # warm-up: graphs captured, modules loaded, allocator filled
        timed(fn)
        print('%s %s: warm-up %.3f ms per step' % (a.grid, n, timed(fn)), file=sys.stderr, flush=True)
    ms = {n: [] for n in forms}
    for _ in range(a.rounds):
        for n, fn in forms.items():
            ms[n].append(timed(fn))
    info = dict(grid=a.grid, shape=shape, physical=g.layout.pd, steps=a.steps, rounds=a.rounds, ms_per_step=ms,
                plain_bytes_per_cell=float(sum(st_plain.stage_bytes_per_cell)), matmap_bytes_per_cell=mm.bytes_per_cell,
                matmap_stage_bytes_per_cell=st_map.stage_bytes_per_cell, captures=[st_plain.captures, st_map.captures])
    print('MATMAP_PROBE ' + json.dumps(info), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
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
            raise SystemExit('matmap_probe: %s failed with status %d' % (grid, p.returncode))
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('MATMAP_PROBE ')][-1]
        r = json.loads(line[len('MATMAP_PROBE '):])
        med = {n: float(np.median(v)) for n, v in r['ms_per_step'].items()}
        r.update(ms_plain=med['plain'], ms_general=med['general'], ms_matmap=med['matmap'],
                 matmap_over_plain=med['matmap'] / med['plain'], matmap_over_general=med['matmap'] / med['general'],
                 byte_estimate_ratio=r['matmap_bytes_per_cell'] / r['plain_bytes_per_cell'])
        summary.append(r)
        print(grid, {n: round(v, 4) for n, v in med.items()}, file=sys.stderr, flush=True)
    out = dict(note='ms per step, medians over `rounds` samples of `steps` steps in one process per shape; plain and matmap are '
                    'graph-replayed StagedStepper.run (incl. one copy in and out), general the plain step forced onto its GENERAL '
                    'dense kernels; byte_estimate_ratio: MaterialMap.bytes_per_cell over the plain stepper\'s bytes per cell',
               summary=summary)
    print(json.dumps(dict(summary=[{k: v for k, v in r.items() if k != 'ms_per_step'} for r in summary])))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
