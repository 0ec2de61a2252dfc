"""Cost of the temperature-dependent surface loss, alternated in one process with device events.

    python scripts/surface_loss_probe.py [--rounds 6] [--steps 20] [--grids box,ellipsoid,head] [--out profiles/surface_loss_probe.json]

Three grids: the 512^3 all-solid box, the 512^3 ellipsoid and the 256 x 256 x 320 synthetic head.  Steel, dx = 0.2 mm,
dt = dx^2 / (2 kappa), theta = 0.5, h = 15 W/m^2/K + emissivity 0.8, field between 20 and 1500 degrees.  Timed per grid,
round-robin so that drift hits every form alike:
  frozen   StagedStepper.run on the LossPacks' packs without the update (coefficients as the last rebuild left them): the
           reference point -- the same per-voxel packs, the same build, the same process
  loss     the same stepper with surface_loss= (adi_surface_loss_update ahead of every step), replayed from the graph
  update   adi_surface_loss_update alone (LossPacks.update), `steps` launches per sample
  torch    the route it replaces: six h fields by torch arithmetic + precompute_coeff_packs_unified(robin_h=fields), per step
           (no step included)
There is no pass bar.  The expectation is byte-derived: the update reads the flags summary, the flags bytes of the bricks that hold
a surface (at most 1 B/cell) and T on exposed cells, and writes 8 B per exposed (cell, axis); the step moves the bytes of
StagedStepper.stage_bytes_per_cell."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import adi_thermal_fields_amd.adi3d_hip_coeff as hip  # noqa: E402
from adi_thermal_fields_amd import waam  # noqa: E402

FACES = ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')
RHO, CP, K = 7800.0, 490.0, 54.0


def make_grid(name):
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
    return shape, mask


def torch_law(T, h, eps, Tinf, off=273.15):
    Tk = T + off
    Ta = Tinf + off
    return (h + 0.0) + ((eps * hip.SurfaceLoss.SIGMA) * (Tk * Tk + Ta * Ta)) * (Tk + Ta)


def timed(fn, per):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / per


def probe(name, a):
    shape, mask = make_grid(name)
    dx = 2e-4
    dt = 0.5 * dx * dx / (K / (RHO * CP))
    Tinf = 25.0
    g = hip.Grid3D(*shape, dx, mask)
    mat, prm = hip.Material(RHO, CP, K), hip.Params(dt, 0.5)
    loss = hip.SurfaceLoss(h=15.0, emissivity=0.8)
    i = np.arange(shape[0], dtype=np.float64)[:, None, None]
    k = np.arange(shape[2], dtype=np.float64)[None, None, :]
    T = hip.to_device(np.broadcast_to(760.0 + 700.0 * np.sin(0.02 * i) * np.cos(0.015 * k), shape))
    lp = hip.LossPacks(g, mat, loss, Tinf, T=T)
    st_frozen = hip.StagedStepper(g, mat, prm, lp.packs, Tinf)
    st_loss = hip.StagedStepper(g, mat, prm, lp.packs, Tinf, surface_loss=lp)

    def update():
        for _ in range(a.steps):
            lp.update(T)

    def torch_route():
        h = {f: hip.DeviceField(torch_law(T.t, 15.0, 0.8, Tinf)) for f in FACES}
        return hip.precompute_coeff_packs_unified(g, mat, robin_h=h)
    forms = dict(frozen=(lambda: st_frozen.run(T, a.steps), a.steps), loss=(lambda: st_loss.run(T, a.steps), a.steps),
                 update=(update, a.steps), torch=(torch_route, 1))
    for f, _ in forms.values():                      # warm-up: graphs captured, modules loaded, allocator filled
        f()
    torch.cuda.synchronize()
    ms = {n: [] for n in forms}
    for _ in range(a.rounds):
        for n, (f, per) in forms.items():
            ms[n].append(timed(f, per))
    med = {n: float(np.median(v)) for n, v in ms.items()}
    mn = {n: float(np.min(v)) for n, v in ms.items()}
    ncell = float(np.prod(shape))
    exposed = [p.exposed_fraction for p in lp.packs]
    any_exposed = float(((g.d_flags & 1) == 1).logical_and((g.d_flags & 0x7e) != 0x7e).sum().item()) / ncell
    step_bytes = float(sum(st_frozen.stage_bytes_per_cell))
    upd_bytes = 1.0 + 8.0 * any_exposed + 8.0 * sum(exposed)
    res = dict(grid=name, shape=shape, physical=g.layout.pd, steps=a.steps, rounds=a.rounds, ms_median=med, ms_min=mn, ms_all=ms,
               overhead_ms_median=med['loss'] - med['frozen'], overhead_fraction_median=(med['loss'] - med['frozen']) / med['frozen'],
               overhead_fraction_min=(mn['loss'] - mn['frozen']) / mn['frozen'],
               exposed_fraction_per_axis=exposed, cells_with_an_exposed_face=any_exposed,
               step_bytes_per_cell=step_bytes, update_bytes_per_cell_upper=upd_bytes,
               byte_estimate_fraction=upd_bytes / step_bytes, torch_route_over_update=med['torch'] / med['update'])
    del st_frozen, st_loss, lp, T, g
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--grids', default='box,ellipsoid,head')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    out = dict(note='frozen / loss: graph-replayed runs of `steps` steps (incl. one copy in and out), ms per step; update: ms per '
                    'launch; torch: ms per rebuild of the packs from six torch-made h fields.  update_bytes_per_cell_upper counts '
                    '1 B/cell of flags (an upper bound: bricks without a surface are skipped), T on cells with an exposed face '
                    'and one store per exposed (cell, axis)',
               results=[])
    for n in a.grids.split(','):
        out['results'].append(probe(n, a))
        print(n, 'done', file=sys.stderr, flush=True)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
