"""cost of a deposit call along a scan path (PathDeposit.deposit) on one GPU: the synthetic head box 256 x 256 x 320, a raster
layer of 4 planes laid on the part below it, theta = 1, one ADI step per path step.  Per step, host clock around N steps that
end in a device synchronise:
    (a)  deposit + flags / bricks / pack rebuild on the returned planes + the step
    (a2) the same with a PhaseField seeded after every deposit (sync_mask)
    (b)  the same step on a frozen mask
    (c)  birth_planes + the same rebuilds on the same plane range + the step, as in run_layer_birth: the yardstick
    (d)  deposit + rebuilds alone, no step
    python scripts/path_deposit_probe.py [--steps N] [--out profiles/path_deposit_probe.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import adi_thermal_fields_amd.adi3d_hip_coeff as hip  # noqa: E402
from adi_thermal_fields_amd import waam  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=40)
ap.add_argument('--warmup', type=int, default=4)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'path_deposit_probe.json'))
args = ap.parse_args()
assert torch.cuda.is_available(), 'path_deposit_probe needs a GPU'

shape = (256, 256, 320)
dx, dt, Tinf, Ts = 1e-3, 0.25, 20.0, 1500.0
STEEL = (7800.0, 490.0, 54.0)
ks, ke = 160, 164                                     # the layer: planes [ks, ke)
full = waam.synthetic_head_mask(*shape)
base = full.copy()
base[:, :, ks:] = False
sec = np.argwhere(full[:, :, ks:ke].any(axis=2))
lo, hi = sec.min(axis=0), sec.max(axis=0) + 1
path = hip.ScanPath.raster((lo[0] * dx, lo[1] * dx), (hi[0] * dx, hi[1] * dx), 4e-3, 0.02, 800.0, depth=(ke - 0.3) * dx,
                           eta=0.8, a=2e-3, b=2e-3, c_f=2e-3, c_r=4e-3)
bead = hip.BeadProfile(4e-3, (ke - ks - 0.4) * dx, 'box')
N, W = args.steps, args.warmup
t_probe = path.t_start + 0.4 * (path.t_end - path.t_start)      # the middle tracks: whole beads inside the section
assert path.t_end - t_probe > (4 * (N + W)) * dt, 'the raster is too short for the probe'
robin = {f: 40.0 for f in ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')}


def setup(phase=False):
    grid = hip.Grid3D(*shape, dx, base)
    mat, prm = hip.Material(*STEEL), hip.Params(dt=dt, theta=1.0)
    T = hip.to_device(np.full(shape, Tinf))
    dep = hip.PathDeposit(grid, path, bead, Ts, within=full)
    bp = hip.BirthPacks(grid, mat, robin_h=robin)
    ph = hip.PhaseField(grid, mat, hip.PhaseChange(2.7e5, 1400.0, 1450.0), T=T) if phase else None
    return grid, mat, prm, T, dep, bp, ph


def timed(fn, n0):
    """ms per call of fn(n) over n = n0 + W .. n0 + W + N - 1 after W warm-up calls"""
    for n in range(n0, n0 + W):
        fn(n)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for n in range(n0 + W, n0 + W + N):
        fn(n)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / N


res = dict(shape=list(shape), layer_planes=[ks, ke], steps=N, warmup=W, dt=dt, device=torch.cuda.get_device_name(0))
for key, phase in (('a_deposit_rebuild_step_ms', False), ('a2_with_phase_sync_ms', True)):
    grid, mat, prm, T, dep, bp, ph = setup(phase)
    kw = {} if ph is None else dict(phase=ph)
    state = dict(T=T)

    def step_a(n):
        rng = dep.deposit(state['T'], t_probe + n * dt, dt)
        if rng is not None:
            bp.update(*rng)
            if ph is not None:
                ph.sync_mask(state['T'])
        state['T'] = hip.adi_step_numba_coeff(state['T'], grid, mat, prm, bp.packs, Tinf=Tinf, **kw)
    res[key] = timed(step_a, 0)
    if not phase:
        box = dep.index_box(t_probe + W * dt, dt)
        res['launch_box_cells'] = int(np.prod([b - a for a, b in box]))
        k_lo, k_hi = max(0, box[2][0] - 1), min(shape[2], box[2][1] + 1)    # what deposit returns: the planes (c) rebuilds too
        res['rebuilt_planes'] = [k_lo, k_hi]
        # (b) the mask as (a) left it, frozen
        res['b_frozen_mask_step_ms'] = timed(lambda n: state.update(T=hip.adi_step_numba_coeff(state['T'], grid, mat, prm, bp.packs, Tinf=Tinf)), 0)
        # (d) the deposit and its rebuilds alone, further along the path
        res['d_deposit_rebuild_only_ms'] = timed(lambda n: bp.update(*(dep.deposit(state['T'], t_probe + n * dt, dt) or (0, 0))), N + W)
        res['cells_born_in_probe'] = int(grid.d_mask.sum().item()) - int(base.sum())
    del grid, T, dep, bp, ph, state

# (c) birth_planes on the same planes + the rebuilds of run_layer_birth + the step
grid, mat, prm, T, dep, bp, _ = setup()
d_full = grid.layout.to_layout(full, torch.uint8)
d_act = grid.d_mask
state = dict(T=T)


def step_c(n):
    hip.birth_planes(state['T'], d_act, d_full, grid, ks, ke, Ts)
    grid.set_mask_device(d_act, k_lo, k_hi, all_solid=False)
    bp.update(k_lo, k_hi)
    state['T'] = hip.adi_step_numba_coeff(state['T'], grid, mat, prm, bp.packs, Tinf=Tinf)


res['c_birth_planes_rebuild_step_ms'] = timed(step_c, 0)
print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'w') as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write('\n')
