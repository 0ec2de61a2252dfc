"""Cost of heating the several-materials step from a ScanPath without a source field, on one GPU.

    python scripts/matmap_path_probe.py [--steps 100] [--samples 5] [--shapes head,512] [--out profiles/matmap_path_probe.json]

512: the 512^3 two-layer box of scripts/matmap_deposit_probe.py, a raster of 100-cell legs on its top face.  head: the 256 x 256
x 320 synthetic head on a copper plate (below plane 40) cut at plane 164, the raster of scripts/path_deposit_probe.py on that
plane.  Two windows each: `leg`, a step inside one leg, and `raster5`, a step from the middle of one leg to the middle of the
next but one -- five segments of the table, three of them powered.  ms per step by device events around `steps` plain launches
of adi_step_numba_coeff (no graph anywhere), the median of `samples` samples after one warm-up sample:
    a  the map step without a source
    b  the field form: ScanPathSource.sample_step_device + the step with S= the field -- the only route before, the yardstick
    c  S=MapPathSource
Every shape runs in a fresh child process under its own time limit; a child that fails ends the probe.  There is no pass bar;
the expectations stated in advance: c < b on both shapes and both windows, and c - a of the order of the
kernel's bytes and arithmetic: 17 B per in-mask cell of the box, up to four erf and one exp per cell and overlapped segment."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEEL = (7800.0, 490.0, 54.0)
COPPER = (8900.0, 385.0, 390.0)
TAG = 'MATMAP_PATH_PROBE '


def windows_of(path, dt_leg):
    """{'leg': (t, dt), 'raster5': (t, dt)} from the raster's table: legs are the even segments, jumps the odd ones"""
    tab = path.table()
    mid = lambda k: 0.5 * (tab[k, 0] + tab[k + 1, 0])      # noqa: E731
    assert tab.shape[0] >= 9 and tab[4, 7] > 0.0 and tab[5, 7] == 0.0
    t5 = mid(4)
    return dict(leg=(mid(4) - 0.5 * dt_leg, dt_leg), raster5=(t5, mid(8) - t5))


def measure(hip, torch, g, mm, path, wins, a):
    Tinf = 20.0
    src = path.on_device()
    msrc = hip.MapPathSource(mm, src)
    T0 = hip.to_device(np.full(g.shape, 300.0))
    N = a.steps
    out = {}
    for wname, (t, dt) in wins.items():
        prm = hip.Params(dt, 0.5)
        k0, k1, box = msrc.window(t, dt)
        assert k1 - k0 == (1 if wname == 'leg' else 5), (wname, k0, k1)

        def run(step):
            T = T0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(N):
                T = step(T)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / N
        kw = dict(Tinf=Tinf, material_map=mm)
        routes = dict(
            a_map_step_ms=lambda T: hip.adi_step_numba_coeff(T, g, mm.mat, prm, mm.packs, **kw),
            b_field_form_step_ms=lambda T: hip.adi_step_numba_coeff(T, g, mm.mat, prm, mm.packs, S=src.sample_step_device(g, t, dt),
                                                                    **kw),
            c_map_path_source_step_ms=lambda T: hip.adi_step_numba_coeff(T, g, mm.mat, prm, mm.packs, S=msrc, t=t, **kw))
        r = {}
        for name, step in routes.items():
            run(step)                                      # warm-up: module loads, allocator, the promise ledger
            s = [run(step) for _ in range(a.samples)]
            r[name], r[name[0] + '_samples'] = float(np.median(s)), s
            print('%s %s %s %.3f ms' % (g.shape, wname, name, r[name]), file=sys.stderr, flush=True)
        cells = int(np.prod([hi - lo for lo, hi in box]))
        sl = tuple(slice(lo, hi) for lo, hi in box)
        in_mask = int(np.asarray(g.mask)[sl].sum())
        q = np.asarray(src.sample_step_device(g, t, dt))
        r.update(t=t, dt=dt, segments=[k0, k1], box=[list(b) for b in box], box_cells=cells, box_in_mask_cells=in_mask,
                 heated_cells=int((q > 0).sum()), kernel_bytes_per_step=17 * in_mask,
                 c_minus_a_ms=r['c_map_path_source_step_ms'] - r['a_map_step_ms'],
                 c_over_a=r['c_map_path_source_step_ms'] / r['a_map_step_ms'],
                 c_over_b=r['c_map_path_source_step_ms'] / r['b_field_form_step_ms'])
        out[wname] = r
    return out


def child_512(a):
    import torch
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    shape = (512, 512, 512)
    dx = 2e-4
    rho, cp, k = STEEL
    dt = 0.5 * dx * dx * rho * cp / k
    mask = np.ones(shape, bool)
    ids = np.zeros(shape, np.uint8)
    ids[:, :256, :] = 1                                    # the raster crosses the interface at j = 256
    g = hip.Grid3D(*shape, dx, mask)
    mm = hip.MaterialMap(g, (STEEL, COPPER), ids, robin_h=40.0)
    path = hip.ScanPath.raster((206 * dx, 206 * dx), (306 * dx, 306 * dx), 10 * dx, 10 * dx / dt, 2000.0, depth=512 * dx, eta=0.8,
                               a=3 * dx, b=3 * dx, c_f=3 * dx, c_r=6 * dx)
    res = dict(shape=list(shape), steps=a.steps, samples=a.samples, device=torch.cuda.get_device_name(0))
    res.update(measure(hip, torch, g, mm, path, windows_of(path, dt), a))
    print(TAG + json.dumps(res), flush=True)


def child_head(a):
    import torch
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from adi_thermal_fields_amd import waam
    shape = (256, 256, 320)
    dx, ks, ke = 1e-3, 160, 164
    full = waam.synthetic_head_mask(*shape)
    sec = np.argwhere(full[:, :, ks:ke].any(axis=2))
    lo, hi = sec.min(axis=0), sec.max(axis=0) + 1
    mask = full.copy()
    mask[:, :, ke:] = False                                # the layer being heated is the top one
    ids = np.zeros(shape, np.uint8)
    ids[:, :, :40] = 1                                     # the base plate: copper
    g = hip.Grid3D(*shape, dx, mask)
    mm = hip.MaterialMap(g, (STEEL, COPPER), ids, robin_h=40.0)
    path = hip.ScanPath.raster((lo[0] * dx, lo[1] * dx), (hi[0] * dx, hi[1] * dx), 4e-3, 0.02, 800.0, depth=(ke - 0.3) * dx,
                               eta=0.8, a=2e-3, b=2e-3, c_f=2e-3, c_r=4e-3)
    res = dict(shape=list(shape), steps=a.steps, samples=a.samples, device=torch.cuda.get_device_name(0))
    res.update(measure(hip, torch, g, mm, path, windows_of(path, 0.25), a))
    print(TAG + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--samples', type=int, default=5)
    ap.add_argument('--shapes', default='head,512')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'matmap_path_probe.json'))
    ap.add_argument('--timeout', type=float, default=300.0, help='seconds a child process may take')
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.child:
        return dict(head=child_head, **{'512': child_512})[a.child](a)
    out = dict(note='ms per step by device events, medians of `samples` samples of `steps` plain launches of the step after one '
                    'warm-up sample; one process per shape; a: no source, b: sample_step_device + S=field, c: S=MapPathSource')
    for shape in a.shapes.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--child', shape, '--steps', str(a.steps), '--samples', str(a.samples)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
        if p.returncode != 0:                              # a child that failed ends the probe: nothing more is started
            sys.stderr.write(p.stdout[-2000:])
            raise SystemExit('matmap_path_probe: %s failed with status %d' % (shape, p.returncode))
        out[shape] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith(TAG)][-1][len(TAG):])
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
