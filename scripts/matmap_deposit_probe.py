"""Cost of carrying a MaterialMap through deposits and a moving source, on one GPU.

    python scripts/matmap_deposit_probe.py [--steps 200] [--samples 5] [--shapes head,512] [--out profiles/matmap_deposit_probe.json]

head: the 256 x 256 x 320 synthetic head on a base plate of another material (copper below plane 40), the raster layer of
scripts/path_deposit_probe.py laid on the part below it, theta = 1, one ADI step per path step.  ms per step, host clock around
`steps` steps that end in a device synchronise, the median of `samples` samples:
    a  the map step on the frozen mask
    b  deposit (ids stamped) + MaterialMap.update on the returned planes + the step
    c  deposit (ids stamped) + MaterialMap.rebuild() in full + the step: the only route before update existed, the yardstick
    d  the one-material figures of profiles/path_deposit_probe.json, copied beside them for comparison (not measured here)
and, with device events around StagedStepper.run (graph replay):
    e  the map step without a source
    f  the same with a MapSource
    g  the field form: GoldakSource.sample_device + one adi_step_numba_coeff(S=field) per call
512: e, f and g on a 512^3 two-layer box.  Every shape runs in a fresh child process under its own time limit; a child that
fails ends the probe.  There is no pass bar; the expectation stated in advance is b <= c and f <= g.
Bytes: update touches 6 x 8 B + the mask per cell of the range only; the source kernel 17 B per in-mask cell of the support."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEEL = (7800.0, 490.0, 54.0)
COPPER = (8900.0, 385.0, 390.0)
TAG = 'MATMAP_DEPOSIT_PROBE '


def _median_of(fn, samples):
    return float(np.median([fn() for _ in range(samples)]))


def child_head(a):
    import torch
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from adi_thermal_fields_amd import waam
    shape = (256, 256, 320)
    dx, dt, Tinf, Ts = 1e-3, 0.25, 20.0, 1500.0
    ks, ke = 160, 164
    full = waam.synthetic_head_mask(*shape)
    base = full.copy()
    base[:, :, ks:] = False
    sec = np.argwhere(full[:, :, ks:ke].any(axis=2))
    lo, hi = sec.min(axis=0), sec.max(axis=0) + 1
    path = hip.ScanPath.raster((lo[0] * dx, lo[1] * dx), (hi[0] * dx, hi[1] * dx), 4e-3, 0.02, 800.0, depth=(ke - 0.3) * dx,
                               eta=0.8, a=2e-3, b=2e-3, c_f=2e-3, c_r=4e-3)
    bead = hip.BeadProfile(4e-3, (ke - ks - 0.4) * dx, 'box')
    N, W = a.steps, 4
    t_probe = path.t_start + 0.2 * (path.t_end - path.t_start)
    robin = {f: 40.0 for f in ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')}
    ids = np.zeros(shape, np.uint8)
    ids[:, :, :40] = 1                                     # the base plate: copper
    res = dict(shape=list(shape), steps=N, samples=a.samples, dt=dt, device=torch.cuda.get_device_name(0))

    def setup():
        grid = hip.Grid3D(*shape, dx, base)
        mm = hip.MaterialMap(grid, (STEEL, COPPER), ids, robin_h=robin)
        T = hip.to_device(np.full(shape, Tinf))
        dep = hip.PathDeposit(grid, path, bead, Ts, within=full, material_map=mm, material_id=0)
        return grid, mm, hip.Params(dt=dt, theta=1.0), dep, dict(T=T)

    def loop(fn, n0):
        for n in range(n0, n0 + W):
            fn(n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for n in range(n0 + W, n0 + W + N):
            fn(n)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / N

    def sample(refresh):
        """one sample of N deposits from t_probe on a fresh grid (every sample lays the same beads)"""
        grid, mm, prm, dep, st = setup()

        def step(n):
            rng = dep.deposit(st['T'], t_probe + n * dt, dt)
            if rng is not None:
                refresh(mm, rng)
            st['T'] = hip.adi_step_numba_coeff(st['T'], grid, mm.mat, prm, mm.packs, Tinf=Tinf, material_map=mm)
        ms = loop(step, 0)
        born = int(grid.d_mask.sum().item()) - int(base.sum())
        return ms, born, (grid, mm, prm, st)
    assert path.t_end - t_probe > (N + W + 1) * dt, 'the raster is too short for the probe'
    b, c, frozen = [], [], []
    for _ in range(a.samples):
        ms, born, (grid, mm, prm, st) = sample(lambda mm, rng: mm.update(*rng))
        b.append(ms)
        res['cells_born_per_sample'] = born
        frozen.append(loop(lambda n: st.update(T=hip.adi_step_numba_coeff(st['T'], grid, mm.mat, prm, mm.packs, Tinf=Tinf,
                                                                         material_map=mm)), 0))
        del grid, mm, st
        ms, born_c, keep = sample(lambda mm, rng: mm.rebuild())
        assert born_c == born
        c.append(ms)
        del keep
        print('head: b %.3f  c %.3f  a %.3f ms' % (b[-1], c[-1], frozen[-1]), file=sys.stderr, flush=True)
    res.update(a_frozen_mask_step_ms=float(np.median(frozen)), b_deposit_update_step_ms=float(np.median(b)),
               c_deposit_rebuild_step_ms=float(np.median(c)), b_samples=b, c_samples=c, a_samples=frozen)
    res.update(graph_forms(hip, torch, shape, dx, base | full, ids, a, src_origin=(0.5 * shape[0] * dx, 0.4 * shape[1] * dx, ke * dx)))
    print(TAG + json.dumps(res), flush=True)


def graph_forms(hip, torch, shape, dx, mask, ids, a, src_origin):
    """e, f, g on `mask`: ms per step by device events, the median of a.samples samples of a.steps steps"""
    Tinf = 20.0
    rho, cp, k = STEEL
    dt = 0.5 * dx * dx * rho * cp / k
    g = hip.Grid3D(*shape, dx, mask)
    mm = hip.MaterialMap(g, (STEEL, COPPER), ids, robin_h=40.0)
    prm = hip.Params(dt, 0.5)
    src = hip.GoldakSource(power=2000.0, eta=0.8, a=3 * dx, b=3 * dx, c_f=3 * dx, c_r=6 * dx, origin=src_origin,
                           velocity=2 * dx / dt / a.steps, travel_axis=1, depth_axis=2)
    T0 = hip.to_device(np.full(shape, 300.0))
    plain = hip.StagedStepper(g, mm.mat, prm, mm.packs, Tinf, material_map=mm)
    withsrc = hip.StagedStepper(g, mm.mat, prm, mm.packs, Tinf, material_map=mm, source=hip.MapSource(mm, src))
    N = a.steps

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / N

    def field_form():
        T = T0
        for i in range(N):
            S = src.sample_device(g, i * dt + 0.5 * dt)
            T = hip.adi_step_numba_coeff(T, g, mm.mat, prm, mm.packs, Tinf=Tinf, material_map=mm, S=S)
    forms = dict(e_graph_map_step_ms=lambda: plain.run(T0, N), f_graph_map_source_step_ms=lambda: withsrc.run(T0, N, t0=0.0),
                 g_field_form_step_ms=field_form)
    out = {}
    for name, fn in forms.items():
        events(fn)                                         # warm-up: capture, module loads, allocator
        out[name] = _median_of(lambda: events(fn), a.samples)
        print('%s %s %.3f ms' % (shape, name, out[name]), file=sys.stderr, flush=True)
    q = src.sample_device(g, 0.5 * dt)
    out['support_in_mask_cells'] = int((np.asarray(q) > 0).sum())
    out['source_bytes_per_step'] = 17 * out['support_in_mask_cells']
    out['captures'] = [plain.captures, withsrc.captures]
    return out


def child_512(a):
    import torch
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    shape = (512, 512, 512)
    dx = 2e-4
    mask = np.ones(shape, bool)
    ids = np.zeros(shape, np.uint8)
    ids[:, :256, :] = 1                                    # the source travels along axis 1 across the interface at j = 256
    res = dict(shape=list(shape), steps=a.steps, samples=a.samples, device=torch.cuda.get_device_name(0))
    res.update(graph_forms(hip, torch, shape, dx, mask, ids, a, src_origin=(256 * dx, 255 * dx, 512 * dx)))
    print(TAG + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--samples', type=int, default=5)
    ap.add_argument('--shapes', default='head,512')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'matmap_deposit_probe.json'))
    ap.add_argument('--timeout', type=float, default=420.0, help='seconds a child process may take')
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.child:
        return dict(head=child_head, **{'512': child_512})[a.child](a)
    out = dict(note='ms per step, medians of `samples` samples of `steps` steps; one process per shape; a-c host clock, e-g device '
                    'events (e, f: StagedStepper.run, graph replay)')
    for shape in a.shapes.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--child', shape, '--steps', str(a.steps), '--samples', str(a.samples)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
        if p.returncode != 0:                              # a child that failed ends the probe: nothing more is started
            sys.stderr.write(p.stdout[-2000:])
            raise SystemExit('matmap_deposit_probe: %s failed with status %d' % (shape, p.returncode))
        r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith(TAG)][-1][len(TAG):])
        r['f_over_e'] = r['f_graph_map_source_step_ms'] / r['e_graph_map_step_ms']
        r['f_over_g'] = r['f_graph_map_source_step_ms'] / r['g_field_form_step_ms']
        if shape == 'head':
            r['b_over_a'] = r['b_deposit_update_step_ms'] / r['a_frozen_mask_step_ms']
            r['b_over_c'] = r['b_deposit_update_step_ms'] / r['c_deposit_rebuild_step_ms']
            try:                                           # (d) the one-material figures, for comparison
                with open(os.path.join(ROOT, 'profiles', 'path_deposit_probe.json')) as f:
                    d = json.load(f)
                r['d_one_material'] = {k: d[k] for k in ('a_deposit_rebuild_step_ms', 'b_frozen_mask_step_ms') if k in d}
            except OSError:
                r['d_one_material'] = None
        out[shape] = r
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
