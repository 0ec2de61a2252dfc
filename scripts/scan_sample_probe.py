"""Cost of a scan path's source field at 512^3, evaluated on the device against built on the host ("Scan
path"), device events and wall clock in one process.

    python scripts/scan_sample_probe.py [--n 512] [--rounds 5] [--out profiles/scan_sample_probe.json]

The box of scripts/source_probe.py (all-solid, steel, Robin h = 500, dx = 0.2 mm, dt = dx^2 / (2 kappa)), the Goldak shape a = b =
c_f = 2 mm, c_r = 4 mm on the top surface.  Two paths: one leg (a step overlaps 1 segment) and a raster whose tracks last 0.4 steps
with jumps of 0.1 (about 5 segments per step).  Timed per path:
  device_sample_ms   ScanPathSource.sample_step_device (k_scan_sample), device events
  device_step_ms     adi_step_numba_coeff(S=<that DeviceField>) on a DeviceField, device events: the field form of the step
  host_sample_ms     ScanPath.sample_step (NumPy), wall clock
  host_step_ms       adi_step_numba_coeff(S=<NumPy array>) on a DeviceField, wall clock with the device synchronised: upload + step"""
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


def events(fn, rounds):
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n, dx = a.n, 2e-4
    rho, cp, k = 7800.0, 500.0, 30.0
    dt = 0.5 * dx * dx / (k / (rho * cp))
    g = hip.Grid3D(n, n, n, dx, np.ones((n, n, n), dtype=bool))
    mat, prm = hip.Material(rho, cp, k), hip.Params(dt, 0.5)
    packs = hip.precompute_coeff_packs_unified(g, mat, robin_h=500.0)
    shp = dict(eta=0.8, a=2e-3, b=2e-3, c_f=2e-3, c_r=4e-3, f_f=0.6)
    z, y0, y1 = n * dx, 0.25 * n * dx, 0.75 * n * dx
    leg = hip.ScanPath(power=2000.0, start=(0.5 * n * dx, y0, z), **shp).line_to((0.5 * n * dx, y1, z), (y1 - y0) / (20 * dt))
    wid, hatch = 0.4 * n * dx, (y1 - y0) / 40.0
    raster = hip.ScanPath.raster((0.3 * n * dx, y0), (0.7 * n * dx, y1), hatch, wid / (0.4 * dt), 2000.0,
                                 jump_speed=hatch / (0.1 * dt), depth=z, **shp)
    T = hip.to_device(np.full((n, n, n), 300.0))
    res = dict(n=n, dx=dx, dt=dt, rounds=a.rounds, paths={})
    for name, path in (('leg', leg), ('raster5', raster)):
        src, t = path.on_device(), 3.0 * dt
        tb = path.table()[:, 0]
        segs = int(np.sum(np.minimum(np.append(tb[1:], path.t_end), t + dt) > np.maximum(tb, t)))
        S = src.sample_step_device(g, t, dt)                  # warm-up
        hip.adi_step_numba_coeff(T, g, mat, prm, packs, 300.0, S=S)
        torch.cuda.synchronize()
        r = dict(segments=path.n_segments, segments_in_the_step=segs,
                 device_sample_ms=events(lambda: src.sample_step_device(g, t, dt), a.rounds),
                 device_step_ms=events(lambda: hip.adi_step_numba_coeff(T, g, mat, prm, packs, 300.0, S=S), a.rounds))
        t0 = time.perf_counter()
        q = path.sample_step(g, t, dt)
        t1 = time.perf_counter()
        hip.adi_step_numba_coeff(T, g, mat, prm, packs, 300.0, S=q)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        r.update(host_sample_ms=1e3 * (t1 - t0), host_step_ms=1e3 * (t2 - t1))
        err = float(np.max(np.abs(np.asarray(S) - q)) / q.max())
        r['device_vs_host_rel_linf'] = err
        res['paths'][name] = r
        print(name, json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
