"""Cost of the moving heat source on the slab decomposition ("slab decomposition"), alternated in one
process with device events.

    python scripts/slab_source_probe.py [--planes 512] [--n 512] [--rounds 5] [--steps 10] [--out profiles/slab_source_probe.json]

A middle rank (4 of 8) rehearsed on one GPU with dist_slab.LoopbackComm(8, 4): `planes` planes of n x n, all solid, steel,
Robin h = 500, dx = 0.2 mm, dt = dx^2 / (2 kappa); the Goldak source of source_probe.py (a = b = c_f = 2 mm, c_r = 4 mm) travelling
along axis 1.  Timed round-robin, ms per step:
  deferred / deferred+src_here / deferred+src_away   the deferred fused form; the support on this rank's planes or far from them
  window   / window+src_here   / window+src_away     the same slab with _allow_deferred = False (the source added to R0)
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (--rounds 1)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import adi_thermal_fields_amd.adi3d_hip_coeff as hip  # noqa: E402
from adi_thermal_fields_amd import dist_slab  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--planes', type=int, default=512)
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    nxl, n, dx = a.planes, a.n, 2e-4
    world, rank = 8, 4
    rho, cp, k = 7800.0, 500.0, 30.0
    dt = 0.5 * dx * dx / (k / (rho * cp))
    i_org = rank * nxl
    mat = hip.Material(rho, cp, k)

    def source(plane):
        return hip.GoldakSource(2000.0, 0.8, 2e-3, 2e-3, 2e-3, 4e-3, origin=((plane + 0.5) * dx, 0.3 * n * dx, n * dx),
                                velocity=0.01)
    steppers, forms = {}, {}
    for form, deferred in (('deferred', True), ('window', False)):
        st = dist_slab.SlabStepper(np.ones((nxl, n, n), dtype=bool), dx, mat, hip.Params(dt, 0.5), 300.0, robin_h=500.0,
                                   comm=dist_slab.LoopbackComm(world, rank))
        st._allow_deferred = deferred
        steppers[form] = st
        for tag, src in (('', None), ('+src_here', source(i_org + nxl // 2)), ('+src_away', source(100))):
            forms[form + tag] = (st, src)
    T0 = torch.full((nxl, n, n), 300.0, dtype=torch.float64, device=hip._device())

    def run(st, src):
        st.set_source(src)
        X = T0
        for i in range(a.steps):
            X = st.step(X, prefetch_halo=i + 1 < a.steps, t=None if src is None else i * dt)
        return X
    for st, src in forms.values():                   # warm-up: plans made, modules loaded
        run(st, src)
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    modes = {}
    for _ in range(a.rounds):
        for name, (st, src) in forms.items():
            run(st, src)                              # (re-plans when the source is attached / detached: not timed)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            X = T0
            e0.record()
            for i in range(a.steps):
                X = st.step(X, prefetch_halo=i + 1 < a.steps, t=None if src is None else i * dt)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.steps)
            modes[name] = st.axis0_mode
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = dict(planes=nxl, n=n, world=world, rank=rank, steps=a.steps, rounds=a.rounds, axis0_mode=modes,
               ms_per_step_median=med, ms_per_step_all=ms,
               source_cost_ms={f + t: med[f + t] - med[f] for f in steppers for t in ('+src_here', '+src_away')},
               note='middle rank of 8 rehearsed over LoopbackComm (no wire time); runs of %d steps, first step of each run '
                    'included' % a.steps)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
