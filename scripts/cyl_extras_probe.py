"""Cost of latent heat and thermal history on the cylindrical loop, alternated in one process with device
events.

    python scripts/cyl_extras_probe.py [--samples 5] [--steps 200] [--out profiles/cyl_extras_probe.json]
                                       [--parent-lines FILE ...] [--head-lines FILE ...]

BASELINE configs[3]: 128 x 256 x 512 cells, dr = dz = 0.25 mm, steel, dt = 0.05 s, Robin on the outer wall and the top; the
graph-replayed StagedCylStepper.run, medians of `samples` runs of `steps` steps, round-robin so that drift hits every case alike:
  a  plain          neither keyword (the in-place loop of bench.py --config cyl; its plain-launch form is timed too, as bench.py
                    times it, so that (a) can be held against that benchmark's figure for the parent commit)
  b  phase_cold     phase= on a field that is cold everywhere: every cell at rest, nothing stored
  c  phase_mushy    phase= with 5 % of the cells between solidus and liquidus
  d  history_cold   history= on a cold field: two persistent fields instead of one, no cell above T_lo
  e  history_hot    history= with 5 % of the cells above T_lo
  f  both_hot       both keywords on the field of (c) and (e)
Expectation by bytes, stated before the measurement and not a pass bar: a step moves 48 B/cell, each pass reads 1 + 8 + 8 = 17
more, so about +35 % for (b) and for (d); (d) also pays for the second field (0.133 -> 0.150 ms on its own).
The check of (a) against the parent commit: --parent-lines are result lines of the PARENT commit's `bench.py --config cyl --gpus 1
--steps 200 --warmup 20`, --head-lines the same of this commit, all taken in the same session on the same GPU.  The JSON records
both sets in ms per step, each set's scatter (max - min over its median), the ratio of the medians, and `agrees`: the medians
differ by no more than the two scatters together.  Without the files the check is recorded as not measured."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import adi_thermal_fields_amd.adi3d_hip_cyl as cyl  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=5)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--out', default=None)
    ap.add_argument('--parent-lines', nargs='*', default=[])
    ap.add_argument('--head-lines', nargs='*', default=[])
    a = ap.parse_args()
    nr, nphi, nz = 128, 256, 512
    g = cyl.GridCyl(nr, nphi, nz, 2.5e-4, 2 * np.pi / nphi, 2.5e-4, 0.032)
    mat, prm = cyl.Material(7800.0, 490.0, 54.0), cyl.Params(0.05, 1.0, "be")
    rr, zbc = cyl.RobinR(400.0, 20.0), cyl.ZBC('neumann0', 'robin', h_top=500.0, T_inf_top=20.0)
    law, levels = cyl.PhaseChange(2.7e5, 1400.0, 1450.0), cyl.HistoryLevels(800.0, 500.0, 1450.0)
    cold = np.full((nr, nphi, nz), 20.0)
    hot = cold.copy()
    hot[:, :, -26:] = 1425.0                            # 5 % of the cells (the top 26 planes): mushy, and above T_lo
    Tc, Th = cyl.to_device(cold), cyl.to_device(hot)
    cap = a.steps * (a.samples + 2)

    def stepper(T, phase, history):
        ph = cyl.CylPhaseField(g, mat, law, T=T) if phase else None
        hi = cyl.CylThermalHistory(g, levels, capacity=cap, T=T) if history else None
        return cyl.StagedCylStepper(g, mat, prm, rr, zbc, phase=ph, history=hi), ph, hi

    cases = dict(a_plain=(Tc, False, False), b_phase_cold=(Tc, True, False), c_phase_mushy=(Th, True, False),
                 d_history_cold=(Tc, False, True), e_history_hot=(Th, False, True), f_both_hot=(Th, True, True))
    built = {k: (v[0],) + stepper(*v) for k, v in cases.items()}

    def prepare(name):
        """every sample starts from the same state; outside the timed region"""
        if name not in built:
            return
        T, st, ph, hi = built[name]
        if ph is not None:
            ph.seed(T)
        if hi is not None:
            hi.reset(T)

    def run(name):
        T, st, ph, hi = built[name]
        return st.run(T, a.steps)

    def plain_launches():
        st = built['a_plain'][1]
        X = g.layout.empty()
        X.copy_(Tc.t)
        for _ in range(a.steps):
            st._step_inplace(X)

    forms = {k: (lambda k=k: run(k)) for k in cases}
    forms['a_plain_launches'] = plain_launches
    for name, f in forms.items():                       # warm-up: graphs captured, modules loaded
        prepare(name)
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(a.samples):
        for name, f in forms.items():
            prepare(name)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.steps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    base = med['a_plain']
    f_end = built['c_phase_mushy'][2].liquid_fraction.t
    res = dict(shape=[nr, nphi, nz], steps=a.steps, samples=a.samples, ms_per_step_median=med, ms_per_step_all=ms,
               ratio_to_plain={k: med[k] / base for k in med},
               expected_by_bytes=dict(b_phase_cold=1.0 + 17.0 / 48.0, d_history_cold=1.0 + 17.0 / 48.0),
               mushy_cells_after_c=int(((f_end > 0) & (f_end < 1)).sum().item()),
               pool_rows_e=int(built['e_history_hot'][3].slot),
               scatter={k: (max(v) - min(v)) / med[k] for k, v in ms.items()},
               parent_check=parent_check(a.parent_lines, a.head_lines),
               note='graph-replayed runs of %d steps (incl. one copy in and out; f and the history are reseeded before each '
                    'sample, outside the timed region), alternated; a_plain_launches: the same steps as plain launches'
                    % a.steps)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


def parent_check(parent_files, head_files):
    """case (a) against the parent commit's bench.py --config cyl loop: see the module docstring"""
    def ms_of(files):
        out = []
        for f in files:
            with open(f) as fh:
                line = json.loads(fh.read().strip().splitlines()[-1])
            out.append(1e3 * line['n_gpus'] / line['value'])          # value: steps/s over all GPUs
        return out
    if not parent_files or not head_files:
        return dict(status='not measured')
    par, head = ms_of(parent_files), ms_of(head_files)
    mp, mh = float(np.median(par)), float(np.median(head))
    sp, sh = (max(par) - min(par)) / mp, (max(head) - min(head)) / mh
    return dict(status='measured', loop='bench.py --config cyl --gpus 1 (200 steps, plain launches, in place)',
                parent_ms_per_step=par, head_ms_per_step=head, parent_median=mp, head_median=mh, parent_scatter=sp,
                head_scatter=sh, ratio_head_to_parent=mh / mp, agrees=bool(abs(mh / mp - 1.0) <= sp + sh))


if __name__ == '__main__':
    main()
