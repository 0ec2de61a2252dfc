"""Shared by tests/test_history_cpu.py and tests/test_history_gpu.py: short multi-segment runs for the thermal-history recorder
over any module with the reference's operator surface (the pinned C oracle in the CPU tests, the HIP module in the GPU tests),
and the loop  B = step(A) -> state, pool = record_reference(state, A, B, mask, t_n, dt, levels)  that defines what the device
must record.

A case: a cold body (Robin on every face) with a hot blob that straddles the brick seam at index 16 of every axis that has one,
and a few single hot cells in the cold part.  Five segments with two values of dt; the third has a source field S that reheats
the part of the blob that has by then completed a cooling cycle.  The levels are T_hi = 800, T_lo = 500, T_melt = 1400.  The
conditions the inputs were chosen for (`conditions`; asserted on the C oracle in tests/test_history_cpu.py):
    at the end there is a cell that crossed T_hi only, one that completed a cycle, one that dropped through both levels in one
    step, and one that was reheated above T_hi after a completed cycle (its t_lo went back to NaN);
    the pool is non-empty and spans two bricks along every axis with more than one brick at some step, and is empty later.
"""
import numpy as np

FACES = ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')
RHO, CP, K = 7800.0, 490.0, 54.0
KAPPA = K / (RHO * CP)
DX, TINF, H, THETA = 1e-3, 25.0, 200.0, 0.5
LEVELS = (800.0, 500.0, 1400.0)
DT_A, DT_B = 0.5 * DX * DX / KAPPA, 3.0 * DX * DX / KAPPA
CASES = ('holes', 'solid')
SHAPES = {'holes': (20, 18, 35), 'solid': (32, 16, 32)}
PADDED = {'holes': (24, 20, 36)}          # the physical box of the padded variant of the GPU tests


def _blob(shape):
    """the hot blob: around index 16 of every axis that reaches past it, else the middle of the axis"""
    sl = []
    for n in shape:
        c = 16 if n > 17 else n // 2
        sl.append(slice(max(c - 5, 0), min(c + 4, n)))
    return tuple(sl)


_cases = {}


def case(name):
    """the inputs of a case, built once, never modified"""
    if name not in _cases:
        shape = SHAPES[name]
        rng = np.random.default_rng(11)
        mask = np.ones(shape, dtype=bool)
        blob = _blob(shape)
        if name == 'holes':
            mask = rng.random(shape) > 0.07
            mask[blob] = True
        T0 = np.full(shape, TINF)
        T0[blob] = 1900.0
        # single hot cells in the cold part, far from the blob: they drop through both levels in one step
        spikes = [(2, 2, 3), (3, shape[1] - 3, shape[2] - 4), (shape[0] - 3, 3, shape[2] - 6)]
        for p in spikes:
            mask[p] = True
            T0[p] = 1000.0
        T0 = np.where(mask, T0, TINF)
        # the source of the third segment: the low-i half of the blob, which has cooled below T_lo by then, back above T_hi
        S = np.zeros(shape)
        half = (slice(blob[0].start, blob[0].start + 4),) + blob[1:]
        S[half] = 1.4e10
        S = np.where(mask, S, 0.0)
        segs = [(DT_A, 6, None), (DT_B, 24, None), (DT_B, 4, S), (DT_A, 6, None), (DT_B, 1, None)]
        c = dict(name=name, shape=shape, mask=mask, T0=T0, segments=segs, blob=blob, spikes=spikes)
        for a in (mask, T0, S):
            a.setflags(write=False)
        _cases[name] = c
    return _cases[name]


def nsteps(c):
    return sum(n for _, n, _ in c['segments'])


def setup(mod, c):
    grid = mod.Grid3D(*c['shape'], DX, np.array(c['mask']))
    mat = mod.Material(RHO, CP, K)
    packs = mod.precompute_coeff_packs_unified(grid, mat, robin_h={f: H for f in FACES})
    return grid, mat, packs


def oracle_trajectory(orc, c):
    """[T0, T1, ...] of the case over the C oracle (whose step has no source argument: S enters through the flux term of the
    axis-0 pack, dt*S/(rho cp) on in-mask cells, as in tests/phase_cases.py)"""
    grid, mat, _ = setup(orc, c)
    T = np.array(c['T0'])
    traj = [T]
    for dt, n, S in c['segments']:
        prm = orc.Params(dt, THETA)
        packs = orc.precompute_coeff_packs_unified(grid, mat, robin_h={f: H for f in FACES})
        if S is not None:
            packs[0].qflux = packs[0].qflux + np.where(c['mask'], S, 0.0) / (RHO * CP)
        for _ in range(n):
            T = orc.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=TINF)
            traj.append(T)
    return traj


def empty_state(shape):
    return tuple(np.full(shape, np.nan) for _ in range(3))


def record_trajectory(hist_cls, levels, c, traj, t=0.0, clock='run', segments=None):
    """the definition over a stored trajectory: states[n], pools[n - 1] after step n, times[n - 1] its end time, and the clock
    at the end.  clock = 'run': as StagedStepper.run keeps it -- within a segment t_n = t0 + n*dt, and the next segment starts
    at t0 + nsteps*dt; clock = 'step': as single recorded steps keep it -- every step is a run of its own, t_n+1 = t_n + dt"""
    mask = c['mask']
    state = hist_cls.seed_reference(empty_state(c['shape']), traj[0], mask)
    states, pools, times = [state], [], []
    k = 0
    for dt, n, _ in (c['segments'] if segments is None else segments):
        t0 = t
        for i in range(n):
            t_n = t0 + i * dt if clock == 'run' else t
            state, pool = hist_cls.record_reference(state, traj[k], traj[k + 1], mask, t_n, dt, levels)
            states.append(state)
            pools.append(pool)
            t = t0 + (i + 1) * dt if clock == 'run' else t_n + dt
            times.append(t)
            k += 1
    return states, pools, times, t


def pool_rows(pools):
    """the log rows { cells, lo[3], hi[3], pad } the device writes for these pools"""
    return np.array([[p['cells'], *p['lo'], *p['hi'], 0] for p in pools], dtype=np.int32).reshape(len(pools), 8)


def conditions(c, traj, states, pools):
    """the kinds of cell and of pool the case was built for -> dict of counts / step numbers (0 / None: missing)"""
    T_hi, T_lo, _ = LEVELS
    mask = c['mask']
    peak, t_hi, t_lo = states[-1]
    hi_only = mask & ~np.isnan(t_hi) & np.isnan(t_lo)
    cycle = mask & ~np.isnan(t_hi) & ~np.isnan(t_lo)
    both = np.zeros(c['shape'], dtype=bool)
    reheated = np.zeros(c['shape'], dtype=bool)
    done = np.zeros(c['shape'], dtype=bool)          # a cycle was complete after some earlier step
    for n in range(1, len(traj)):
        A, B = traj[n - 1], traj[n]
        both |= mask & (A > T_hi) & (B <= T_lo)
        _, th, tl = states[n]
        reheated |= done & (B > T_hi)
        done |= mask & ~np.isnan(th) & ~np.isnan(tl)
    again = reheated & ~np.isnan(t_hi) & np.isnan(t_lo)
    nb = [(n + 15) // 16 for n in c['shape']]
    wide = [n for n, p in enumerate(pools, 1)
            if p['cells'] > 0 and all(b == 1 or (p['lo'][a] // 16 < p['hi'][a] // 16) for a, b in enumerate(nb))]
    empty_later = [n for n, p in enumerate(pools, 1) if p['cells'] == 0 and wide and n > wide[0]]
    return dict(hi_only=int(hi_only.sum()), cycle=int(cycle.sum()), both=int((both & cycle).sum()), reheated=int(again.sum()),
                pool_wide_step=wide[0] if wide else None, pool_empty_step=empty_later[0] if empty_later else None)
