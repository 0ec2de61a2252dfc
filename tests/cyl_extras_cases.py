"""Cases of the cylindrical step's latent heat and thermal history (CylPhaseField, CylThermalHistory), shared by
test_cyl_extras_cpu.py and test_cyl_extras_gpu.py: the shapes and modes, a prescribed sequence of steps per case, the
reference loop over the NumPy definitions, the same loop over the host twins of the C ABI, and the reference loop of the spiral
deposition driver (the oracle's adi_step_masked, then the two definitions).  NumPy and ctypes only: no GPU."""
import ctypes
import math

import numpy as np

# the smallest shapes at which the kernels can go wrong: scalar form with an odd stride; nphi = 1 with the pair form; nr = 1;
# an odd nz past one workgroup per plane; more than one workgroup along z with the pair form
SHAPES = [(3, 5, 7), (2, 1, 36), (1, 4, 130), (5, 8, 129), (2, 3, 1030)]
MODES = ['all', 'random', 'births']
R_INS = [0.0, 0.03]
NSTEPS = 6
DT = 0.25
T0_CLOCK = 1.5

CP = 500.0
LAW_ARGS = (2.7e5, 1400.0, 1450.0)           # latent heat, solidus, liquidus
LEVEL_ARGS = (1073.15, 773.15, 1450.0)       # T_hi, T_lo, T_melt
TDEP = 1600.0                                # above the liquidus
SENTINEL_T, SENTINEL_F = -12345.678, 0.3125  # what inactive cells hold where a test looks for stray writes

GUARD = 8
GUARD_WORD = 0x5a5a5a5a
LOG_INTS = 12
EMPTY_ROW = np.array([0, 2**31 - 1, 2**31 - 1, 2**31 - 1, -1, -1, -1, 0, 0, 0, 0, 0], dtype=np.int32)


def case_ids():
    """(shape, mode, R_in): every shape in every mode, the two inner radii in turn"""
    return [(s, m, R_INS[(i + j) % 2]) for i, s in enumerate(SHAPES) for j, m in enumerate(MODES)]


def case_name(c):
    return '%dx%dx%d-%s-Rin%g' % (c[0] + (c[1], c[2]))


def make_case(shape, mode, seed=0, skip=(False, False)):
    """A prescribed sequence of NSTEPS steps on `shape`: per step the active mask, the increment the "sweeps" add to the
    step's input, and the columns born before it.  The step's input is the previous step's final result (the recorder's
    precondition), with the newborn columns set to TDEP.  The increments of +-600 make single steps cross both levels at once;
    inactive cells hold sentinels."""
    rng = np.random.default_rng(1000 * shape[0] + 10 * shape[2] + seed)
    nr, nphi, nz = shape
    if mode == 'all':
        acts = [None] * NSTEPS
    elif mode == 'random':
        a = rng.random(shape) < 0.7
        a[0, 0, 0] = True
        acts = [a] * NSTEPS
    else:
        cols = rng.permutation(nphi * nz)
        a = np.zeros(shape, dtype=bool)
        acts = []
        for n in range(NSTEPS):
            k = max(1, (n + 1) * len(cols) // (NSTEPS + 1))
            a = a.copy()
            a.reshape(nr, -1)[:, cols[:k]] = True                 # whole radial columns
            acts.append(a)
    T0 = rng.uniform(300.0, 1700.0, shape)
    T0.flat[::7] = rng.uniform(1395.0, 1455.0, T0.flat[::7].shape)          # a good share around the mushy range
    deltas = [rng.uniform(-600.0, 600.0, shape) for _ in range(NSTEPS)]
    for d in deltas:
        d.flat[::5] = 0.0                                           # cells the sweeps leave alone: rest states keep their bits
    return dict(shape=shape, mode=mode, acts=acts, T0=T0, deltas=deltas, skip=skip)


def objects():
    from adi_thermal_fields_amd.phase import PhaseChange
    from adi_thermal_fields_amd.history import HistoryLevels
    return PhaseChange(*LAW_ARGS), HistoryLevels(*LEVEL_ARGS)


def _start(case):
    """(T, f, state) before the first step: sentinels and NaN on inactive cells, f = 0 on the cells active at construction"""
    shape, a0 = case['shape'], case['acts'][0]
    T = case['T0'].copy()
    if a0 is None:
        f = np.zeros(shape)
    else:
        T[~a0] = SENTINEL_T
        f = np.where(a0, 0.0, np.nan)
    if case['mode'] == 'births':
        T[a0] = TDEP                                                # (the first columns are deposited too)
        f = np.full(shape, np.nan)                                  # ... and nothing has been seen active yet
    state = tuple(np.full(shape, np.nan) for _ in range(3))
    return T, f, state


def _step_input(case, n, T):
    """the input of step n from the previous result: the columns born before it at TDEP"""
    if case['mode'] != 'births' or n == 0:
        return T
    born = case['acts'][n] & ~case['acts'][n - 1]
    A = T.copy()
    A[born] = TDEP
    return A


def _t_star(case, n, A):
    """what the sweeps hand to the passes: the input plus the prescribed increment on active cells, the input elsewhere"""
    act = case['acts'][n]
    Ts = A + case['deltas'][n]
    idx = np.arange(A.size).reshape(A.shape)
    quench = (idx % 11 == n) & (A > LEVEL_ARGS[0])                  # from above T_hi to below T_lo in one step
    Ts = np.where(quench, 700.0 + 0.125 * (idx % 64), Ts)
    return Ts if act is None else np.where(act, Ts, A)


def reference_loop(case, capacity=NSTEPS):
    """the NSTEPS steps through the NumPy definitions -> list per step of dict(A, T, f, state, pool), and the log rows
    (capacity + 1, LOG_INTS) with `slot`"""
    from adi_thermal_fields_amd.cyl_extras import CylPhaseField, CylThermalHistory
    law, levels = objects()
    skip = CylPhaseField.skip_planes(case['shape'], *case['skip'])
    T, f, state = _start(case)
    log = np.tile(EMPTY_ROW, (capacity + 1, 1))
    steps = []
    for n in range(NSTEPS):
        act = case['acts'][n]
        A = _step_input(case, n, T)
        Tn, f = CylPhaseField.apply_reference(_t_star(case, n, A), f, A, act, skip, law, CP)
        t_n = T0_CLOCK + n * DT
        state, pool = CylThermalHistory.record_reference(state, A, Tn, act, t_n, DT, levels)
        merge_row(log[min(n, capacity)], CylThermalHistory.pool_row(pool))
        steps.append(dict(A=A, T=Tn, f=f, state=state, pool=pool))
        T = Tn
    return steps, log


def merge_row(row, new):
    """accumulate the row of one step into a log row, as the atomics do (the spill row collects several steps)"""
    row[0] += new[0]
    row[1:4] = np.minimum(row[1:4], new[1:4])
    row[4:7] = np.maximum(row[4:7], new[4:7])
    s = row[8:10].copy().view(np.int64) + new[8:10].copy().view(np.int64)
    row[8:10] = s.view(np.int32)


# ---- the host twins ----------------------------------------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def host_log(capacity):
    """(store, rows): the log between its guard words, rows a view of the capacity + 1 rows, empty"""
    store = np.full((capacity + 1) * LOG_INTS + 2 * GUARD, GUARD_WORD, dtype=np.int32)
    rows = store[GUARD:GUARD + (capacity + 1) * LOG_INTS].reshape(capacity + 1, LOG_INTS)
    rows[:] = EMPTY_ROW
    return store, rows


def host_block(t0, dt, capacity):
    """the history's block on the host: (bytes, float view, int view) = { t0, dt; n, slot, capacity }"""
    blk = np.zeros(5, dtype=np.int64)
    blk.view(np.float64)[0:2] = (t0, dt)
    blk[4] = capacity
    return blk


def host_phase_apply(law, T, f, T_in, act, skip=(False, False)):
    """adi_cyl_phase_apply_host on dense arrays, T and f in place"""
    from adi_thermal_fields_amd import _lib
    a8 = None if act is None else np.ascontiguousarray(act).view(np.uint8)
    _lib.check(_lib.lib.adi_cyl_phase_apply_host(ctypes.byref(law.as_c()), CP, _ptr(T), _ptr(f), _ptr(T_in), _ptr(a8),
                                                 int(skip[0]), int(skip[1]), *T.shape, 0))


def host_history_record(levels, blk, A, B, state, rows, act):
    """adi_cyl_history_record_host on dense arrays, the state and the row in place, then the tick (n += 1, slot += 1)"""
    from adi_thermal_fields_amd import _lib
    a8 = None if act is None else np.ascontiguousarray(act).view(np.uint8)
    _lib.check(_lib.lib.adi_cyl_history_record_host(ctypes.byref(levels.as_c()), _ptr(blk), _ptr(A), _ptr(B), _ptr(state[0]),
                                                    _ptr(state[1]), _ptr(state[2]), _ptr(rows), _ptr(a8), *A.shape, 0))
    blk[2] += 1
    blk[3] += 1


def host_loop(case, capacity=NSTEPS):
    """the NSTEPS steps through the host twins -> (steps as reference_loop gives them, without pool), the log store, the rows
    and the block"""
    law, levels = objects()
    T, f, state = _start(case)
    state = tuple(np.ascontiguousarray(s) for s in state)
    store, rows = host_log(capacity)
    blk = host_block(T0_CLOCK, DT, capacity)
    steps = []
    for n in range(NSTEPS):
        act = case['acts'][n]
        A = np.ascontiguousarray(_step_input(case, n, T))
        Tn = np.ascontiguousarray(_t_star(case, n, A))
        f = f.copy()
        host_phase_apply(law, Tn, f, A, act, case['skip'])
        state = tuple(s.copy() for s in state)
        host_history_record(levels, blk, A, Tn, state, rows, act)
        steps.append(dict(A=A, T=Tn, f=f, state=state))
        T = Tn
    return steps, store, rows, blk


def same_bits(a, b):
    """bit equality of two fp64 arrays, NaN payloads and the sign of zero included"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def same_values(a, b):
    """bit equality of two fp64 arrays, the sign of zero included, after every NaN is mapped to the canonical one (a NaN's
    payload is not part of the contract: NumPy's where() and the device may hand on different ones)"""
    a, b = (np.array(x, dtype=np.float64) for x in (a, b))
    a[np.isnan(a)] = np.nan
    b[np.isnan(b)] = np.nan
    return same_bits(a, b)


# ---- the spiral deposition driver ------------------------------------------------------------------------------------------------
SPIRAL = dict(mat=dict(rho=7800.0, cp=500.0, k=30.0), Tinf=25.0, Tdep=1600.0, R_in=0.03, wall=0.008, h_side=15.0, h_end=10.0,
              z_back=0.004, layer_h=0.002, n_layers=2, tau=0.6, nr=4, nphi=12)
SPIRAL_TIMES = [0.4, 0.9, 2.0]                # 40 steps of tau / nphi: two layers (1.2 s), then cooling
SPIRAL_LAW = (2.7e5, 1400.0, 1450.0)
# degrees C, as Tinf and Tdep; chosen so that the short run cools through both and that no compared value of the reference loop
# comes within 1e-6 relative of a level (3e-4 at the closest, asserted in test_cyl_extras_cpu.py)
SPIRAL_LEVELS = (1300.0, 1000.0, 1450.0)


def spiral_args(times=SPIRAL_TIMES):
    s = SPIRAL
    return (times, s['mat'], s['Tinf'], s['Tdep'], s['R_in'], s['wall'], s['h_side'], s['h_end'], s['z_back'], s['layer_h'],
            s['n_layers'], s['tau'], s['nr'], s['nphi'])


def spiral_reference(law, levels, times=SPIRAL_TIMES):
    """run_spiral_deposition's loop with the oracle's adi_step_masked followed by the two definitions -> dict(fields, masks, f,
    state, rows (one LOG_INTS row per step), t_end (per step), dts, margin): margin is the smallest relative distance of a
    compared value from the level it is compared with, over every step (the caller asserts it is large, so that no comparison
    can flip inside the tolerance)"""
    from oracle import cyl_oracle as cyl
    from adi_thermal_fields_amd.cyl_extras import CylPhaseField, CylThermalHistory
    s = SPIRAL
    nr, nphi, tau, layer_h, n_layers = s['nr'], s['nphi'], s['tau'], s['layer_h'], s['n_layers']
    dr = s['wall'] / nr
    nz = int(round((s['z_back'] + layer_h * n_layers) / layer_h))
    grid = cyl.GridCyl(nr, nphi, nz, dr, 2.0 * math.pi / nphi, layer_h, s['R_in'] + s['wall'], R_in=s['R_in'])
    m = cyl.Material(**s['mat'])
    wall_bc = cyl.RobinR(s['h_side'], s['Tinf'])
    zbc = cyl.ZBC(kind_bot='neumann0', kind_top='robin', h_top=s['h_end'], T_inf_top=s['Tinf'])
    iz0 = int(round(s['z_back'] / layer_h))
    T = np.full((nr, nphi, nz), float(s['Tinf']))
    active = np.zeros((nr, nphi, nz), bool)
    active[:, :, :iz0] = True
    f = np.where(active, 0.0, np.nan)
    state = (np.where(active, T, np.nan), np.full(T.shape, np.nan), np.full(T.shape, np.nan))     # (seeded from T at t = 0)
    dt, omega = tau / nphi, 2.0 * math.pi / tau
    prm = cyl.Params(dt, 1.0, "be")
    layer, angle, t = 0, 0.0, 0.0
    L, Ts, Tl = law.validate()
    _, Hs, Hl, _ = law.constants(s['mat']['cp'])
    T_hi, T_lo, T_melt = levels.validate()
    out = dict(fields=[], masks=[], rows=[], t_end=[], dts=[], margin=np.inf)

    def near(values, level):
        v = np.asarray(values)
        v = v[np.isfinite(v)]
        return np.inf if v.size == 0 else float(np.min(np.abs(v - level)) / abs(level))

    for t_goal in times:
        while t < t_goal - 1e-12:
            t_next = min(t + dt, t_goal)
            left = omega * (t_next - t)
            while left > 0.0 and layer < n_layers:
                seg = min(left, 2.0 * math.pi - angle)
                if seg > 0.0:
                    iz = iz0 + layer
                    if 0 <= iz < nz:
                        first = int(math.floor(angle / grid.dphi))
                        last = max(first, int(math.floor((angle + seg - 1e-12) / grid.dphi)))
                        for c in range(first, last + 1):
                            if not active[0, c % nphi, iz]:
                                active[:, c % nphi, iz] = True
                                T[:, c % nphi, iz] = s['Tdep']
                    angle += seg
                    left -= seg
                if angle >= 2.0 * math.pi - 1e-15:
                    angle = 0.0
                    layer += 1
                    if iz0 + layer > nz - 1:
                        layer = n_layers
            prm.dt = t_next - t
            A = T.copy()
            Tst = cyl.adi_step_masked(A, grid, m, prm, wall_bc, zbc, active, robin_inner=wall_bc, robin_void=wall_bc)
            f_start = np.where(active & np.isnan(f), law.f_eq(A), f)
            H = s['mat']['cp'] * Tst + L * f_start                   # the enthalpy the correction branches on
            Tn, f = CylPhaseField.apply_reference(Tst, f, A, active, None, law, s['mat']['cp'])
            state, pool = CylThermalHistory.record_reference(state, A, Tn, active, t, prm.dt, levels)
            # every comparison the two passes make, on active cells: T* and H against the law's points, A and B against the levels
            for vals, level in ((Tst[active], Ts), (Tst[active], Tl), (A[active], T_hi), (A[active], T_lo), (Tn[active], T_hi),
                                (Tn[active], T_lo), (Tn[active], T_melt), (A[active], Ts), (A[active], Tl),
                                (H[active], Hs), (H[active], Hl)):
                out['margin'] = min(out['margin'], near(vals, level))
            # dt / (A - B) of the step in which a cell's t_hi / t_lo was last written: what an error of T costs its crossing time
            with np.errstate(divide='ignore', invalid='ignore'):
                slope = prm.dt / (A - Tn)
            for key, level in (('slope_hi', T_hi), ('slope_lo', T_lo)):
                crossed = active & (A > level) & (Tn <= level)
                out[key] = np.where(crossed, slope, out.get(key, np.full(T.shape, np.nan)))
            out['rows'].append(CylThermalHistory.pool_row(pool))
            out['t_end'].append(t_next)
            out['dts'].append(prm.dt)
            T = Tn
            t = t_next
        out['fields'].append(T.copy())
        out['masks'].append(active.copy())
    out.update(f=f, state=state, grid=grid)
    return out
