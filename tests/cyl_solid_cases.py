"""Cases of the cylindrical step's solidification record (CylSolidificationRecord), shared by test_cyl_solid_cpu.py and
test_cyl_solid_gpu.py: the shapes and modes, the chained steps of a case (cyl_extras_cases.make_case), the reference loop over
the NumPy definition, the same loop over the host twin of the C ABI, the neighbour situations of the freezing cells, and the
reference loop of the spiral deposition driver (the oracle's adi_step_masked, CylPhaseField.apply_reference, then the
definition).  NumPy and ctypes only: no GPU."""
import ctypes
import math

import numpy as np

from cyl_extras_cases import make_case, same_values, spiral_reference  # noqa: F401  (re-exported for the tests)
import cyl_extras_cases as cc

# the smallest shapes at which the kernel can go wrong: scalar form, odd stride, one partial tile; no phi neighbour, pair form;
# no r neighbour, two tiles with the boundary inside a z line; both phi neighbours the same cell; odd nz, three tiles per plane;
# a z line longer than two tiles (z neighbours in another workgroup's tile, the seam neighbours five tiles apart)
SHAPES = [(3, 5, 7), (2, 1, 36), (1, 4, 130), (2, 2, 8), (5, 8, 129), (2, 3, 1030)]
MODES = cc.MODES
R_INS = cc.R_INS
NSTEPS = cc.NSTEPS
DT = cc.DT
T0_CLOCK = cc.T0_CLOCK
T_F = 1425.0
TILE = 512
SENTINEL = cc.SENTINEL_F

GUARD, GUARD_WORD, LOG_INTS, EMPTY_ROW = cc.GUARD, cc.GUARD_WORD, cc.LOG_INTS, cc.EMPTY_ROW
merge_row, host_log, host_block, same_bits = cc.merge_row, cc.host_log, cc.host_block, cc.same_bits


def case_ids():
    """(shape, mode, R_in): every shape in every mode, the two inner radii in turn"""
    return [(s, m, R_INS[(i + j) % 2]) for i, s in enumerate(SHAPES) for j, m in enumerate(MODES)]


def case_name(c):
    return '%dx%dx%d-%s-Rin%g' % (c[0] + (c[1], c[2]))


class Grid:
    """the geometry the definition reads: R_in, dr, dphi, dz (no device, no layout)"""

    def __init__(self, shape, r_in=0.0, dr=1.0e-3, dz=1.2e-3):
        self.nr, self.nphi, self.nz = shape
        self.shape = tuple(shape)
        self.R_in, self.dr, self.dphi, self.dz = float(r_in), float(dr), 2.0 * math.pi / shape[1], float(dz)
        self.r = self.R_in + (np.arange(self.nr, dtype=np.float64) + 0.5) * self.dr


def chain(case):
    """the NSTEPS steps (A, B, active) of a case: B is what the "sweeps" hand on, A of the next step is B with the newborn
    columns at TDEP -- on cells active before and after, A is bitwise the previous B"""
    T = cc._start(case)[0]
    out = []
    for n in range(NSTEPS):
        A = np.ascontiguousarray(cc._step_input(case, n, T))
        B = np.ascontiguousarray(cc._t_star(case, n, A))
        out.append((A, B, case['acts'][n]))
        T = B
    return out


def nan_state(shape):
    return tuple(np.full(shape, np.nan) for _ in range(3))


def reference_loop(case, grid, capacity=NSTEPS, T_f=T_F):
    """the steps through the NumPy definition -> list per step of dict(A, B, act, state, front), and the log rows
    (capacity + 1, LOG_INTS)"""
    from adi_thermal_fields_amd.cyl_solid import CylSolidificationRecord as Rec
    state = nan_state(case['shape'])
    log = np.tile(EMPTY_ROW, (capacity + 1, 1))
    steps = []
    for n, (A, B, act) in enumerate(chain(case)):
        state, front = Rec.record_reference(state, A, B, act, T0_CLOCK + n * DT, DT, grid, T_f)
        merge_row(log[min(n, capacity)], Rec.front_row(front))
        steps.append(dict(A=A, B=B, act=act, state=state, front=front))
    return steps, log


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def act8(act):
    return None if act is None else np.ascontiguousarray(act).view(np.uint8)


def host_hot(shape, value=1):
    """(store, words): the hot words between their guard words, every word `value`"""
    nr, nphi, nz = shape
    n = nr * ((nphi * nz + TILE - 1) // TILE)
    store = np.full(n + 2 * GUARD, GUARD_WORD, dtype=np.int32)
    words = store[GUARD:GUARD + n]
    words[:] = value
    return store, words


def host_record(grid, blk, A, B, state, rows, act, hot=None, T_f=T_F):
    """adi_cyl_solid_record_host on dense arrays, the state, the row and the words in place, then the tick"""
    from adi_thermal_fields_amd import _lib
    _lib.check(_lib.lib.adi_cyl_solid_record_host(T_f, grid.R_in, grid.dr, grid.dphi, grid.dz, _ptr(blk), _ptr(A), _ptr(B),
                                                  _ptr(state[0]), _ptr(state[1]), _ptr(state[2]), _ptr(rows), _ptr(act8(act)),
                                                  _ptr(hot), *A.shape, 0))
    blk[2] += 1
    blk[3] += 1


def host_hot_seed(T, act, hot, T_f=T_F):
    from adi_thermal_fields_amd import _lib
    _lib.check(_lib.lib.adi_cyl_solid_hot_seed_host(T_f, _ptr(T), _ptr(act8(act)), _ptr(hot), *T.shape, 0))


def host_loop(case, grid, capacity=NSTEPS, hot=False, T_f=T_F):
    """the steps through the host twin -> (list per step of dict(state, hot), the log store, the rows, the block).  hot: the
    words are seeded from the first input and passed to every record"""
    state = nan_state(case['shape'])
    store, rows = host_log(capacity)
    blk = host_block(T0_CLOCK, DT, capacity)
    hot_store, words = host_hot(case['shape'])
    steps = []
    for n, (A, B, act) in enumerate(chain(case)):
        if hot and n == 0:
            host_hot_seed(A, act, words, T_f)
        state = tuple(s.copy() for s in state)
        host_record(grid, blk, A, B, state, rows, act, words if hot else None, T_f)
        steps.append(dict(state=state, hot=words.copy()))
    assert (hot_store[:GUARD] == GUARD_WORD).all() and (hot_store[-GUARD:] == GUARD_WORD).all()
    return steps, store, rows, blk


def neighbour_situations(fz, act):
    """per axis the set of situations ('both', 'lo', 'hi', 'none') that occur among the freezing cells `fz`"""
    shape = fz.shape
    m = np.ones(shape, bool) if act is None else act
    out = []
    for axis in range(3):
        if axis == 1:
            if shape[1] == 1:
                lo = hi = np.zeros(shape, bool)
            else:
                lo, hi = np.roll(m, 1, axis=1), np.roll(m, -1, axis=1)
        else:
            mp = np.pad(m, 1)
            sl = lambda d: tuple(slice(1 + (d if a == axis else 0), 1 + (d if a == axis else 0) + n)   # noqa: E731
                                 for a, n in enumerate(shape))
            lo, hi = mp[sl(-1)], mp[sl(+1)]
        seen = set()
        for name, where in (('both', lo & hi), ('lo', lo & ~hi), ('hi', hi & ~lo), ('none', ~lo & ~hi)):
            if (fz & where).any():
                seen.add(name)
        out.append(seen)
    return out


# ---- the spiral deposition driver ------------------------------------------------------------------------------------------------
SPIRAL_T_FREEZE = 1400.0


def spiral_solid_reference(times=cc.SPIRAL_TIMES, T_f=SPIRAL_T_FREEZE):
    """run_spiral_deposition's loop with the oracle's adi_step_masked, CylPhaseField.apply_reference and the definition of the
    solidification record -> dict(fields, masks, state, rows, t_end, margin, min_drop, froze_steps, slope, den): margin is the
    smallest relative distance of a compared A or B from T_freeze over every step, slope = dt / (A - B) and den = A - B of the
    step in which a cell last froze"""
    from oracle import cyl_oracle as cyl
    from adi_thermal_fields_amd.cyl_extras import CylPhaseField
    from adi_thermal_fields_amd.cyl_solid import CylSolidificationRecord as Rec
    from adi_thermal_fields_amd.phase import PhaseChange
    law = PhaseChange(*cc.SPIRAL_LAW)
    s = cc.SPIRAL
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
    state = nan_state(T.shape)
    dt, omega = tau / nphi, 2.0 * math.pi / tau
    prm = cyl.Params(dt, 1.0, "be")
    layer, angle, t = 0, 0.0, 0.0
    out = dict(fields=[], masks=[], rows=[], t_end=[], margin=np.inf, min_drop=np.inf, froze_steps=0,
               slope=np.full(T.shape, np.nan), den=np.full(T.shape, np.nan), grid=grid)
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
            Tn, f = CylPhaseField.apply_reference(Tst, f, A, active, None, law, s['mat']['cp'])
            state, front = Rec.record_reference(state, A, Tn, active, t, prm.dt, grid, T_f)
            for vals in (A[active], Tn[active]):
                out['margin'] = min(out['margin'], float(np.min(np.abs(vals - T_f)) / abs(T_f)))
            fz = active & (A > T_f) & (Tn <= T_f)
            if fz.any():
                out['froze_steps'] += 1
                out['min_drop'] = min(out['min_drop'], float(np.min((A - Tn)[fz])))
                with np.errstate(divide='ignore', invalid='ignore'):
                    out['slope'] = np.where(fz, prm.dt / (A - Tn), out['slope'])
                out['den'] = np.where(fz, A - Tn, out['den'])
            out['rows'].append(Rec.front_row(front))
            out['t_end'].append(t_next)
            T = Tn
            t = t_next
        out['fields'].append(T.copy())
        out['masks'].append(active.copy())
    out.update(state=state, f=f)
    return out
