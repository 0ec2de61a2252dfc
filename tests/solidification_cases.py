"""Shared by tests/test_solidification_cpu.py and tests/test_solidification_gpu.py: short runs for the solidification recorder
over any module with the reference's operator surface (the pinned C oracle in the CPU tests, the HIP module in the GPU tests),
and the loop  B = step(A) -> state = record_reference(state, A, B, mask, t_n, dt, dx, T_freeze)  that defines what the device
must record.

A case: a cold body (Robin on every face) and source fields that melt cells for a step or two and then let them freeze.  The
heated set is a product I x J x K with I = {0, 15, 16, n - 1} along every axis: cells on both sides of the brick seam 15 | 16
of every axis, and cells on every face, edge and corner of the box, so the freezing cells between them show every one of the
27 combinations of (both neighbours / the plus one only / the minus one only) over the three axes.  In the case with holes
the mask is forced solid one cell around the heated set, so that the box decides those combinations, and a few more heated
cells sit next to a hole.  Four segments with two values of dt: a pulse, cooling, a second pulse on the eight cells in the middle (cells
that froze melt and freeze again), cooling.  `conditions` counts what the inputs were chosen for; tests/test_solidification_cpu.py
asserts it on the C oracle and tests/test_solidification_gpu.py on the device's own fields."""
import itertools

import numpy as np

FACES = ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')
RHO, CP, K = 7800.0, 490.0, 54.0
KAPPA = K / (RHO * CP)
DX, TINF, H, THETA = 1e-3, 25.0, 200.0, 0.5
T_FREEZE = 1400.0
DT_A, DT_B = 0.5 * DX * DX / KAPPA, 3.0 * DX * DX / KAPPA
CASES = ('holes', 'solid')
SHAPES = {'holes': (19, 21, 37), 'solid': (32, 32, 32)}
PADDED = {'holes': (20, 24, 40)}          # the physical box of the padded variant of the GPU tests
S_PULSE = 1.0e12                          # W/m^3: dt*S/(rho cp) = 1e12 * 0.0354 / 3.8e6, about 9 000 K ahead of the sweeps


def _axis_set(n):
    return [0, 15, 16, n - 1]


_cases = {}


def case(name):
    """the inputs of a case, built once, never modified"""
    if name not in _cases:
        shape = SHAPES[name]
        rng = np.random.default_rng(23)
        heated = np.zeros(shape, dtype=bool)
        heated[np.ix_(*[_axis_set(n) for n in shape])] = True
        middle = np.zeros(shape, dtype=bool)
        middle[15:17, 15:17, 15:17] = True
        mask = np.ones(shape, dtype=bool)
        near_hole = np.zeros(shape, dtype=bool)
        if name == 'holes':
            mask = rng.random(shape) > 0.07
            grown = np.pad(heated, 1)
            for ax, d in itertools.product(range(3), (-1, 1)):
                grown |= np.roll(np.pad(heated, 1), d, axis=ax)
            mask |= grown[1:-1, 1:-1, 1:-1]
            # a few more heated cells: in the mask, next to a hole, away from the box faces
            mp = np.pad(mask, 1, constant_values=True)
            holey = np.zeros(shape, dtype=bool)
            for ax, d in itertools.product(range(3), (-1, 1)):
                holey |= ~np.roll(mp, d, axis=ax)[1:-1, 1:-1, 1:-1]
            cand = np.argwhere(mask & holey & ~heated)
            near_hole[tuple(cand[rng.choice(len(cand), 12, replace=False)].T)] = True
        T0 = np.full(shape, TINF)
        # (the pulse varies from cell to cell, 0.6 .. 1.3 of S_PULSE, so that the cells do not all freeze in the same step)
        S1 = np.where((heated | near_hole) & mask, S_PULSE * (0.6 + 0.7 * rng.random(shape)), 0.0)
        S2 = np.where(middle, 0.26 * S_PULSE, 0.0)
        segs = [(DT_A, 1, S1), (DT_A, 4, None), (DT_B, 1, S2), (DT_B, 3, None)]
        c = dict(name=name, shape=shape, mask=mask, T0=T0, segments=segs, heated=heated, middle=middle, near_hole=near_hole)
        for a in (mask, T0, S1, S2, heated, middle, near_hole):
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
    axis-0 pack, dt*S/(rho cp) on in-mask cells, as in tests/history_cases.py)"""
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


def record_trajectory(rec_cls, c, traj, t=0.0, clock='run', segments=None, T_freeze=T_FREEZE, dx=DX):
    """the definition over a stored trajectory: states[n] after step n, and the clock at the end.  clock = 'run': as
    StagedStepper.run keeps it -- within a segment t_n = t0 + n*dt, and the next segment starts at t0 + nsteps*dt; clock =
    'step': as single recorded steps keep it -- every step is a run of its own, t_n+1 = t_n + dt"""
    mask = c['mask']
    state = rec_cls.seed_reference(empty_state(c['shape']), traj[0], mask)
    states = [state]
    k = 0
    for dt, n, _ in (c['segments'] if segments is None else segments):
        t0 = t
        for i in range(n):
            t_n = t0 + i * dt if clock == 'run' else t
            state = rec_cls.record_reference(state, traj[k], traj[k + 1], mask, t_n, dt, dx, T_freeze)
            states.append(state)
            t = t0 + (i + 1) * dt if clock == 'run' else t_n + dt
            k += 1
    return states, t


def freezing(c, A, B, T_freeze=T_FREEZE):
    return c['mask'] & (A > T_freeze) & (B <= T_freeze)


def neighbour_class(mask):
    """per cell a number 0 .. 63: two bits per axis, bit 0 the minus neighbour is in the mask, bit 1 the plus neighbour"""
    mp = np.pad(np.asarray(mask, dtype=bool), 1)
    cls = np.zeros(mask.shape, dtype=np.int64)
    for ax in range(3):
        lo = np.roll(mp, 1, axis=ax)[1:-1, 1:-1, 1:-1]
        hi = np.roll(mp, -1, axis=ax)[1:-1, 1:-1, 1:-1]
        cls |= (lo.astype(np.int64) | (hi.astype(np.int64) << 1)) << (2 * ax)
    return cls


def conditions(c, traj, T_freeze=T_FREEZE):
    """what the case was built for -> dict:
    combos      how many of the 27 combinations of (minus only, plus only, both) over the three axes the freezing cells show
    seam_sides  for every axis, freezing cells with index <= 15 and with index >= 16
    late_brick  freezing cells (step n: T[n-1] -> T[n]) of a brick none of whose in-mask cells was above T_freeze in T[n-2]
    refrozen    cells that froze in two different steps
    at_hole     freezing cells with a neighbour inside the box that is off the mask
    still_hot   in-mask cells above T_freeze at the end"""
    mask = c['mask']
    cls = neighbour_class(mask)
    box = neighbour_class(np.ones(c['shape'], dtype=bool))
    seen, count = set(), np.zeros(c['shape'], dtype=np.int64)
    late = at_hole = 0
    sides = [[False, False] for _ in range(3)]
    nb = [(n + 15) // 16 for n in c['shape']]
    for n in range(1, len(traj)):
        fz = freezing(c, traj[n - 1], traj[n], T_freeze)
        if not fz.any():
            continue
        count += fz
        idx = np.argwhere(fz)
        seen.update(int(v) for v in cls[fz])
        at_hole += int((cls[fz] != box[fz]).sum())
        for ax in range(3):
            sides[ax][0] |= bool((idx[:, ax] <= 15).any())
            sides[ax][1] |= bool((idx[:, ax] >= 16).any())
        if n >= 2:
            hot2 = mask & (traj[n - 2] > T_freeze)
            pad = [(0, b * 16 - s) for b, s in zip(nb, c['shape'])]
            brick_hot = np.pad(hot2, pad).reshape(nb[0], 16, nb[1], 16, nb[2], 16).any(axis=(1, 3, 5))
            late += int((~brick_hot[idx[:, 0] // 16, idx[:, 1] // 16, idx[:, 2] // 16]).sum())
    want = {a | (b << 2) | (d << 4) for a in (1, 2, 3) for b in (1, 2, 3) for d in (1, 2, 3)}
    return dict(combos=len(seen & want), seam_sides=all(a and b for a, b in sides), late_brick=late,
                refrozen=int((count >= 2).sum()), at_hole=at_hole, still_hot=int((mask & (traj[-1] > T_freeze)).sum()))


def assert_conditions(c, traj):
    """a case that does not reach what it claims fails"""
    got = conditions(c, traj)
    print(c['name'], got)
    assert got['combos'] == 27, got
    assert got['seam_sides'] and got['late_brick'] > 0 and got['refrozen'] > 0 and got['still_hot'] == 0, got
    if c['name'] == 'holes':
        assert got['at_hole'] > 0, got
    return got
