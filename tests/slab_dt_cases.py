"""Cases, runner and expected forms of tests/test_slab_increment_cpu.py and tests/test_slab_increment_gpu.py: ONE step of the
slab-decomposed Cartesian step (dist_slab.SlabStepper, ranks as threads over dist_slab.LocalComm) over the range of time steps,
measured against the extended-precision reference tests/cart_ref_ld.py stepping ONE domain.  Reference-free.

Metric, bar, A, EPS64 and the cfl lists are cart_dt_cases' (why rel_linf cannot see these regimes: its docstring).  What is new
here is the path: the reduced interface system with couplings below DECAY_TOL dropped, six forms of the sharded-axis sweep chosen
per (dt, theta, mask), three pass-A forms, and a quick planner that proves a form from a bound.  A slab run whose ranks do not
talk to each other changes the field by 5e-14 of its size at cfl 1e-13: it passes every rel_linf test and misses this bar 7 x.

A case is (grid, option set, theta, cfl); the reference depends on (grid, theta, cfl) alone and is shared by the option sets.
The GPU test runs the shapes of GRIDS; the CPU test the same nx and slabs on planes of CPU_PLANES (tests/cpu_engine.py solves
every line densely)."""
import functools
import threading
import types
import zlib

import numpy as np

import cart_dt_cases as cd

A = cd.A                 # no form needed a factor of its own: every case meets the bar of the single-domain step

CPU_PLANES = (4, 5)

# name: (shape, slabs, mask, boundary data) -- each the smallest shape at which a test of test_dist_slab_gpu.py reaches the kernel
GRIDS = {
    'holes': ((256, 10, 40), [64] * 4, 'holes5', 'scalar'),           # two-pass forms, generic + in-register condense
    'solid': ((256, 16, 64), [64] * 4, 'solid', 'voxel_h'),           # deferred, deferred_exact; without them the FAST two-pass forms
    'solid_uneven': ((254, 16, 64), [64, 62, 64, 64], 'solid', 'voxel_h'),    # generic condense, uneven slabs
    'curved': ((256, 48, 64), [64] * 4, 'ellipsoid', 'scalar'),       # surface segments (TAIL / HEAD) in pass A; deferred_lines
    'dirichlet': ((254, 16, 64), [64, 62, 64, 64], 'holes2', 'dirichlet'),    # Dirichlet rows cut the coupling; deferred_lines
    'ragged': ((192, 70, 90), [64] * 3, 'ellipsoid', 'scalar'),       # padded planes
    'thin_solid': ((128, 16, 64), [16] * 8, 'solid', 'voxel_h'),      # no decay across a slab at moderate cfl: deferred_exact, 8 ranks
    'thin_holes': ((128, 16, 64), [16] * 8, 'holes5', 'scalar'),      # ... and exact
    'general': ((192, 24, 40), [64] * 3, 'holes5', 'scalar'),         # nz no multiple of 16: GENERAL axis-1 kernels (with no_pad)
}
CPU_PAD = {'ragged': (3, 2)}          # the CPU engine pads nothing by itself: the stepper's padded planes, on CPU ranks

# the knobs of test_dist_slab_gpu._run_slabs (its PASS_A forms among them)
OPTS = {
    'default': {},
    'dots': dict(dots_max=1.0),
    'fused': dict(allow_dots=False),
    'fused_recompute': dict(allow_dots=False, keep_r0=False),
    'separate': dict(allow_dots=False, allow_fused=False),
    'no_deferred': dict(allow_deferred=False),
    'lines': dict(allow_deferred_lines=True),
    'force_exact': dict(force_exact=True),
    'no_window': dict(allow_window=False),
    'dots_no_window': dict(dots_max=1.0, allow_window=False),     # dot-product pass A at every time step ('window' has none)
    'no_pad': dict(no_pad=True),
}
GRID_OPTS = {
    'holes': ('default', 'dots', 'fused', 'fused_recompute', 'separate', 'lines', 'force_exact', 'no_window', 'dots_no_window'),
    'solid': ('default', 'no_deferred', 'force_exact', 'no_window'),
    'solid_uneven': ('default', 'no_deferred'),
    'curved': ('default', 'dots', 'fused', 'fused_recompute', 'separate', 'lines', 'dots_no_window'),
    'dirichlet': ('default', 'lines'),
    'ragged': ('default', 'force_exact'),
    'thin_solid': ('default', 'no_deferred'),
    'thin_holes': ('default',),
    'general': ('no_pad',),
}
THETA_1 = (('holes', 'default'), ('solid', 'default'), ('curved', 'default'), ('curved', 'lines'))      # ... also at theta = 1

# Every (grid, option set) keeps these; 1.9e-9 and 2.1e-9 straddle theta*gamma = kMixedMinTg, 0.3 is where 'window' ends
KEPT_EVERYWHERE = (1e-13, 1e-11, 1.9e-9, 2.1e-9, 1e-3, 0.3, 200.0, 1e6)
# ... and these are left to the first option set of each grid: between 2.1e-9 and 1e-3, and between 200 and 1e6, the planner
# picks the form of a kept neighbour and the kernels take that neighbour's path (tg on the same side of the gate, the same
# variant); an option set changes pass A or the form, not that
THINNED = (1e-7, 1e-5, 3e4)
assert sorted(KEPT_EVERYWHERE + THINNED) == cd.CFL[0.5]
_KEPT_1 = tuple(b for a, b in zip(cd.CFL[0.5], cd.CFL[1.0]) if a in KEPT_EVERYWHERE)        # the same positions of the theta = 1 list


def keys():
    """(grid, option set, theta, cfl) of every case"""
    out = []
    for grid, optsets in GRID_OPTS.items():
        for i, opt in enumerate(optsets):
            out += [(grid, opt, 0.5, cfl) for cfl in cd.CFL[0.5] if i == 0 or cfl in KEPT_EVERYWHERE]
        for i, opt in enumerate(optsets):
            if (grid, opt) in THETA_1:
                out += [(grid, opt, 1.0, cfl) for cfl in cd.CFL[1.0] if i == 0 or cfl in _KEPT_1]
    return out


def tag(key):
    return '%s-%s-theta%g-cfl%g' % key


def params(select=lambda key: True):
    ks = [k for k in keys() if select(k)]
    return dict(argnames='key', argvalues=ks, ids=[tag(k) for k in ks])


def shape_of(grid, full):
    shape = GRIDS[grid][0]
    return shape if full else (shape[0],) + CPU_PLANES


@functools.lru_cache(maxsize=None)
def _static(grid, full, theta):
    """everything of a case but the time step; built once, read-only"""
    _, _, mname, bc = GRIDS[grid]
    shape = shape_of(grid, full)
    rng = np.random.default_rng(zlib.crc32(repr((grid, shape, theta)).encode()))
    if mname == 'solid':
        mask = np.ones(shape, bool)
    elif mname == 'ellipsoid':
        mask = cd._mask(shape, 'ellipsoid')
    else:
        mask = rng.random(shape) > {'holes5': 0.05, 'holes2': 0.02}[mname]
    # a Neumann flux on x- and a Robin end row on x+: the first and the last rank carry modified end rows
    c = dict(shape=shape, dx=cd.DX, mat=dict(cd.STEEL), mask=mask, T0=rng.uniform(20.0, 1500.0, shape), dir_mask=None,
             dir_value=None, neumann={'x-': 2e5}, robin_h=350.0, Tinf=cd.TINF, theta=theta, nsteps=1, births=None)
    if bc == 'voxel_h':
        c['robin_h'] = rng.uniform(100.0, 600.0, shape)
    if bc == 'dirichlet':
        c.update(dir_mask=(rng.random(shape) < 0.01) & mask, dir_value=rng.uniform(100.0, 400.0, shape))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def dt_of(cfl):
    return cfl * cd.DX * cd.DX / cd.ALPHA


def case(key, full):
    grid, opt, theta, cfl = key
    c = dict(_static(grid, full, theta))
    c['dt'] = dt_of(cfl)
    return c


def sizes(key):
    return list(GRIDS[key[0]][1])


def options(key, full):
    o = dict(OPTS[key[1]])
    if not full and key[0] in CPU_PAD:
        o['pad'] = CPU_PAD[key[0]]
    return o


@functools.lru_cache(maxsize=None)
def _reference(grid, full, theta, cfl):
    return cd.reference_of(case((grid, None, theta, cfl), full))


def reference(key, full):
    """cart_ref_ld, one step of one domain from the same float64 T0; once per (grid, theta, cfl) and session"""
    return _reference(key[0], full, key[2], key[3])


def figures(X, key, full):
    return cd.figures_of(X, case(key, full), reference(key, full))


def step_figures(X, c, T_in, dt):
    """figures of one step of the case c taken from the float64 field T_in with the time step dt (a step of a sequence, judged
    from its own input)"""
    cs = dict(c, T0=np.array(T_in, dtype=np.float64), dt=dt, nsteps=1)
    return cd.figures_of(X, cs, cd.reference_of(cs)), cs


# ---- the runner -----------------------------------------------------------------------------------------------------------
def hip_engine():
    import torch
    from adi_thermal_fields_amd import dist_slab
    torch.cuda.set_device(0)
    return dist_slab.HipEngine()


def run_slabs(engine_factory, mod, c, sizes, opts=None, nsteps=1, dts=None, keep_steps=False):
    """The steps of case c on len(sizes) ranks, one thread per rank over dist_slab.LocalComm, with engine_factory()'s engine on
    every rank and mod's Material / Params (and to_device, where it has one).  opts: the knobs of the tests of the slab step
    (test_dist_slab_gpu._run_slabs is this function).  dts: one time step per step (an event loop) instead of nsteps x c['dt'].
    -> namespace(T: the assembled field, modes: the ranks' axis0_mode after the last step, steps: the assembled field after
    every step (keep_steps), plans: per step the set over the ranks of (axis0_mode, fused, dots, quick))"""
    import torch
    from adi_thermal_fields_amd import dist_slab
    world = len(sizes)
    o = opts or {}
    dts = [c['dt']] * nsteps if dts is None else list(dts)
    comms = dist_slab.LocalComm.make(world)
    out = [None] * world
    kept = [[None] * world for _ in dts]
    plans = [[None] * world for _ in dts]
    modes = set()
    errs = []

    def get(T):
        return T.get() if hasattr(T, 'get') else np.array(dist_slab.SlabStepper.local_numpy(T))

    def work(rank):
        try:
            engine = engine_factory()
            i0 = sum(sizes[:rank]); i1 = i0 + sizes[rank]

            def loc(a):
                return a if (a is None or np.isscalar(a)) else np.asarray(a)[i0:i1]
            neumann = None if c['neumann'] is None else {f: loc(v) for f, v in c['neumann'].items()}
            robin_h = {f: loc(v) for f, v in c['robin_h'].items()} if isinstance(c['robin_h'], dict) else loc(c['robin_h'])
            if o.get('no_pad'):                        # the caller's planes as they are (ragged lines on the GENERAL kernels)
                engine.plane_dims = lambda ny, nz: (ny, nz)
            if o.get('pad'):                           # padded planes on an engine that pads nothing by itself
                dy, dz = o['pad']
                engine.plane_dims = lambda ny, nz: (ny + dy, nz + dz)
            st = dist_slab.SlabStepper(c['mask'][i0:i1], c['dx'], mod.Material(**c['mat']),
                                       mod.Params(dts[0], c['theta']), c['Tinf'], dir_mask=loc(c['dir_mask']),
                                       dir_value=loc(c['dir_value']), neumann=neumann, robin_h=robin_h,
                                       comm=comms[rank], engine=engine)
            st._force_exact = bool(o.get('force_exact', False))
            st._allow_window = bool(o.get('allow_window', True))
            st._allow_fused = bool(o.get('allow_fused', True))
            st._allow_dots = bool(o.get('allow_dots', True))
            st._keep_r0 = bool(o.get('keep_r0', True))
            st._allow_deferred = bool(o.get('allow_deferred', True))
            st._allow_deferred_exact = bool(o.get('allow_deferred_exact', True))
            # (off unless a test asks for it: most cases were written for the two-pass forms it would otherwise replace)
            st._allow_deferred_lines = bool(o.get('allow_deferred_lines', False))
            # (solids riddled with voids: every line is flagged -- the sparse pass at its fullest; the product's cost rule would
            # leave them to the window form unless a case asks for the rule with 'cost_rule')
            st._deferred_lines_cost_ratio = 1.0 if o.get('cost_rule') else float('inf')
            if 'dots_max' in o:
                st.DOTS_MAX_NONUNIFORM = o['dots_max']
            T0 = np.ascontiguousarray(c['T0'][i0:i1])
            T = mod.to_device(T0) if hasattr(mod, 'to_device') else torch.from_numpy(T0.copy())
            for s, dt in enumerate(dts):
                st.params.dt = dt
                T = st.step(T, prefetch_halo=bool(o.get('prefetch', False)) and s + 1 < len(dts))
                p = st._a0 or {}
                plans[s][rank] = (st.axis0_mode, bool(p.get('fused')), bool(p.get('dots')), bool(p.get('quick')))
                if keep_steps and s + 1 < len(dts):
                    kept[s][rank] = get(T)
            out[rank] = get(T)
            kept[-1][rank] = out[rank]
            modes.add(st.axis0_mode)
        except Exception as e:   # surface the failure and release the other ranks
            errs.append(e)
            comms[rank].sh.barrier.abort()

    ths = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=120)
    if errs:
        raise errs[0]
    steps = [np.concatenate(k, axis=0) for k in kept if k[0] is not None]
    return types.SimpleNamespace(T=np.concatenate(out, axis=0), modes=modes, steps=steps, plans=[set(p) for p in plans])


def run_case(engine_factory, mod, key, full, **kw):
    return run_slabs(engine_factory, mod, case(key, full), sizes(key), options(key, full), **kw)


# ---- the dt sequence of the quick plans (an event loop's residual sub-steps): one full plan, then hops between the regimes -----
SEQ_CFL = (0.1, 0.1, 1e-11, 200.0, 2.1e-9, 1e6, 1e-13, 0.3)



def hold(X, c, f, what):
    """finite; off-mask cells bit-equal to T0, Dirichlet cells to dir_value; the bar"""
    assert np.all(np.isfinite(X)), what
    assert cd.untouched_exact(X, c), what
    assert f['abs_err'] <= cd.bar(f, A), (what, f, cd.bar(f, A))


def sequence_holds(engine_factory, mod, grid, full, report=print):
    """A first full plan at cfl 3 ('slab': a plan in 'window' form leaves the choice of pass A open, and the planner keeps
    measuring until a whole-slab plan has made it), then slab_dt_cases.SEQ_CFL: every change of the time step is a quick plan, the
    three two-pass forms are all met, and every step holds the bar against the reference stepping from that step's own input."""
    key = (grid, 'default', 0.5, 3.0)
    c = case(key, full)
    dts = [dt_of(cfl) for cfl in (3.0,) + SEQ_CFL]
    run = run_slabs(engine_factory, mod, c, sizes(key), options(key, full), dts=dts, keep_steps=True)
    assert len(run.steps) == len(dts)
    T_in, forms = c['T0'], set()
    for s, (dt, X) in enumerate(zip(dts, run.steps)):
        (mode, fused, dots, quick), = run.plans[s]
        f, cs = step_figures(X, c, T_in, dt)
        report('seq %s step %d cfl %-8g %-7s quick %d  inc %.2e K  err %.2e K = %8.2f ulp = %.1e inc' % (
            grid, s, ((3.0,) + SEQ_CFL)[s], mode, quick, f['inc'], f['abs_err'], f['ulp'], f['of_inc']))
        hold(X, cs, f, (grid, s))
        assert quick == (s >= 1), (s, mode, quick)            # (step 2 repeats step 1's time step: the same quick plan)
        if quick:
            forms.add(mode)
        T_in = X
    assert forms == {'window', 'slab', 'exact'}, forms


# ---- the form each case is there for ---------------------------------------------------------------------------------------
# axis0_mode per (grid, option set, theta), one letter per time step of the case's list (keys()), as the reference engine
# (tests/cpu_engine.py, planes of CPU_PLANES) ran it:  w window, s slab, e exact, d deferred, x deferred_exact, l deferred_lines
LETTER = dict(w='window', s='slab', e='exact', d='deferred', x='deferred_exact', l='deferred_lines')
FORMS_CPU = {
    ('holes', 'default', 0.5): 'wwwwwwwssss',          # (voids cut every line: the measured couplings have decayed even at cfl 1e6)
    ('holes', 'dots', 0.5): 'wwwwwsss',
    ('holes', 'fused', 0.5): 'wwwwwsss',
    ('holes', 'fused_recompute', 0.5): 'wwwwwsss',
    ('holes', 'separate', 0.5): 'wwwwwsss',
    ('holes', 'lines', 0.5): 'llllllss',
    ('holes', 'force_exact', 0.5): 'eeeeeeee',
    ('holes', 'no_window', 0.5): 'ssssssss',
    ('holes', 'dots_no_window', 0.5): 'ssssssss',
    ('holes', 'default', 1.0): 'wwwwwwwseee',
    ('solid', 'default', 0.5): 'ddddddddxxx',
    ('solid', 'no_deferred', 0.5): 'wwwwwsee',
    ('solid', 'force_exact', 0.5): 'xxxxxxxx',
    ('solid', 'no_window', 0.5): 'ddddddxx',
    ('solid', 'default', 1.0): 'ddddddddxxx',
    ('solid_uneven', 'default', 0.5): 'ddddddddxxx',
    ('solid_uneven', 'no_deferred', 0.5): 'wwwwwsee',
    ('curved', 'default', 0.5): 'wwwwwwwseee',
    ('curved', 'dots', 0.5): 'wwwwwsee',
    ('curved', 'fused', 0.5): 'wwwwwsee',
    ('curved', 'fused_recompute', 0.5): 'wwwwwsee',
    ('curved', 'separate', 0.5): 'wwwwwsee',
    ('curved', 'lines', 0.5): 'llllllee',
    ('curved', 'dots_no_window', 0.5): 'ssssssee',
    ('curved', 'default', 1.0): 'wwwwwwwseee',
    ('curved', 'lines', 1.0): 'llllllee',
    ('dirichlet', 'default', 0.5): 'wwwwwwwseee',
    ('dirichlet', 'lines', 0.5): 'llllllee',
    ('ragged', 'default', 0.5): 'wwwwwwwseee',
    ('ragged', 'force_exact', 0.5): 'eeeeeeee',
    ('thin_solid', 'default', 0.5): 'dddddddxxxx',
    ('thin_solid', 'no_deferred', 0.5): 'ssssseee',
    ('thin_holes', 'default', 0.5): 'ssssssseeee',
    ('general', 'no_pad', 0.5): 'wwwwwwwseee',
}
# ... and where HipEngine on the full shapes decides otherwise: (grid, option set, theta, cfl) -> (form, why)
_WHY = 'on (10, 40) planes some line runs through a whole slab without a void: the measured coupling has not decayed'
FORMS_HIP = {key: ('exact', _WHY) for key in keys() if key[0] == 'holes' and key[2] == 0.5 and key[3] >= 200.0
             and key[1] not in ('force_exact',)}


def expected_form(key, full):
    if full and key in FORMS_HIP:
        return FORMS_HIP[key][0]
    grid, opt, theta, cfl = key
    cfls = [k[3] for k in keys() if k[:3] == key[:3]]
    return LETTER[FORMS_CPU[key[:3]][cfls.index(cfl)]]


def forms_cover(full):
    """the pinned forms (each case asserts that it ran in its own): all six are reached, each on both sides of theta*gamma =
    kMixedMinTg -- 'deferred_exact' below it through force_exact on the all-solid grid -- and at theta 0.5 and 1; no (grid, option
    set) drops a value of KEPT_EVERYWHERE"""
    gate = cd.K_MIXED_MIN_TG
    seen = {}
    for key in keys():
        grid, opt, theta, cfl = key
        seen.setdefault(expected_form(key, full), set()).add((theta, theta * cfl < gate))
    assert set(seen) == set(LETTER.values()), seen
    for form, where in seen.items():
        assert {(0.5, True), (0.5, False)} <= where, (form, where)
        assert {th for th, _ in where} == {0.5, 1.0}, (form, where)
    for grid, optsets in GRID_OPTS.items():
        for opt in optsets:
            assert set(KEPT_EVERYWHERE) <= {key[3] for key in keys() if key[:3] == (grid, opt, 0.5)}, (grid, opt)
    assert 0.5 * 1.9e-9 < gate < 0.5 * 2.1e-9 and 1.0 * _KEPT_1[2] < gate < 1.0 * _KEPT_1[3]
