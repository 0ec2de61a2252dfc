"""waam -- the layer-birth / moving-deposit time loops of the reference's WAAM drivers, backend-agnostic.

The loops are restated from waam_from_stl_v7_mm.py (layers :436-456, birth times :458-471, activate_layer
:487-495, event loop :515-550) and single_track_on_plate.py:150-177 (column-by-column deposit).  They drive ANY
module with the reference's operator surface (`Grid3D`, `Material`, `Params`,
`precompute_coeff_packs_unified`, `adi_step_numba_coeff`): the HIP backend in production, the CPU oracle in
the parity tests.  The mask of a part comes from `voxelize.load_voxel_from_stl_mm` (STL -> solid mask on the device, no
trimesh); `synthetic_head_mask` supplies the formula-generated stand-in for the missing `11091_FemaleHead_v4.stl`
(SURVEY.md 8(d) config 5).

With the HIP backend the temperature stays in HBM for the whole run: births are a masked fill on the
device, the mask/pack rebuild is one upload (1 B/cell) plus two kernels, frames download only at output times.
"""
import math

import numpy as np

__all__ = ['synthetic_head_mask', 'plan_layers', 'birth_times', 'layer_birth_schedule', 'run_layer_birth', 'run_single_track',
           'run_layer_birth_slab', 'run_single_track_slab', 'ring_source', 'run_spiral_deposition', 'path_steps',
           'run_path_deposition']


def synthetic_head_mask(nx, ny, nz):
    """Union of an ellipsoid (semi-axes 0.35/0.42/0.45 of the box, centred at 0.5/0.5/0.55) and a neck
    cylinder (radius 0.16 of the box, lower 40 %), by formula."""
    x = (np.arange(nx) + 0.5) / nx - 0.5
    y = (np.arange(ny) + 0.5) / ny - 0.5
    z = (np.arange(nz) + 0.5) / nz
    X, Y, Z = np.meshgrid(x, y, z, indexing='ij')
    ell = (X / 0.35) ** 2 + (Y / 0.42) ** 2 + ((Z - 0.55) / 0.45) ** 2 <= 1.0
    neck = (X ** 2 + Y ** 2 <= 0.16 ** 2) & (Z <= 0.4)
    return ell | neck


def plan_layers(mask_full, n_per_layer):
    """Plane ranges (ks, ke) along axis 2, the layer list of waam_from_stl_v7_mm.py:436-456: a layer starts at the next
    occupied plane, spans at most `n_per_layer` planes and ends on an occupied plane; empty planes belong to no layer.
    Computed on the sorted indices of the occupied planes (two binary searches per layer) instead of the reference's
    plane-by-plane scan; the list is the same (tests/test_waam_harness.py pins it against the reference's on gapped masks)."""
    occ = np.flatnonzero(np.asarray(mask_full).any(axis=(0, 1)))
    if occ.size == 0:
        raise RuntimeError("empty voxel model")
    n = max(1, int(n_per_layer))
    layers, p = [], 0
    while p < occ.size:
        ks = int(occ[p])
        q = int(np.searchsorted(occ, ks + n - 1, side='right')) - 1     # last occupied plane inside the span
        layers.append((ks, int(occ[q])))
        p = q + 1
    return layers


def birth_times(mask_full, layers, dx, bead_width, scan_speed, eta_fill=1.0):
    """Cumulative deposition time per layer (waam_from_stl_v7_mm.py:458-471): the layer's mean cross-section divided by
    the bead width gives the track length, the scan speed its duration.  One reduction over the mask for all plane
    areas; the floating-point operations per layer are the reference's (count*dx*dx, mean, running sum), so the times
    are bit-identical."""
    areas = np.asarray(mask_full).sum(axis=(0, 1)).astype(np.float64) * dx * dx
    bw, v, eta = max(bead_width, 1e-12), max(scan_speed, 1e-12), max(eta_fill, 1.0)
    dur = [float(np.mean(areas[ks:ke + 1])) / bw * eta / v for ks, ke in layers]
    return [float(t) for t in np.cumsum(np.asarray(dur, dtype=np.float64))] if dur else []


def layer_birth_schedule(times_birth, times_out):
    """The clock of the reference's event loop (waam_from_stl_v7_mm.py:515-550) as a stream of actions, in its order:
         ('advance', seconds)   integrate the field over this interval (the consumer splits it into sub-steps under its
                                time-step cap and skips it while nothing is active, :524-528)
         ('birth', layer)       activate layer number `layer` (:487-495) and rebuild the packs (:534)
         ('frame', t)           an output time has been reached (:540-548)
    Between two consecutive event times every birth that is due is taken first, each preceded by the time that has passed
    since the previous action; intervals of at most 1e-15 s are dropped, output times are matched to 1e-12 s -- the
    reference's tolerances.  One schedule drives the single-domain loop and the per-rank slab loop alike."""
    nb = len(times_birth)
    nxt, t_now = 0, 0.0
    for te in sorted(set(times_out) | set(times_birth)):
        while nxt < nb and times_birth[nxt] <= te + 1e-15:
            t_b = times_birth[nxt]
            if t_b - t_now > 1e-15:
                yield ('advance', t_b - t_now)
            t_now = t_b
            yield ('birth', nxt)
            nxt += 1
        if te - t_now > 1e-15:
            yield ('advance', te - t_now)
        t_now = te
        if any(abs(te - to) <= 1e-12 for to in times_out):
            yield ('frame', te)


GRAPH_MIN_NSUB = 16      # segments at least this long run through StagedStepper.run (graph capture costs about a step)


def history_result(hist):
    """what the loops return of a ThermalHistory: T_peak, cooling_time, t_hi, t_lo as NumPy arrays (NaN off the mask and where
    it never happened) and melt_pool(), the log of the run"""
    return dict(T_peak=np.asarray(hist.T_peak), cooling_time=np.asarray(hist.cooling_time), t_hi=np.asarray(hist.t_hi),
                t_lo=np.asarray(hist.t_lo), melt_pool=hist.melt_pool())


def solidification_result(rec):
    """what the loops return of a SolidificationRecord: t_solid, cooling_rate, G and R as NumPy arrays (NaN off the mask and
    where the cell never froze; G = sqrt(g2) and R = cooling_rate / G formed here, R = inf where G = 0)"""
    rate = np.asarray(rec.cooling_rate)
    with np.errstate(divide='ignore', invalid='ignore'):
        G = np.sqrt(np.asarray(rec.g2))
        R = rate / G
    return dict(t_solid=np.asarray(rec.t_solid), cooling_rate=rate, G=G, R=R)


def monitor_result(mon, mat):
    """what the loops return of a FieldMonitor, two values: traces() and region_log(mat)"""
    return mon.traces(), mon.region_log(mat)


def _is_device_backend(backend):
    return hasattr(backend, 'to_device')


def _require_device_loop(who, backend, dev_loop, classes=None, **asked):
    """ValueError for an option (name = value) that is set where the loop cannot serve it.  classes: {option: the backend's
    class that serves it} where that is not the Cartesian one"""
    for name, cls in (('surface_loss', 'LossPacks'), ('phase_change', 'PhaseField'), ('history', 'ThermalHistory'),
                      ('material_law', 'NonlinearPacks'), ('solidification', 'SolidificationRecord'),
                      ('monitor', 'FieldMonitor'), ('material_map', 'MaterialMap')):
        cls = (classes or {}).get(name, cls)
        if asked.get(name) is not None and not (dev_loop and hasattr(backend, cls)):
            raise ValueError("%s: %s needs the device loop of a backend with %s" % (who, name, cls))


class _LoopExtras:
    """The bookkeeping of the optional parts that live through a device loop, once for the three run_* loops: the PhaseField
    (`ph`), the ThermalHistory (`hist`), the SolidificationRecord (`sol`) and the FieldMonitor (`mon`) of the backend, each None
    when its option is.  T: the field they are seeded from (phase_T: the PhaseField's; None seeds nothing, all solid); rows: the
    capacity of the history's log and the monitor's; t: where their clocks start.
    mm: the loop's MaterialMap (None: one material).  With it `phase_change` is a sequence of PhaseChange / None per material and
    `ph` a MapPhaseField, the monitor is built with material_map=mm (its region_log reports sum_wT), and step_kw carries
    material_map=mm."""

    def __init__(self, backend, grid, mat, T, rows=1, t=0.0, phase_T=None, phase_change=None, history=None, solidification=None,
                 monitor=None, mm=None):
        self.mat, self.mm = mat, mm
        self.ph = self.hist = self.sol = self.mon = None
        if phase_change is not None and mm is not None:
            self.ph = backend.MapPhaseField(mm, phase_change, T=phase_T)
        elif phase_change is not None:
            self.ph = backend.PhaseField(grid, mat, phase_change, T=phase_T)
        if history is not None:
            self.hist = backend.ThermalHistory(grid, history, capacity=rows, T=T, t=t)
        if solidification is not None:
            self.sol = backend.SolidificationRecord(grid, solidification, T=T, t=t)
        if monitor is not None:                        # (a dict of FieldMonitor's keywords; the capacity is the run's)
            more = {} if mm is None else {'material_map': mm}
            self.mon = backend.FieldMonitor(grid, **dict(dict({'t': t}, **monitor), capacity=max(1, int(rows)), **more))

    def step_kw(self, surface_loss=None, material=None):
        """the keywords of a step / a stepper for the parts that are present, with the loop's LossPacks or NonlinearPacks"""
        return {k: v for k, v in (('surface_loss', surface_loss), ('phase', self.ph), ('history', self.hist),
                                  ('material', material), ('solidification', self.sol), ('monitor', self.mon),
                                  ('material_map', self.mm)) if v is not None}

    def sync(self, T):
        """after a birth / a new column / a deposit: the newborn cells at f_eq(T), at T_peak = T and "never froze" (cells born
        above T_freeze set their brick's word); the monitor is stateless"""
        for x in (self.ph, self.hist, self.sol):
            if x is not None:
                x.sync_mask(T)

    def idle(self, seconds):
        """an interval without a step: the global time moves on all the same"""
        for x in (self.hist, self.sol, self.mon):
            if x is not None:
                x.t = x.t + seconds

    def results(self):
        """what a loop's return value ends with, for the parts that are present: the liquid fraction, history_result,
        solidification_result, the two of monitor_result"""
        res = () if self.ph is None else (np.asarray(self.ph.liquid_fraction),)
        res = res if self.hist is None else res + (history_result(self.hist),)
        res = res if self.sol is None else res + (solidification_result(self.sol),)
        return res if self.mon is None else res + monitor_result(self.mon, self.mat)


MAP_DOC = """material_map (a dict; device loop only): several materials in one grid -- materials=[(rho, cp, k), ...] and ids= (uint8,
    the full shape, the id of every cell the run can activate; EVERY id must name a material, off the final shape too).  The loop
    builds one MaterialMap, with robin_h from the scalar `h` unless surface_loss is given, and passes material_map= to every step and
    stepper; the step's material is materials[0] (mat_args is not used).  surface_loss may then be one SurfaceLoss or a sequence
    per material (a MapLossPacks), phase_change is a sequence of PhaseChange / None per material (a MapPhaseField, newborn cells
    seeded by sync_mask); history, solidification and monitor run as without it, the monitor's region_log reports sum_wT.  Not
    together with material_law (ValueError).  None: the loop without it, unchanged."""


def _loop_map(who, backend, grid, material_map, h, Tinf, surface_loss, material_law=None, keys=('materials', 'ids')):
    """the MaterialMap of a device loop and its MapLossPacks (None without surface_loss) from the `material_map` dict"""
    if material_law is not None:
        raise ValueError("%s: material_map cannot be combined with material_law (k(T) and cp(T) per material are not served)" % who)
    if not isinstance(material_map, dict) or set(material_map) != set(keys):
        raise ValueError("%s: material_map must be a dict with the keys %s" % (who, ', '.join(keys)))
    robin = None if surface_loss is not None else {f: h for f in ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')}
    mm = backend.MaterialMap(grid, material_map['materials'], np.asarray(material_map['ids']), robin_h=robin)
    return mm, (None if surface_loss is None else backend.MapLossPacks(mm, surface_loss, Tinf))


def _step(backend, T, grid, mat, params, packs, Tinf):
    fn = getattr(backend, 'adi_step_hip_coeff', None) or backend.adi_step_numba_coeff
    return fn(T, grid, mat, params, packs, Tinf=Tinf)


def _birth(backend, T, grid, newborn, Ts):
    """T[newborn] = Ts (waam_from_stl_v7_mm.py:489-493)"""
    if _is_device_backend(backend) and hasattr(T, 'fill_where'):
        import torch
        T.fill_where(grid.layout.to_layout(newborn, torch.uint8), Ts)
    else:
        T[newborn] = Ts
    return T


def run_layer_birth(backend, mask_full, dx, mat_args, h, Tinf, Ts, theta, cfl, layers, times_birth, times_out,
                    on_frame=None, device_resident=True, device_loop=True, surface_loss=None, phase_change=None, history=None,
                    solidification=None, monitor=None, material_map=None):
    """The event loop of waam_from_stl_v7_mm.py:515-550.  Returns (T_final as NumPy, number of ADI steps).
    material_map: see waam.MAP_DOC -- mask_full may then hold several materials (a plate and a part): after a birth the map's
    packs are rewritten on the planes that changed (MaterialMap.update), nothing is read back; the time-step cap is taken with the
    largest diffusivity among the materials.
    surface_loss (a SurfaceLoss of the backend): the surface loses heat by that law, evaluated at the temperature at the start
    of every sub-step, in place of the constant `h` (which is then not used); device loop only.  None: the reference's loop.
    phase_change (a PhaseChange of the backend): latent heat of melting and freezing; one PhaseField lives through the run, every
    sub-step ends with its correction, newborn cells are seeded at f_eq(Ts); device loop only.  The return value is then
    (T_final, number of ADI steps, final liquid fraction as NumPy).  None: the loop without it, unchanged.
    history (a HistoryLevels of the backend): peak temperature, cooling time and melt pool; one ThermalHistory lives through the
    run, sized from the schedule, every sub-step is recorded at the global time (which runs through the recorder's clock, idle
    intervals included), newborn cells are seeded at Ts; device loop only.  The return value gains a last element, the result
    dict of history_result.  None: the loop without it, unchanged.
    solidification (T_freeze, a number): the conditions at the freezing front; one SolidificationRecord of the backend lives
    through the run on the global time like the history, and sync_mask(T) follows every birth; device loop only.  The return
    value gains a last element (after history's), the dict of solidification_result.  None: the loop without it, unchanged.
    monitor (a dict of FieldMonitor's keyword arguments: probes, regions, extra): one FieldMonitor of the backend lives through
    the run, sized from the schedule like the history, on the global time; stateless, so a birth needs no call; device loop
    only.  The return value gains two last elements, its traces() and region_log(mat).  None: the loop without it, unchanged."""
    nx, ny, nz = mask_full.shape
    mask_act = np.zeros_like(mask_full, dtype=bool)
    grid = backend.Grid3D(nx, ny, nz, dx, mask_act)
    mat = backend.Material(*mat_args)
    params = backend.Params(dt=1e-3, theta=theta)
    alpha = mat_args[2] / (mat_args[0] * mat_args[1])
    if isinstance(material_map, dict) and 'materials' in material_map:
        alpha = max(float(k) / (float(rho) * float(cp)) for rho, cp, k in material_map['materials'])
    dt_cap = cfl * dx * dx / alpha
    T = np.full((nx, ny, nz), float(Tinf), dtype=np.float64)
    if device_resident and _is_device_backend(backend):
        T = backend.to_device(T)
    robin = {f: h for f in ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')}
    mm = None

    def build_packs():
        return backend.precompute_coeff_packs_unified(grid, mat, dir_mask=None, dir_value=None, neumann=None,
                                                      robin_h=robin, robin_Tinf=Tinf)
    packs = None
    nsteps = 0

    def advance(seg):
        nonlocal T, nsteps
        nsub = max(1, int(math.ceil(seg / dt_cap)))
        params.dt = max(seg / nsub, 1e-15)
        kw = ex.step_kw(surface_loss=None if surface_loss is None else bpacks)
        if nsub >= GRAPH_MIN_NSUB and hasattr(backend, 'StagedStepper') and hasattr(T, 'fill_where'):
            # a long segment on the device backend: the nsub launches of this segment replayed from a HIP graph
            T = backend.StagedStepper(grid, mat, params, packs, Tinf, **kw).run(T, nsub)
        elif kw:
            for _ in range(nsub):
                T = backend.adi_step_numba_coeff(T, grid, mat, params, packs, Tinf=Tinf, **kw)
        else:
            for _ in range(nsub):
                T = _step(backend, T, grid, mat, params, packs, Tinf)
        nsteps += nsub

    # device loop: the full mask, the active mask, the field and the packs live in HBM.  A birth
    # is ONE kernel on the layer's planes (newborn = full & ~active, T[newborn] = Ts, active |= full: adi_birth_planes),
    # then the flags and the six coefficient arrays are rebuilt on the planes whose exposure can have changed (the layer
    # and one plane either side) -- in place, no allocation, no host synchronisation: nothing crosses PCIe between
    # output times and nothing waits for the device between births
    dev_loop = device_loop and device_resident and hasattr(backend, 'BirthPacks') and hasattr(T, 'fill_where')
    _require_device_loop('run_layer_birth', backend, dev_loop, surface_loss=surface_loss, phase_change=phase_change,
                         history=history, solidification=solidification, monitor=monitor, material_map=material_map)
    ex = _LoopExtras(backend, grid, mat, T)                            # (nothing was asked for where there is no device loop)
    if dev_loop:
        import torch
        d_full = grid.layout.to_layout(mask_full, torch.uint8)
        d_act = grid.layout.empty(torch.uint8, zero=True)
        grid.set_mask_device(d_act, all_solid=False)
        # (with a surface loss: LossPacks, whose coefficients follow the field -- `update` ahead of every sub-step, inside the
        # step; `rebuild` on the planes a birth changed)
        if material_map is not None:
            # several materials: the map's own packs, rewritten on the planes a birth changed (MaterialMap.update); its
            # MapLossPacks needs no call of its own there -- update leaves zeros and the step's loss update writes the exposed cells
            mm, bpacks = _loop_map('run_layer_birth', backend, grid, material_map, h, Tinf, surface_loss)
            mat, packs = mm.mat, mm.packs
        else:
            bpacks = backend.BirthPacks(grid, mat, robin_h=robin) if surface_loss is None else \
                backend.LossPacks(grid, mat, surface_loss, Tinf)
            packs = bpacks.packs
        plane_cells = np.asarray(mask_full).sum(axis=(0, 1)).astype(np.int64)      # newborn cells per plane, host-known
        plane_born = np.zeros(nz, dtype=bool)
        rows = 1
        if history is not None or monitor is not None:                 # one log row per sub-step the schedule can ask for
            rows = max(1, sum(max(1, int(math.ceil(a / dt_cap))) for w, a in layer_birth_schedule(times_birth, times_out)
                              if w == 'advance'))
        # (the PhaseField unseeded: nothing is active yet, all solid)
        ex = _LoopExtras(backend, grid, mat, T, rows, phase_change=phase_change, history=history, solidification=solidification,
                         monitor=monitor, mm=mm)
    else:
        packs = build_packs()
    n_active = 0

    def birth(ks, ke):
        nonlocal T, packs, n_active
        if dev_loop:
            backend.birth_planes(T, d_act, d_full, grid, ks, ke + 1, Ts)          # :489-493 + mask_act |= born
            fresh = ~plane_born[ks:ke + 1]
            n_active += int(plane_cells[ks:ke + 1][fresh].sum())
            plane_born[ks:ke + 1] = True
            grid.set_mask_device(d_act, ks - 1 if ks > 0 else 0, min(nz, ke + 2), all_solid=False)   # :494-495
            if mm is not None:
                packs = mm.update(ks - 1, ke + 2)
            elif surface_loss is None:
                packs = bpacks.update(ks - 1, ke + 2)                             # :534, the planes that changed
            else:
                packs = bpacks.rebuild(T, ks - 1, ke + 2)
            ex.sync(T)
            return
        born = np.zeros_like(mask_full, dtype=bool)
        born[:, :, ks:ke + 1] = mask_full[:, :, ks:ke + 1]
        newborn = born & (~mask_act)
        if newborn.any():
            T = _birth(backend, T, grid, newborn, Ts)
        mask_act[...] = mask_act | born
        n_active = int(mask_act.sum())
        grid.mask = mask_act                           # :494-495
        packs = build_packs()                          # :534

    for what, arg in layer_birth_schedule(times_birth, times_out):
        if what == 'advance':
            if n_active > 0:                           # no ADI steps while nothing is active (:524)
                advance(arg)
            else:
                ex.idle(arg)
        elif what == 'birth':
            birth(*layers[arg])
        elif on_frame is not None:
            on_frame(arg, np.asarray(T), d_act.cpu().contiguous().numpy().astype(bool) if dev_loop else mask_act.copy())
    return (np.asarray(T), nsteps) + ex.results()


def track_source(heat_source, track_box, dx, yi, t_step):
    """the heat source of column yi of run_single_track: `heat_source`'s power, efficiency and shape, its centre on the top
    of the column at the column's start -- ((x0 + x1)/2 dx, (yi + 1/2) dx, z1 dx) -- travelling along +axis 1 at
    dx / t_step, depth along axis 2; time counts from the start of the column"""
    x0, x1, z0, z1, _ = track_box
    s = heat_source
    return type(s)(s.power, s.eta, s.a, s.b, s.c_f, s.c_r, f_f=s.f_f,
                   origin=(0.5 * (x0 + x1) * dx, (yi + 0.5) * dx, z1 * dx), velocity=dx / t_step,
                   travel_axis=1, travel_sign=1, depth_axis=2)


def run_single_track(backend, plate_mask, track_box, dx, mat_args, h, Tinf, T_track, theta, dt, t_step,
                     device_resident=True, heat_source=None, surface_loss=None, phase_change=None, history=None,
                     material_law=None, solidification=None, monitor=None, material_map=None):
    """single_track_on_plate.py:150-177: the deposit advances one column per t_step along axis 1; packs are
    rebuilt after every column.  track_box = (x0, x1, z0, z1, n_columns).
    material_map: see waam.MAP_DOC -- e.g. a track of one alloy on a plate of another: the map's packs are rebuilt in full after
    every column (MaterialMap.rebuild, the shape of this loop), `heat_source` becomes a MapSource of the map, and columns of at
    least GRAPH_MIN_NSUB sub-steps are replayed from a HIP graph.
    heat_source (a GoldakSource of the backend): the arc / laser as a moving volumetric source (track_source) during the
    sub-steps of every column, on top of the newborn cells set to T_track.  None: the reference's driver, unchanged.
    surface_loss (a SurfaceLoss of the backend): the surface loses heat by that law, evaluated at the temperature at the start
    of every sub-step, in place of the constant `h`; device loop only; columns of at least GRAPH_MIN_NSUB sub-steps are
    replayed from a HIP graph.  None: the constant-h packs, unchanged.
    phase_change (a PhaseChange of the backend): latent heat of melting and freezing; one PhaseField lives through the run, every
    sub-step ends with its correction, the cells of a new column are seeded at f_eq(T_track); device loop only.  The return
    value is then (T_final, final liquid fraction), both NumPy.  None: the loop without it, unchanged.
    history (a HistoryLevels of the backend): peak temperature, cooling time and melt pool; one ThermalHistory lives through the
    run, sized from the schedule, every sub-step is recorded at the global time (the recorder's clock; the source's time still
    counts from the start of each column), the cells of a new column are seeded at T_track; device loop only.  The return
    value gains a last element, the result dict of history_result.  None: the loop without it, unchanged.  With a recorder the
    track box must not overlap the plate: T_track is written onto the whole box but only newborn cells are seeded (ValueError).
    material_law (a MaterialLaw of the backend): temperature-dependent k(T) and cp(T), with the law's latent heat; one
    NonlinearPacks lives through the run and is rebuilt after every column.  rho comes from mat_args, whose cp and k are not
    used; the scalar `h` becomes SurfaceLoss(h=h) unless surface_loss is given; device loop only; not together with
    phase_change (ValueError).  None: the loop without it, unchanged.
    solidification (T_freeze, a number): the conditions at the freezing front; one SolidificationRecord of the backend lives
    through the run on the global time like the history, and sync_mask(T) follows every column; device loop only; the track
    box must not overlap the plate either.  The return value gains a last element (after history's), the dict of
    solidification_result.  None: the loop without it, unchanged.
    monitor (a dict of FieldMonitor's keyword arguments: probes, regions, extra): one FieldMonitor of the backend lives through
    the run, one log row per sub-step, on the global time; stateless, so a new column needs no call; device loop only.  The
    return value gains two last elements, its traces() and region_log(mat).  None: the loop without it, unchanged."""
    x0, x1, z0, z1, ncol = track_box
    if material_law is not None and phase_change is not None:
        raise ValueError("run_single_track: phase_change cannot be combined with material_law (the MaterialLaw carries the "
                         "latent heat)")
    if (history is not None or solidification is not None) and np.asarray(plate_mask)[x0:x1, :ncol, z0:z1].any():
        n = int(np.asarray(plate_mask)[x0:x1, :ncol, z0:z1].sum())
        raise ValueError("run_single_track: the track box [%d:%d, 0:%d, %d:%d] overlaps the plate in %d cells; T_track is written "
                         "onto those live cells without a seed, so the history / solidification recorder would miss it (a peak below the field, "
                         "crossings skipped)" % (x0, x1, ncol, z0, z1, n))
    nx, ny, nz = plate_mask.shape
    mask = plate_mask.copy()
    grid = backend.Grid3D(nx, ny, nz, dx, mask)
    mat = backend.Material(*mat_args)
    params = backend.Params(dt=dt, theta=theta)
    T = np.full((nx, ny, nz), float(Tinf), dtype=np.float64)
    if device_resident and _is_device_backend(backend):
        T = backend.to_device(T)
    robin = {f: h for f in ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')}
    dev_loop = device_resident and hasattr(grid, 'set_mask_device') and hasattr(T, 'fill_where')
    _require_device_loop('run_single_track', backend, dev_loop, surface_loss=surface_loss, phase_change=phase_change,
                         history=history, material_law=material_law, solidification=solidification, monitor=monitor,
                         material_map=material_map)
    if dev_loop:                                    # the mask lives in HBM: a new column is two slice assignments
        import torch
        d_mask = grid.layout.to_layout(mask, torch.uint8)
    nm = mm = None
    if material_map is not None:
        mm, maploss = _loop_map('run_single_track', backend, grid, material_map, h, Tinf, surface_loss, material_law)
        mat = mm.mat
    if material_law is not None:
        nm = backend.NonlinearPacks(grid, mat.rho, material_law, Tinf,
                                    loss=surface_loss if surface_loss is not None else backend.SurfaceLoss(h=h))
        mat = nm.mat
    lpacks = backend.LossPacks(grid, mat, surface_loss, Tinf) if surface_loss is not None and nm is None and mm is None else None
    ex = _LoopExtras(backend, grid, mat, T, ncol * max(1, int(math.ceil(t_step / dt))), phase_T=T, phase_change=phase_change,
                     history=history, solidification=solidification, monitor=monitor, mm=mm)
    kw = ex.step_kw(surface_loss=lpacks if mm is None else maploss, material=nm)
    for yi in range(ncol):
        if dev_loop:
            d_mask[x0:x1, yi:yi + 1, z0:z1] = 1
            grid.set_mask_device(d_mask)
        else:
            mask[x0:x1, yi:yi + 1, z0:z1] = True
            grid.mask = mask
        if mm is not None:
            mm.rebuild()                            # (its MapLossPacks needs no call: rebuild left zeros, the step writes the rest)
            packs = mm.packs
        elif lpacks is None and nm is None:
            packs = backend.precompute_coeff_packs_unified(grid, mat, robin_h=robin, robin_Tinf=Tinf)
        T[x0:x1, yi:yi + 1, z0:z1] = T_track
        if lpacks is not None or nm is not None:
            packs = (nm or lpacks).rebuild(T)        # the column changed the exposure: every cell, stale ones zeroed
        ex.sync(T)
        n_sub = max(1, int(math.ceil(t_step / dt)))
        dt_orig = params.dt
        params.dt = t_step / n_sub
        if kw:
            src = None if heat_source is None else track_source(heat_source, track_box, dx, yi, t_step)
            if src is not None and mm is not None:
                src = backend.MapSource(mm, src)
            if n_sub >= GRAPH_MIN_NSUB:
                T = backend.StagedStepper(grid, mat, params, packs, Tinf, source=src, **kw).run(T, n_sub, t0=0.0)
            else:
                for i in range(n_sub):
                    T = backend.adi_step_numba_coeff(T, grid, mat, params, packs, Tinf=Tinf, S=src, t=i * params.dt, **kw)
        elif heat_source is None:
            for _ in range(n_sub):
                T = _step(backend, T, grid, mat, params, packs, Tinf)
        else:
            src = track_source(heat_source, track_box, dx, yi, t_step)
            for i in range(n_sub):
                T = backend.adi_step_numba_coeff(T, grid, mat, params, packs, Tinf=Tinf, S=src, t=i * params.dt)
        params.dt = dt_orig
    res = (np.asarray(T),) + ex.results()
    return res if len(res) > 1 else res[0]


def path_steps(t_start, t_end, dt):
    """the steps [(t, dt_n)] of run_path_deposition: from t_start in steps of dt, the last one shortened to end at t_end, the
    time accumulated as t = t + dt_n"""
    steps, t = [], float(t_start)
    while t < t_end:
        d = dt if t + dt <= t_end else t_end - t
        if not t + d > t:
            break
        steps.append((t, d))
        t = t + d
    return steps


def run_path_deposition(backend, base_mask, path, bead, dx, mat_args, h, Tinf, Ts, theta, dt, t_end=None, within=None,
                        heat=False, surface_loss=None, phase_change=None, history=None, solidification=None, on_frame=None,
                        monitor=None, material_map=None):
    """Material laid along a scan path, bead by bead (README, "Deposition along a path"): from path.t_start to t_end (default
    path.t_end) in steps of dt (path_steps), every step preceded by the births of its interval -- the bead of the step [t, t + dt]
    is born at the step's start, at Ts, on top of `base_mask` (the plate; may be empty).  Device loop only: mask, field and packs
    live in HBM, a deposit is one kernel on the bead's index box (backend.PathDeposit.deposit) and the rebuild of flags, bricks
    and packs on the planes it can have changed; nothing is read back between frames.  No ADI step is taken while the base mask
    is empty and no segment has deposited yet (known from the path on the host).
    path: a ScanPath or ScanPathSource of the backend; bead: a BeadProfile; within: optional bool array, the part's final
    shape -- no cell outside it is born.
    heat: True -- every step also takes the path's step-averaged heat input, S=path.sample_step_device(grid, t, dt), so the same
    path heats what it lays; False -- the reference's kind of deposit, newborn cells at Ts and nothing else.
    surface_loss, phase_change, history, solidification: as in run_single_track -- the newborn cells of a step are seeded at
    f_eq(Ts) / Ts / "never froze", the recorders run on the global time, from path.t_start, and the history's log holds one row
    per step.
    monitor: as in run_single_track -- one FieldMonitor, one log row per step, its clock from path.t_start; a deposit needs no call.
    material_map: see waam.MAP_DOC, with one more key, wire=m: the id of what the path lays -- a wire of one alloy on a base plate
    of another.  Every deposit writes m into the map's device id field on its newborn cells (PathDeposit(material_map=,
    material_id=)) and the map's packs are rewritten on the planes it changed (MaterialMap.update); nothing is read back.
    With heat=True the path enters the map's step itself, S=backend.MapPathSource(mm, path): added to the explicit stage's
    output on the window's index box, bit for bit what the field gives, without the field.
    on_frame(t, T, active): called after every step with the time reached and NumPy copies (a download; None: none).
    Returns (T_final, active mask, number of ADI steps), all host side, then the final liquid fraction, history_result and
    solidification_result for those that were asked for, in this order, then the monitor's traces() and region_log(mat)."""
    nx, ny, nz = base_mask.shape
    grid = backend.Grid3D(nx, ny, nz, dx, np.array(base_mask, dtype=bool))
    mat = backend.Material(*mat_args)
    params = backend.Params(dt=dt, theta=theta)
    T = np.full((nx, ny, nz), float(Tinf), dtype=np.float64)
    if _is_device_backend(backend):
        T = backend.to_device(T)
    dev_loop = hasattr(backend, 'PathDeposit') and hasattr(backend, 'BirthPacks') and hasattr(T, 'fill_where')
    if not dev_loop:
        raise ValueError("run_path_deposition: needs the device loop of a backend with PathDeposit")
    _require_device_loop('run_path_deposition', backend, dev_loop, surface_loss=surface_loss, phase_change=phase_change,
                         history=history, solidification=solidification, monitor=monitor, material_map=material_map)
    src = path.on_device() if hasattr(path, 'on_device') else path
    steps = path_steps(src.t_start, src.t_end if t_end is None else float(t_end), float(dt))
    robin = {f: h for f in ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')}
    mm = None
    if material_map is not None:
        mm, bpacks = _loop_map('run_path_deposition', backend, grid, material_map, h, Tinf, surface_loss,
                               keys=('materials', 'ids', 'wire'))
        dep = backend.PathDeposit(grid, src, bead, Ts, within=within, material_map=mm, material_id=material_map['wire'])
        mat, packs = mm.mat, mm.packs
        msrc = backend.MapPathSource(mm, src) if heat else None
    else:
        dep = backend.PathDeposit(grid, src, bead, Ts, within=within)
        bpacks = backend.BirthPacks(grid, mat, robin_h=robin) if surface_loss is None else \
            backend.LossPacks(grid, mat, surface_loss, Tinf)
        packs = bpacks.packs
    ex = _LoopExtras(backend, grid, mat, T, max(1, len(steps)), t=src.t_start, phase_T=T, phase_change=phase_change,
                     history=history, solidification=solidification, monitor=monitor, mm=mm)
    kw = ex.step_kw(surface_loss=None if surface_loss is None else bpacks)
    live = bool(np.asarray(base_mask).any())
    nsteps = 0
    for t, d in steps:
        rng = dep.deposit(T, t, d)
        if rng is not None:                            # something could have been born: the planes that changed
            if mm is not None:
                packs = mm.update(*rng)
            else:
                packs = bpacks.update(*rng) if surface_loss is None else bpacks.rebuild(T, *rng)
            ex.sync(T)
            live = True
        if live:
            params.dt = d
            S = None if not heat else (msrc if mm is not None else src.sample_step_device(grid, t, d))
            T = backend.adi_step_numba_coeff(T, grid, mat, params, packs, Tinf=Tinf, S=S, t=t, **kw)
            nsteps += 1
        else:
            ex.idle(d)
        if on_frame is not None:
            on_frame(t + d, np.asarray(T), grid.d_mask.cpu().contiguous().numpy().astype(bool))
    return (np.asarray(T), grid.d_mask.cpu().contiguous().numpy().astype(bool), nsteps) + ex.results()


def ring_source(heat_source, R_in, wall, z_top, tau):
    """the heat source of one ring of run_spiral_deposition: `heat_source`'s power, efficiency and shape, its centre on the
    nozzle -- mid-wall radius R_in + wall/2, angle 0 at t = 0 turning at 2 pi / tau, height z_top (the top of the ring being
    deposited), no axial travel"""
    s = heat_source
    return type(s)(s.power, s.eta, s.a, s.b, s.c_f, s.c_r, f_f=s.f_f, r_c=R_in + 0.5 * wall, phi0=0.0,
                   omega=2.0 * math.pi / tau, z0=z_top, v_z=0.0, depth=s.depth)


def run_spiral_deposition(backend, times, mat_args, Tinf, Tdep, R_in, wall, h_side, h_end, z_back, layer_h, n_layers, tau,
                          nr, nphi, heat_source=None, device_resident=True, phase_change=None, history=None, monitor=None,
                          solidification=None):
    """The ring-by-ring deposition loop of quick_spiral_deposition_gif_v5.py on an annular wall (R_in, R_in + wall): one
    z-cell per layer, nphi cells per turn, dt = tau / nphi, BE.  Before each step the arc swept during it is activated at Tdep
    in whole radial columns, then adi_step_masked advances the field (Robin h_side on the outer wall, neumann0 below, Robin
    h_end on top; voids and the inner row clamped to Tinf).  mat_args = dict(rho=, cp=, k=).
    heat_source (a CylGoldakSource of the backend): the arc as a moving volumetric source on the ring being deposited
    (ring_source; the ring's top z, a new one when a layer completes), on active cells, during the steps that deposit; None:
    the reference's loop.  With a device backend and device_resident, T and the active mask stay in HBM and an arc's
    activation is two slice assignments.  Returns (grid, fields, masks): NumPy (nr, nphi, nz) fields and masks at `times`.
    phase_change (a PhaseChange) / history (HistoryLevels): latent heat and the thermal history, device loop only.  One
    CylPhaseField / CylThermalHistory of the backend lives through the run (the log holds one row per step) and goes to every
    adi_step_masked; a newborn column is seeded by the step that first sees it active, so an activation needs no call.  Then
    the liquid fraction (NumPy, 0 where never active) and / or history_result's dict follow the three usual values.
    monitor (dict(probes=, regions=, extra_f=False)): a CylFieldMonitor of the backend, device loop only, one through the run
    on the global time with one row per step; extra_f=True needs phase_change and sums the phase field's f as `extra`.  Its
    traces() and region_log(mat) follow the values above.
    solidification (T_freeze): the conditions at the freezing front, device loop only.  One CylSolidificationRecord of the
    backend lives through the run on the global time with one log row per step and goes to every adi_step_masked; a birth
    needs no call.  After the liquid fraction and the history's dict, and before the monitor's two values, follows the dict of
    solidification_result with `front`, the record's front() log, added."""
    dr = wall / nr
    nz = int(round((z_back + layer_h * n_layers) / layer_h))
    grid = backend.GridCyl(nr, nphi, nz, dr, 2.0 * math.pi / nphi, layer_h, R_in + wall, R_in=R_in)
    m = backend.Material(mat_args['rho'], mat_args['cp'], mat_args['k'])
    wall_bc = backend.RobinR(h_side, Tinf)
    zbc = backend.ZBC(kind_bot='neumann0', kind_top='robin', h_top=h_end, T_inf_top=Tinf)
    iz0 = int(round(z_back / layer_h))
    T = np.full((nr, nphi, nz), float(Tinf))
    active = np.zeros((nr, nphi, nz), bool)
    active[:, :, :iz0] = True
    dev = device_resident and _is_device_backend(backend)
    _require_device_loop('run_spiral_deposition', backend, dev,
                         classes=dict(phase_change='CylPhaseField', history='CylThermalHistory', monitor='CylFieldMonitor',
                                      solidification='CylSolidificationRecord'),
                         phase_change=phase_change, history=history, monitor=monitor, solidification=solidification)
    ph = hist = mon = sol = None
    if phase_change is not None:
        ph = backend.CylPhaseField(grid, m, phase_change, active=active)
    if history is not None or monitor is not None or solidification is not None:
        rows, tt = 0, 0.0
        for t_goal in times:                      # the steps of the loop below, counted with its own arithmetic
            while tt < t_goal - 1e-12:
                tt = min(tt + tau / nphi, t_goal)
                rows += 1
    if history is not None:
        hist = backend.CylThermalHistory(grid, history, capacity=max(1, rows), T=T, t=0.0, active=active)
    if monitor is not None:
        extra_f = bool(monitor.get('extra_f', False))
        if extra_f and ph is None:
            raise ValueError("run_spiral_deposition: monitor extra_f=True needs phase_change")
        mon = backend.CylFieldMonitor(grid, probes=monitor.get('probes', ()), regions=monitor.get('regions', ()),
                                      capacity=max(1, rows), extra=ph.f if extra_f else None, t=0.0)
    if solidification is not None:
        sol = backend.CylSolidificationRecord(grid, solidification, capacity=max(1, rows), t=0.0)
    extras = {k: v for k, v in (('phase', ph), ('history', hist), ('monitor', mon), ('solidification', sol)) if v is not None}
    if dev:                                       # T and the mask in HBM: an activation is two slice assignments
        import torch
        T = grid.layout.to_layout(T, torch.float64)           # (a native-layout tensor in, a tensor out of every step)
        active = grid.layout.to_layout(active, torch.uint8)
    dt, omega = tau / nphi, 2.0 * math.pi / tau
    prm = backend.Params(dt, 1.0, "be")
    layer, angle, t = 0, 0.0, 0.0
    fields, masks = [], []
    for t_goal in times:
        while t < t_goal - 1e-12:
            t_next = min(t + dt, t_goal)
            left = omega * (t_next - t)
            src = None
            if heat_source is not None and layer < n_layers and 0 <= iz0 + layer < nz:
                src = ring_source(heat_source, R_in, wall, (iz0 + layer + 1) * layer_h, tau)
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
                                T[:, c % nphi, iz] = Tdep
                    angle += seg
                    left -= seg
                if angle >= 2.0 * math.pi - 1e-15:
                    angle = 0.0
                    layer += 1
                    if iz0 + layer > nz - 1:
                        layer = n_layers
            prm.dt = t_next - t
            if src is None:
                T = backend.adi_step_masked(T, grid, m, prm, wall_bc, zbc, active, robin_inner=wall_bc, robin_void=wall_bc,
                                            **extras)
            else:
                T = backend.adi_step_masked(T, grid, m, prm, wall_bc, zbc, active, robin_inner=wall_bc, robin_void=wall_bc,
                                            S=src, t=t, **extras)
            if not dev:
                T = np.asarray(T).copy()
            t = t_next
        if dev:
            fields.append(T.cpu().numpy().copy())
            masks.append(active.cpu().numpy().astype(bool))
        else:
            fields.append(T.copy())
            masks.append(active.copy())
    more = ()
    if ph is not None:
        more += (np.asarray(ph.liquid_fraction),)
    if hist is not None:
        more += (history_result(hist),)
    if sol is not None:
        more += (dict(solidification_result(sol), front=sol.front()),)
    if mon is not None:
        more += (mon.traces(), mon.region_log(m))
    return (grid, fields, masks) + more


def run_layer_birth_slab(comm, i0, i1, mask_full, dx, mat, params_cls, h, Tinf, Ts, theta, cfl, layers, times_birth,
                         times_out, engine=None, on_frame=None):
    """The same event loop on ONE RANK of a slab decomposition (planes [i0, i1) of memory axis 0; BASELINE.json
    configs[4] runs it on 4 GPUs).  Every rank knows the full host mask (bookkeeping only, 1 bit of information per
    cell) and owns the temperature of its slab on its GPU; a birth is a masked fill of the local slab followed by
    SlabStepper.set_mask (mask halo exchange + flags + pack rebuild).  Returns (local field as NumPy, steps)."""
    from . import dist_slab
    nx, ny, nz = mask_full.shape
    mask_act = np.zeros_like(mask_full, dtype=bool)
    params = params_cls(dt=1e-3, theta=theta)
    alpha = mat.k / (mat.rho * mat.cp)
    dt_cap = cfl * dx * dx / alpha
    robin = {f: h for f in ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')}
    st = dist_slab.SlabStepper(mask_act[i0:i1], dx, mat, params, Tinf, robin_h=robin, comm=comm, engine=engine)
    T = np.full((i1 - i0, ny, nz), float(Tinf), dtype=np.float64)
    on_device = getattr(st.engine.device, 'type', 'cpu') == 'cuda'
    if on_device:                                   # the slab's field stays in HBM: step() hands back device tensors
        import torch
        T = torch.from_numpy(T).to(st.engine.device)
    # device loop (as run_layer_birth's): the slab's part of the full mask and its active mask live in HBM; a birth is one
    # kernel on the layer's planes of the slab + SlabStepper.set_mask_device (mask halo planes, flags and packs rebuilt in
    # place on those planes).  The host keeps only per-plane bookkeeping: which planes are born, how many cells are active.
    dev_loop = on_device and st.device_births_supported()
    if dev_loop:
        E = st.engine
        m_ext = np.zeros((i1 - i0 + 2, st.ny, st.nz), dtype=np.bool_)          # (the slab's planes may be padded: st.pad)
        m_ext[1:-1] = st.pad(np.asarray(mask_full[i0:i1], dtype=np.bool_), False)
        d_full_int = st.Lext.to_layout(m_ext, torch.uint8)[1:-1]
        count = torch.zeros(1, dtype=torch.int64, device=E.device)
        plane_cells = np.asarray(mask_full).sum(axis=(0, 1)).astype(np.int64)
        plane_born = np.zeros(nz, dtype=bool)
    n_active = 0
    nsteps = 0

    def advance(seg):
        nonlocal T, nsteps
        nsub = max(1, int(math.ceil(seg / dt_cap)))
        params.dt = max(seg / nsub, 1e-15)
        for s in range(nsub):
            T = st.step(T, prefetch_halo=(s + 1 < nsub))
        nsteps += nsub

    def birth(ks, ke):
        nonlocal T, n_active
        if dev_loop:
            T = st.state_interior(T)                     # the state buffer itself (also when nothing has stepped yet)
            E.birth_planes(st.Lint, T, st.mask_interior(), d_full_int, ks, ke + 1, Ts, count)
            fresh = ~plane_born[ks:ke + 1]
            n_active += int(plane_cells[ks:ke + 1][fresh].sum())
            plane_born[ks:ke + 1] = True
            st.set_mask_device(ks, ke + 1)
            return
        born = np.zeros_like(mask_full, dtype=bool)
        born[:, :, ks:ke + 1] = mask_full[:, :, ks:ke + 1]
        newborn = (born & (~mask_act))[i0:i1]
        if newborn.any():
            if on_device:
                T[torch.from_numpy(newborn).to(T.device)] = Ts      # in place (the last sub-step sent no halo ahead)
            else:
                Tl = np.array(st.local_numpy(T))
                Tl[newborn] = Ts
                T = Tl
        mask_act[...] = mask_act | born
        n_active = int(mask_act.sum())
        st.set_mask(mask_act[i0:i1])

    for what, arg in layer_birth_schedule(times_birth, times_out):
        if what == 'advance':
            if n_active > 0:
                advance(arg)
        elif what == 'birth':
            birth(*layers[arg])
        elif on_frame is not None:
            act = st.mask_interior(logical=True).cpu().contiguous().numpy().astype(bool) if dev_loop \
                else mask_act[i0:i1].copy()
            on_frame(arg, np.array(st.local_numpy(T)), act)
    return np.array(st.local_numpy(T)), nsteps


def run_single_track_slab(comm, i0, i1, plate_mask, track_box, dx, mat, params_cls, h, Tinf, T_track, theta, dt, t_step,
                          engine=None, heat_source=None):
    """The moving deposit of single_track_on_plate.py:150-177 on ONE RANK of a slab decomposition (planes [i0, i1) of
    memory axis 0; BASELINE.json configs[4]: "layer-birth + moving source, 4 GPUs").  The track box spans planes
    [x0, x1) of the SHARDED axis, so a new column lands on every rank whose slab meets that range: those ranks switch
    the column's cells on in their part of the mask and set them to T_track (:159-160, :166), every rank then rebuilds
    flags and packs for its slab -- SlabStepper.set_mask: mask halo exchange (a column next to a slab boundary changes the
    neighbour's halo coupling bits), flags, packs (:163) -- and takes the n_sub sub-steps of the column (:168-176).
    Every rank keeps the full host mask for bookkeeping (1 bit of information per cell), as run_layer_birth_slab does.
    heat_source (a GoldakSource): the arc / laser of run_single_track (track_source, global coordinates) during the sub-steps of
    every column, sub-step i at t = i * dt_sub from the column's start.  None: the loop without it, unchanged.
    Returns the local field as NumPy."""
    from . import dist_slab
    x0, x1, z0, z1, ncol = track_box
    nx, ny, nz = plate_mask.shape
    mask = np.array(plate_mask, dtype=bool)
    params = params_cls(dt=dt, theta=theta)
    robin = {f: h for f in ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')}
    st = dist_slab.SlabStepper(mask[i0:i1], dx, mat, params, Tinf, robin_h=robin, comm=comm, engine=engine)
    T = np.full((i1 - i0, ny, nz), float(Tinf), dtype=np.float64)
    on_device = getattr(st.engine.device, 'type', 'cpu') == 'cuda'
    if on_device:
        import torch
        T = torch.from_numpy(T).to(st.engine.device)
    lx0, lx1 = max(x0, i0) - i0, min(x1, i1) - i0            # the track box inside this slab (empty when lx0 >= lx1)
    dev_loop = on_device and st.device_births_supported()      # the mask stays in HBM: a column is a slice assignment
    for yi in range(ncol):
        if dev_loop:
            if lx0 < lx1:
                st.mask_interior()[lx0:lx1, yi:yi + 1, z0:z1] = 1
            st.set_mask_device(z0, z1)                         # collective: halo planes of the mask, flags and packs in place
        else:
            mask[x0:x1, yi:yi + 1, z0:z1] = True
            st.set_mask(mask[i0:i1])                           # collective: every rank, whether the column touches it or not
        if lx0 < lx1:
            if on_device:
                T[lx0:lx1, yi:yi + 1, z0:z1] = T_track         # in place: the last sub-step sent no halo ahead
            else:
                Tl = np.array(st.local_numpy(T))
                Tl[lx0:lx1, yi:yi + 1, z0:z1] = T_track
                T = Tl
        n_sub = max(1, int(math.ceil(t_step / dt)))
        params.dt = t_step / n_sub
        if heat_source is None:
            for s_ in range(n_sub):
                T = st.step(T, prefetch_halo=(s_ + 1 < n_sub))
        else:
            st.set_source(track_source(heat_source, track_box, dx, yi, t_step))
            for s_ in range(n_sub):
                T = st.step(T, prefetch_halo=(s_ + 1 < n_sub), t=s_ * params.dt)
        params.dt = dt
    return np.array(st.local_numpy(T))
