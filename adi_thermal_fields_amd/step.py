"""The Cartesian ADI step: the stage entry points, the record of the step's optional parts (`StepExtras`) with its checks
(`_check_extras`), THE launch sequence (`_launch_step`), `adi_step_hip_coeff` with the reference's two names for it, and
`StagedStepper`."""
import ctypes

import torch

from . import _lib
from ._lib import lib, check
from ._ledger import PromiseLedger
from .fields import DeviceField, _as_state, _wrap, _p, _stream
from .packs import _fc_arg, MaterialMap, _MapLoss, _MapPhase, _MapSource, _MapPathSource, _MapTransitions
from .heat_source import GoldakSource, ScanPath, ScanPathSource, _source_block, _source_work
from .surface_loss import LossPacks
from .phase import PhaseField, NonlinearPacks
from .history import _StepRecorder


def _gam(grid, mat, params):
    kappa = mat.k / (mat.rho * mat.cp)                    # adi3d_numba_coeff.py:292
    return kappa, kappa * params.dt / (grid.dx * grid.dx)


def adi_explicit_rhs(Tn, grid, mat, params):
    """R0 of adi3d_numba_coeff.py:292-298 (stage entry point for per-stage parity tests / benchmarks)."""
    t, kind = _as_state(Tn, grid)
    kappa, _ = _gam(grid, mat, params)
    out = grid.layout.empty()
    check(lib.adi_explicit_rhs(_p(t), _p(grid.d_flags), *grid.layout.pd, grid.dx, params.dt,
                               kappa, params.theta, _p(out), _stream()))
    return _wrap(out, kind)


def _sparse_arg(grid, pack, dense):
    """the `sparse` argument of the sweep entry points: bit 0 = the pack arrays may be read only where the flags say a
    cell is exposed, bit 1 = all-solid box hint.  Bit 0 needs packs built for the mask the flags describe: after
    `grid.mask = new` WITHOUT a pack rebuild the reference pairs the stale packs with the live mask
    (adi3d_numba_coeff.py:150-162 reads coeff at every in-mask cell), so stale packs are read densely here too."""
    fresh = getattr(pack, 'mask_version', None) == grid.mask_version
    return int(pack.sparse_ok and fresh and not dense) | (2 if getattr(grid, 'all_solid', False) else 0)


def _ledger_key(grid, pack, entry, axis, v, sp, work, tg, plain=True):
    """-> (the PromiseLedger kept on the PACK: every stepper on it shares it; this call's key, None when not eligible)"""
    nf = pack.__dict__.get('_nofb')
    if nf is None:
        nf = pack._nofb = PromiseLedger()
    if not nf.eligible(sp, work, tg, plain):
        return nf, None
    return nf, (entry, axis, v, sp, grid.mask_version, getattr(pack, 'mask_version', None), grid.shape, grid.sx,
                None if pack.d_dir_mask is None else pack.d_dir_mask.data_ptr())


def _sweep_into(axis, t_in, t_out, grid, mat, params, pack, Tinf, variant=None, xlo=None, xhi=None, dense=False):
    _, gam = _gam(grid, mat, params)
    _, work, wb = grid.scratch(2)
    v = pack.variant if variant is None else variant
    sp = _sparse_arg(grid, pack, dense)
    nf, key = _ledger_key(grid, pack, 'sweep', axis, v, sp, work, params.theta * gam,
                          plain=not (axis == 2 and (xlo is not None or xhi is not None)))
    check(lib.adi_sweep_bricks(axis, v, _p(t_in), _p(grid.d_flags), _p(grid.d_bricks), _p(pack.d_coeff), _p(pack.d_dir_mask),
                        _p(pack.d_dir_val), _p(pack.d_qflux), *grid.layout.pd,
                        sp | nf.bit(key), params.theta,
                        gam, params.dt, float(Tinf), _p(t_out),
                        _p(xlo), _p(xhi), _fc_arg(grid, pack, sp),
                        _p(work), wb, _stream()))
    nf.learn(key, work, grid.mask_version)


def fused_supported(grid, cond_pass=False):
    """explicit stage folded into the axis-0 sweep (adi_explicit_sweep0, ABI v7) available for this grid"""
    return bool(lib.adi_explicit_fused_supported(*grid.layout.pd, 1 if cond_pass else 0))


def valid_range(t):
    """element offsets relative to t's first element that lie inside its storage: the [valid_lo, valid_hi) of
    adi_explicit_sweep0 / adi_explicit_condense0"""
    off = t.storage_offset()
    return -off, t.untyped_storage().nbytes() // t.element_size() - off


def _explicit_sweep0_into(t, t_out, grid, mat, params, pack, Tinf, variant=None, dense=False):
    """stages 1+2 of adi_step_numba_coeff (adi3d_numba_coeff.py:292-299) in one pass: R0 is evaluated inside the
    loads of the axis-0 sweep.  Neighbours are read anywhere inside t's storage."""
    kappa, gam = _gam(grid, mat, params)
    _, work, wb = grid.scratch(2)
    v = pack.variant if variant is None else variant
    vlo, vhi = valid_range(t)
    sp = _sparse_arg(grid, pack, dense)
    nf, key = _ledger_key(grid, pack, 'fused', 0, v, sp, work, params.theta * gam)
    check(lib.adi_explicit_sweep0_bricks(v, _p(t), vlo, vhi, _p(grid.d_flags), _p(grid.d_bricks), _p(pack.d_coeff),
                                         _p(pack.d_dir_mask),
                                  _p(pack.d_dir_val), _p(pack.d_qflux), *grid.layout.pd,
                                  sp | nf.bit(key), grid.dx, params.dt, kappa, params.theta,
                                  float(Tinf), _p(t_out), None, None, _fc_arg(grid, pack, sp), _p(work), wb, _stream()))
    nf.learn(key, work, grid.mask_version)


def adi_explicit_sweep_axis0(Tn, grid, mat, params, pack, Tinf=0.0, variant=None, dense=False):
    """U of adi3d_numba_coeff.py:299 straight from Tn (stage entry point of the fused kernel)."""
    t, kind = _as_state(Tn, grid)
    if variant == _lib.SWEEP_GENERAL or (variant is None and pack.variant == _lib.SWEEP_GENERAL):
        _ensure_general(pack)
    out = grid.layout.empty()
    _explicit_sweep0_into(t, out, grid, mat, params, pack, Tinf, variant, dense)
    return _wrap(out, kind)


def adi_sweep_axis(axis, stage_in, grid, mat, params, pack, Tinf=0.0, variant=None, dense=False):
    """sweep_axis0/1/2 of adi3d_numba_coeff.py:133-237 for one axis (stage entry point).
    variant=None picks the leanest kernel the pack allows; variant=_lib.SWEEP_GENERAL with dense=True forces
    the 42 B/cell general-pack kernel that reads every pack array in full, like the reference does."""
    t, kind = _as_state(stage_in, grid)
    if variant == _lib.SWEEP_GENERAL or (variant is None and pack.variant == _lib.SWEEP_GENERAL):
        _ensure_general(pack)
    out = grid.layout.empty()
    _sweep_into(axis, t, out, grid, mat, params, pack, Tinf, variant, dense=dense)
    return _wrap(out, kind)


def _ensure_general(pack):
    """materialise the arrays a forced general-pack sweep reads (zeros, like the reference's packs)"""
    L = pack.layout
    if pack.d_dir_mask is None:
        pack.d_dir_mask = L.empty(torch.uint8, zero=True)
    if pack.d_dir_val is None:
        pack.d_dir_val = L.empty(zero=True)
    if pack.d_qflux is None:
        pack.d_qflux = L.empty(zero=True)


class StepExtras:
    """The nine optional parts of a step in one record: adi_step_hip_coeff and StagedStepper build it from their keywords,
    _check_extras, _launch_step and StagedStepper.run take it.  A tenth part is a name here (and in `graph_key`), its check in
    _check_extras, its line in _launch_step and its own module.
        recorders   history, solidification, monitor: those present, in the order they launch; each keeps a clock of its own
        stateful    phase, transitions, then the recorders: what a step changes besides the field (run() holds a snapshot of
                    each over its warm-up steps; `material` is stateless and `surface_loss` is rewritten from the field at
                    every step)"""
    __slots__ = ('source', 'surface_loss', 'phase', 'history', 'material', 'solidification', 'material_map', 'monitor',
                 'transitions', 'recorders')

    def __init__(self, source=None, surface_loss=None, phase=None, history=None, material=None, solidification=None,
                 material_map=None, monitor=None, transitions=None):
        self.source, self.surface_loss, self.phase, self.history = source, surface_loss, phase, history
        self.material, self.solidification, self.material_map, self.monitor = material, solidification, material_map, monitor
        self.transitions = transitions
        self.recorders = [x for x in (history, solidification, monitor) if x is not None]

    @property
    def stateful(self):
        return [x for x in (self.phase, self.transitions) if x is not None] + self.recorders

    def graph_key(self):
        """What a graph captured by StagedStepper.run holds of the optional parts: one entry each, None for an absent one, in
        the order below (the monitor's and the transitions' only when there is one: without them the key is what it was before
        there were any).
        Every launch named here is captured with the step (X -> Y reads X, Y -> X reads Y).
          source: the moving source, corrected after sweep 0 (adi_source_lines0), its time read from a device block whose step
            counter a captured tick advances -- power, origin, velocity, eta and f_f may change between runs without a new graph;
            the extent of its support (shape_key) is what the key holds.
          surface_loss: temperature-dependent surface loss, the packs' Robin coefficients rewritten from the step's INPUT buffer,
            the first launch of every step; the law travels by value in that launch, so its parameters are the entry.
          phase: latent heat, the correction of the step's OUTPUT buffer, the last launch before the recorders'; the law travels by
            value and f and the summary by pointer, so all three are in the entry.
          history: the record of the step input -> output and the tick of its block; the levels travel by value and the five
            buffers by pointer.
          material: k(T), cp(T) -- the Kirchhoff transform of the step's INPUT buffer (with the loss update, the first launches)
            and the recovery of its OUTPUT buffer after sweep 2; the laws and the ambient travel by value, the Kirchhoff field by
            pointer.  Stateless: the warm-up steps need no snapshot.
          solidification: the record of the step input -> output and the tick of its block, after the history's; T_freeze and dx
            travel by value and the five buffers by pointer.
          material_map: several materials, the step's four launches are the MaterialMap's; its pair table travels by value in them
            (so dt and theta, in run()'s key already, cover it) and its id field by pointer.  With it surface_loss is a
            MapLossPacks (the laws in a device table by pointer, the ambient by value) and phase a MapPhaseField (laws by value,
            f, the summary and the bricks' id sets by pointer): each answers graph_key() for itself.  With it `source` is a
            MapSource: the source added to the explicit stage's output (adi_matmap_source_add_r0), its time read from the same
            device block by pointer and ticked in the capture; the extent of its support travels by value (shape_key) and the
            C table by value in the launch, everything else of the source through the block, as for a GoldakSource.
          monitor: the record of the step's OUTPUT buffer and the tick of its block, the last launches of all; probes, regions
            and weights travel by value and its buffers by pointer.
          transitions: a MaterialTransitions of the material_map: the change of the id, pack values and f of the cells of the
            step's OUTPUT buffer that got hot enough (adi_matmap_transition), one launch after the phase's and before the
            recorders'; the rules travel by value, the id field, the bricks' id sets, the counter, the six pack arrays and the
            phase's f and summary by pointer.  A transition is not a change of the map's ids in the sense of its version: the
            graph holds the id field by pointer and replays on."""
        key = (None if self.source is None else self.source.shape_key(),) + tuple(
            None if x is None else x.graph_key()
            for x in (self.surface_loss, self.phase, self.history, self.material, self.solidification, self.material_map))
        if self.monitor is not None:
            key += (self.monitor.graph_key(),)
        if self.transitions is not None:
            key += (('transitions', self.transitions.graph_key()),)
        return key


def _check_extras(grid, mat, params, packs, extras, stepper=False):
    """TypeError / ValueError for an optional part of the step that is of the wrong kind or was made for other packs, another
    grid or another cp, and the rules about which parts combine: once per adi_step_hip_coeff call and once per StagedStepper,
    before anything is launched.
    One asymmetry, kept because code that builds a StagedStepper before `sync_mask` works and must go on working: the mask of
    the solidification record is checked here, the history's is not -- adi_step_hip_coeff checks it itself before it launches,
    StagedStepper.__init__ does not, and StagedStepper.run checks every recorder.
    stepper: the caller is a StagedStepper, whose steps a graph may replay: a MapPathSource is refused there."""
    x = extras
    source, surface_loss, phase, material, mm = x.source, x.surface_loss, x.phase, x.material, x.material_map
    tr = x.transitions
    if stepper and isinstance(source, _MapPathSource):
        raise TypeError("source: a MapPathSource does not ride a captured graph (the window of each step travels by value from "
                        "the host in a plain launch); step with adi_step_numba_coeff(..., material_map=mm, S=msrc, t=t)")

    def same_grid(kw, part, cls):
        if part.grid is not grid:
            raise ValueError("%s: the %s belongs to another grid" % (kw, cls))

    def own_packs(kw, part, owner):
        if len(packs) != 3 or any(p is not q for p, q in zip(packs, part.packs)):
            raise ValueError("%s: the step must be given the %s own packs (%s.packs)" % (kw, owner, kw))

    def own_material(kw, part, owner, why=""):
        m = part.mat
        if (float(mat.rho), float(mat.cp), float(mat.k)) != (m.rho, m.cp, m.k):
            raise ValueError("%s: the step must be given the %s own material (%s.mat)%s" % (kw, owner, kw, why))

    if mm is not None:
        if not isinstance(mm, MaterialMap):
            raise TypeError("material_map must be a MaterialMap")
        same_grid('material_map', mm, 'MaterialMap')
        own_packs('material_map', mm, "MaterialMap's")
        own_material('material_map', mm, "MaterialMap's")
        if source is not None and not isinstance(source, _MapSource):
            raise ValueError("material_map: a GoldakSource object cannot be combined with it (its sweep-0 correction assumes "
                             "uniform coupling); pass the source as a field, S=path.sample_step(grid, t, dt)")
        if source is not None and source.mm is not mm:
            raise ValueError("source: the MapSource belongs to another MaterialMap")
        if ((surface_loss is not None and not isinstance(surface_loss, _MapLoss))
                or (phase is not None and not isinstance(phase, _MapPhase)) or material is not None):
            raise ValueError("material_map: surface_loss= / phase= / material= cannot be combined with it; each assumes one cp")
        if surface_loss is not None and surface_loss.mm is not mm:
            raise ValueError("surface_loss: the MapLossPacks belongs to another MaterialMap")
        if phase is not None and phase.mm is not mm:
            raise ValueError("phase: the MapPhaseField belongs to another MaterialMap")
        mm._check_fresh()
        if phase is not None:
            phase._check_fresh()
    if tr is not None:
        if not isinstance(tr, _MapTransitions):
            raise TypeError("transitions must be a MaterialTransitions")
        if mm is None:
            raise ValueError("transitions: a MaterialTransitions needs material_map= (its MaterialMap's step)")
        if tr.mm is not mm:
            raise ValueError("transitions: the MaterialTransitions belongs to another MaterialMap")
        if tr.phase is not phase:
            raise ValueError("transitions: the MaterialTransitions' phase is not the step's phase= (the same MapPhaseField in "
                             "both places, or none in both: a changed cell's liquid fraction is set in the step's own field)")
        tr._check_fresh()
    if material is not None:
        if not isinstance(material, NonlinearPacks):
            raise TypeError("material must be a NonlinearPacks")
        same_grid('material', material, 'NonlinearPacks')
        own_packs('material', material, "NonlinearPacks'")
        own_material('material', material, "NonlinearPacks'", ": the linear step runs with (rho, cp_ref, k_ref)")
        if phase is not None or surface_loss is not None:
            raise ValueError("material: phase= / surface_loss= cannot be combined with it; the MaterialLaw carries the latent "
                             "heat and the NonlinearPacks the surface loss")
        if params.theta < material.law.min_theta():
            raise ValueError("material: theta = %r is below the law's stability limit cp_ref / (2 min c_eff) = %r"
                             % (params.theta, material.law.min_theta()))
    if isinstance(source, _MapSource) and mm is None:
        raise ValueError("source: a MapSource needs material_map= (its MaterialMap's step); without one pass the GoldakSource "
                         "itself")
    if source is not None and not isinstance(source, (GoldakSource, _MapSource)):
        raise TypeError("source must be a GoldakSource (pass a source field, e.g. ScanPath.sample_step, to "
                        "adi_step_numba_coeff)")
    if surface_loss is not None and mm is None:
        if not isinstance(surface_loss, LossPacks):
            raise TypeError("surface_loss must be a LossPacks")
        own_packs('surface_loss', surface_loss, "LossPacks'")
    if phase is not None and mm is None:
        if not isinstance(phase, PhaseField):
            raise TypeError("phase must be a PhaseField")
        same_grid('phase', phase, 'PhaseField')
        if float(phase.mat.cp) != float(mat.cp):
            raise ValueError("phase: the PhaseField was made for cp = %r, the step runs with %r" % (phase.mat.cp, mat.cp))
    for kw, cls in (('history', 'ThermalHistory'), ('solidification', 'SolidificationRecord'), ('monitor', 'FieldMonitor')):
        rec = getattr(x, kw)
        if rec is None:
            continue
        if not isinstance(rec, _StepRecorder) or rec._keyword != kw:
            raise TypeError("%s must be a %s" % (kw, cls))
        same_grid(kw, rec, cls)
        if kw == 'solidification':
            rec._check_mask()                              # (and not the history's: the asymmetry above)
    if x.monitor is not None and x.monitor.material_map is not mm:
        raise ValueError("monitor: the FieldMonitor's material_map is not the step's")


def _no_mark():
    pass


def _launch_step(t_in, out, grid, mat, params, packs, Tinf, fused, extras, d_S=None, owner=None, t_set=None, captured=False,
                 mark=_no_mark):
    """THE launch sequence of one step t_in -> out (fp64 tensors in the grid's layout; nothing is allocated): the surface-loss
    update from t_in, the explicit stage and sweep 0 (one launch when `fused`), the moving source's correction of sweep 0's
    output, sweeps 1 and 2, the latent-heat correction of `out`, then the recorders in their order: the history record, the
    solidification record, the monitor's.  With `extras.material` (a NonlinearPacks): its `begin(t_in)` first, the launches above
    on its Kirchhoff field with Theta(Tinf) as the ambient, its `recover(t_in, out)` after sweep 2, and the recorders on (t_in,
    out) as ever.  Every form of the step calls it -- adi_step_hip_coeff with or without a source field, StagedStepper.step, and
    what StagedStepper.run captures -- with a StepExtras that _check_extras has passed.
    d_S: a source FIELD in the grid's layout; the explicit stage takes it (adi_explicit_rhs_src), never fused.
    extras.source, owner: a GoldakSource and the object that holds its device block and workspace; t_set: the step's start time
    if the block is to be set here, just ahead of the correction (None: the caller has set it).
    captured: a graph may replay these launches and the caller keeps the clocks: the source's block is ticked after the
    correction, and the recorders launch their records without moving their host clocks.  Otherwise no tick, and each recorder's
    public `record`.
    mark: called at the stage boundaries of per-stage timing: before the explicit stage, between it and sweep 0 when they are
    two launches, after sweep 0 with the source's correction, after sweep 1 and after sweep 2.
    extras.material_map: a MaterialMap: the explicit stage (with d_S, if any) and the three sweeps are ITS four launches
    (adi_matmap_explicit, adi_matmap_sweep), never fused; with it `surface_loss` is a MapLossPacks, whose update from t_in comes
    first, and `phase` a MapPhaseField, whose correction of `out` follows sweep 2; the recorders follow as ever.  With it
    `extras.source` is a MapSource and the order is: the map's explicit stage, the source added to its output
    (adi_matmap_source_add_r0, the block set just ahead of it when t_set is given), adi_source_tick when captured, sweep 0 -- no
    correction after sweep 0.  A MapPathSource takes the same place with one plain launch (adi_matmap_scan_add_r0 on the window
    of [t_set, t_set + dt], found on the host): no block, no tick, and only adi_step_hip_coeff reaches here with one.
    extras.monitor: a FieldMonitor: its record of `out` and its tick are the last launches of all, after solidification's.
    extras.transitions: a MaterialTransitions of the material_map: its pass over `out` (adi_matmap_transition) follows the
    latent-heat correction and precedes the recorders, which so record the step's final (T, f, id)."""
    x, mm = extras, extras.material_map
    (ta, tb), _, _ = grid.scratch(2)
    u = t_in                                               # what the linear step runs on
    if mm is not None:
        mm._check_fresh()
        if x.transitions is not None:
            x.transitions._check_fresh()                   # (before the first launch, not after the sweeps)
        fused = False

        def explicit(dst):
            mm._explicit_into(u, d_S, dst, params)

        def sweep(axis, a, b):
            mm._sweep_into(axis, a, b, params, Tinf)
    else:
        if x.material is not None:
            u, Tinf = x.material.begin(t_in), x.material.theta_inf

        def explicit(dst):
            if d_S is None:
                kappa, _ = _gam(grid, mat, params)
                check(lib.adi_explicit_rhs(_p(u), _p(grid.d_flags), *grid.layout.pd, grid.dx, params.dt,
                                           kappa, params.theta, _p(dst), _stream()))
            else:
                _explicit_src_into(u, d_S, dst, grid, mat, params)

        def sweep(axis, a, b):
            _sweep_into(axis, a, b, grid, mat, params, packs[axis], Tinf)
    if x.surface_loss is not None:
        x.surface_loss.update(t_in, Tinf)
    mark()
    if fused and d_S is None:
        _explicit_sweep0_into(u, tb, grid, mat, params, packs[0], Tinf)
    else:
        explicit(ta)
        if isinstance(x.source, _MapPathSource):
            x.source.add_r0(ta, params, t_set)             # (a plain launch, the window by value: never captured)
        elif mm is not None and x.source is not None:
            if t_set is not None:
                x.source.set_block(_source_block(owner), t_set, params.dt)
            x.source.add_r0(ta, params, _source_block(owner))
            if captured:
                check(lib.adi_source_tick(_p(_source_block(owner)), _stream()))
        mark()
        sweep(0, ta, tb)
    if x.source is not None and mm is None:
        if t_set is not None:
            x.source.set_block(_source_block(owner), t_set, params.dt)
        _source_lines0_into(tb, grid, mat, params, packs[0], x.source, owner)
        if captured:
            check(lib.adi_source_tick(_p(_source_block(owner)), _stream()))
    mark()
    sweep(1, tb, ta)
    mark()
    sweep(2, ta, out)
    mark()
    if x.material is not None:
        x.material.recover(t_in, out)
    if x.phase is not None:
        x.phase.apply(out, packs[2].d_dir_mask if packs[2].has_dir else None)
    if x.transitions is not None:
        x.transitions.apply(out, packs[2].d_dir_mask if packs[2].has_dir else None)
    for rec in x.recorders:
        rec._record_step(t_in, out, params.dt, captured)


def adi_step_hip_coeff(Tn, grid, mat, params, packs, Tinf=0.0, S=None, t=0.0, surface_loss=None, phase=None, history=None,
                       material=None, solidification=None, material_map=None, monitor=None, transitions=None):
    """adi3d_numba_coeff.py:290-302 / adi3d_gpu_coeff.py:213-230: explicit stage, then the three
    implicit sweeps in the order axis 0, 1, 2.  Returns a NEW array of the kind it was given;
    `Tn` is never modified.

    S: volumetric heat source in W/m^3 (include/adi_hip.h, "Volumetric heat source"): R0 gains dt*q/(rho cp) on in-mask
    cells, q evaluated at the step's mid-time.  None: the step of the reference, the same launches as without the keyword.
    An array of the grid's shape (NumPy / torch / DeviceField): the field form -- explicit stage with the source
    (adi_explicit_rhs_src), then the three unfused sweeps.  A GoldakSource: evaluated at t + dt/2 on the device and added
    to the output of sweep 0 by superposition (adi_source_lines0), after whichever sweep-0 form the step uses.  A ScanPath or a
    ScanPathSource is not accepted here: pass the field, ScanPath.sample_step(grid, t, dt) or, evaluated on the device,
    ScanPathSource.sample_step_device(grid, t, dt).
    t: the step's start time, used only by a source object.
    surface_loss: a LossPacks whose `.packs` are `packs`: their Robin coefficients are first rewritten from Tn (the law at the
    temperature at the start of the step, adi_surface_loss_update), then the step runs as above.  None: no such launch.
    phase: a PhaseField of the grid: after sweep 2 the step's output is corrected for the latent heat from the liquid fraction
    the PhaseField holds, which moves on with it (adi_phase_apply, the last launch, on the freshly allocated output).  None: no
    such launch.
    history: a ThermalHistory of the grid: the step Tn -> result (after the correction of `phase`) is recorded at the recorder's
    own clock, which moves on by dt (adi_history_record and adi_history_tick, the last launches).  None: no such launch.
    material: a NonlinearPacks of the grid, with `packs` its `.packs` and `mat` its `.mat`: temperature-dependent k(T) and cp(T)
    (and latent heat) by its MaterialLaw, surface loss by its SurfaceLoss.  The step runs on the Kirchhoff temperature and the
    enthalpy is put back on its curve afterwards (adi_matlaw_theta first, adi_matlaw_recover after sweep 2); the
    ambient is the NonlinearPacks' own, `Tinf` here is not used.  Combines with S= in either form and history=, not with phase=
    or surface_loss=; params.theta must reach law.min_theta().  None: no such launch.
    solidification: a SolidificationRecord of the grid: the cells that freeze in the step Tn -> result (after the correction of
    `phase` or the recovery of `material`) get their crossing time, cooling rate and squared gradient at the recorder's own
    clock, which moves on by dt (adi_solid_record and adi_history_tick on its block, the last launches, after `history`'s).
    None: no such launch.
    material_map: a MaterialMap of the grid, with `packs` its `.packs` and `mat` its `.mat`: several materials in one grid, a
    material id per cell.  The step is then four launches of its own kernels -- explicit stage, sweeps 0, 1, 2 -- whose couplings
    come from the map's pair table.  Combines with S= as a field and with history= and solidification=; with
    surface_loss= when that is a MapLossPacks of the map and with phase= when that is a MapPhaseField of the map (one law per
    material: adi_matmap_loss_update first, adi_matmap_phase_apply after sweep 2); not with a GoldakSource object,
    a LossPacks, a PhaseField or material=.  A moving Goldak source goes in wrapped, S=MapSource(mm, src): it is added to the
    explicit stage's output with each cell's own C (adi_matmap_source_add_r0).  A scan path goes in wrapped too,
    S=MapPathSource(mm, path): its step-averaged source of [t, t + dt] is added in the same place on the window's index box
    (adi_matmap_scan_add_r0, one plain launch), without the field.  None: the launches of before.
    monitor: a FieldMonitor of the grid (with the step's material_map, if any): the result's value at its probes and the count,
    extrema and sums of its regions become one row of its device log, and its clock moves on by dt (adi_monitor_record and
    adi_history_tick on its block, the last launches of all).  Combines with every other argument.  None: no such launch.
    transitions: a MaterialTransitions of the material_map (made with the step's `phase`, if any): after the latent-heat correction
    the in-mask cells of the result that are at or above the threshold of their material's rule change their material -- id, pack
    values and liquid fraction, at constant temperature (adi_matmap_transition, one launch before the recorders'; DESIGN.md
    6l4).  Needs material_map=.  None: no such launch.
    Every optional argument is checked before the first launch (_check_extras); the launches are _launch_step's."""
    if isinstance(S, (ScanPath, ScanPathSource)):
        raise TypeError("adi_step_hip_coeff: a scan path enters the step as its field: S=path.sample_step(grid, t, dt) from the "
                        "host, or S=path.on_device().sample_step_device(grid, t, dt) evaluated on the device")
    source = S if isinstance(S, (GoldakSource, _MapSource)) else None
    extras = StepExtras(source, surface_loss, phase, history, material, solidification, material_map, monitor, transitions)
    _check_extras(grid, mat, params, packs, extras)
    if history is not None:
        history._check_mask()                              # (here and not in _check_extras: see there)
    t_in, kind = _as_state(Tn, grid)
    d_S = None
    if S is not None and source is None:
        if tuple(S.shape) != grid.shape:
            raise ValueError("S has shape %s, the grid %s" % (tuple(S.shape), grid.shape))
        d_S = grid.layout.to_layout(S, torch.float64)
    out = grid.layout.empty()
    _launch_step(t_in, out, grid, mat, params, packs, Tinf, fused_supported(grid), extras, d_S=d_S, owner=grid, t_set=t)
    return _wrap(out, kind)


def _explicit_src_into(t, d_S, out, grid, mat, params):
    kappa, _ = _gam(grid, mat, params)
    check(lib.adi_explicit_rhs_src(_p(t), _p(d_S), _p(grid.d_flags), *grid.layout.pd, grid.dx, params.dt, kappa,
                                   params.theta, mat.rho, mat.cp, _p(out), _stream()))


def _source_lines0_into(U, grid, mat, params, pack, src, owner):
    """U += A0^-1 s on the axis-0 lines the support can meet (adi_source_lines0), in place; the block and the workspace
    are `owner`'s"""
    _, gam = _gam(grid, mat, params)
    sp = _sparse_arg(grid, pack, False)
    work = _source_work(owner, grid.layout.pd[:3], grid.dx, src)
    check(lib.adi_source_lines0(_p(_source_block(owner)), ctypes.byref(src.as_c()), _p(U), _p(grid.d_flags),
                                _p(pack.d_coeff), _p(pack.d_dir_mask if pack.has_dir else None), *grid.layout.pd, sp,
                                grid.dx, params.theta, gam, params.dt, mat.rho, mat.cp, _fc_arg(grid, pack, sp),
                                _p(work), 0 if work is None else work.numel(), _stream()))


# the reference's backend-specific names, so its drivers run unchanged on this module
adi_step_numba_coeff = adi_step_hip_coeff
adi_step_gpu_coeff = adi_step_hip_coeff


class StagedStepper:
    """The step of adi_step_hip_coeff with its arguments resolved once, for tight loops over a
    device-resident field (drivers call the step `nsub` times with the same packs and dt,
    quick_compare_dirichlet_robin.py:169-178).  `events`: optional list of 5 torch.cuda.Event recorded on
    the launch stream before/between/after the four stage kernels (per-stage HIP-event timing).  With `phase=` (a PhaseField
    of the grid) the latent-heat correction is the last launch of every step, after the last of the five marks: the stage
    times stay those of the stage kernels.  With `history=` (a ThermalHistory of the grid) the record launch and its tick follow,
    the last launches of every step; `run` sets the recorder's block from the recorder's own clock `history.t` (not from `t0`,
    which stays the source's time origin) and moves that clock on by nsteps*dt.  With `solidification=` (a SolidificationRecord
    of the grid) its record launch and tick come after those, the last launches of every step, on the recorder's own clock in
    the same way.  With `monitor=` (a FieldMonitor of the grid) its record of the step's output and its tick are the last launches
    of all, on the monitor's own clock in the same way.  With `transitions=` (a MaterialTransitions of the material_map) its pass
    follows the latent-heat correction and precedes the recorders; `run` captures it with the step, and its warm-up steps leave
    ids, packs, f and the bricks' words as they were."""

    def __init__(self, grid, mat, params, packs, Tinf=0.0, fused=None, source=None, surface_loss=None, phase=None,
                 history=None, material=None, solidification=None, material_map=None, monitor=None, transitions=None):
        # the optional parts: what each does in a step and what a captured graph holds of it is written at StepExtras.graph_key
        self.extras = StepExtras(source, surface_loss, phase, history, material, solidification, material_map, monitor,
                                 transitions)
        _check_extras(grid, mat, params, packs, self.extras, stepper=True)
        self.grid, self.mat, self.params, self.packs, self.Tinf = grid, mat, params, packs, float(Tinf)
        self.captures = 0              # HIP graphs captured by run() so far
        self.fused = fused_supported(grid) if fused is None else (bool(fused) and fused_supported(grid))
        if material_map is not None:
            self.fused = False
            self.stage_names = ['matmap_explicit', 'matmap_sweep_axis0', 'matmap_sweep_axis1', 'matmap_sweep_axis2']
            per_line = [n > 1024 for n in grid.layout.pd[:3]]
            self.stage_bytes_per_cell = [18.0] + [18.0 + (32.0 if t else 0.0) for t in per_line]
        elif self.fused:
            # the fused kernel reads T + flags (+ the pack arrays of the axis-0 sweep) and writes U: the sweep's own
            # byte count (SURVEY.md 8(d) variant rule); R0 never reaches HBM
            self.stage_names = ['explicit+sweep_axis0', 'sweep_axis1', 'sweep_axis2_contig']
            self.stage_bytes_per_cell = [p.bytes_per_cell for p in packs]
        else:
            self.stage_names = ['explicit', 'sweep_axis0', 'sweep_axis1', 'sweep_axis2_contig']
            self.stage_bytes_per_cell = [float(_lib.EXPLICIT_BYTES_PER_CELL)] + [p.bytes_per_cell for p in packs]

    def sweep_into(self, axis, t_in, t_out, variant=None, dense=False):
        if variant == _lib.SWEEP_GENERAL:
            _ensure_general(self.packs[axis])
        _sweep_into(axis, t_in, t_out, self.grid, self.mat, self.params, self.packs[axis], self.Tinf, variant,
                    dense=dense)

    def _step_into(self, t, out, captured=True, mark=_no_mark):
        """one step t -> out (both native-layout device tensors), no allocation: what a HIP graph captures"""
        _launch_step(t, out, self.grid, self.mat, self.params, self.packs, self.Tinf, self.fused, self.extras, owner=self,
                     captured=captured, mark=mark)

    def run(self, T, nsteps, graph=True, t0=0.0):
        """The drivers' `nsub` loop (quick_compare_dirichlet_robin.py:169-178, waam_from_stl_v7_mm.py:525-528): `nsteps`
        steps with the same packs and dt on a device-resident field, returned as a new DeviceField.  The launches of
        two steps (X -> Y -> X) are captured once into a HIP graph and replayed, so small grids are not bound by the
        host's launch path (64^3: 3 kernels + 3 memsets per step, each a ctypes call); the graph is rebuilt when dt,
        theta, Tinf, the mask or the packs change.  graph=False: plain launches.
        t0: time at the start of the first step (a source's step i runs at t0 + i*dt + dt/2); the source's block is
        written here, so its power / origin / velocity as they are now hold for this run, and a change of its support's
        extent recaptures."""
        g, prm = self.grid, self.params
        nsteps = int(nsteps)
        x = self.extras
        key = (float(prm.dt), float(prm.theta), self.Tinf, g.mask_version, tuple(id(p) for p in self.packs),
               tuple(getattr(p, 'mask_version', None) for p in self.packs),
               tuple(None if p.d_coeff is None else p.d_coeff.data_ptr() for p in self.packs), self.fused) + x.graph_key()
        for rec in x.recorders:
            rec._check_mask()
        st = getattr(self, '_graph', None)
        if st is None or st['key'] != key:
            # (zeroed where the box is padded, as Layout.to_layout does: the cells outside the logical grid are identity rows of
            # the sweeps, and a NaN left there by whoever owned the memory before comes back in every cell of the result)
            X, Y = g.layout._fresh(torch.float64), g.layout._fresh(torch.float64)
            st = self._graph = dict(key=key, X=X, Y=Y, g=None)
        X, Y = st['X'], st['Y']
        X.copy_(g.layout.to_layout(T, torch.float64))
        if x.source is not None:
            x.source.set_block(_source_block(self), t0, prm.dt)
        if graph and nsteps >= 2 and st['g'] is None:
            g.scratch(2)                                   # every buffer exists before the capture
            held = [s.snapshot() for s in x.stateful]      # (the warm-up steps would advance f, the recorders, log and clocks)
            for rec in x.recorders:
                rec.set_clock(prm.dt)
            self._step_into(X, Y); self._step_into(Y, X)   # warm-up outside the capture (lazy module loads, and the
            self._step_into(X, Y); self._step_into(Y, X)   # no-fallback promise is learnt on the third step); harmless:
            X.copy_(g.layout.to_layout(T, torch.float64))  # X is restored
            for s, snap in zip(x.stateful, held):
                s.restore(snap)                            # ... and so is what the extras hold
            torch.cuda.synchronize()
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg):
                self._step_into(X, Y)
                self._step_into(Y, X)
            st['g'] = cg
            self.captures += 1
        if x.source is not None:
            x.source.set_block(_source_block(self), t0, prm.dt)   # (after the warm-up: the counter starts at 0)
        for rec in x.recorders:
            rec.set_clock(prm.dt)                          # (likewise; each recorder's own clock, not t0)
        done = 0
        if graph and st['g'] is not None:
            for _ in range(nsteps // 2):
                st['g'].replay()
            done = 2 * (nsteps // 2)
            if done and x.transitions is not None:
                x.transitions.after_replay()               # (no Python ran between the replayed steps: ids changed unseen)
        cur, oth = X, Y
        for _ in range(nsteps - done):
            self._step_into(cur, oth)
            cur, oth = oth, cur
        for rec in x.recorders:
            rec.advance_clock(rec.t, float(prm.dt), nsteps)
        out = g.layout.empty()
        out.copy_(cur)
        return DeviceField(out)

    def step(self, T, events=None, t=0.0):
        """one step from time t (the source, if any, at t + dt/2)"""
        g, prm = self.grid, self.params
        if self.extras.source is not None:
            self.extras.source.set_block(_source_block(self), t, prm.dt)
        t_in = g.layout.to_layout(T, torch.float64)
        out = g.layout.empty()
        ev = iter(events or ())
        self._step_into(t_in, out, captured=False, mark=(lambda: next(ev).record()) if events else _no_mark)
        return DeviceField(out)
