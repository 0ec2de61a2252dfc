"""Latent heat and temperature-dependent surface loss on a grid of several materials: `MapPhaseField`, the
liquid fraction of a MaterialMap's grid under one PhaseChange law per material, and `MapLossPacks`, the MaterialMap's own packs
rewritten in place by one SurfaceLoss per material; `MapSource`, a moving GoldakSource inside the step of a MaterialMap
(DESIGN.md section 6l3); `MapPathSource`, a ScanPath inside it without a source field; and `MaterialTransitions`, cells that change their material when they get hot enough (DESIGN.md section
6l4)."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import lib, check, ptr_array, FACES
from .fields import DeviceField, _SeededForMask, _as_state, _device, _native_f64, _p, _stream, _wrap
from .packs import MaterialMap, _MapLoss, _MapPhase, _MapSource, _MapPathSource, _MapTransitions, _triples, _face_spec_args
from .heat_source import GoldakSource, ScanPath, ScanPathSource, _source_block
from .surface_loss import SurfaceLoss
from .phase import PhaseChange


class MapPhaseField(_SeededForMask, _MapPhase):
    """The liquid fraction of a MaterialMap's grid, on the device: PhaseField with the law of the cell's own material.
    laws: one entry per material of `mm`, a PhaseChange or None (the material never melts in this run: a backing bar).  It holds
        f           fp64, the grid's layout, 0 off the mask and 0 in every cell of a law-less material
        summary     one word per 16^3 brick, 0 exactly when every f of the brick is 0 (PhaseField's)
        brick_ids   one word per brick: bits 0-7 the set of material ids among the brick's in-mask cells, 0 if it has none --
                    adi_matmap_phase_apply reads it first and leaves a brick without a law at once, runs a brick of one material
                    without reading ids, and reads the id bytes only in a brick of several
    All buffers live as long as the object, so a StagedStepper's graph holds their pointers.  T (optional): the field f is seeded
    from, f = f_eq(T) of the cell's own law; without it everything is solid.  dir_mask (optional): the Dirichlet cells of `apply`
    calls that are not given any (the step passes its pack's).
    The object remembers grid.mask_version and the MaterialMap's id field: after either changed `apply` raises ValueError until
    sync_mask(T), which seeds the cells that joined the mask and rebuilds brick_ids.
        apply(T, d_dir_mask=None)   the correction on a device field in the grid's layout, T and f in place: one launch
        seed(T, sel=None)           f = f_eq(T) on the in-mask cells `sel` selects (None: all), 0 off the mask and without a law
        sync_mask(T)                see above
        snapshot() / restore(s)     f and the summary
    `correct_of` / `correct` is the definition of apply, `f_eq_of` of seed, in NumPy fp64."""

    def __init__(self, mm, laws, T=None, dir_mask=None):
        if not isinstance(mm, MaterialMap):
            raise TypeError("MapPhaseField: mm must be a MaterialMap")
        self.laws = self._checked_laws(laws, mm.materials)
        self.mm, self.grid = mm, mm.grid
        L = self.grid.layout
        self._flat = torch.zeros(L.numel_padded, dtype=torch.float64, device=_device())
        self.f = self._flat.as_strided(L.shape, L.strides)
        self.summary = torch.zeros(self._words(), dtype=torch.int32, device=_device())
        self.brick_ids = torch.zeros(self._words(), dtype=torch.int32, device=_device())
        self.d_dir_mask = None if dir_mask is None else L.to_layout(dir_mask, torch.uint8)
        self._ids_version = None
        if T is not None:
            self.seed(T)
        else:
            self._seed_nothing()

    @staticmethod
    def _checked_laws(laws, materials):
        """the laws as a tuple after the checks of the constructor (nothing is launched before they pass)"""
        try:
            laws = tuple(laws)
        except TypeError:
            raise TypeError("MapPhaseField: laws must be a sequence with one PhaseChange or None per material")
        if len(laws) != len(materials):
            raise ValueError("MapPhaseField: %d laws for %d materials" % (len(laws), len(materials)))
        for law, (_, cp, _) in zip(laws, _triples(materials)):
            if law is None:
                continue
            if not isinstance(law, PhaseChange):
                raise TypeError("MapPhaseField: a law must be a PhaseChange or None, got %r" % type(law).__name__)
            law.constants(cp)
        return laws

    def _words(self):
        n = int(lib.adi_phase_summary_words(*self.grid.layout.pd[:3]))
        if n <= 0:
            raise ValueError("MapPhaseField: bad grid")
        return n

    def _c_laws(self):
        n = len(self.laws)
        none = _lib.PhaseChangeLaw(0.0, 0.0, 0.0)
        return (n, (_lib.PhaseChangeLaw * n)(*[none if w is None else w.as_c() for w in self.laws]),
                (ctypes.c_int * n)(*[0 if w is None else 1 for w in self.laws]))

    def _remember_mask(self):
        super()._remember_mask()
        self._ids_version = self.mm._ids_version

    def _check_fresh(self):
        if self.grid.mask_version != self._mask_version or self.mm._ids_version != self._ids_version:
            raise ValueError("MapPhaseField: the grid's mask or the MaterialMap's ids changed since the liquid fraction was "
                             "seeded; call sync_mask(T)")

    @property
    def liquid_fraction(self):
        """a copy of f as a DeviceField of the grid's shape"""
        return DeviceField(self.f).copy()

    def apply(self, T, d_dir_mask=None):
        """adi_matmap_phase_apply on T (a DeviceField or device tensor in the grid's layout), in place; d_dir_mask: the
        Dirichlet cells as a uint8 device tensor in the grid's layout (default: the ones given at construction)"""
        g = self.grid
        t = _native_f64(g, T, "MapPhaseField.apply: T must be a fp64 device field in the grid's layout (it is corrected in place)")
        self._check_fresh()
        assert self.summary.numel() == self._words()
        dm = self.d_dir_mask if d_dir_mask is None else d_dir_mask
        if dm is not None:
            assert g.layout.is_native(dm) and dm.dtype == torch.uint8
        n, laws, on = self._c_laws()
        cp = (ctypes.c_double * n)(*[float(m.cp) for m in self.mm.materials])
        check(lib.adi_matmap_phase_apply(n, laws, on, cp, _p(t), _p(self.f), _p(g.d_flags), _p(g.d_bricks), _p(self.mm._d_ids),
                                         _p(dm), _p(self.summary), _p(self.brick_ids), *g.layout.pd, _stream()))
        return T

    def seed(self, T, sel=None):
        """adi_matmap_phase_seed: f = f_eq(T) of the cell's own law on the in-mask cells `sel` selects (bool / uint8 array or
        tensor of the grid's shape; None: every in-mask cell), 0 off the mask and in law-less cells; the summary and brick_ids
        are rewritten for the grid's mask and the MaterialMap's ids as they are now"""
        g = self.grid
        d_sel = None if sel is None else g.layout.to_layout(sel, torch.uint8)
        assert self.summary.numel() == self._words()
        n, laws, on = self._c_laws()
        check(lib.adi_matmap_phase_seed(n, laws, on, _p(_native_f64(g, T)), _p(self.f), _p(g.d_flags), _p(g.d_bricks),
                                        _p(self.mm._d_ids), _p(d_sel), _p(self.summary), _p(self.brick_ids), *g.layout.pd,
                                        _stream()))
        self._remember_mask()

    def _seed_nothing(self):
        """a seed that selects no cell: every in-mask f of a material with a law is kept, the rest zeroed, and every entry of the
        summary and of brick_ids rewritten"""
        g = self.grid
        self.seed(g.layout.empty(zero=True), sel=g.layout.empty(torch.uint8, zero=True))

    def sync_mask(self, T):
        """after `grid.mask` or the MaterialMap's ids changed: the cells that joined the mask since the last seed / sync are
        seeded from T, those that left it are cleared, every other cell keeps its f (0 where its material has no law now), and
        brick_ids is rebuilt"""
        if self.grid.mask_version != self._mask_version:
            super().sync_mask(T)
        elif self.mm._ids_version != self._ids_version:
            self._seed_nothing()

    def set_liquid_fraction(self, f):
        """load f (array / tensor / DeviceField of the grid's shape; taken as 0 off the mask and in law-less cells) and rebuild
        the summary from it on the device"""
        self.f.copy_(self.grid.layout.to_layout(f, torch.float64))
        self._seed_nothing()

    def snapshot(self):
        return self._flat.clone(), self.summary.clone()

    def restore(self, s):
        self._flat.copy_(s[0])
        self.summary.copy_(s[1])

    def graph_key(self):
        """what a captured graph holds of the field: the laws and heat capacities by value, the buffers by pointer"""
        return (tuple(None if w is None else w.key() for w in self.laws), tuple(float(m.cp) for m in self.mm.materials),
                self.f.data_ptr(), self.summary.data_ptr(), self.brick_ids.data_ptr(), self.mm._d_ids.data_ptr(),
                None if self.d_dir_mask is None else self.d_dir_mask.data_ptr())

    # ---- the definition in NumPy fp64 -------------------------------------------------------------------------------------
    @staticmethod
    def correct_of(laws, materials, T_star, f, mask, ids, dir_mask):
        """(T, f) after the correction of the step's result T_star from the liquid fraction f it started with: THE DEFINITION.
        For each material m that has a law it is laws[m].correct(T_star, f, mask & (ids == m), dir_mask, cp_m), one fp64
        operation per line there; the results are composed over the disjoint cell sets.  Cells of a material without a law,
        off-mask cells, Dirichlet cells and cells at rest keep T_star and f bit for bit."""
        Tst = np.asarray(T_star, dtype=np.float64)
        f = np.asarray(f, dtype=np.float64)
        mask = np.asarray(mask, dtype=bool)
        ids = np.asarray(ids)
        laws = MapPhaseField._checked_laws(laws, materials)
        T_out, f_out = Tst, f
        for m, (law, (_, cp, _)) in enumerate(zip(laws, _triples(materials))):
            if law is None:
                continue
            cells = mask & (ids == m)
            Tm, fm = law.correct(Tst, f, cells, dir_mask, cp)
            T_out = np.where(cells, Tm, T_out)
            f_out = np.where(cells, fm, f_out)
        return T_out, f_out

    def correct(self, T_star, f, mask, ids, dir_mask):
        """correct_of with this object's laws and its MaterialMap's materials"""
        return self.correct_of(self.laws, self.mm.materials, T_star, f, mask, ids, dir_mask)

    @staticmethod
    def f_eq_of(laws, T, mask, ids):
        """what seed(T) leaves in f: f_eq(T) of the cell's own law on the mask, 0 off it and where the material has none"""
        T = np.asarray(T, dtype=np.float64)
        mask = np.asarray(mask, dtype=bool)
        ids = np.asarray(ids)
        f = np.zeros(T.shape)
        for m, law in enumerate(laws):
            if law is not None:
                f = np.where(mask & (ids == m), law.f_eq(T), f)
        return f


class MapLossPacks(_MapLoss):
    """The packs of a MaterialMap whose Robin coefficient arrays are REWRITTEN IN PLACE on the device from the temperature field
    (adi_matmap_loss_update), every exposed cell by the SurfaceLoss and the heat capacity of its own material.
    loss: one SurfaceLoss for every material, or a sequence with one per material; they are taken as they are at construction
    (their constants go into a small device table this object owns and uploads here, never inside a captured region).  The
    MaterialMap must have been built with robin_h=None: its coefficient arrays are rewritten here.  `.packs is mm.packs`; pass
    the object to the step as `surface_loss=` next to `material_map=mm`.
        update(T, Tinf=None)                         before a step: the in-mask cells exposed along an axis only
        rebuild(T, k_begin=0, k_end=None, Tinf=None) the planes [k_begin, k_end) of axis 2 in full: zeros where not exposed
    A stale MapLossPacks is not an error: after `grid.mask` changed, `mm.rebuild()` (which the step demands) leaves the
    coefficient arrays zero wherever no h was given -- everywhere -- and the next update writes every cell that is exposed now, so
    the arrays are those of the new mask without a rebuild here.  T (optional, here): the field the arrays are evaluated from at
    once.  `coeff_reference` is the definition in NumPy fp64."""

    def __init__(self, mm, loss, Tinf, T=None):
        if not isinstance(mm, MaterialMap):
            raise TypeError("MapLossPacks: mm must be a MaterialMap")
        n = len(mm.materials)
        self.losses = self._checked_losses(loss, n)
        for w in self.losses:
            w.validate(Tinf)
        if mm._bc['robin_h'] is not None:
            raise ValueError("MapLossPacks: the MaterialMap was built with robin_h; build it with robin_h=None, its coefficient "
                             "arrays are rewritten in place")
        self.mm, self.grid, self.Tinf = mm, mm.grid, float(Tinf)
        self.packs = mm.packs
        self._coeff = ptr_array([p.d_coeff.data_ptr() for p in self.packs])
        self._keys = tuple(w.key() for w in self.losses)
        self._min_offset = min(float(w.T_offset) for w in self.losses)
        nbytes = int(lib.adi_matmap_loss_table_bytes())
        host = torch.zeros(nbytes, dtype=torch.uint8)
        laws = (_lib.SurfaceLossLaw * n)(*[w.as_c() for w in self.losses])
        C = (ctypes.c_double * n)(*[m.rho * m.cp for m in mm.materials])
        check(lib.adi_matmap_loss_table(n, laws, C, self.grid.dx, ctypes.c_void_p(host.data_ptr()), nbytes))
        self._table = host.to(_device())
        if T is not None:
            self.rebuild(T)

    @staticmethod
    def _checked_losses(loss, n):
        losses = (loss,) * n if isinstance(loss, SurfaceLoss) else loss
        try:
            losses = tuple(losses)
        except TypeError:
            raise TypeError("MapLossPacks: loss must be a SurfaceLoss or a sequence with one per material")
        if len(losses) != n:
            raise ValueError("MapLossPacks: %d losses for %d materials" % (len(losses), n))
        if not all(isinstance(w, SurfaceLoss) for w in losses):
            raise TypeError("MapLossPacks: loss must be a SurfaceLoss or a sequence with one per material")
        return losses

    def _launch(self, T, Tinf, k0, k1, full):
        g = self.grid
        t = _native_f64(g, T)                                 # host arrays / foreign tensors: a copy (not the step's path)
        check(lib.adi_matmap_loss_update(_p(self._table), float(self.Tinf if Tinf is None else Tinf), self._min_offset, _p(t),
                                         _p(g.d_flags), _p(g.d_bricks), _p(self.mm._d_ids), *g.layout.pd, g.dx, self._coeff,
                                         int(k0), int(k1), int(full), _stream()))

    def update(self, T, Tinf=None):
        """the per-step mode over the whole box, from the device field T (DeviceField or tensor in the grid's layout);
        Tinf: the step's ambient (default: the one given at construction)"""
        self._launch(T, Tinf, 0, self.grid.layout.pz, 0)
        return self.packs

    def rebuild(self, T, k_begin=0, k_end=None, Tinf=None):
        """the full mode on the planes [k_begin, k_end) of axis 2 (clipped to the box), for the grid's CURRENT mask"""
        g = self.grid
        whole = k_end is None and int(k_begin) <= 0
        k0 = max(0, int(k_begin))
        k1 = g.layout.pz if whole else min(g.nz, g.nz if k_end is None else int(k_end))
        if k1 > k0:
            self._launch(T, Tinf, k0, k1, 1)
        return self.packs

    def graph_key(self):
        """what a captured launch holds: the laws by value (as uploaded), the ambient given here, the table by pointer"""
        return (self._keys, self.Tinf, self._table.data_ptr())

    @staticmethod
    def coeff_reference(T, mask, ids, materials, dx, losses, Tinf):
        """the three coefficient arrays: THE DEFINITION -- the `coeff` arrays of MaterialMap.packs_reference(mask, ids, materials,
        dx, robin_h={face: h_face}) with h_face = losses[ids].h_of(T, face, Tinf) chosen cell by cell"""
        mask = np.asarray(mask, dtype=bool)
        losses = MapLossPacks._checked_losses(losses, len(_triples(materials)))
        idm = np.where(mask, ids, 0)
        h = {}
        for face in FACES:
            hf = np.zeros(mask.shape)
            for m, w in enumerate(losses):
                hf = np.where(idm == m, w.h_of(T, face, Tinf), hf)
            h[face] = hf
        return tuple(p.coeff for p in MaterialMap.packs_reference(mask, ids, materials, dx, robin_h=h))


class MapSource(_MapSource):
    """A moving GoldakSource for the step of one MaterialMap: pass it as `S=` of adi_step_numba_coeff or `source=` of
    StagedStepper next to `material_map=mm`.  The one-material step corrects the output of sweep 0 by superposition, which
    assumes one coupling along a line; here the source is added to the explicit stage's output instead, one thread per cell of the
    support (adi_matmap_source_add_r0):
        R0 = R0 + (dt * q(t_n + dt/2)) / C[id]     on the in-mask cells the support reaches,
    the operations of the field form S=src.sample_device(grid, t + dt/2), in its order, without the field.  The time comes from
    the device block of adi_source_set / adi_source_tick, so a captured step replays it; power, origin, velocity, eta and f_f of
    `src` may change between the runs of a StagedStepper without a new graph, the extent of its support recaptures.
    It is not a GoldakSource: the bare object next to material_map= is still refused."""

    def __init__(self, mm, src):
        if not isinstance(mm, MaterialMap):
            raise TypeError("MapSource: mm must be a MaterialMap")
        if not isinstance(src, GoldakSource):
            raise TypeError("MapSource: src must be a GoldakSource, got %s" % type(src).__name__)
        src.validate()
        self.mm, self.grid, self.src = mm, mm.grid, src

    def shape_key(self):
        """what the launch box depends on (a change recaptures a stepper's graph): the wrapped source's, marked as a map's"""
        return ('map',) + self.src.shape_key()

    def set_block(self, blk, t0, dt, n=0):
        self.src.set_block(blk, t0, dt, n)

    def add_r0(self, R0, params, blk):
        """R0 (a device tensor in the grid's layout, the explicit stage's output) gains the source of the block `blk` at its
        mid-step time, in place: one launch"""
        mm, g = self.mm, self.grid
        _, C = mm._tables(params.dt)
        check(lib.adi_matmap_source_add_r0(_p(blk), ctypes.byref(self.src.as_c()), _p(R0), _p(g.d_flags), _p(mm._d_ids),
                                           *g.layout.pd, g.dx, params.dt, len(mm.materials), C, _stream()))

    def explicit_rhs(self, T, params, t=0.0):
        """R0 of the step that starts at time t (stage entry point): mm.explicit_rhs(T, params) plus this source at t + dt/2"""
        mm, g = self.mm, self.grid
        mm._check_fresh()
        x, kind = _as_state(T, g)
        out = g.layout.empty()
        mm._explicit_into(x, None, out, params)
        blk = _source_block(self)
        self.set_block(blk, t, params.dt)
        self.add_r0(out, params, blk)
        return _wrap(out, kind)


class MapPathSource(_MapPathSource):
    """A ScanPath for the step of one MaterialMap, without a source field: pass it as `S=` of adi_step_numba_coeff next to
    `material_map=mm` and `t=`.  src: a ScanPathSource, or a ScanPath, which is frozen here with on_device().  After the map's
    explicit stage and before sweep 0 one launch adds the step-averaged source of [t, t + dt] to the stage's output,
        R0 = R0 + (dt * q_step(x; t, dt)) / C[id]     on the in-mask cells of the window's index box,
    the operations of the field form S=src.sample_step_device(grid, t, dt), in its order, with q_step evaluated in the kernel
    (adi_matmap_scan_add_r0): the results are equal bit for bit, and neither the field's pass over the grid nor its 8 B/cell in
    the explicit stage is paid.  The segment range and the box of each step are found on the host from the snapshot's table
    and travel by value, so these are plain launches only: a StagedStepper refuses it (TypeError), and nothing is replayed.
    Combines with everything the field form combines with.  `window(t, dt)` is what a step will launch on."""

    def __init__(self, mm, src):
        if not isinstance(mm, MaterialMap):
            raise TypeError("MapPathSource: mm must be a MaterialMap")
        if isinstance(src, ScanPath):
            src = src.on_device()
        if not isinstance(src, ScanPathSource):
            raise TypeError("MapPathSource: src must be a ScanPath or a ScanPathSource, got %s" % type(src).__name__)
        self.mm, self.grid, self.src = mm, mm.grid, src

    def _h_table(self):
        """the library's path arguments with the snapshot's HOST table: (shape, table, K, t_end)"""
        return self.src._path_args(self.src._h_table.ctypes.data)

    def window(self, t, dt):
        """(k0, k1, ((i0, i1), (j0, j1), (k0', k1'))): the segments [k0, k1) the step [t, t + dt] can overlap and the index box
        its launch covers, [lo, hi) per axis; the box is all zeros when the step meets no powered piece"""
        g = self.grid
        seg, box = (ctypes.c_int * 2)(), (ctypes.c_int * 6)()
        check(lib.adi_scan_window_box(*self._h_table(), int(g.nx), int(g.ny), int(g.nz), float(g.dx), float(t), float(dt),
                                      seg, box))
        return seg[0], seg[1], ((box[0], box[1]), (box[2], box[3]), (box[4], box[5]))

    def add_r0(self, R0, params, t):
        """R0 (a device tensor in the grid's layout, the explicit stage's output) gains the source of the step [t, t + dt], in
        place: one launch on the window's box, none when it is empty"""
        mm, g, s = self.mm, self.grid, self.src
        _, C = mm._tables(params.dt)
        shape, h_table, K, t_end = self._h_table()
        check(lib.adi_matmap_scan_add_r0(shape, h_table, _p(s.d_table), K, t_end, _p(R0),
                                         _p(g.d_flags), _p(mm._d_ids), *g.layout.pd, g.dx, float(t), params.dt,
                                         len(mm.materials), C, None, _stream()))

    def explicit_rhs(self, T, params, t=0.0):
        """R0 of the step that starts at time t (stage entry point): mm.explicit_rhs(T, params) plus this path over [t, t + dt]"""
        mm, g = self.mm, self.grid
        mm._check_fresh()
        x, kind = _as_state(T, g)
        out = g.layout.empty()
        mm._explicit_into(x, None, out, params)
        self.add_r0(out, params, t)
        return _wrap(out, kind)


class MaterialTransitions(_MapTransitions):
    """Cells of a MaterialMap that change their material because of what the step did to them: loose powder that reaches its
    liquidus is dense metal for the rest of the run, a flux burns off, a wire that was molten once has other properties.
    rules: one entry per material of `mm`, None or (to, T_at): a cell of that material whose temperature is at or above T_at
        (finite) becomes material `to` (another material of the map).
    phase (optional): the MapPhaseField of the same map the step runs with; a changed cell's f becomes f_eq(T) under the law of
        its new material, 0 if that has none (the field's invariant: f = 0 in law-less cells).
    Pass it to the step as `transitions=` next to `material_map=mm` (and `phase=` if given here): one launch on the step's output
    after the latent-heat correction and before the recorders, captured into a StagedStepper's graph -- so ids change between
    replayed steps, without a host round trip or a rebuild().

    THE MODEL: the properties switch at constant temperature.  T is never written, so the heat content sum C_id V T jumps by
    (C_to - C_m) V T per changed cell, as in finite-element powder-bed codes that swap the property set at the liquidus; the
    switch does not conserve enthalpy (a FieldMonitor's sum_wT shows the jump, with the new ids).  A cell changes at most once
    per step: where the new material has a rule of its own and the cell is hot enough for that too, it waits for the next step.
    In-mask cells only; Dirichlet cells never change.

    A changed cell gets its id byte, its six pack values (those mm.rebuild() would write: they depend on the cell's own id and
    its neighbours' mask only) and, with `phase`, its f.  With a MapLossPacks the map was built with robin_h=None, so the three
    `coeff` values written here are the zeros of that build until the next step's adi_matmap_loss_update -- the first launch of
    that step -- rewrites every exposed cell: no step ever reads the zeros, and no second loss evaluation is made here.

    The pass reads one word per 16^3 brick first, the set of ids among the brick's in-mask cells: `phase.brick_ids` itself when a
    phase is given (no copy; the pass keeps those words exact), an array of the same definition this object owns otherwise
    (adi_matmap_brick_sets).  The object remembers grid.mask_version and the map's id version: after either changed the step
    raises ValueError until sync_mask() (after mph.sync_mask(T) when there is a phase).  A transition itself is no such change:
    a captured graph holds the id field by pointer.  After a launch `mm.ids` downloads the field, after the replays of
    StagedStepper.run too (after_replay).  Needs mm.ids_all_valid.
        apply(T, d_dir_mask=None)   the pass on a device field in the grid's layout (T is only read): one launch
        changed / reset_count()     the cells changed since construction or the last reset (reading it synchronises)
        sync_mask()                 see above
        snapshot() / restore(s)     the id field, the words and the counter; restore also rewrites the packs (mm.update)
    `apply_reference` is the definition in NumPy fp64."""

    def __init__(self, mm, rules, phase=None):
        if not isinstance(mm, MaterialMap):
            raise TypeError("MaterialTransitions: mm must be a MaterialMap")
        self.rules = self._checked_rules(rules, len(mm.materials))
        if phase is not None:
            if not isinstance(phase, MapPhaseField):
                raise TypeError("MaterialTransitions: phase must be a MapPhaseField, got %s" % type(phase).__name__)
            if phase.mm is not mm:
                raise ValueError("MaterialTransitions: the MapPhaseField belongs to another MaterialMap")
        if not mm.ids_all_valid:
            raise ValueError("MaterialTransitions: the id field holds an id that names no material (off the mask); restore() "
                             "rewrites the packs with MaterialMap.update, which needs every id below %d" % len(mm.materials))
        self.mm, self.grid, self.phase = mm, mm.grid, phase
        self._count = torch.zeros(1, dtype=torch.int64, device=_device())
        n = len(self.rules)
        self._to = (ctypes.c_int * n)(*[-1 if r is None else r[0] for r in self.rules])
        self._T_at = (ctypes.c_double * n)(*[0.0 if r is None else r[1] for r in self.rules])
        self._C = (ctypes.c_double * n)(*[m.rho * m.cp for m in mm.materials])
        self._mask_version = self._ids_version = None
        if phase is None:
            nw = int(lib.adi_phase_summary_words(*self.grid.layout.pd[:3]))
            if nw <= 0:
                raise ValueError("MaterialTransitions: bad grid")
            self.brick_ids = torch.zeros(nw, dtype=torch.int32, device=_device())
        else:
            self.brick_ids = phase.brick_ids
        self.sync_mask()

    @staticmethod
    def _checked_rules(rules, nmat):
        """the rules as a tuple of None / (int to, float T_at) after the checks of the constructor (nothing is launched before
        they pass)"""
        try:
            rules = tuple(rules)
        except TypeError:
            raise TypeError("MaterialTransitions: rules must be a sequence with one (to, T_at) or None per material")
        if len(rules) != nmat:
            raise ValueError("MaterialTransitions: %d rules for %d materials" % (len(rules), nmat))
        out = []
        for m, rule in enumerate(rules):
            if rule is None:
                out.append(None)
                continue
            try:
                to, T_at = rule
            except (TypeError, ValueError):
                raise TypeError("MaterialTransitions: a rule must be (to, T_at) or None, got %r" % (rule,))
            if isinstance(to, bool) or not isinstance(to, (int, np.integer)):
                raise TypeError("MaterialTransitions: the new material of a rule must be an int, got %r" % (to,))
            if not 0 <= int(to) < nmat:
                raise ValueError("MaterialTransitions: material %d turns into %d, there are %d materials" % (m, to, nmat))
            if int(to) == m:
                raise ValueError("MaterialTransitions: material %d turns into itself" % m)
            try:
                T_at = float(T_at)
            except (TypeError, ValueError):
                raise TypeError("MaterialTransitions: the temperature of a rule must be a real number, got %r" % (T_at,))
            if not np.isfinite(T_at):
                raise ValueError("MaterialTransitions: the temperature of the rule of material %d is not finite" % m)
            out.append((int(to), T_at))
        return tuple(out)

    def _check_fresh(self):
        if self.grid.mask_version != self._mask_version or self.mm._ids_version != self._ids_version:
            raise ValueError("MaterialTransitions: the grid's mask or the MaterialMap's ids changed since the bricks' id sets "
                             "were built; call sync_mask()")
        if self.phase is not None:
            self.phase._check_fresh()

    def sync_mask(self):
        """after `grid.mask` or the MaterialMap's ids changed (a birth, a deposit, set_ids): the bricks' id sets are rebuilt
        when this object owns them; with a phase they are the MapPhaseField's, whose own sync_mask(T) comes first"""
        g = self.grid
        if self.phase is not None:
            self.phase._check_fresh()
        else:
            check(lib.adi_matmap_brick_sets(_p(g.d_flags), _p(g.d_bricks), _p(self.mm._d_ids), _p(self.brick_ids), *g.layout.pd,
                                            _stream()))
        self._mask_version, self._ids_version = g.mask_version, self.mm._ids_version

    @property
    def changed(self):
        """the cells changed since construction or reset_count() (synchronises)"""
        return int(self._count.item())

    def reset_count(self):
        self._count.zero_()

    def apply(self, T, d_dir_mask=None):
        """adi_matmap_transition from T (a DeviceField or device tensor in the grid's layout; only read); d_dir_mask: the
        Dirichlet cells as a uint8 device tensor in the grid's layout (default: those of the map's packs)"""
        g, mm, ph = self.grid, self.mm, self.phase
        t = _native_f64(g, T, "MaterialTransitions.apply: T must be a fp64 device field in the grid's layout")
        self._check_fresh()
        mm._check_fresh()
        dm = d_dir_mask
        if dm is None and mm.packs[2].has_dir:
            dm = mm.packs[2].d_dir_mask
        if dm is not None:
            assert g.layout.is_native(dm) and dm.dtype == torch.uint8
        laws = on = None
        if ph is not None:
            _, laws, on = ph._c_laws()
        h_specs, q_specs = mm._face_args()
        check(lib.adi_matmap_transition(len(self.rules), self._to, self._T_at, laws, on, _p(t), _p(mm._d_ids), _p(g.d_flags),
                                        _p(g.d_bricks), _p(g.d_mask), _p(dm), _p(None if ph is None else ph.f),
                                        _p(None if ph is None else ph.summary), _p(self.brick_ids), _p(self._count),
                                        *g.layout.pd, g.dx, self._C, *_face_spec_args(h_specs), *_face_spec_args(q_specs),
                                        ptr_array([p.d_coeff.data_ptr() for p in mm.packs]),
                                        ptr_array([p.d_qflux.data_ptr() for p in mm.packs]), _stream()))
        mm._ids_stamped = True
        return T

    def after_replay(self):
        """StagedStepper.run calls this after it replayed a graph that holds this object's pass: the device id field may have
        changed without a call of apply(), so the map's host copy is stale and `mm.ids` downloads the field when it is read next.
        Nothing is launched or synchronised here."""
        self.mm._ids_stamped = True

    def snapshot(self):
        return self.mm._d_ids.clone(), self.brick_ids.clone(), self._count.clone()

    def restore(self, s):
        """the id field, the words and the counter as they were, and the packs rewritten for those ids (MaterialMap.update over
        the whole box: one launch, nothing read back)"""
        self.mm._d_ids.copy_(s[0])
        self.brick_ids.copy_(s[1])
        self._count.copy_(s[2])
        self.mm.update(0, self.grid.layout.pz)

    def graph_key(self):
        """what a captured launch holds: the rules by value; the id field, the words, the counter and the six pack arrays by
        pointer; of the phase its laws by value and f and the summary by pointer"""
        ph = self.phase
        return (self.rules, self.mm._d_ids.data_ptr(), self.brick_ids.data_ptr(), self._count.data_ptr(),
                tuple(p.d_coeff.data_ptr() for p in self.mm.packs), tuple(p.d_qflux.data_ptr() for p in self.mm.packs),
                None if ph is None else (tuple(None if w is None else w.key() for w in ph.laws), ph.f.data_ptr(),
                                         ph.summary.data_ptr()))

    # ---- the definition in NumPy fp64 -------------------------------------------------------------------------------------
    @staticmethod
    def apply_reference(rules, T, f, mask, ids, dir_mask, laws):
        """(ids_new, f_new, n_changed) of one pass over the field T: THE DEFINITION.  A cell changes exactly when it is in the
        mask, is not a Dirichlet cell (dir_mask; None: none), its material m has a rule (to, T_at) and T >= T_at -- equality
        changes it, a NaN does not -- and it changes once: the test is made on the ids the pass found.  f, laws: the liquid
        fraction and the laws of the MapPhaseField (both None: no phase, f_new is None); a changed cell gets f_eq(T) of the
        law of its new material (MapPhaseField.f_eq_of's operations), 0 where that has none; every other f is kept."""
        T = np.asarray(T, dtype=np.float64)
        mask = np.asarray(mask, dtype=bool)
        ids = np.asarray(ids)
        rules = MaterialTransitions._checked_rules(rules, len(rules))
        free = mask if dir_mask is None else mask & ~np.asarray(dir_mask, dtype=bool)
        ids_new = np.array(ids)
        f_new = None if f is None else np.array(f, dtype=np.float64)
        changed = np.zeros(mask.shape, bool)
        for m, rule in enumerate(rules):
            if rule is None:
                continue
            to, T_at = rule
            with np.errstate(invalid='ignore'):
                hot = T >= T_at
            of_m = ids == m
            cells = free & of_m
            cells = cells & hot
            ids_new = np.where(cells, np.asarray(to, ids_new.dtype), ids_new)
            changed = changed | cells
            if f_new is not None:
                law = laws[to]
                fe = np.zeros(T.shape) if law is None else law.f_eq(T)
                f_new = np.where(cells, fe, f_new)
        return ids_new, f_new, int(changed.sum())
