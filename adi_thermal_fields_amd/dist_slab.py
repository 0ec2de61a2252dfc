"""dist_slab -- the Cartesian ADI step on a grid cut into slabs along memory axis 0, one slab per GPU.

The reference is single-process (no NCCL/MPI anywhere); this module is the multi-GPU
part of the north star: one process per GPU, `torch.distributed` (backend "nccl" = RCCL over xGMI).

Per step and rank (nxl local planes, halo planes at both ends of every extended array):
  1. halo exchange of the state: one (ny, nz) plane to each neighbour (send/recv, 2 MiB at 512^2);
     the mask halo travels only when the mask changes (pack rebuild).
  2. explicit stage on the extended slab (interior result used).
  3. axis-0 sweep, whose lines span all ranks, as a reduced-interface solve:
       pass A  adi_sweep_condense: rows of every local line -> 6 numbers (first/last unknown as affine functions
               of the neighbours' adjacent unknowns),
       exchange + interface solve -> the two boundary values of every line,
       pass B  adi_sweep with the boundary values injected: the ordinary local sweep.
     Two forms of the middle step, chosen per (dt, theta, mask) by looking at the condensed matrix entries:
       neighbour-only ("windowed"): the coupling of a slab's last unknown to the unknown BEFORE the slab (aL), and
               of its first unknown to the one AFTER it (cF), decays like rho^rows (rho < 1 from diagonal
               dominance).  When both are <= 1e-17 on every line -- below the rounding of the data they would
               multiply -- the interface system splits into independent 2x2 systems between neighbours:
               send (gF,aF) down and (gL,aL,cL) up (send/recv, 6.3 + 4.2 MB at 512^2), adi_interface_pair.
               When the decay length K is below half the slab, pass A runs only on the first and last K planes
               (the same argument applied to the window) and its exchange hides behind the explicit stage of
               the middle planes.
       exact:  all_gather of the (6, ny*nz) block (12.6 MB per rank at 512^2) + adi_interface_solve (each rank
               merges the slabs below/above it and solves a 2x2 system per line); thin slabs / huge dt.
     Either way the result equals the single-domain sweep to rounding.
  4. axis-1 and axis-2 sweeps: lines are local, no communication.

The numerical work is behind an `engine` (slab_engine.HipEngine: HIP kernels through the C ABI in production) and the
exchange behind a `comm` (slab_comm; both re-exported here), so the algebra of the decomposition can be tested on CPU ranks over gloo with a
reference engine (tests/) and, on one GPU, with several in-process ranks.
"""
import ctypes
import types

import numpy as np
import torch

from .slab_comm import (TorchDistComm, HostStagedDistComm, LocalComm, LoopbackComm, SelfLoopDistComm, split_planes,   # noqa: F401
                        rccl_env_defaults, gather_slabs)
from .slab_engine import HipEngine

__all__ = ['SlabStepper', 'TorchDistComm', 'HostStagedDistComm', 'LocalComm', 'LoopbackComm', 'SelfLoopDistComm', 'HipEngine',
           'split_planes', 'rccl_env_defaults', 'gather_slabs']


def _interior(t_ext):
    """planes 1..n-2 of an extended array: same strides, pointer advanced by one plane"""
    return t_ext[1:-1]


class SlabStepper:
    """One rank's slab.  step(T) takes / returns the LOCAL (nxl, ny, nz) field (DeviceField, torch tensor or
    NumPy array); the state stays in HBM when fed back what step() returned."""

    _comm_priority = -1           # the side stream is a high-priority one: a HSA queue of its own (see rccl_env_defaults)

    def __init__(self, mask_local, dx, mat, params, Tinf=0.0, dir_mask=None, dir_value=None, neumann=None,
                 robin_h=None, comm=None, engine=None, source=None):
        self.engine = engine or HipEngine()
        self.comm = comm or TorchDistComm()
        self.rank, self.world = self.comm.rank, self.comm.world
        self._first, self._last = self.rank == 0, self.rank == self.world - 1      # the ranks at the ends of the global grid
        self.mat, self.params, self.Tinf, self.dx = mat, params, float(Tinf), float(dx)
        self._bc = dict(dir_mask=dir_mask, dir_value=dir_value, neumann=neumann, robin_h=robin_h)
        mask_local = np.asarray(mask_local).astype(np.bool_)
        E = self.engine
        # Padded planes: a ragged (ny, nz) would send every strided line to the GENERAL kernels (adi_recommended_dims, DESIGN.md
        # section 2), so every internal array of the slab has planes of (self.ny, self.nz) >= the caller's (self.lny, self.lnz);
        # the cells beyond are off-mask, the planes that travel are the physical ones, and step() / set_mask() take and return
        # the logical box.  The extents depend on (ny, nz) alone: every rank picks the same.
        self.nxl, self.lny, self.lnz = mask_local.shape
        self.ny, self.nz = E.plane_dims(self.lny, self.lnz) if hasattr(E, 'plane_dims') else (self.lny, self.lnz)
        self._padded = (self.ny, self.nz) != (self.lny, self.lnz)
        self.Lext = E.layout(self.nxl + 2, self.ny, self.nz)
        self.Lint = E.layout(self.nxl, self.ny, self.nz)
        assert self.Lint.sx == self.Lext.sx
        self.nlines = self.ny * self.nz
        # zero-filled once: the outer halo planes of the first / last rank and the padded tail of every plane are never
        # written; the kernels read them only through selects today, and must not meet NaNs if that ever changes
        self._ext_bufs = [self.Lext.empty(zero=True), self.Lext.empty(zero=True)]
        self._cur = 0
        self._tmp = [self.Lext.empty(zero=True), self.Lext.empty(zero=True)]
        self._mask_version = 0
        self._a0_key, self._a0, self.axis0_mode = None, None, None
        self._no_overlap, self._force_exact = False, False
        self._allow_window = True                  # False keeps 'window' plans off (whole-slab condensation only)
        self._allow_fused = True                   # False: explicit stage as its own kernel (R0 through HBM)
        self.fused = False
        self._keep_r0 = True                       # False: pass B re-evaluates the explicit stage instead of reading R0
        self._allow_dots = True                    # False: pass A as its own kernel (reads the slab a second time)
        self._allow_deferred = True                # False: never the deferred form (zero-boundary solve + correction on load)
        self._allow_deferred_exact = True          # False: thin slabs (no decay) keep the two-pass all-gather form
        self._allow_deferred_lines = True          # False: lines that are not uniform keep the two-pass forms
        self._deferred_lines_cost_ratio = 1.0      # ... and so do slabs whose flagged lines cost more than this x pass A (tests: inf)
        self._plan_steps = None                    # steps taken under the current axis-0 plan (None: no plan yet)
        self._allow_quick_replan = True            # False: every plan is made by the full (measuring) planner
        self._dots_sticky, self._nx_all, self._fused_by_K, self._chunk_cache = None, None, {}, {}
        self._send_g_only = True                   # False: every step exchanges the matrix parts of the interface too
        self._comm_stream, self._use_streams = None, False
        self._halo_ready, self._halo_event = None, None
        self._gam = 0.0
        self.source, self._i_org = None, None
        self.set_source(source)
        self.set_mask(mask_local)

    def _pad(self, a, fill=0):
        """host array over the caller's planes (n, lny, lnz) -> the slab's physical planes (n, ny, nz); scalars / None as they are"""
        if not self._padded or a is None or np.isscalar(a):
            return a
        a = np.asarray(a)
        assert a.shape[1:] == (self.lny, self.lnz), (a.shape, (self.lny, self.lnz))
        out = np.full((a.shape[0], self.ny, self.nz), fill, dtype=a.dtype)
        out[:, :self.lny, :self.lnz] = a
        return out

    pad = _pad

    def _logical(self, t):
        """the caller's box of an internal (n, ny, nz) tensor (a view)"""
        return t[:, :self.lny, :self.lnz] if self._padded else t

    def state_interior(self, T):
        """the caller's box of the state buffer holding the local field T, for writing into the state in place between steps (a
        layer birth): T itself when it is what step() returned, else the buffer's view after T has been copied in (nothing
        stepped yet)"""
        if isinstance(T, torch.Tensor) and T.data_ptr() == _interior(self._ext_bufs[self._cur]).data_ptr():
            return T
        return self._logical(_interior(self._load_state(T)))

    def mask_interior(self, logical=False):
        """the device mask of the slab's own planes (a view of d_mask_ext; uint8, physical planes, or the caller's box of them):
        cells switched on in it take effect with the next set_mask_device"""
        m = _interior(self.d_mask_ext)
        return self._logical(m) if logical else m

    @classmethod
    def from_local(cls, T0_local, mask_local, dx, mat, params, Tinf, **kw):
        """convenience for bench.py: stepper for this rank's slab (T0 only fixes nothing here; the field is
        passed to step())."""
        return cls(mask_local, dx, mat, params, Tinf, **kw)

    # -- mask / packs (rebuilt together, like the reference's drivers do after every birth) ----------
    def set_mask(self, mask_local):
        """grid.mask = ...; packs = precompute_coeff_packs_unified(...) for this slab.  Exchanges the mask
        halo planes, rebuilds the neighbour flags and the coefficient packs on the extended slab."""
        E, L = self.engine, self.Lext
        self._mask_version += 1
        if hasattr(E, 'mask_epoch'):
            E.mask_epoch += 1                      # what the engine learnt about empty unit queues belongs to the old mask
            E._nofb.clear()
        solid_logical = bool(np.asarray(mask_local).all())
        mask_local = self._pad(np.asarray(mask_local).astype(np.bool_), False)
        m_ext = np.zeros((self.nxl + 2, self.ny, self.nz), dtype=np.bool_)
        m_ext[1:-1] = mask_local
        d_mask = L.to_layout(m_ext, torch.uint8)
        lo = d_mask[0].contiguous(); hi = d_mask[-1].contiguous()
        self.comm.exchange_planes(d_mask[1].contiguous(), d_mask[-2].contiguous(), lo, hi)
        if self.rank > 0:
            d_mask[0].copy_(lo)
        if self.rank < self.world - 1:
            d_mask[-1].copy_(hi)
        self.d_mask_ext = d_mask
        if hasattr(E, 'box_hint'):                 # all-solid on every rank -> the kernels' leaner build (a hint only)
            self._solid_everywhere = self._all_ranks(solid_logical)          # the caller's box, on every rank
            E.box_hint = 2 if (self._solid_everywhere and not self._padded) else 0   # (the kernels' hint is about the physical box)
        self.flags_ext = E.build_flags(L, d_mask)

        def ext(a, fill):
            if a is None or np.isscalar(a):
                return a
            e = np.full((self.nxl + 2, self.ny, self.nz), fill, dtype=np.asarray(a).dtype)
            e[1:-1] = self._pad(a, fill)
            return e
        bc = self._bc
        neumann = None if bc['neumann'] is None else {f: ext(v, 0.0) for f, v in bc['neumann'].items()}
        robin_h = bc['robin_h']
        if isinstance(robin_h, dict):
            robin_h = {f: ext(v, 0.0) for f, v in robin_h.items()}
        else:
            robin_h = ext(robin_h, 0.0)
        self.packs_ext = E.build_packs(L, d_mask, self.flags_ext, self.dx, self.mat, ext(bc['dir_mask'], False),
                                       ext(bc['dir_value'], 0.0), neumann, robin_h)
        self.variant = self.packs_ext[0].variant
        from . import _lib
        self._bpc = [getattr(p, 'bytes_per_cell', float(_lib.SWEEP_BYTES_PER_CELL[self.variant])) for p in self.packs_ext]
        self._explicit_bpc = float(_lib.EXPLICIT_BYTES_PER_CELL)

        def interior_pack(p):
            return tuple(None if t is None else _interior(t) for t in (p.d_coeff, p.d_dir_mask, p.d_dir_val, p.d_qflux))
        self.packs_int = [interior_pack(p) for p in self.packs_ext]
        self.flags_int = _interior(self.flags_ext)

    def set_source(self, src):
        """Attach a moving heat source (an adi3d_hip_coeff.GoldakSource; its origin in global coordinates, cell centres at
        ((i0 + i + 1/2) dx, (j + 1/2) dx, (k + 1/2) dx) for local plane i of the slab that starts at global plane i0) or detach
        it (None).  Every rank attaches and detaches the same source at the same step: the plan depends on it (collective).
        Then step() needs t, the step's start time; the source is evaluated at t + dt/2."""
        if src is not None:
            from .heat_source import GoldakSource
            if not isinstance(src, GoldakSource):
                raise TypeError("SlabStepper: source must be a GoldakSource or None, not %s" % type(src).__name__)
            if not all(hasattr(self.engine, m) for m in ('source_set', 'source_lines0', 'source_add_r0')):
                raise NotImplementedError("SlabStepper: the engine %s has no heat-source kernels" % type(self.engine).__name__)
            src.validate()
        if (src is None) != (self.source is None):
            self._plan_steps = None                # attaching / detaching is no mask event: the next plan is a full one
        self.source = src

    def _plane_origin(self):
        """global plane of this rank's local plane 0 (collective the first time: the slab sizes of all ranks)"""
        if self._i_org is None:
            self._i_org = 0 if self.world == 1 else int(sum(self._slab_planes_of_all_ranks()[:self.rank]))
        return self._i_org

    def _source_meets(self, src, t, dt, i_org):
        """whether the support can meet this rank's planes at t + dt/2: the kernels' extent along axis 0 (src_extent), widened by
        one plane each side"""
        from ._lib import SOURCE_E_CUT
        R = np.sqrt(SOURCE_E_CUT / 3.0)
        if src.travel_axis == 0:
            lo, hi = (R * src.c_r, R * src.c_f) if src.travel_sign > 0 else (R * src.c_f, R * src.c_r)
        else:
            lo = hi = R * (src.b if src.depth_axis == 0 else src.a)
        c0 = float(src.center(float(t) + 0.5 * float(dt))[0])
        g_first = np.ceil((c0 - lo) / self.dx - 0.5) - 1.0
        g_last = np.floor((c0 + hi) / self.dx - 0.5) + 1.0
        return bool(g_last >= i_org and g_first <= i_org + self.nxl - 1)

    def _scalar_specs(self):
        """(h_mode, h_scalar, q_mode, q_scalar) ctypes arrays when every face specification is a scalar or absent, else None"""
        from ._lib import FACES, FACE_NONE, FACE_SCALAR
        bc = self._bc
        if bc['dir_mask'] is not None:
            return None
        hm, hs, qm, qs = [], [], [], []
        for f in FACES:
            rh = bc['robin_h']
            v = None if rh is None else (rh.get(f, 0.0) if isinstance(rh, dict) else rh)
            q = None if bc['neumann'] is None else bc['neumann'].get(f)
            for val, m_, s_ in ((v, hm, hs), (q, qm, qs)):
                if val is None:
                    m_.append(FACE_NONE); s_.append(0.0)
                elif np.isscalar(val):
                    m_.append(FACE_SCALAR); s_.append(float(val))
                else:
                    return None
        return ((ctypes.c_int * 6)(*hm), (ctypes.c_double * 6)(*hs), (ctypes.c_int * 6)(*qm), (ctypes.c_double * 6)(*qs))

    def device_births_supported(self):
        """layer births can be applied to the device mask in place (set_mask_device): the product engine, face
        specifications that are scalars, no Dirichlet cells"""
        return hasattr(self.engine, 'build_flags_planes') and self._scalar_specs() is not None

    def set_mask_device(self, k_begin, k_end):
        """`grid.mask = ...; packs = precompute_...` after a layer birth that switched cells on IN the device mask of the slab
        (the interior planes of self.d_mask_ext, planes [k_begin, k_end) of axis 2; waam.run_layer_birth_slab): the mask halo
        planes travel, the flags and the six coefficient arrays are rebuilt in place on the planes whose exposure can have
        changed -- no host copy of the mask, no allocation.  Collective (every rank calls it for every birth)."""
        E, L = self.engine, self.Lext
        specs = self._scalar_specs()
        assert specs is not None and hasattr(E, 'build_flags_planes')
        self._mask_version += 1
        E.mask_epoch += 1
        E._nofb.clear()
        d_mask = self.d_mask_ext
        self.comm.exchange_planes(d_mask[1], d_mask[-2], d_mask[0], d_mask[-1])     # (no neighbour: the halo plane stays empty)
        k0, k1 = max(0, int(k_begin) - 1), min(self.nz, int(k_end) + 1)
        E.build_flags_planes(L, d_mask, self.flags_ext, k0, k1)
        E.build_packs_planes(L, d_mask, self.packs_ext, self.dx, self.mat, specs, k0, k1)
        E.box_hint = 0                 # a part that is still growing is not an all-solid box
        self._solid_everywhere = False

    @property
    def stage_names(self):
        a0, a1 = ('sweep_axis0_distributed', 'sweep_axis1')
        if self._is_deferred(self._a0):
            a0, a1 = ('sweep_axis0_zero_boundary', 'interface+sweep_axis1_corrected')
        return (['halo+explicit+' + a0] if self._fused_now() else ['halo+explicit', a0]) + [a1, 'sweep_axis2_contig']

    @property
    def pass_a_form(self):
        """how pass A of the sharded-axis sweep runs under the current plan (bench.py reports it)"""
        p = self._a0 or {}
        if self._is_deferred(self._a0):
            return 'none (zero-boundary solve; planes 0 and n-1 of its result are the pass-A right-hand sides)'
        return 'dots_in_explicit' if p.get('dots') else ('fused' if p.get('fused') else 'separate')

    @property
    def stage_bytes_per_cell(self):
        """algorithmic HBM bytes per local cell of the stages (pass A re-reads the inputs of the rows it covers)"""
        bpc, p, fused = self._bpc, self._a0 or {}, self._fused_now()
        if self._is_deferred(self._a0):
            a0 = bpc[0]        # one pass per sweep; the two interface planes the axis-1 sweep re-reads are 2 * ny * nz values per slab
        elif fused and p.get('keep_r0'):
            a0 = 2.0 * bpc[0]                              # pass A: state + flags in, R0 out; pass B: R0 + flags in, U out
        else:
            frac = 0.0                                     # share of the slab that pass A reads a second time
            if self.world > 1 and not p.get('dots'):       # (dots: pass A rides on the explicit stage)
                frac = min(1.0, 2.0 * p['K'] / self.nxl) if p.get('mode') == 'window' else 1.0
            a0 = bpc[0] + frac * (bpc[0] - 8)
        return ([] if fused else [self._explicit_bpc]) + [a0, bpc[1], bpc[2]]

    def _fused_supported(self, K):
        """explicit stage folded into pass B (whole slab) and, with neighbours, into pass A on K planes"""
        E, L = self.engine, self.Lint
        if not self._allow_fused or not hasattr(E, 'sweep0_fused'):
            return False
        ok = E.fused_supported(self.nxl, self.ny, self.nz, L.sx, False)
        if self.world > 1:
            ok = ok and E.fused_supported(K, self.ny, self.nz, L.sx, True)
        return bool(ok)

    def _fused_now(self):
        if self.world > 1 and self._a0 is not None:
            return bool(self._a0['fused'])
        return self._fused_supported(self.nxl)

    @staticmethod
    def _as_tensor(T):
        """a local field in whatever form step() takes or returns it -> the torch tensor behind it (a NumPy array as it is)"""
        return T if isinstance(T, (torch.Tensor, np.ndarray)) else getattr(T, 't', T)

    @staticmethod
    def local_numpy(T):
        """host copy of a local field in whatever form step() returned it"""
        t = SlabStepper._as_tensor(T)
        return t if isinstance(t, np.ndarray) else t.cpu().contiguous().numpy()

    # -- the step -----------------------------------------------------------------------------------
    def _load_state(self, T):
        """-> extended buffer whose interior holds T (no copy when T is the view step() returned)."""
        t = self._as_tensor(T)
        for i, buf in enumerate(self._ext_bufs):
            if isinstance(t, torch.Tensor) and t.device == buf.device and \
                    t.data_ptr() == _interior(buf).data_ptr() and tuple(t.stride()) == tuple(buf.stride()):
                self._cur = i
                return buf
        buf = self._ext_bufs[self._cur]
        self._halo_ready = None                    # a foreign field: whatever halo was prefetched is not its halo
        src = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(t), dtype=np.float64))
        self._logical(_interior(buf)).copy_(src)
        return buf

    # -- how the axis-0 interface system is solved ------------------------------------------------------
    DECAY_TOL = 1e-17      # |aL|, |cF| at or below this are dropped (they multiply values of the size of the data)
    SLAB_CHUNK_EDGES = None      # e.g. (0.125, 0.5): cumulative line fractions of the 'slab' pipeline's chunks (None: halves)
    DOTS_MAX_NONUNIFORM = 0.05   # share of axis-0 lines that are not uniform above which pass A leaves the dot-product form

    def _chunk_ranges(self, nch, fractions=None):
        """chunks of lines (ranges of j) of the axis-0 pipeline.  fractions: cumulative edges in (0, 1), e.g. a small
        first chunk whose exchange is the only exposed one, each later exchange hiding behind the previous chunk's pass B"""
        if fractions is not None and self.ny >= 64:
            edges = [0] + [int(round(f * self.ny / 2.0)) * 2 for f in fractions] + [self.ny]
        else:
            nch = nch if self.ny >= 8 * nch else 1
            edges = [round(i * self.ny / nch) for i in range(nch + 1)]
        edges = sorted(set(edges))
        return [(edges[i], edges[i + 1]) for i in range(len(edges) - 1) if edges[i + 1] > edges[i]]

    def _streams(self):
        E = self.engine
        self._use_streams = (E.device.type == 'cuda') and isinstance(self.comm, TorchDistComm) \
            and not self._no_overlap
        if self._use_streams and self._comm_stream is None:
            self._comm_stream = torch.cuda.Stream(device=E.device, priority=self._comm_priority)
        return self._use_streams

    def _window_guess(self, gam):
        """rows after which the coupling through a run of interior rows (-tg, 1+2tg, -tg) has decayed below
        DECAY_TOL: rho = 2tg / (1 + 2tg + sqrt(1 + 4tg)) per row; every other row is more dominant"""
        tg = self.params.theta * gam
        if tg <= 0.0:
            return 8
        rho = 2.0 * tg / (1.0 + 2.0 * tg + np.sqrt(1.0 + 4.0 * tg))
        need = int(np.ceil(np.log(self.DECAY_TOL) / np.log(rho))) + 2
        K = 8
        while K < need:            # powers of two: the in-register condensation kernels tile those
            K *= 2
        return K

    # The plan of the axis-0 sweep is a plain dict, made once per (dt, theta, mask, knobs) and kept in self._a0.  Every form:
    #   mode      'window' | 'slab' | 'exact' (two passes) | 'deferred' | 'deferred_exact' | 'deferred_lines' (_is_deferred)
    #   K         planes pass A covers at each end ('window'), the slab's planes ('slab', 'exact'), the weights' reach (deferred; plus a margin in 'deferred_lines')
    #   fused     the explicit stage is folded into the axis-0 kernels;  keep_r0: ... and pass A stores R0 for pass B
    #   dots      pass A rides on the explicit stage as dot products, with dd = the engine's dots_setup (two-pass forms only)
    #   chunks    per chunk of lines of the two-pass pipeline (_chunk_buffers): j0, j1, nl, Lc, Lb, xlo, xhi and cond, cond_all
    #             ('exact') or cond_lo, cond_hi, prev_hi, next_lo; matrix_sent once the matrix parts have travelled; [] when deferred
    #   quick     True on a plan made by _quick_plan
    # and per form:
    #   window, slab      Lw, worst (layout and largest entry of the decay measurement; worst None on a quick plan)
    #   deferred*         dfr (the engine's deferred_setup: w, omega, reach), ulo, uhi
    #   deferred          prev_last, next_first
    #   deferred_exact    g, g_all, mat_all, scal_all, xlo, xhi, dx (the engine's deferred_exact_setup)
    #   deferred_lines    om, sides, nflag, ulo_uni, uhi_uni, prev_last, next_first
    @staticmethod
    def _is_deferred(plan):
        return plan is not None and plan['mode'].startswith('deferred')

    def _gather_flags(self, values):
        """every rank's `values` (a few numbers) -> (world, len(values)) fp64 tensor, the same on every rank.  Collective: ONE
        all-gather of len(values) doubles per rank"""
        E = self.engine
        mine = E.vec(len(values))
        for i, x in enumerate(values):
            mine[i] = float(x)
        allv = E.vec(len(values) * self.world)
        self.comm.all_gather(allv, mine)
        return allv.view(self.world, len(values))

    def _all_ranks(self, flag):
        """`flag` holds on every rank (collective: one number per rank)"""
        return bool(float(self._gather_flags([flag]).min()) >= 1.0)

    def _plan_axis0(self, Ti, gam):
        """-> plan dict for the current (dt, theta, mask) (the keys: above).  Collective: every rank calls it at the same step,
        and every candidate below is tried -- or not -- by all ranks alike."""
        prm = self.params
        key = (float(prm.dt), float(prm.theta), self._mask_version, self._force_exact, self._no_overlap,
               self._allow_fused, self._allow_window, self._keep_r0, self._allow_dots, self._allow_deferred,
               self._allow_deferred_exact, self._allow_deferred_lines, self._deferred_lines_cost_ratio, self._allow_quick_replan,
               self.source is not None)
        if self._a0_key == key:
            self._plan_steps += 1
            return self._a0
        # a plan that lives for a few steps only (a layer-birth loop: every birth changes the mask) does not repay the two
        # extra sweeps and host synchronisations the per-line deferred form costs per plan; the same on every rank
        short_lived = self._plan_steps is not None and self._plan_steps < 16
        self._plan_steps = 0
        self._streams()
        src_on = self.source is not None
        plan = self._quick_plan(gam, src_on) if short_lived and self._allow_quick_replan else None
        if plan is None:
            plan, fused_ok = self._plan_deferred(gam)
            plan = plan or self._plan_deferred_lines(gam, fused_ok, short_lived) or self._plan_two_pass(Ti, gam, src_on)
        self._a0_key, self._a0 = key, plan
        self.axis0_mode = plan['mode']
        return plan

    def _plan_deferred(self, gam):
        """-> (plan of the deferred form or None, whether every rank's fused kernel takes its whole slab).
        Deferred form first (its eligibility costs one pass over the flags and a host-side solve): every sharded-axis
        line of every slab uniform -- solid, no Dirichlet cell -- and the homogeneous solution decayed across every slab.
        Where the weights have NOT decayed across a slab (thin slabs: strong scaling) the same algebra holds with the
        interface system of all ranks (all-gather) and per-line end corrections on the first / last rank: 'deferred_exact'."""
        E, prm, nl_ = self.engine, self.params, self.nlines
        fl, pk = self.flags_int, self.packs_int[0]
        dfr, uniform = None, False
        if self._allow_deferred and hasattr(E, 'deferred_setup') and self.nxl >= 2 and prm.theta * gam > 0.0:
            # uniform lines need every cell of the slab in the mask: where the engine keeps the collective all-solid hint
            # (set_mask / set_mask_device) a slab that is not all-solid is not classified at all -- one kernel and one host
            # synchronisation less in every plan of a layer-birth loop
            if self._padded:
                # padded planes: the lines of the padding are off-mask, so the device classification would say "not uniform";
                # but they are identity rows of a state that is zero there for good, their boundary planes are zero, their
                # interface values and with them the correction come out as exact zeros -- what decides is the caller's box
                uniform = bool(getattr(self, '_solid_everywhere', False)) and self._bc['dir_mask'] is None
            else:
                uniform = (getattr(E, 'box_hint', 2) == 2) and bool(E.lines_all_uniform(self.Lint, fl, pk[1]))
            if uniform:
                dfr = E.deferred_setup(self.nxl, prm.theta, gam, self.DECAY_TOL)
        # (the rank-local gate above sits in front of an all-gather every rank takes part in, whatever it found)
        alld = self._gather_flags([dfr is not None,
                                   self._allow_fused and hasattr(E, 'sweep0_fused')
                                   and E.fused_supported(self.nxl, self.ny, self.nz, self.Lint.sx, False),
                                   dfr is not None and dfr['reach'] < self.nxl])
        fused_ok = bool(float(alld[:, 1].min()) >= 1.0)
        if float(alld[:, 0].min()) < 1.0:
            return None, fused_ok
        all_decayed = float(alld[:, 2].min()) >= 1.0 and not self._force_exact
        plan = dict(mode='deferred' if all_decayed else 'deferred_exact', K=dfr['reach'], dfr=dfr, fused=fused_ok, dots=False,
                    keep_r0=False, chunks=[], ulo=E.vec(nl_), uhi=E.vec(nl_))
        if all_decayed:
            plan.update(prev_last=E.vec(nl_), next_first=E.vec(nl_))
        elif hasattr(E, 'deferred_exact_setup') and self._allow_deferred_exact:
            plan['dfr'] = E.deferred_setup(self.nxl, prm.theta, gam, 0.0)          # no weight is cut
            mat, scal = E.vec(4 * nl_), E.vec(2)
            plan.update(g=E.vec(2 * nl_), g_all=E.vec(2 * nl_ * self.world), mat_all=E.vec(4 * nl_ * self.world),
                        scal_all=E.vec(2 * self.world), xlo=E.vec(nl_), xhi=E.vec(nl_))
            plan['dx'] = E.deferred_exact_setup(self.Lint, fl, pk, prm.theta, gam, prm.dt, plan['dfr'], mat, scal)
            self.comm.all_gather(plan['mat_all'], mat)          # the matrix entries travel once per plan
            self.comm.all_gather(plan['scal_all'], scal)
        else:
            plan = None
        return plan, fused_ok

    def _plan_two_pass(self, Ti, gam, src_on):
        """-> plan of a two-pass form: 'window' (pass A on the first / last K planes), 'slab' (the whole slab is its own
        window) or 'exact' (all-gather), which is always valid.
        Every rank evaluates BOTH candidate forms on its own slab and the form is agreed collectively: the eligibility
        of 'window' (4 K <= planes of this rank) and the decay tests depend on the rank's slab -- split_planes hands out
        slabs that differ by two planes -- and ranks running different forms would exchange messages of different sizes
        (a hang or corruption on RCCL).  window: all ranks pass it with the same K; else slab: all ranks pass it;
        else exact."""
        E, prm, v = self.engine, self.params, self.variant
        nl, fl, pk = self.nlines, self.flags_int, self.packs_int[0]

        def decayed(k):
            Lw = E.layout(k, self.ny, self.nz, self.Lint.sx)
            worst = 0.0
            c = E.vec(6 * nl)
            if not self._first:      # first-rows window: (gF, aF) are used, cF must have decayed
                E.condense(0, v, Lw, Ti[:k], fl[:k], tuple(None if t is None else t[:k] for t in pk), prm.theta,
                           gam, prm.dt, self.Tinf, c)
                worst = max(worst, float(c.view(6, nl)[2].abs().max()))
            if not self._last:       # last-rows window: (gL, cL) are used, aL must have decayed
                o = self.nxl - k
                E.condense(0, v, Lw, Ti[o:], fl[o:], tuple(None if t is None else t[o:] for t in pk), prm.theta,
                           gam, prm.dt, self.Tinf, c)
                worst = max(worst, float(c.view(6, nl)[4].abs().max()))
            return Lw, worst, bool(worst <= self.DECAY_TOL)          # NaN compares false -> not decayed
        K = self._window_guess(gam)
        cand = {}
        if not self._force_exact:
            # windows pay off when they are a small part of the slab (pass A on 2K planes instead of all of them)
            if self._allow_window and 4 * K <= self.nxl:
                cand['window'] = (K,) + decayed(K)
            cand['slab'] = (self.nxl,) + decayed(self.nxl)
        allp = self._gather_flags(['window' in cand and cand['window'][3], K, 'slab' in cand and cand['slab'][3]])
        if float(allp[:, 0].min()) >= 1.0 and float(allp[:, 1].min()) == float(allp[:, 1].max()):
            k, Lw, worst, _ = cand['window']
            plan = dict(mode='window', K=k, Lw=Lw, worst=worst)
        elif float(allp[:, 2].min()) >= 1.0:
            k, Lw, worst, _ = cand['slab']
            plan = dict(mode='slab', K=k, Lw=Lw, worst=worst)
        else:
            plan = dict(mode='exact', K=self.nxl)
        mode = plan['mode']
        # fused: the same on every rank (sizes only), but slabs may differ by two planes: made collective
        fused = self._all_ranks(self._fused_supported(plan['K']) and not src_on)
        dots = self._all_ranks(self._dots_possible(mode, src_on))
        if dots:
            # the dot products serve lines that are uniform along the axis; the others are condensed one thread per
            # line from R0.  On a curved solid most lines are of the second kind: there the tiled pass-A kernels (which
            # take surface segments, section 3.2b of DESIGN.md) are the better pass A.  Collective decision.
            dd = E.dots_setup(self.Lint, fl, pk[1], prm.theta, gam)
            frac = float(E.dots_nonuniform_fraction(dd)) if hasattr(E, 'dots_nonuniform_fraction') else 0.0
            dots = not float(self._gather_flags([frac]).max()) > self.DOTS_MAX_NONUNIFORM
            if dots:
                plan['dd'] = dd
        plan.update(self._pass_a_options(mode, src_on, fused, dots))
        plan['chunks'] = self._chunk_buffers(mode, plan['K'], self._chunk_ranges_for(mode, dots))
        if mode != 'window':
            # a re-plan of a short-lived plan keeps this decision (_quick_plan).  (With a source the dot products are off for
            # another reason: a decision already made is kept for later plans)
            self._dots_sticky = dots if not src_on or self._dots_sticky is None else self._dots_sticky
        return plan

    # ---- what the full and the quick planner share ----------------------------------------------------------------------
    def _dots_possible(self, mode, src_on):
        """this rank could run a whole-slab pass A without a second read of the slab: the marching explicit kernel accumulates
        the dot products pass A needs while it writes R0 (uniform lines; the others are condensed from R0); pass B is the plain
        sweep"""
        E = self.engine
        return bool(self._allow_dots and not src_on and mode != 'window' and hasattr(E, 'dots_setup')
                    and E.dots_supported(self.nxl, self.ny, self.nz, self.Lint.sx))

    def _pass_a_options(self, mode, src_on, fused, dots):
        """-> the plan's fused / keep_r0 / dots from what the ranks agreed on: `fused`, the fused kernels take K planes of every
        slab, and `dots`, pass A as dot products.  With a source the two-pass forms add it to R0 (_begin_step: `ex`), so every
        pass that reads R0 must read the stored one: no fused passes (they evaluate the explicit stage themselves) and no dot
        products (accumulated while R0 is written).  A whole-slab fused pass A ('slab', 'exact') stores R0 and pass B is the
        plain sweep; 'window' condenses only the boundary planes, so its pass B evaluates the explicit stage itself."""
        fused = bool(fused and not src_on and not dots)
        return dict(fused=fused, keep_r0=bool(fused and mode != 'window' and self._keep_r0), dots=bool(dots))

    def _chunk_ranges_for(self, mode, dots):
        """chunks of lines of the axis-0 pipeline.  Tiled pass A: the exchange of a chunk hides behind pass A of the next
        (2 chunks, 4 for the all-gather form).  Dot-product pass A has no pass-A kernel to hide behind and every extra
        exchange costs its fixed latency: ONE chunk (RCCL self-loop rehearsal at 512^3: 2.06 ms with two halves, 1.97 with
        one chunk; finer first chunks were slower still).  A window's exchange hides behind the middle planes' explicit stage."""
        if dots or mode == 'window':
            return self._chunk_ranges(1)
        if mode == 'exact':
            # (small slabs: the kernels of a quarter of the lines take microseconds and the step is bound by the host's
            # launch path -- 64 x 256 x 320 in the layer-birth loop: 0.94 -> 0.5 ms of host time per step)
            return self._chunk_ranges(4 if self.nxl * self.ny * self.nz >= (1 << 25) else 1)
        return self._chunk_ranges(2, self.SLAB_CHUNK_EDGES)

    def _chunk_buffers(self, mode, K, ranges):
        """fresh interface buffers of the chunks of lines `ranges` (the plan's 'chunks')"""
        E = self.engine
        bufs = []
        for j0, j1 in ranges:
            n = (j1 - j0) * self.nz
            Lc = E.layout(K, j1 - j0, self.nz, self.Lint.sx)
            Lb = E.layout(self.nxl, j1 - j0, self.nz, self.Lint.sx)
            b = dict(j0=j0, j1=j1, nl=n, Lc=Lc, Lb=Lb, xlo=E.vec(n), xhi=E.vec(n))
            if mode == 'exact':
                b.update(cond=E.vec(6 * n), cond_all=E.vec(6 * n * self.world))
            else:
                b['cond_hi'] = E.vec(6 * n)
                b['cond_lo'] = E.vec(6 * n) if mode == 'window' else b['cond_hi']
                b['prev_hi'] = E.vec(3 * n)        # (gL, aL, cL) of the slab below
                b['next_lo'] = E.vec(2 * n)        # (gF, aF) of the slab above
            bufs.append(b)
        return bufs


    # ---- re-planning inside an event loop ---------------------------------------------------------------------------------
    # A layer-birth loop changes the mask and the time step at every birth, i.e. the plan lives for a step or two, and the
    # full planner above costs eight host synchronisations per plan (the measured decay of the condensed entries, the
    # collective flags, the share of non-uniform lines): 0.5 ms per birth, 44 % of the per-rank loop of BASELINE.json
    # configs[4] on 64-plane slabs (scripts/waam_slab_profile.py).  While plans are short-lived they are made WITHOUT reading
    # anything back:
    #   * the interface form from the rigorous bound instead of the measurement: the coupling through k rows is at most rho^k,
    #     rho the per-row factor of solid interior rows (-tg, 1+2tg, -tg) -- every other row is more dominant, a row that lacks a
    #     neighbour or is a Dirichlet cell cuts the coupling altogether -- so rho^K <= DECAY_TOL with 4 K <= the thinnest slab
    #     proves 'window', rho^n <= DECAY_TOL proves 'slab', and 'exact' is always valid.  (The measurement can accept 'slab' where
    #     the bound cannot -- thin-walled parts whose lines never run through a whole slab; the next long-lived plan measures again.)
    #   * whether the fused kernels take the slab: a function of the extents, agreed collectively once per K;
    #   * dot-product or tiled pass A: what the last full plan found (a performance choice, both are exact);
    #   * the interface buffers of the previous plan of the same form are reused.
    # Everything above is the same on every rank, so the ranks keep agreeing on the form without talking.
    def _slab_planes_of_all_ranks(self):
        if self._nx_all is None:
            self._nx_all = [int(round(x)) for x in self._gather_flags([self.nxl])[:, 0].tolist()]
        return self._nx_all

    def _fused_collective(self, K):
        if K not in self._fused_by_K:
            self._fused_by_K[K] = self._all_ranks(self._fused_supported(K))
        return self._fused_by_K[K]

    def _quick_plan(self, gam, src_on=False):
        """plan for the current (dt, theta, mask) without a host synchronisation, or None (no full plan has been made yet, or
        the slab is an all-solid box: the deferred forms need the full planner).  src_on: a source is attached (no fused
        passes, no dot products: see _pass_a_options)"""
        E, prm = self.engine, self.params
        if self._dots_sticky is None or getattr(self, '_solid_everywhere', False) or getattr(E, 'box_hint', 0) == 2:
            return None
        nmin = min(self._slab_planes_of_all_ranks())
        Kg = self._window_guess(gam)
        mode, K = 'exact', self.nxl                          # always valid
        if not self._force_exact and prm.theta * gam > 0.0:
            if self._allow_window and 4 * Kg <= nmin:
                mode, K = 'window', Kg
            elif Kg <= nmin:
                mode = 'slab'
        plan = dict(mode=mode, K=K, quick=True)
        if mode != 'exact':
            plan.update(Lw=E.layout(K, self.ny, self.nz, self.Lint.sx), worst=None)
        fused = self._fused_collective(K)
        dots = bool(self._dots_sticky and self._dots_possible(mode, src_on))
        plan.update(self._pass_a_options(mode, src_on, fused, dots))
        if dots:
            plan['dd'] = E.dots_setup(self.Lint, self.flags_int, self.packs_int[0][1], prm.theta, gam)
        ranges = self._chunk_ranges_for(mode, dots)
        ck = (mode, K, tuple(ranges))
        bufs = self._chunk_cache.get(ck)
        if bufs is None:
            bufs = self._chunk_cache[ck] = self._chunk_buffers(mode, K, ranges)
        for b in bufs:
            b.pop('matrix_sent', None)            # a new plan: the matrix parts of the interface travel again
        plan['chunks'] = bufs
        return plan

    def _plan_deferred_lines(self, gam, fused_ok, short_lived):
        """plan of the deferred form with per-line homogeneous solutions, or None (not tried, or not decayed on some rank).
        Lines that are not uniform (curved solids, voids, Dirichlet cells): the same algebra as 'deferred' with the two
        homogeneous solutions of EVERY line, where they have decayed across every slab (include/adi_hip.h ABI v17).
        Per rank and plan: two axis-0 sweeps of a zero field with unit boundary values -> w_lo, w_hi of every line; K planes of
        each are kept (beyond them every entry must be below DECAY_TOL, checked on the device), the planes next to the
        interfaces travel to the neighbours once.  fused_ok: the ranks' agreement from _plan_deferred.  Collective."""
        E, prm, n, nl_ = self.engine, self.params, self.nxl, self.nlines
        # (every term of this gate is the same on every rank: what depends on the rank's own slab -- its thickness, the decay
        # of its lines -- is decided below, behind the all-gather; a rank-local `nxl >= 2` here hung slabs of [8, 1] planes)
        if not (self._allow_deferred and self._allow_deferred_lines and hasattr(E, 'homogeneous_solution')
                and not self._force_exact and not short_lived and prm.theta * gam > 0.0):
            return None
        fl, pk = self.flags_int, self.packs_int[0]
        # where to look: the reach of the uniform row's solution plus a margin (a run that ends in a line start reflects);
        # what decides is the check below
        dfr = E.deferred_setup(n, prm.theta, gam, self.DECAY_TOL)
        K = min(n, int(dfr['reach']) + 8)
        ok = n >= 2 and K < n
        om, sides = {}, {}
        dm = pk[1]                                  # Dirichlet mask of the slab (None: no Dirichlet cells)

        def sort_lines(Wr, fr, dr):
            """(uniform marks [nlines] uint8, cells of the flagged lines int32, their weights [K][nflag]) of one side.  Wr, fr,
            dr: the K planes of the homogeneous solution, the flags and the Dirichlet mask within reach of the interface, counted
            from it.  A line is uniform when every one of them is a solid interior row (bit 0 and both sharded-axis neighbour
            bits of its flags byte) without a Dirichlet cell -- its homogeneous solution is then the scalar w[i] there, up to
            the decay tolerance --, off when none is in the mask (identity rows: weight 0), flagged otherwise."""
            uni = ((fr & 7) == 7).all(dim=0)
            if dr is not None:
                uni &= ~(dr != 0).any(dim=0)
            off = ((fr & 1) == 0).all(dim=0)
            cells = (~(uni | off)).reshape(-1).nonzero().reshape(-1)
            wc = Wr.reshape(Wr.shape[0], -1).index_select(1, cells).contiguous()
            # rows of each flagged line that can carry a non-zero weight: everything beyond its first row outside the mask is an
            # exact zero (identity rows cut the coupling) and need not even be read
            rows = torch.arange(1, wc.shape[0] + 1, device=wc.device, dtype=torch.int32).reshape(-1, 1)
            nrows = ((wc != 0).to(torch.int32) * rows).amax(dim=0).to(torch.int32).contiguous() if cells.numel() else cells.to(torch.int32)
            return uni.reshape(-1).to(torch.uint8).contiguous(), cells.to(torch.int32).contiguous(), wc, nrows
        nflag = 0
        for side, absent, near, far, own in (('lo', self._first, slice(0, K), slice(K, n), 0),
                                             ('hi', self._last, slice(n - K, n), slice(0, n - K), n - 1)):
            if not ok or absent:
                continue
            W = E.homogeneous_solution(self.variant, self.Lint, fl, pk, prm.theta, gam, prm.dt, side == 'lo')
            ok = bool(float(W[far].abs().max()) <= self.DECAY_TOL)             # NaN compares false
            om[side + '_own'] = W[own].clone()
            if ok:                                                             # ('hi': row r of the weights is plane n-1-r)
                sides[side] = sort_lines(W[near] if side == 'lo' else W[near].flip(0), fl[near], None if dm is None else dm[near])
                nflag += int(sides[side][1].numel())
            del W
        # ... and where it pays: the sparse pass moves 24 B per flagged line and row within reach (its weight, the value read
        # and written); what it replaces is pass A of the two-pass forms, 17 B per cell of the 2 K planes of a window or of the
        # whole slab.  A solid riddled with voids (every line flagged) is left to those; a part with a few cavities is not.
        ok = ok and 24.0 * nflag * K <= self._deferred_lines_cost_ratio * 17.0 * nl_ * min(2 * K, n)
        if not self._all_ranks(ok):
            return None
        # the planes next to the interfaces, once per plan: mine down / up, the neighbours' back
        dummy = E.vec(nl_).view(self.ny, self.nz)
        om['hi_prev'] = None if self._first else E.vec(nl_).view(self.ny, self.nz)
        om['lo_next'] = None if self._last else E.vec(nl_).view(self.ny, self.nz)
        self.comm.exchange_planes(om.get('lo_own', dummy), om.get('hi_own', dummy),
                                  dummy if self._first else om['hi_prev'], dummy if self._last else om['lo_next'])
        return dict(mode='deferred_lines', K=K, fused=fused_ok, dots=False, keep_r0=False, chunks=[], om=om, dfr=dfr, sides=sides,
                    nflag=nflag, ulo=E.vec(nl_), uhi=E.vec(nl_), ulo_uni=E.vec(nl_), uhi_uni=E.vec(nl_),
                    prev_last=E.vec(nl_), next_first=E.vec(nl_))

    def _condense_box(self, plan, L, src, p0, p1, j0, j1, cond):
        """pass A on planes [p0, p1), rows [j0, j1) of the slab.  src: the explicit stage's output (interior view) or,
        when the explicit stage is folded into the pass, the extended state itself."""
        E, prm, v = self.engine, self.params, self.variant
        cut = lambda t: None if t is None else t[p0:p1, j0:j1, :]
        fl, pk = cut(self.flags_int), tuple(cut(t) for t in self.packs_int[0])
        if plan['fused']:
            # a pass A over the whole slab leaves R0 in the scratch field for pass B (no second explicit evaluation)
            r0 = _interior(self._tmp[0])[p0:p1, j0:j1, :] if plan['keep_r0'] else None
            E.condense0_fused(v, L, src, 1 + p0, j0, fl, pk, self.dx, prm.dt, self._kappa, prm.theta, self.Tinf, cond, r0)
        else:
            E.condense(0, v, L, cut(src), fl, pk, prm.theta, self._gam, prm.dt, self.Tinf, cond)

    def _condense_windows(self, plan, Ai, b):
        """pass A on one chunk of lines: the condensations this rank's neighbours need"""
        K, n = plan['K'], self.nxl
        j0, j1 = b['j0'], b['j1']
        whole = b['cond'] if plan['mode'] == 'exact' else b['cond_hi']          # where a pass A over the whole slab goes
        if plan['dots']:
            E, prm = self.engine, self.params
            E.dots_finish(self.variant, self.Lint, plan['dd'], Ai, self.flags_int, self.packs_int[0], prm.theta, self._gam,
                          prm.dt, self.Tinf, j0 * self.nz, j1 * self.nz, whole)
        elif plan['mode'] != 'window':
            self._condense_box(plan, b['Lb'], Ai, 0, n, j0, j1, whole)
        else:
            if self.rank > 0:
                self._condense_box(plan, b['Lc'], Ai, 0, K, j0, j1, b['cond_lo'])
            if self.rank < self.world - 1:
                self._condense_box(plan, b['Lc'], Ai, n - K, n, j0, j1, b['cond_hi'])

    def _exchange_interface(self, plan, b):
        if plan['mode'] == 'exact':
            self.comm.all_gather(b['cond_all'], b['cond'])
        else:
            n = b['nl']
            if b.get('matrix_sent') and self._send_g_only:
                # aF and (aL, cL) are entries of the condensed MATRIX: they depend on dt, theta and the mask only (this
                # plan), so after the first exchange only the right-hand-side parts gF / gL travel (2 of 5 arrays)
                self.comm.exchange_planes(b['cond_lo'].view(6, n)[0:1], b['cond_hi'].view(6, n)[3:4],
                                          b['prev_hi'].view(3, n)[0:1], b['next_lo'].view(2, n)[0:1])
            else:
                self.comm.exchange_planes(b['cond_lo'].view(6, n)[0:2], b['cond_hi'].view(6, n)[3:6],
                                          b['prev_hi'].view(3, n), b['next_lo'].view(2, n))
                b['matrix_sent'] = True

    def _solve_and_sweep(self, plan, Ai, Bi, b):
        """interface values of one chunk of lines, then pass B: the local sweep with them injected"""
        E, prm, v = self.engine, self.params, self.variant
        j0, j1, n = b['j0'], b['j1'], self.nxl
        fl, pk = self.flags_int, self.packs_int[0]
        if plan['mode'] == 'exact':
            E.interface(b['cond_all'], self.world, self.rank, b['nl'], b['xlo'], b['xhi'])
        else:
            E.interface_pair(b['cond_lo'], b['cond_hi'], b['prev_hi'] if self.rank > 0 else None,
                             b['next_lo'] if self.rank < self.world - 1 else None, b['nl'], b['xlo'], b['xhi'])
        cut = lambda t: None if t is None else t[:, j0:j1, :]
        if plan['fused'] and not plan['keep_r0']:
            E.sweep0_fused(v, b['Lb'], Ai, 1, j0, cut(fl), tuple(cut(t) for t in pk), self.dx, prm.dt, self._kappa,
                           prm.theta, self.Tinf, cut(Bi), b['xlo'], b['xhi'])
        else:       # R0 is in the scratch field: the explicit stage's output, or what a fused pass A over the whole slab stored
            E.sweep(0, v, b['Lb'], cut(_interior(self._tmp[0])), cut(fl), tuple(cut(t) for t in pk), prm.theta, self._gam,
                    prm.dt, self.Tinf, cut(Bi), b['xlo'], b['xhi'])

    def _on_comm_stream(self, fn):
        """fn() -- an exchange -- after everything issued so far on the main stream.  With streams on it goes to the comm
        stream, beside whatever the main stream is given next, and the event that marks its end is returned; with streams off
        it runs inline and None is returned."""
        if not self._use_streams:
            fn()
            return None
        main = torch.cuda.current_stream()
        ready = torch.cuda.Event(); ready.record(main)
        with torch.cuda.stream(self._comm_stream):
            self._comm_stream.wait_event(ready)
            fn()
            done = torch.cuda.Event(); done.record(self._comm_stream)
        return done

    def _axis0_pipeline(self, plan, Ai):
        """pass A over the chunks of lines; with RCCL the exchange of chunk c is issued at once on the second stream, so that it
        runs while chunk c+1 is condensed and chunk c-1 is solved -> the exchanges' events.  (Without streams nothing would
        run beside an exchange: they are left to _axis0_finish, each in front of its chunk's solve.)"""
        ev_x = []
        for b in plan['chunks']:
            self._condense_windows(plan, Ai, b)
            if self._use_streams:
                ev_x.append(self._on_comm_stream(lambda: self._exchange_interface(plan, b)))
        return ev_x

    def _axis0_finish(self, plan, Ai, Bi, ev_x):
        """per chunk of lines: its exchange (awaited, or made here), the interface solve and pass B"""
        main = torch.cuda.current_stream() if ev_x else None
        for i, b in enumerate(plan['chunks']):
            if ev_x:
                main.wait_event(ev_x[i])
            else:
                self._exchange_interface(plan, b)
            self._solve_and_sweep(plan, Ai, Bi, b)

    def self_check(self, T):
        """One step as configured (neighbour-only interface solve where the decay allows it, exchanges on the
        second stream) and one with the exact all-gather solve and every exchange on the main stream, from the same
        input; they must agree to rounding.  If they do not (a stream-ordering problem on this software stack),
        the conservative configuration is kept for the rest of the run.
        Returns (max relative difference, fast configuration enabled)."""
        src = self._as_tensor(T).clone()
        a = self._as_tensor(self.step(src)).clone()
        keep = (self._no_overlap, self._force_exact, self._allow_deferred)
        self._no_overlap, self._force_exact, self._allow_deferred = True, True, False     # the two-pass all-gather form
        b = self._as_tensor(self.step(src))
        den = float(b.abs().max())
        err = float((a - b).abs().max()) / (den if den > 0 else 1.0)
        agreed = self._all_ranks(err <= 1e-12)          # the ranks must not end up in different configurations
        self._allow_deferred = keep[2]
        self._plan_steps = None                   # the plans of this check do not count as short-lived ones
        if agreed:
            self._no_overlap, self._force_exact = keep[:2]
        return err, not self._no_overlap

    def step(self, T, events=None, prefetch_halo=False, t=None):
        """One ADI step of the local slab.  prefetch_halo=True promises that the returned field is passed to the
        next step() unmodified (an nsub loop).  Used by the 'window' form, whose step starts with the planes next
        to the halos: the boundary planes of the result are then computed first and sent to the neighbours while
        the rest of the last sweep runs.  (The other forms start with the planes that need no halo, which hides
        the exchange just as well.)
        t: the step's start time, required with a source attached (set_source), which is evaluated at t + dt/2."""
        if self.source is not None and t is None:
            raise ValueError("SlabStepper.step: a heat source is attached, so the step's start time t is required")
        E = self.engine
        if hasattr(E, '_stream_ptr'):
            E._stream_ptr = E.hip._stream()        # every kernel of this step goes to the stream that is current now
        try:
            return self._step(T, events, prefetch_halo, t)
        finally:
            if hasattr(E, '_stream_ptr'):
                E._stream_ptr = None

    def _step(self, T, events, prefetch_halo, t=None):
        s = self._begin_step(T, events, t)
        plan = s.plan
        # 2. explicit stage, 3. axis-0 sweep
        if plan is None:
            self._axis0_zero_boundary(s)                    # one rank: the lines end in the slab, this is the whole sweep
        elif self._is_deferred(plan):
            self._axis0_deferred(s, plan)
        else:
            self._axis0_two_pass(s, plan)
        # 4. local sweeps
        Oi = self._logical(self._local_sweeps(s, plan, prefetch_halo))
        if isinstance(T, np.ndarray):
            return Oi.cpu().contiguous().numpy()
        return Oi if isinstance(T, torch.Tensor) else type(T)(Oi)

    def _begin_step(self, T, events, t):
        """the state loaded, the plan made, the state halos on their way -> the step's working set: the buffers (Text: extended
        state; A / Ai: the explicit stage's output R0; Bi: the axis-0 sweep's; nxt: the extended buffer of the result), the plan,
        and mark() (the stage boundary for bench.py's events), ex(b, e) (the explicit stage on extended planes [b, e), with the
        source where it belongs to R0), src_lines0() (the source after a zero-boundary axis-0 solve), wait_halo()"""
        E, prm, mat = self.engine, self.params, self.mat
        kappa = self._kappa = mat.k / (mat.rho * mat.cp)         # adi3d_numba_coeff.py:292
        gam = self._gam = kappa * prm.dt / (self.dx * self.dx)
        Text = self._load_state(T)
        nxt = self._ext_bufs[self._cur ^ 1]
        A, B = self._tmp
        Ai, Bi, Li, fl = _interior(A), _interior(B), self.Lint, self.flags_int
        ne = 0

        def mark():
            nonlocal ne
            if events is not None:
                events[ne].record()
            ne += 1
        mark()
        # moving source: superposition after the local sweep 0 where that sweep solves with zero boundary values (one rank,
        # the deferred forms), otherwise added to R0 by every explicit-stage call; a rank the support cannot meet skips both
        src = self.source
        i_org = self._plane_origin() if src is not None else 0
        src_here = src is not None and self._source_meets(src, t, prm.dt, i_org)
        plan = self._plan_axis0(_interior(Text), gam) if self.world > 1 else None
        fused = plan['fused'] if plan is not None else self._fused_supported(self.nxl)
        streams = self._streams() and self.world > 1
        main = torch.cuda.current_stream() if streams else None
        src_r0 = src_here and plan is not None and not self._is_deferred(plan)
        src_lines = src_here and not src_r0
        if src_here:
            E.source_set(src, t, prm.dt)

        def ex(b, e):
            E.explicit(self.Lext, Text, self.flags_ext, self.dx, prm.dt, kappa, prm.theta, A, b, e)
            if src_r0:                                  # (extended planes [b, e) = local planes [b - 1, e - 1))
                E.source_add_r0(src, Li, Ai, fl, self.packs_int[0][1], i_org, b - 1, e - 1, self.dx, prm.dt, mat.rho, mat.cp)

        def src_lines0():
            if src_lines:
                E.source_lines0(src, Li, Bi, fl, self.packs_int[0], self.dx, prm.theta, gam, prm.dt, mat.rho, mat.cp, i_org)

        # 1. state halos (zeros outside the global grid are never read: the flags carry no coupling there)
        halo_ev = None
        if self._halo_ready == self._cur and self._halo_ready is not None:
            halo_ev = self._halo_event                       # sent at the end of the previous step
        elif self.world > 1:                                 # (sent once Text is complete)
            halo_ev = self._on_comm_stream(lambda: self.comm.exchange_planes(Text[1], Text[-2], Text[0], Text[-1]))
        self._halo_ready = None

        def wait_halo():
            if halo_ev is not None and streams:
                main.wait_event(halo_ev)
        return types.SimpleNamespace(plan=plan, fused=fused, Text=Text, nxt=nxt, A=A, Ai=Ai, Bi=Bi, mark=mark, ex=ex,
                                     src_lines0=src_lines0, wait_halo=wait_halo)

    def _explicit_around_halo(self, s, ex, margin, split):
        """the explicit stage `ex(begin, end)` of the whole slab around the halo wait.  split: the planes that touch no halo
        -- all but `margin` at each end -- run while the halo planes are in flight"""
        nl = self.nxl
        if split:
            ex(1 + margin, nl + 1 - margin)
            s.wait_halo()
            ex(1, 1 + margin); ex(nl + 1 - margin, nl + 1)
        else:
            s.wait_halo()
            ex(1, nl + 1)

    def _axis0_zero_boundary(self, s):
        """explicit stage, then every axis-0 line of the slab solved with ZERO boundary values by the single-domain kernels,
        then the source's share of that solve"""
        E, prm, v, Li, fl = self.engine, self.params, self.variant, self.Lint, self.flags_int
        if s.fused:
            s.wait_halo()
            E.sweep0_fused(v, Li, s.Text, 1, 0, fl, self.packs_int[0], self.dx, prm.dt, self._kappa, prm.theta, self.Tinf, s.Bi)
        else:
            self._explicit_around_halo(s, s.ex, 1, self.nxl >= 4 and self.world > 1)
            s.mark()
            E.sweep(0, v, Li, s.Ai, fl, self.packs_int[0], prm.theta, self._gam, prm.dt, self.Tinf, s.Bi)
        s.src_lines0()

    def _axis0_deferred(self, s, plan):
        """the zero-boundary solve; the first and last plane of that result go to the neighbours, the 2 x 2 interface systems
        give the two boundary values of every line, and the axis-1 sweep adds  ulo * w[i] + uhi * w[n-1-i]  to what it loads
        (_local_sweeps)"""
        E, Li, nl, Bi = self.engine, self.Lint, self.nxl, s.Bi
        self._axis0_zero_boundary(s)                        # (with the source: before planes 0 and n-1 of Bi travel)
        s.mark()
        if plan['mode'] == 'deferred_exact':
            # no decay: all-gather of (plane 0, plane n-1) of x0 -- the right-hand sides of the interface system, whose matrix
            # is the plan's -- the interface solve over all ranks, then the per-line coefficients of w[i] and w[n-1-i]
            g2 = plan['g'].view(2, self.ny, self.nz)
            g2[0].copy_(Bi[0]); g2[1].copy_(Bi[nl - 1])
            ev = self._on_comm_stream(lambda: self.comm.all_gather(plan['g_all'], plan['g']))
            if ev is not None:
                torch.cuda.current_stream().wait_event(ev)
            E.interface_uniform(plan['g_all'], plan['mat_all'], plan['scal_all'], self.world, self.rank, self.nlines,
                                plan['xlo'], plan['xhi'])
            E.deferred_exact_coef(plan['dx'], plan['xlo'], plan['xhi'], self.nlines, plan['ulo'], plan['uhi'])
            return
        # issued on the main stream: nothing can run beside this exchange (the next kernel needs the planes), and
        # every hop through another stream is a cross-queue dependency of 10 - 20 us on the critical path
        self.comm.exchange_planes(Bi[0], Bi[nl - 1], plan['prev_last'].view(self.ny, self.nz),
                                  plan['next_first'].view(self.ny, self.nz))
        prev_last = None if self._first else plan['prev_last']
        next_first = None if self._last else plan['next_first']
        if plan['mode'] == 'deferred_lines':
            # the interface values of every line, and the same masked to the lines that are uniform within reach (the
            # scalar weights of the axis-1 sweep multiply those); the flagged lines get their own weights here, in memory
            sd = plan['sides']
            E.interface_deferred_lines(Bi[0], Bi[nl - 1], prev_last, next_first, plan['om'], self.nlines, plan['ulo'],
                                       plan['uhi'], sd['lo'][0] if 'lo' in sd else None, sd['hi'][0] if 'hi' in sd else None,
                                       plan['ulo_uni'], plan['uhi_uni'])
            if 'lo' in sd:
                E.deferred_lines_apply(Li, Bi, sd['lo'][1], sd['lo'][2], plan['ulo'], False, sd['lo'][3])
            if 'hi' in sd:
                E.deferred_lines_apply(Li, Bi, sd['hi'][1], sd['hi'][2], plan['uhi'], True, sd['hi'][3])
        else:
            E.interface_deferred(Bi[0], Bi[nl - 1], prev_last, next_first, plan['dfr']['omega'], self.nlines, plan['ulo'],
                                 plan['uhi'])

    def _axis0_two_pass(self, s, plan):
        """explicit stage, pass A, exchange, interface solve, pass B.  What differs between the forms is how the explicit stage
        is laid around the halo wait and around pass A; the pipeline over the chunks of lines is the same."""
        E, prm, nl = self.engine, self.params, self.nxl
        window = plan['mode'] == 'window' and not plan['fused']
        K = plan['K']
        src = s.Ai                      # what pass A and pass B read: R0
        if plan['fused']:
            # R0 never reaches HBM: both passes of the axis-0 sweep evaluate it from the state (halo planes included,
            # so they must have landed; in an nsub loop they were sent while the previous step's last sweep ran)
            s.wait_halo()
            src = s.Text
        elif plan['dots']:
            # one pass over the slab: R0 and, per line, the two dot products of pass A; the chunks of planes that touch no halo
            # run while the halo planes are in flight
            # (running the explicit stage chunk by chunk of LINES, so that a chunk's interface exchange travels behind
            # the next chunk's explicit stage, was measured over the RCCL self-loop: no gain, 1.99 -> 2.02 ms)
            exd = lambda b, e: E.explicit_dots(self.Lext, s.Text, self.flags_ext, self.dx, prm.dt, self._kappa, prm.theta, s.A,
                                               b, e, plan['dd'], 1, nl)
            ich = E.dots_ichunk(nl) if hasattr(E, 'dots_ichunk') else nl
            self._explicit_around_halo(s, exd, ich, nl >= 3 * ich and nl % ich == 0)
            s.mark()
        elif window:
            # the boundary windows first: their condensation travels while the middle planes are computed
            s.wait_halo()
            if 2 * K < nl:
                s.ex(1, K + 1); s.ex(nl - K + 1, nl + 1)
            else:
                s.ex(1, nl + 1)
        else:
            self._explicit_around_halo(s, s.ex, 1, nl >= 4)
            s.mark()
        ev_x = self._axis0_pipeline(plan, src)
        if window:
            if 2 * K < nl:
                s.ex(K + 1, nl - K + 1)
            s.mark()
        self._axis0_finish(plan, src, s.Bi, ev_x)

    def _local_sweeps(self, s, plan, prefetch_halo):
        """the axis-1 sweep (with the deferred forms' correction added to what it loads) and the axis-2 sweep into the other
        state buffer, whose halo planes are sent ahead on request -> the interior of that buffer"""
        E, prm, v, Li, fl, nl = self.engine, self.params, self.variant, self.Lint, self.flags_int, self.nxl
        gam, Ai, Bi, nxt = self._gam, s.Ai, s.Bi, s.nxt
        Oi = _interior(nxt)
        if self._is_deferred(plan):
            # (the scalar weights multiply the interface values, 'deferred_lines': those of the lines uniform within reach; an end
            # rank has no neighbour on one side, but 'deferred_exact' carries a Sherman-Morrison term on both vectors there)
            ulo, uhi = (plan['ulo_uni'], plan['uhi_uni']) if plan['mode'] == 'deferred_lines' else (plan['ulo'], plan['uhi'])
            both = plan['mode'] == 'deferred_exact'
            E.sweep_corrected(v, Li, Bi, fl, self.packs_int[1], prm.theta, gam, prm.dt, self.Tinf, Ai,
                              None if (self._first and not both) else ulo, None if (self._last and not both) else uhi,
                              plan['dfr']['w'])
        else:
            s.mark()
            E.sweep(1, v, Li, Bi, fl, self.packs_int[1], prm.theta, gam, prm.dt, self.Tinf, Ai)
        s.mark()
        pk2 = self.packs_int[2]
        sw2 = lambda p0, p1: E.sweep(2, v, E.layout(p1 - p0, self.ny, self.nz, Li.sx), Ai[p0:p1], fl[p0:p1],
                                     tuple(None if t is None else t[p0:p1] for t in pk2), prm.theta, gam, prm.dt,
                                     self.Tinf, Oi[p0:p1])
        # the fused passes and the 'window' form start with planes that need the halos: send them early
        if prefetch_halo and self.world > 1 and nl >= 4 and (plan['mode'] == 'window' or s.fused):
            sw2(0, 1); sw2(nl - 1, nl)                        # the two planes the neighbours need
            self._halo_event = self._on_comm_stream(lambda: self.comm.exchange_planes(nxt[1], nxt[-2], nxt[0], nxt[-1]))
            self._halo_ready = self._cur ^ 1
            sw2(1, nl - 1)
        else:
            sw2(0, nl)
        s.mark()
        self._cur ^= 1
        return Oi
