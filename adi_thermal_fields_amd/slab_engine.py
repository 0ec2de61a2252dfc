"""slab_engine -- the numerical work of a slab decomposition (dist_slab.SlabStepper's `engine`) in production: hand-written HIP
kernels through the C ABI.  tests/cpu_engine.py restates the same calls with NumPy and the oracle."""
import ctypes

import torch

__all__ = ['HipEngine']


class HipEngine:
    """The product engine: hand-written HIP kernels through the C ABI (include/adi_hip.h)."""

    def __init__(self):
        from . import adi3d_hip_coeff as hip
        from . import _lib
        from ._ledger import PromiseLedger
        self.hip, self._lib, self.lib, self.check = hip, _lib, _lib.lib, _lib.check
        self.device = hip._device()
        self.box_hint = 0          # 2: every cell of every slab is in the mask (SlabStepper.set_mask decides, collectively)
        self.mask_epoch = 0        # bumped by SlabStepper.set_mask: the flags / packs are rebuilt in place
        self._nofb = PromiseLedger()   # no-fallback promise per sweep configuration (bit 2 of `sparse`); set_mask clears it
        self._fconsts = {}         # coefficient storage -> per-face scalars of the pack built on it (h_face_consts)
        self._stream_ptr = None    # launch stream of the step in progress (SlabStepper.step pins it: one lookup per step)
        self._wb = {}              # workspace bytes per box shape

    def _sp(self):
        """the hipStream_t every kernel of this engine is launched on: torch's current stream, looked up once per step"""
        return self._stream_ptr if self._stream_ptr is not None else self.hip._stream()

    def plane_dims(self, ny, nz):
        """physical (ny, nz) of a slab's planes: adi_recommended_dims for a box with long lines along axis 0 (whatever the slab
        thickness of this rank: all ranks must agree)"""
        return tuple(self.hip.recommended_dims(64, ny, nz)[1:])

    def layout(self, nx, ny, nz, sx=None):
        # no padding at this level (Layout's default for whole grids): the stepper pads the planes of a slab itself
        # (SlabStepper: plane_dims), and its extended arrays, halo planes and sub-boxes all share one plane stride
        return self.hip.Layout(nx, ny, nz, sx, phys=(nx, ny, nz))

    def vec(self, n):
        """plan-time fp64 buffer (receive buffers, interface values, flags): ZERO-filled, so a protocol slip shows as a wrong
        number and never as a read of uninitialised memory (round 3's one GPU memory fault: 0 / 1 plane flags built on an
        uninitialised vec()).  Never called per step."""
        return torch.zeros(n, dtype=torch.float64, device=self.device)

    def build_flags(self, L, mask_ext):
        flags = L.empty(torch.uint8, zero=True)
        self.check(self.lib.adi_build_nbr_flags(self.hip._p(mask_ext), L.nx, L.ny, L.nz, L.sx, self.hip._p(flags),
                                                self._sp()))
        return flags

    def _fc(self, pack):
        """h_face_consts of a pack tuple (coeff, dir_mask, dir_val, qflux) or of any view cut out of it: the per-face scalars
        the pack was built from (registered by build_packs under the coefficient array's storage), or None"""
        return self._fconsts.get(pack[0].untyped_storage().data_ptr())

    def build_packs(self, L, mask_ext, flags_ext, dx, mat, dir_mask, dir_value, neumann, robin_h):
        """precompute_coeff_packs_unified on the extended slab; returns packs whose arrays are extended too."""
        g = self.hip.Grid3D.__new__(self.hip.Grid3D)
        g.nx, g.ny, g.nz, g.dx, g.layout = L.nx, L.ny, L.nz, float(dx), L
        g._mask, g._d_mask, g._d_flags, g._scratch, g.mask_version = None, mask_ext, flags_ext, None, next(self.hip._MASK_VERSIONS)
        g.sync_mask = lambda: mask_ext            # the device mask (with halos) is authoritative here
        packs = self.hip.precompute_coeff_packs_unified(g, mat, dir_mask=dir_mask, dir_value=dir_value,
                                                        neumann=neumann, robin_h=robin_h)
        self._fconsts = {p.d_coeff.untyped_storage().data_ptr(): p.face_consts for p in packs if p.face_consts is not None}
        return packs

    # in-place updates after a layer birth (planes [k0, k1) of axis 2): what Grid3D.set_mask_device / BirthPacks.update do
    # for one domain, here on the extended arrays of a slab
    def build_flags_planes(self, L, mask_ext, flags_ext, k0, k1):
        self.check(self.lib.adi_build_nbr_flags_planes(self.hip._p(mask_ext), L.nx, L.ny, L.nz, L.sx, self.hip._p(flags_ext),
                                                       int(k0), int(k1), self._sp()))

    def build_packs_planes(self, L, mask_ext, packs_ext, dx, mat, specs, k0, k1):
        h = self.hip
        hm, hs, qm, qs = specs
        none6 = h.ptr_array([None] * 6)
        self.check(self.lib.adi_build_coeffs_planes(h._p(mask_ext), L.nx, L.ny, L.nz, L.sx, float(dx), mat.rho, mat.cp,
                                                    hm, hs, none6, qm, qs, none6,
                                                    h.ptr_array([p.d_coeff.data_ptr() for p in packs_ext]),
                                                    h.ptr_array([p.d_qflux.data_ptr() for p in packs_ext]),
                                                    int(k0), int(k1), self._sp()))

    def birth_planes(self, Li, T_int, act_int, full_int, k0, k1, Ts, count):
        """adi_birth_planes on the interior of a slab (pointers one plane into the extended arrays)"""
        h = self.hip
        self.check(self.lib.adi_birth_planes(h._p(T_int), h._p(act_int), h._p(full_int), Li.nx, Li.ny, Li.nz, Li.sx,
                                             int(k0), int(k1), float(Ts), h._p(count), self._sp()))

    def explicit(self, L, T_ext, flags_ext, dx, dt, kappa, theta, out_ext, i_begin=0, i_end=None):
        h = self.hip
        i_end = L.nx if i_end is None else i_end
        self.check(self.lib.adi_explicit_rhs_planes(h._p(T_ext), h._p(flags_ext), L.nx, L.ny, L.nz, L.sx, dx, dt, kappa,
                                                    theta, h._p(out_ext), i_begin, i_end, self._sp()))

    def _args(self, variant, Li, t_in, flags, pack, sparse, theta, gam, dt, Tinf):
        h = self.hip
        return (variant, h._p(t_in), h._p(flags), h._p(pack[0]), h._p(pack[1]), h._p(pack[2]), h._p(pack[3]),
                Li.nx, Li.ny, Li.nz, Li.sx, sparse, theta, gam, dt, float(Tinf))

    def _workspace(self, Li):
        """unit queue of the FAST/GENERAL kernel pair (sized for the largest box seen)"""
        key = (Li.nx, Li.ny, Li.nz, Li.sx)
        need = self._wb.get(key)
        if need is None:
            need = self._wb[key] = self.hip._sweep_workspace_bytes(*key)
        if getattr(self, '_work', None) is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._work

    def _nofb_begin(self, entry, axis, variant, Li, flags, pack, tg, plain=True):
        """first half of a sweep under the no-fallback promise (_ledger.PromiseLedger) -> (workspace, key, `sparse` with the
        bit); the caller launches with them and ends with self._nofb.learn(key, workspace)"""
        w = self._workspace(Li)
        sp, key = 1 | self.box_hint, None         # packs from adi_build_coeffs: sparse
        if self._nofb.eligible(sp, w, tg, plain):
            key = (entry, axis, variant, Li.nx, Li.ny, Li.nz, Li.sx, flags.data_ptr(), pack[0].data_ptr(),
                   None if pack[1] is None else pack[1].data_ptr(), self.box_hint, self.mask_epoch)
        return w, key, sp | self._nofb.bit(key)

    def sweep(self, axis, variant, Li, t_in, flags, pack, theta, gam, dt, Tinf, t_out, xlo=None, xhi=None):
        h = self.hip
        w, key, sp = self._nofb_begin('sweep', axis, variant, Li, flags, pack, theta * gam,
                                      plain=not (axis == 2 and (xlo is not None or xhi is not None)))
        self.check(self.lib.adi_sweep(axis, *self._args(variant, Li, t_in, flags, pack, sp, theta, gam, dt, Tinf), h._p(t_out),
                                      h._p(xlo), h._p(xhi), self._fc(pack), h._p(w), w.numel(), self._sp()))
        self._nofb.learn(key, w)

    def condense(self, axis, variant, Li, t_in, flags, pack, theta, gam, dt, Tinf, cond):
        h = self.hip
        w = self._workspace(Li)
        self.check(self.lib.adi_sweep_condense(axis, *self._args(variant, Li, t_in, flags, pack, 1 | self.box_hint, theta,
                                                                 gam, dt, Tinf),
                                               h._p(cond), self._fc(pack), h._p(w), w.numel(), self._sp()))

    # explicit stage folded into the axis-0 sweep / condensation (ABI v7).  The box (L.nx, L.ny, L.nz) starts at plane
    # i0, row j0 of the extended state T_ext; neighbours outside the box are read from T_ext itself.
    def fused_supported(self, nx, ny, nz, sx, cond_pass):
        return bool(self.lib.adi_explicit_fused_supported(nx, ny, nz, sx, 1 if cond_pass else 0))

    def _fused_args(self, variant, L, T_ext, i0, j0, flags, pack, sparse, dx, dt, kappa, theta, Tinf):
        h = self.hip
        tv = T_ext[i0:i0 + L.nx, j0:j0 + L.ny, :]
        vlo, vhi = h.valid_range(tv)
        return (variant, h._p(tv), vlo, vhi, h._p(flags), h._p(pack[0]), h._p(pack[1]), h._p(pack[2]), h._p(pack[3]),
                L.nx, L.ny, L.nz, L.sx, sparse, dx, dt, kappa, theta, float(Tinf))

    def sweep0_fused(self, variant, L, T_ext, i0, j0, flags, pack, dx, dt, kappa, theta, Tinf, t_out, xlo=None, xhi=None):
        h = self.hip
        w, key, sp = self._nofb_begin('fused', 0, variant, L, flags, pack, theta * (kappa * dt / (dx * dx)))
        self.check(self.lib.adi_explicit_sweep0(*self._fused_args(variant, L, T_ext, i0, j0, flags, pack, sp, dx, dt, kappa,
                                                                  theta, Tinf),
                                                h._p(t_out), h._p(xlo), h._p(xhi), self._fc(pack), h._p(w), w.numel(),
                                                self._sp()))
        self._nofb.learn(key, w)

    # deferred form of the sharded-axis sweep (include/adi_hip.h, ABI v12): every line solved with zero boundary values by
    # the single-domain kernel, one plane to each neighbour, 2 x 2 interface systems, and the rank-two correction added by
    # the axis-1 sweep to what it loads
    def lines_all_uniform(self, Li, flags_int, dmask_int):
        """every sharded-axis line of the slab is solid and free of Dirichlet cells (reads one int: synchronises)"""
        h = self.hip
        nl = Li.ny * Li.nz
        cls = torch.empty(nl, dtype=torch.uint8, device=self.device)
        lst = torch.empty(nl + 1, dtype=torch.int32, device=self.device)
        self.check(self.lib.adi_axis0_classify(h._p(flags_int), h._p(dmask_int), Li.nx, Li.ny, Li.nz, Li.sx, h._p(cls),
                                               h._p(lst), self._sp()))
        return int(lst[0].item()) == 0

    def deferred_setup(self, n, theta, gam, tol):
        """-> dict(w: device weights with exact zeros beyond their reach, omega = w[0], reach)"""
        h = self.hip
        w = self.vec(n)
        om, reach = ctypes.c_double(0.0), ctypes.c_int(0)
        self.check(self.lib.adi_axis0_deferred_setup(n, theta, gam, tol, h._p(w), ctypes.byref(om), ctypes.byref(reach),
                                                     self._sp()))
        return dict(w=w, omega=om.value, reach=reach.value)

    def deferred_exact_setup(self, Li, flags_int, pack, theta, gam, dt, dfr, mat, scal):
        """once per plan: this rank's matrix entries mat [4][nlines] = (aF, cF, aL, cL), its (w[0], w[n-1]) in `scal`, and the
        per-line Sherman-Morrison factors of a global end row (first / last rank) -> opaque handle for deferred_exact_coef"""
        h = self.hip
        nl = Li.ny * Li.nz
        kap = self.vec(2 * nl)
        w = dfr['w']
        w0, wn = float(w[0].item()), float(w[Li.nx - 1].item())
        scal[0] = w0; scal[1] = wn
        self.check(self.lib.adi_deferred_exact_setup(h._p(flags_int[0]), h._p(flags_int[Li.nx - 1]), h._p(pack[0][0]),
                                                     h._p(pack[0][Li.nx - 1]), theta, gam, dt, w0, wn, nl, h._p(mat), h._p(kap),
                                                     self._sp()))
        return dict(kap=kap)

    def interface_uniform(self, g_all, mat_all, scal_all, world, rank, nlines, xlo, xhi):
        h = self.hip
        self.check(self.lib.adi_interface_solve_uniform(h._p(g_all), h._p(mat_all), h._p(scal_all), world, rank, nlines,
                                                        h._p(xlo), h._p(xhi), self._sp()))

    def deferred_exact_coef(self, dx_, xlo, xhi, nlines, clo, chi):
        h = self.hip
        self.check(self.lib.adi_deferred_exact_coef(h._p(xlo), h._p(xhi), h._p(dx_['kap']), nlines, h._p(clo), h._p(chi),
                                                    self._sp()))

    def interface_deferred(self, first, last, prev_last, next_first, omega, nlines, ulo, uhi):
        h = self.hip
        self.check(self.lib.adi_interface_deferred(h._p(first), h._p(last), h._p(prev_last), h._p(next_first), omega,
                                                   nlines, h._p(ulo), h._p(uhi), self._sp()))

    def sweep_corrected(self, variant, Li, t_in, flags, pack, theta, gam, dt, Tinf, t_out, ulo, uhi, w_corr):
        """axis-1 sweep of t_in + w[i] * ulo + w[n-1-i] * uhi (the correction is added to what the sweep loads)"""
        h = self.hip
        w, key, sp = self._nofb_begin('sweep', 1, variant, Li, flags, pack, theta * gam)
        self.check(self.lib.adi_sweep_corrected(*self._args(variant, Li, t_in, flags, pack, sp, theta, gam, dt, Tinf),
                                                h._p(t_out), h._p(ulo), h._p(uhi), h._p(w_corr), self._fc(pack),
                                                h._p(w), w.numel(), self._sp()))
        self._nofb.learn(key, w)

    # the deferred form for lines that are not uniform (ABI v17): per-line homogeneous solutions
    def homogeneous_solution(self, variant, Li, flags, pack, theta, gam, dt, lower):
        """w_lo (lower=True: unit value of the unknown below the slab) or w_hi of every sharded-axis line: the ordinary axis-0
        sweep of a zero field with Tinf = 0, no fluxes, zero Dirichlet values and d_xlo (d_xhi) = 1 -> (nx, ny, nz) tensor"""
        from . import _lib
        nl = Li.ny * Li.nz
        has_dir = variant in (_lib.SWEEP_GENERAL, _lib.SWEEP_NO_Q)
        v = _lib.SWEEP_NO_Q if has_dir else _lib.SWEEP_LEAN
        zero = Li.empty(zero=True)
        one = torch.ones(nl, dtype=torch.float64, device=self.device)
        pk = (pack[0], pack[1], (Li.empty(zero=True) if has_dir else None), None)
        out = Li.empty()
        # (dense reads, no face constants: the coefficient arrays as they are; a one-off per plan)
        h = self.hip
        w = self._workspace(Li)
        self.check(self.lib.adi_sweep(0, *self._args(v, Li, zero, flags, pk, 0, theta, gam, dt, 0.0), h._p(out),
                                      h._p(one if lower else None), h._p(None if lower else one), None,
                                      h._p(w), w.numel(), self._sp()))
        return out

    def interface_deferred_lines(self, first, last, prev_last, next_first, om, nlines, ulo, uhi, uni_lo=None, uni_hi=None,
                                 ulo_uni=None, uhi_uni=None):
        """ulo / uhi: the interface values of every line; ulo_uni / uhi_uni: the same on the lines uni_lo / uni_hi mark
        (one byte per line) and 0 elsewhere -- what the scalar weights of adi_sweep_corrected multiply"""
        h = self.hip
        self.check(self.lib.adi_interface_deferred_lines(h._p(first), h._p(last), h._p(prev_last), h._p(next_first),
                                                         h._p(om.get('lo_own')), h._p(om.get('hi_prev')), h._p(om.get('hi_own')),
                                                         h._p(om.get('lo_next')), nlines, h._p(ulo), h._p(uhi), h._p(uni_lo),
                                                         h._p(uni_hi), h._p(ulo_uni), h._p(uhi_uni), self._sp()))

    def deferred_lines_apply(self, Li, x, cells, wc, u, from_high_end, nrows=None):
        """x[i][cells[q]] += wc[r][q] * u[cells[q]], i = r or nx-1-r: the flagged lines of one side get their own weights
        (nrows[q]: rows of line q that can carry a non-zero weight; the rest is not read)"""
        h = self.hip
        if cells.numel() == 0:
            return
        self.check(self.lib.adi_deferred_lines_apply(h._p(x), Li.nx, Li.sx, Li.ny * Li.nz, h._p(cells), cells.numel(), h._p(wc),
                                                     int(wc.shape[0]), h._p(u), 1 if from_high_end else 0, h._p(nrows), self._sp()))


    def condense0_fused(self, variant, L, T_ext, i0, j0, flags, pack, dx, dt, kappa, theta, Tinf, cond, r0_out=None):
        """r0_out (optional, a view of the box in an array laid out like T_ext): also receives R0"""
        h = self.hip
        w = self._workspace(L)
        self.check(self.lib.adi_explicit_condense0(*self._fused_args(variant, L, T_ext, i0, j0, flags, pack, 1 | self.box_hint,
                                                                     dx, dt, kappa, theta, Tinf),
                                                   h._p(cond), h._p(r0_out), self._fc(pack), h._p(w), w.numel(), self._sp()))

    # pass A folded into the marching explicit kernel: dot products of R0 with fixed weights (uniform lines), the rest
    # condensed from the stored R0 (include/adi_hip.h, adi_axis0_dots_*)
    def dots_supported(self, nxl, ny, nz, sx):
        return bool(self.lib.adi_axis0_dots_supported(nxl, ny, nz, sx))

    def dots_setup(self, Li, flags_int, dmask_int, theta, gam):
        """once per (dt, mask): weights, line classes, partial-sum buffer"""
        h = self.hip
        pb, lb = ctypes.c_size_t(0), ctypes.c_size_t(0)
        self.check(self.lib.adi_axis0_dots_workspace(Li.nx, Li.ny, Li.nz, ctypes.byref(pb), ctypes.byref(lb)))
        dd = dict(weights=self.vec(Li.nx), part=self.vec(pb.value // 8),
                  cls=torch.empty(Li.ny * Li.nz, dtype=torch.uint8, device=self.device),
                  list=torch.empty(lb.value // 4, dtype=torch.int32, device=self.device))
        self.check(self.lib.adi_axis0_dots_setup(Li.nx, theta, gam, h._p(dd['weights']), self._sp()))
        self.check(self.lib.adi_axis0_classify(h._p(flags_int), h._p(dmask_int), Li.nx, Li.ny, Li.nz, Li.sx,
                                               h._p(dd['cls']), h._p(dd['list']), self._sp()))
        return dd

    def dots_nonuniform_fraction(self, dd):
        """share of the lines adi_axis0_classify left to the per-line condensation (reads one int: synchronises)"""
        return int(dd['list'][0].item()) / float(dd['cls'].numel())

    def dots_ichunk(self, n_line):
        return int(self.lib.adi_axis0_dots_ichunk(n_line))

    def explicit_dots(self, L, T_ext, flags_ext, dx, dt, kappa, theta, out_ext, i_begin, i_end, dd, i_org, n_line):
        """planes [i_begin, i_end) of lines that occupy planes [i_org, i_org + n_line): whole chunks of dots_ichunk(n_line)"""
        h = self.hip
        self.check(self.lib.adi_explicit_rhs_dots(h._p(T_ext), h._p(flags_ext), L.nx, L.ny, L.nz, L.sx, dx, dt, kappa,
                                                  theta, h._p(out_ext), i_begin, i_end, i_org, n_line,
                                                  h._p(dd['weights']), h._p(dd['part']), self._sp()))

    def dots_finish(self, variant, Li, dd, r0, flags, pack, theta, gam, dt, Tinf, line_begin, line_end, cond):
        h = self.hip
        self.check(self.lib.adi_axis0_dots_finish(variant, h._p(dd['part']), h._p(dd['weights']), h._p(dd['cls']),
                                                  h._p(dd['list']), h._p(r0), h._p(flags), h._p(pack[0]), h._p(pack[1]),
                                                  h._p(pack[2]), h._p(pack[3]), Li.nx, Li.ny, Li.nz, Li.sx, theta, gam, dt,
                                                  float(Tinf), line_begin, line_end, h._p(cond), self._sp()))

    def interface(self, cond_all, world, rank, nlines, xlo, xhi):
        h = self.hip
        self.check(self.lib.adi_interface_solve(h._p(cond_all), world, rank, nlines, h._p(xlo), h._p(xhi),
                                                self._sp()))


    def interface_pair(self, my_lo, my_hi, prev_hi, next_lo, nlines, xlo, xhi):
        h = self.hip
        self.check(self.lib.adi_interface_pair(h._p(my_lo), h._p(my_hi), h._p(prev_hi), h._p(next_lo), nlines,
                                               h._p(xlo), h._p(xhi), self._sp()))

    # moving heat source (include/adi_hip.h, "Volumetric heat source"): one device block and one workspace per rank
    def source_set(self, src, t, dt):
        """the block of this rank: `src` (a GoldakSource) for the step that starts at t"""
        h = self.hip
        self.check(self.lib.adi_source_set(h._p(h._source_block(self)), ctypes.byref(src.as_c()), float(t), float(dt), 0,
                                           self._sp()))

    def source_lines0(self, src, Li, U, flags, pack, dx, theta, gam, dt, rho, cp, i_org):
        """U += A0^-1 s on the slab's axis-0 lines with zero values beyond both ends (the deferred forms' local solve)"""
        h = self.hip
        work = h._source_work(self, (Li.nx, Li.ny, Li.nz), dx, src)
        self.check(self.lib.adi_source_lines0_slab(h._p(self._src_block), ctypes.byref(src.as_c()), h._p(U), h._p(flags),
                                                   h._p(pack[0]), h._p(pack[1]), Li.nx, Li.ny, Li.nz, Li.sx, int(i_org),
                                                   1 | self.box_hint, dx, theta, gam, dt, rho, cp, self._fc(pack),
                                                   h._p(work), 0 if work is None else work.numel(), self._sp()))

    def source_add_r0(self, src, Li, R0, flags, dir_mask, i_org, i_begin, i_end, dx, dt, rho, cp):
        """R0 += dt*q/(rho cp) on local planes [i_begin, i_end) of the slab (in-mask, non-Dirichlet cells)"""
        h = self.hip
        self.check(self.lib.adi_source_add_r0(h._p(self._src_block), ctypes.byref(src.as_c()), h._p(R0), h._p(flags),
                                              h._p(dir_mask), Li.nx, Li.ny, Li.nz, Li.sx, int(i_org), int(i_begin), int(i_end),
                                              dx, dt, rho, cp, self._sp()))
