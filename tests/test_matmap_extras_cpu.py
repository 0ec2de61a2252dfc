"""CPU: the definitions of latent heat and surface loss with one law per material of a MaterialMap (MapPhaseField.correct_of,
MapLossPacks.coeff_reference) against the one-material definitions they compose, the enthalpy they must conserve,
the C ABI's argument checks and the new kernels' footprint.  Laws, fields and the coverage condition: tests/matmap_extras_cases.py.
No GPU (the built library is needed for the imports)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import matmap_cases as mc
import matmap_extras_cases as xc
from adi_thermal_fields_amd import _lib
from adi_thermal_fields_amd.matmap_extras import MapLossPacks, MapPhaseField
from adi_thermal_fields_amd.packs import MaterialMap
from adi_thermal_fields_amd.surface_loss import SurfaceLoss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOLES = mc.case(('holes', mc.HOLES, 'random3', 'general', 0.5, 200.0))


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---- 1. one material, one law: the definitions they compose --------------------------------------------------------------------
def test_one_material_one_law_is_phase_change_correct():
    mask, ids0 = HOLES['mask'], np.zeros(mc.HOLES, np.uint8)
    for law, mat in zip(xc.LAWS[:2], mc.MATERIALS[:2]):
        fl = xc.fields(mask, ids0, (law,))
        f0 = law.f_eq(fl['T_seed']) * mask
        got = MapPhaseField.correct_of((law,), (mat,), fl['T_star'], f0, mask, ids0, fl['dir_mask'])
        want = law.correct(fl['T_star'], f0, mask, fl['dir_mask'], mat[1])
        assert _bits(got[0], want[0]) and _bits(got[1], want[1])
        assert not _bits(got[0], fl['T_star']) and not _bits(got[1], f0)
        got = MapPhaseField.correct_of((law,), (mat,), fl['T_star'], f0, mask, ids0, None)
        want = law.correct(fl['T_star'], f0, mask, None, mat[1])
        assert _bits(got[0], want[0]) and _bits(got[1], want[1])


def test_one_shared_loss_is_the_packs_reference_with_the_six_h_fields():
    mask, T = HOLES['mask'], HOLES['T0']
    loss = xc.LOSSES[0]
    h = {face: loss.h_of(T, face, xc.TINF) for face in _lib.FACES}
    # one material
    ids0 = np.zeros(mc.HOLES, np.uint8)
    want = MaterialMap.packs_reference(mask, ids0, (mc.STEEL,), mc.DX, robin_h=h)
    got = MapLossPacks.coeff_reference(T, mask, ids0, (mc.STEEL,), mc.DX, (loss,), xc.TINF)
    for a in range(3):
        assert _bits(got[a], want[a].coeff) and np.any(got[a] != 0.0)
    # three materials, one loss for all of them (given once, or once per material)
    ids = HOLES['ids']
    want = MaterialMap.packs_reference(mask, ids, mc.MATERIALS, mc.DX, robin_h=h)
    for losses in (loss, (loss,) * 3):
        got = MapLossPacks.coeff_reference(T, mask, ids, mc.MATERIALS, mc.DX, losses, xc.TINF)
        for a in range(3):
            assert _bits(got[a], want[a].coeff)
    # one loss per material: the h of the cell's own
    got = MapLossPacks.coeff_reference(T, mask, ids, mc.MATERIALS, mc.DX, xc.LOSSES, xc.TINF)
    want = MaterialMap.packs_reference(mask, ids, mc.MATERIALS, mc.DX, robin_h=xc.h_fields(T, mask, ids, mc.MATERIALS, xc.TINF))
    for a in range(3):
        assert _bits(got[a], want[a].coeff)
        for m in range(3):
            only = MapLossPacks.coeff_reference(T, mask, ids, mc.MATERIALS, mc.DX, xc.LOSSES[m], xc.TINF)
            cells = mask & (ids == m)
            assert _bits(got[a][cells], only[a][cells])
    assert not _bits(got[0], MapLossPacks.coeff_reference(T, mask, ids, mc.MATERIALS, mc.DX, loss, xc.TINF)[0])


# ---- 2. what the correction may not touch --------------------------------------------------------------------------------------
def test_lawless_offmask_and_dirichlet_cells_come_back_bit_identical():
    mask, ids = HOLES['mask'], HOLES['ids']
    fl = xc.fields(mask, ids, xc.LAWS)
    xc.assert_covered(fl['T_star'], fl['f0'], mask, ids, fl['dir_mask'], mc.MATERIALS, 'holes')
    rng = np.random.default_rng(3)
    lawless = mask & (ids == 2)
    f0 = np.where(mask & ~lawless, fl['f0'], rng.uniform(0.0, 1.0, mask.shape))        # (garbage where no law reads it)
    T_star = np.where(mask & ~lawless, fl['T_star'], np.nan)                               # (and NaN where none reads T)
    T1, f1 = MapPhaseField.correct_of(xc.LAWS, mc.MATERIALS, T_star, f0, mask, ids, fl['dir_mask'])
    keep = ~mask | lawless | fl['dir_mask']
    assert lawless.sum() > 1000 and (~mask).sum() > 1000 and fl['dir_mask'].sum() > 500
    assert _bits(T1[keep], T_star[keep]) and _bits(f1[keep], f0[keep])
    changed = (T1.view(np.uint64) != T_star.view(np.uint64)) | (f1.view(np.uint64) != f0.view(np.uint64))
    assert changed.any() and not (changed & keep).any()
    # per material, the one-material definition on that material's cells
    for m in (0, 1):
        cells = mask & (ids == m)
        Tm, fm = xc.LAWS[m].correct(T_star, f0, cells, fl['dir_mask'], mc.MATERIALS[m][1])
        assert _bits(T1[cells], Tm[cells]) and _bits(f1[cells], fm[cells])
    # every law None: nothing moves
    T2, f2 = MapPhaseField.correct_of((None,) * 3, mc.MATERIALS, T_star, f0, mask, ids, fl['dir_mask'])
    assert _bits(T2, T_star) and _bits(f2, f0)


# ---- 3. enthalpy ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfl', [0.3, 200.0])
def test_enthalpy_of_an_adiabatic_three_material_body_is_conserved(cfl):
    """one definition step plus the correction: sum rho_m (cp_m T + L_m f) over the mask changes by at most (N + 8) eps64 of
    sum rho_m (cp_m |T| + L_m), N the in-mask cells: N for the step (test_heat_of_an_adiabatic_body_is_conserved argues it) and 8
    for the rounded operations of the correction in a cell"""
    shape = (20, 18, 35)
    rng = np.random.default_rng(7)
    mask = rng.random(shape) > 0.25
    ids = rng.integers(0, 3, shape).astype(np.uint8)
    T0 = rng.uniform(900.0, 1700.0, shape)                  # straddles 1083-1085 and 1400-1450
    f0 = MapPhaseField.f_eq_of(xc.LAWS, T0, mask, ids)
    dt = cfl * mc.DX ** 2 / mc.ALPHA_MAX
    pk = MaterialMap.packs_reference(mask, ids, mc.MATERIALS, mc.DX)
    W = MaterialMap.step_reference(T0, mask, ids, mc.MATERIALS, mc.DX, dt, 0.5, pk, mc.TINF)
    T1, f1 = MapPhaseField.correct_of(xc.LAWS, mc.MATERIALS, W, f0, mask, ids, None)
    h0, scale = xc.enthalpy(T0, f0, mask, ids, mc.MATERIALS)
    h1, _ = xc.enthalpy(T1, f1, mask, ids, mc.MATERIALS)
    n = int(mask.sum())
    print('cfl %g: enthalpy changes by %.3e, bar %.3e (%.2f of it)' % (cfl, float(abs(h1 - h0)), float((n + 8) * mc.EPS64 * scale),
                                                                     float(abs(h1 - h0) / ((n + 8) * mc.EPS64 * scale))))
    assert abs(h1 - h0) <= (n + 8) * mc.EPS64 * scale
    assert not _bits(T1, W) and not _bits(f1, f0) and (f1 > 0).any() and (f1 < 1).any()


# ---- what the constructors and the C entries refuse, without a GPU ------------------------------------------------------------------
def test_laws_and_losses_are_checked():
    with pytest.raises(ValueError, match='2 laws for 3 materials'):
        MapPhaseField.correct_of(xc.LAWS[:2], mc.MATERIALS, HOLES['T0'], HOLES['T0'], HOLES['mask'], HOLES['ids'], None)
    with pytest.raises(TypeError, match='PhaseChange or None'):
        MapPhaseField._checked_laws((xc.LAWS[0], 'steel', None), mc.MATERIALS)
    with pytest.raises(TypeError):
        MapPhaseField._checked_laws(5, mc.MATERIALS)
    with pytest.raises(ValueError, match='2 losses for 3 materials'):
        MapLossPacks._checked_losses(xc.LOSSES[:2], 3)
    with pytest.raises(TypeError, match='SurfaceLoss'):
        MapLossPacks._checked_losses((xc.LOSSES[0], None, xc.LOSSES[2]), 3)


def test_argument_errors_of_the_c_entries():
    lib, check = _lib.lib, _lib.check
    p8 = ctypes.c_void_p(8)
    n = 3
    laws = (_lib.PhaseChangeLaw * n)(*[_lib.PhaseChangeLaw(2.7e5, 1400.0, 1450.0)] * n)
    on = (ctypes.c_int * n)(1, 1, 0)
    cp = (ctypes.c_double * n)(490.0, 385.0, 900.0)
    with pytest.raises(ValueError, match='null argument'):
        check(lib.adi_matmap_phase_apply(n, laws, on, cp, p8, ctypes.c_void_p(16), p8, None, None, None, p8, p8, 4, 4, 4, 0, None))
    with pytest.raises(ValueError, match='aliases'):
        check(lib.adi_matmap_phase_apply(n, laws, on, cp, p8, p8, p8, None, p8, None, p8, p8, 4, 4, 4, 0, None))
    with pytest.raises(ValueError, match='9 materials'):
        check(lib.adi_matmap_phase_seed(9, laws, on, p8, ctypes.c_void_p(16), p8, None, p8, None, p8, p8, 4, 4, 4, 0, None))
    bad = (_lib.PhaseChangeLaw * n)(_lib.PhaseChangeLaw(2.7e5, 1400.0, 1450.0), _lib.PhaseChangeLaw(2.7e5, 1450.0, 1400.0),
                                    _lib.PhaseChangeLaw(0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match='T_liquidus'):
        check(lib.adi_matmap_phase_apply(n, bad, on, cp, p8, ctypes.c_void_p(16), p8, None, p8, None, p8, p8, 4, 4, 4, 0, None))
    # (the record of a material without a law is not read)
    on2 = (ctypes.c_int * n)(1, 0, 0)
    with pytest.raises(ValueError, match='bad grid'):
        check(lib.adi_matmap_phase_apply(n, bad, on2, cp, p8, ctypes.c_void_p(16), p8, None, p8, None, p8, p8, 0, 4, 4, 0, None))
    nbytes = int(lib.adi_matmap_loss_table_bytes())
    assert 4096 < nbytes < 8192
    buf = (ctypes.c_char * nbytes)()
    C = (ctypes.c_double * n)(*[rho * c for rho, c, _ in mc.MATERIALS])
    sl = (_lib.SurfaceLossLaw * n)(*[w.as_c() for w in xc.LOSSES])
    check(lib.adi_matmap_loss_table(n, sl, C, mc.DX, buf, nbytes))
    assert any(b != 0 for b in buf.raw)
    with pytest.raises(ValueError, match='needs %d bytes' % nbytes):
        check(lib.adi_matmap_loss_table(n, sl, C, mc.DX, buf, nbytes - 8))
    with pytest.raises(ValueError, match='0 materials'):
        check(lib.adi_matmap_loss_table(0, sl, C, mc.DX, buf, nbytes))
    neg = SurfaceLoss(h=1.0).as_c()
    neg.h[2] = -1.0
    with pytest.raises(ValueError, match='h < 0'):
        check(lib.adi_matmap_loss_table(1, (_lib.SurfaceLossLaw * 1)(neg), C, mc.DX, buf, nbytes))
    co = _lib.ptr_array([8, 8, 8])
    with pytest.raises(ValueError, match='ambient in kelvin'):
        check(lib.adi_matmap_loss_update(p8, -300.0, 273.15, p8, p8, None, p8, 4, 4, 4, 0, mc.DX, co, 0, 4, 0, None))
    with pytest.raises(ValueError, match='bad plane range'):
        check(lib.adi_matmap_loss_update(p8, 20.0, 273.15, p8, p8, None, p8, 4, 4, 4, 0, mc.DX, co, 0, 5, 0, None))
    with pytest.raises(ValueError, match='null argument'):
        check(lib.adi_matmap_loss_update(p8, 20.0, 273.15, p8, p8, None, None, 4, 4, 4, 0, mc.DX, co, 0, 4, 0, None))


# ---- the kernels' footprint ----------------------------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_meta
    if not os.path.isdir(kernel_meta.LLVM):
        pytest.skip('no ROCm LLVM tools at %s' % kernel_meta.LLVM)
    ks = [k for k in kernel_meta.all_kernels() if k['obj'] in ('adi_matmap_phase.o', 'adi_matmap_loss.o')]
    names = {re.match(r'adi::(\w+)', k['short']).group(1) for k in ks}
    assert names == {'k_mapphase_apply', 'k_mapphase_seed', 'k_maploss'} and len(ks) == 6
    for k in ks:
        print('%-32s %3d VGPRs %3d SGPRs %4d B LDS %d B scratch' % (k['short'], k['vgpr_count'], k['sgpr_count'], k['lds'],
                                                                    k['scratch']))
    bad = ['%s: %d B scratch, %d spilled VGPRs' % (k['short'], k['scratch'], k.get('vgpr_spill_count', 0))
           for k in ks if k['scratch'] != 0 or k.get('vgpr_spill_count', 0) != 0]
    assert not bad, '\n'.join(bad)
