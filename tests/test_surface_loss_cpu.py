"""CPU: the temperature-dependent surface loss (SurfaceLoss, adi_surface_loss_update) without a GPU -- the NumPy statement of the
law against the h fields the golden vectors were generated with (tests/golden/make_golden_surface_loss.py restates the law
on its own), parameter validation in Python and in the C ABI (every rejection happens before any HIP call), and the pinned
C oracle driven with `h_of` arrays against every golden temperature field: that oracle loop is what the GPU tests compare
with where the reference is not present."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import adi_thermal_fields_amd.adi3d_hip_coeff as hip  # noqa: E402
from adi_thermal_fields_amd import _lib  # noqa: E402
from oracle import adi_oracle as orc  # noqa: E402
import surface_loss_cases as slc  # noqa: E402
from surface_loss_cases import FACES  # noqa: E402


def _last_input(c):
    """the field the last step of the case started from"""
    s, _, nsteps, _, _ = slc.segments(c)[-1]
    return c['seg%d_T%d' % (s, nsteps - 1)]


@pytest.mark.parametrize('name', slc.CASES)
def test_h_of_is_the_golden_law_bit_for_bit(name):
    c = slc.load(name)
    loss = slc.loss_of(c, hip.SurfaceLoss)
    Tinf = float(c['Tinf'])
    for f in FACES:
        first = loss.h_of(c['T0'], f, Tinf)
        assert first.dtype == np.float64 and np.array_equal(first, c['h_first_' + f]), (name, f)
        assert np.array_equal(loss.h_of(_last_input(c), f, Tinf), c['h_last_' + f]), (name, f)
    if name == 'table':
        # the case holds temperatures below the first knot, above the last and exactly on every knot
        T0, xp = c['T0'], c['table_T']
        assert (T0 < xp[0]).any() and (T0 > xp[-1]).any() and all((T0 == x).any() for x in xp)
        on = loss.h_of(xp, 'z+', Tinf)
        assert np.array_equal(on, float(c['h'][5]) + c['table_h'])                    # (emissivity 0: rad = 0)
        assert np.array_equal(loss.h_of(T0, 'y+', Tinf), np.zeros_like(T0))         # no h, no emissivity: no table either


def test_scalar_and_dict_specifications_agree():
    T = np.linspace(20.0, 1500.0, 41)
    a = hip.SurfaceLoss(h=12.0, emissivity=0.7)
    b = hip.SurfaceLoss(h={f: 12.0 for f in FACES}, emissivity={f: 0.7 for f in FACES})
    for f in FACES:
        assert np.array_equal(a.h_of(T, f, 25.0), b.h_of(T, f, 25.0))
    # the five lines, written out
    Tk, Ta = T + 273.15, 25.0 + 273.15
    want = (12.0 + 0.0) + ((0.7 * 5.670374419e-8) * (Tk * Tk + Ta * Ta)) * (Tk + Ta)
    assert np.array_equal(a.h_of(T, 'x-', 25.0), want)
    # a missing face carries nothing
    assert np.array_equal(hip.SurfaceLoss(h={'x-': 3.0}, emissivity={'x-': 0.5}).h_of(T, 'y+', 25.0), np.zeros_like(T))
    # the order of magnitude the issue is about: deposit against interpass temperature
    rad = hip.SurfaceLoss(emissivity=1.0)
    assert rad.h_of(np.array([1500.0]), 'z+', 25.0)[0] > 10.0 * rad.h_of(np.array([150.0]), 'z+', 25.0)[0]


def test_validation_errors():
    SL = hip.SurfaceLoss
    with pytest.raises(ValueError, match='emissivity'):
        SL(emissivity=1.2)
    with pytest.raises(ValueError, match='emissivity'):
        SL(emissivity={'x-': -0.1})
    with pytest.raises(ValueError, match='h < 0'):
        SL(h={'z+': -1.0})
    with pytest.raises(ValueError, match='do not increase'):
        SL(h=1.0, table=([0.0, 100.0, 100.0], [1.0, 2.0, 3.0]))
    with pytest.raises(ValueError, match='do not increase'):
        SL(h=1.0, table=([0.0, 200.0, 100.0], [1.0, 2.0, 3.0]))
    with pytest.raises(ValueError, match='knots'):
        SL(h=1.0, table=(np.arange(17.0), np.ones(17)))
    with pytest.raises(ValueError, match='knots'):
        SL(h=1.0, table=([5.0], [1.0]))
    SL(h=1.0, table=(np.arange(16.0), np.ones(16)))                               # 16 knots are allowed
    with pytest.raises(ValueError, match='bad face'):
        SL(h={'w-': 1.0})
    with pytest.raises(ValueError, match='bad face'):
        SL(emissivity={'top': 0.5})
    ok = SL(h=5.0, emissivity=0.5)
    with pytest.raises(ValueError, match='bad face'):
        ok.h_of(np.zeros(3), 'q+', 20.0)
    with pytest.raises(ValueError, match='Tinf'):
        ok.h_of(np.zeros(3), 'x-', -273.15)
    with pytest.raises(ValueError, match='Tinf'):
        ok.validate(Tinf=-300.0)
    with pytest.raises(ValueError, match='Tinf'):
        SL(emissivity=0.5, T_offset=0.0).validate(Tinf=0.0)                        # a field in kelvin, ambient at 0 K
    ok.emissivity = 2.0                                                            # attributes may change; validate() re-checks
    with pytest.raises(ValueError, match='emissivity'):
        ok.validate()


def _law(**kw):
    d = dict(h=[10.0] * 6, emissivity=[0.5] * 6, T_offset=273.15, n_knots=0, knot_T=[0.0] * 16, knot_h=[0.0] * 16)
    d.update(kw)
    D6, D16 = ctypes.c_double * 6, ctypes.c_double * 16
    return _lib.SurfaceLossLaw(D6(*d['h']), D6(*d['emissivity']), d['T_offset'], d['n_knots'], 0, D16(*d['knot_T']),
                               D16(*d['knot_h']))


def _call(law, Tinf=20.0, d_T=8, d_flags=8, coeff=(8, 8, 8), dims=(4, 4, 4), k=(0, 4), full=0, null_law=False, null_coeff=False):
    arr = None if null_coeff else _lib.ptr_array([p or None for p in coeff])
    return _lib.lib.adi_surface_loss_update(None if null_law else ctypes.byref(law), Tinf, ctypes.c_void_p(d_T or None),
                                            ctypes.c_void_p(d_flags or None), None, dims[0], dims[1], dims[2], 0, 1e-3, 7800.0,
                                            490.0, arr, k[0], k[1], full, None)


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    """every call here must fail on its arguments: the pointers are not device memory, so a launch would be a fault"""
    chk = _lib.check
    good = _law()
    with pytest.raises(ValueError, match='null argument'):
        chk(_call(good, null_law=True))
    with pytest.raises(ValueError, match='null argument'):
        chk(_call(good, d_T=0))
    with pytest.raises(ValueError, match='null argument'):
        chk(_call(good, d_flags=0))
    with pytest.raises(ValueError, match='null argument'):
        chk(_call(good, null_coeff=True))
    with pytest.raises(ValueError, match='null output'):
        chk(_call(good, coeff=(8, 0, 8)))
    with pytest.raises(ValueError, match='bad plane range'):
        chk(_call(good, k=(3, 2)))
    with pytest.raises(ValueError, match='bad plane range'):
        chk(_call(good, k=(0, 5)))
    with pytest.raises(ValueError, match='bad plane range'):
        chk(_call(good, k=(-1, 2), full=1))
    with pytest.raises(ValueError, match='bad grid'):
        chk(_call(good, dims=(0, 4, 4)))
    with pytest.raises(ValueError, match='emissivity'):
        chk(_call(_law(emissivity=[0.5, 0.5, 1.5, 0.5, 0.5, 0.5])))
    with pytest.raises(ValueError, match='emissivity'):
        chk(_call(_law(emissivity=[0.5, float('nan'), 0.5, 0.5, 0.5, 0.5])))
    with pytest.raises(ValueError, match='h < 0'):
        chk(_call(_law(h=[1.0, 1.0, 1.0, 1.0, -2.0, 1.0])))
    with pytest.raises(ValueError, match='Tinf \\+ T_offset'):
        chk(_call(good, Tinf=-273.15))
    with pytest.raises(ValueError, match='knots'):
        chk(_call(_law(n_knots=1)))
    with pytest.raises(ValueError, match='knots'):
        chk(_call(_law(n_knots=17)))
    with pytest.raises(ValueError, match='do not increase'):
        chk(_call(_law(n_knots=3, knot_T=[0.0, 5.0, 5.0] + [0.0] * 13)))
    # an empty plane range with valid arguments is a no-op that reaches no HIP call
    assert _call(good, k=(2, 2)) == _lib.ADI_OK
    # and the Python law hands the C struct what it validated
    s = hip.SurfaceLoss(h={'x+': 3.0}, emissivity=0.25, table=([0.0, 10.0], [1.0, 2.0]), T_offset=273.15).as_c(20.0)
    assert list(s.h) == [0.0, 3.0, 0.0, 0.0, 0.0, 0.0] and list(s.emissivity) == [0.25] * 6
    assert s.n_knots == 2 and list(s.knot_T)[:2] == [0.0, 10.0] and list(s.knot_h)[:2] == [1.0, 2.0]


@pytest.mark.parametrize('name', slc.CASES)
def test_oracle_with_h_of_reproduces_the_golden_fields(name):
    """the pinned C oracle + SurfaceLoss.h_of is the reference's lagged loop: every golden T to <= 1e-12 relative L-inf, every
    golden coefficient array bit for bit"""
    c = slc.load(name)
    loss = slc.loss_of(c, hip.SurfaceLoss)
    seen = []

    def visit(s, n, T, packs):
        if n == 0:
            for ax, p in zip('xyz', packs):
                assert np.array_equal(p.coeff, c['seg%d_coeff_%s' % (s, ax)]), (name, s, ax)
            return
        e = slc.rel_linf(T, c['seg%d_T%d' % (s, n)])
        seen.append(e)
        assert e <= 1e-12, (name, s, n, e)
        last = slc.segments(c)[-1]
        if s == last[0] and n == last[2]:
            for ax, p in zip('xyz', packs):
                assert np.array_equal(p.coeff, c['coeff_last_' + ax]), (name, ax)
    slc.run_lagged(orc, c, loss, visit)
    assert len(seen) == sum(seg[2] for seg in slc.segments(c))
    print(name, 'max rel L-inf vs the reference: %.3e' % max(seen))


def test_plain_case_is_the_scalar_h_pack():
    """emissivity 0, no table: (h + 0) + 0 = h, so the golden arrays are those of the ordinary per-face scalar packs"""
    c = slc.load('plain')
    grid = orc.Grid3D(*c['mask'].shape, float(c['dx']), c['mask'])
    packs = orc.precompute_coeff_packs_unified(grid, orc.Material(float(c['rho']), float(c['cp']), float(c['k'])),
                                               robin_h={f: float(v) for f, v in zip(FACES, c['h'])})
    for ax, p in zip('xyz', packs):
        assert np.array_equal(p.coeff, c['seg0_coeff_' + ax]) and np.array_equal(p.coeff, c['coeff_last_' + ax])
        assert p.coeff.max() > 0.0


def test_golden_cases_hold_what_they_are_there_to_catch():
    c = slc.load('holes')
    m = np.pad(c['mask'], 1)
    for a in range(3):
        sl = lambda d: tuple(slice(1 + (d if i == a else 0), 1 + (d if i == a else 0) + c['mask'].shape[i]) for i in range(3))
        lo, hi = ~m[sl(-1)] & c['mask'], ~m[sl(+1)] & c['mask']
        for want in ((lo & ~hi), (hi & ~lo), (lo & hi), (c['mask'] & ~lo & ~hi)):     # minus, plus, both, neither
            assert want.any(), a
    assert (c['h'] == 0).sum() == 1 and (c['emissivity'] == 0).sum() == 1 and bool(c['has_dir']) and c['neumann_on'].any()
    assert 0.6 < float(c['k']) / (float(c['rho']) * float(c['cp'])) * float(c['seg0_dt']) / float(c['dx']) ** 2 < 0.8
    c = slc.load('long')
    assert c['mask'].shape == (37, 6, 70) and int(c['seg0_nsteps']) == 6 and float(c['theta']) == 1.0
    c = slc.load('birth')
    assert int(c['nseg']) == 4 and len({float(c['seg%d_dt' % s]) for s in range(4)}) == 4
    # a cell exposed before a birth and covered by it: its coefficient must fall to zero (stale exposure)
    assert ((c['seg0_coeff_z'] != 0) & (c['seg1_coeff_z'] == 0)).any()
    for name in slc.CASES:
        c = slc.load(name)
        assert c['T0'][c['mask']].min() >= 20.0 and c['T0'].max() <= 1500.0, name
