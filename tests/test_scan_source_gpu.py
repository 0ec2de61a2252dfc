"""GPU: a ScanPathSource (a frozen ScanPath evaluated on the device) against the host definition ScanPath.sample_step -- as a
field (sample_step_device), and that field as the source field of the step, where the yardstick is the pinned CPU oracle with the
host field folded into the axis-0 pack (scan_cases.oracle_step).  Bars: scan_source_cases."""
import numpy as np
import pytest

import scan_cases as sc
import scan_source_cases as ssc
from scan_cases import DT, DX, RHO, CP, K, rel_linf
from test_scan_path_gpu import _two_leg_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from oracle import adi_oracle as orc
    return hip, orc


@pytest.fixture(scope='module')
def all_cases(mods):
    return {c[0]: c for c in ssc.cases(mods[0])}


# ----------------------------------------------------------------------------------------------------------------- the field
@pytest.mark.parametrize('name', ssc.CASE_IDS)
def test_device_field_vs_sample_step(mods, all_cases, name):
    hip, _ = mods
    _, path, shape, mask, t, dt, bar, deposits = all_cases[name]
    g = hip.Grid3D(*shape, DX, np.ones(shape, dtype=bool) if mask is None else mask)
    want = path.sample_step(g, t, dt)
    got = np.asarray(path.on_device().sample_step_device(g, t, dt))
    if not deposits:
        assert not want.any()
        np.testing.assert_array_equal(got, 0.0)
        return
    err = rel_linf(got, want)
    print('%s: device field vs sample_step %.2e (bar %.0e)' % (name, err, bar))
    assert err <= bar
    np.testing.assert_array_equal(got[~np.asarray(g.mask, dtype=bool)], 0.0)
    np.testing.assert_array_equal(got[~ssc.support_boxes(path, shape, t, dt)], 0.0)


# ------------------------------------------------------------------------- the device field as the source field of the step
@pytest.mark.parametrize('shape,s', [((37, 29, 45), sc.SHAPE), ((130, 12, 20), sc.SMALL)], ids=['37x29x45', '130x12x20'])
def test_step_with_the_device_field_vs_oracle(mods, shape, s):
    """a step that holds a corner, S= the DeviceField of sample_step_device (nothing crosses PCIe), against the oracle with the
    host field folded into the axis-0 pack: the existing bar of the field form"""
    hip, orc = mods
    g, go, mat, mato, prm, prmo, packs, kw, T0 = sc.setup(hip, orc, shape)
    path = _two_leg_path(hip, shape, s, 0.25 * DT)
    t = 0.6 * DT
    assert path._piece(0, t, t + DT) and path._piece(1, t, t + DT)
    S = path.on_device().sample_step_device(g, t, DT)
    assert isinstance(S, hip.DeviceField)
    got = hip.adi_step_numba_coeff(T0, g, mat, prm, packs, Tinf=300.0, S=S)
    want = sc.oracle_step(orc, T0, go, mato, prmo, kw, path.sample_step(go, t, DT))
    err = rel_linf(got, want)
    print('%s: step with the device field vs oracle %.2e' % (shape, err))
    assert err <= ssc.bar_of(path, t, DT)
    np.testing.assert_array_equal(got[~go.mask], T0[~go.mask])
    dm = kw['dir_mask']
    assert dm.any()
    np.testing.assert_array_equal(got[dm], want[dm])
    plain = orc.adi_step_numba_coeff(T0, go, mato, prmo, orc.precompute_coeff_packs_unified(go, mato, **kw), Tinf=300.0)
    assert rel_linf(want, plain) > 1e-4                     # the source matters at this scale


def test_raster_20_steps_with_the_device_field_vs_oracle(mods):
    """the raster of test_scan_path_gpu.test_raster_20_steps_vs_oracle, every step fed by the device field; the oracle loop takes
    the host field: the project's bar for several steps"""
    hip, orc = mods
    shape = (40, 48, 24)
    g, go, mat, mato, prm, prmo, packs, kw, T0 = sc.setup(hip, orc, shape)
    length = 3 * 20 * DX + 2 * 8 * DX
    path = hip.ScanPath.raster((10 * DX, 14 * DX), (30 * DX, 30.5 * DX), 8 * DX, length / (19.3 * DT), 800.0, depth=22 * DX,
                               t_start=0.4 * DT, **sc.SHAPE)
    assert path.n_segments == 5 and path.t_end < 20 * DT
    src = path.on_device()
    T, To = hip.to_device(T0), T0.copy()
    for n in range(20):
        T = hip.adi_step_numba_coeff(T, g, mat, prm, packs, Tinf=300.0, S=src.sample_step_device(g, n * DT, DT))
        To = sc.oracle_step(orc, To, go, mato, prmo, kw, path.sample_step(go, n * DT, DT))
    got = np.asarray(T)
    err = rel_linf(got, To)
    print('raster, 20 steps with the device field: vs oracle %.2e' % err)
    assert err <= 1e-10
    assert got.max() > T0.max() + 5.0
    np.testing.assert_array_equal(got[~go.mask], T0[~go.mask])


def test_a_source_is_refused_as_the_path_is(mods):
    """neither the step nor the stepper takes the frozen path for something else: the TypeError still points to sample_step"""
    hip, orc = mods
    shape = (16, 12, 10)
    g = hip.Grid3D(*shape, DX, np.ones(shape, dtype=bool))
    mat, prm = hip.Material(RHO, CP, K), hip.Params(DT, 0.5)
    packs = hip.precompute_coeff_packs_unified(g, mat)
    src = sc.leg_path(hip, sc.SMALL, (4 * DX, 5 * DX, 5 * DX), 0.0, 6 * DX, 0.4).on_device()
    with pytest.raises(TypeError, match='sample_step_device'):
        hip.adi_step_numba_coeff(np.zeros(shape), g, mat, prm, packs, S=src)
    with pytest.raises(TypeError, match='sample_step'):
        hip.StagedStepper(g, mat, prm, packs, source=src)
