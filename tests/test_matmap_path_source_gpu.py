"""GPU: a ScanPath inside the step of a MaterialMap without a source field (MapPathSource).  The stage and the step
against the field form S=src.sample_step_device(grid, t, dt), bit for bit: both run scan_q_step on the same arguments and add
(dt * q) / C[id] to the same R0, so equality is asked, not a tolerance.  The windows are those of tests/matmap_path_cases.py
(checked without a device by test_matmap_path_source_cpu.py, and here again from `window()` before the launch).  The device
against the library's host twin at the bar of scan_source_cases; the step against the long-double reference and
MaterialMap.step_reference at the bar of tests/test_matmap_gpu.py; the driver against its loop written out with the field."""
import numpy as np
import pytest

import matmap_deposit_cases as dc
import matmap_eight_cases as ec
import matmap_extras_cases as xc
import matmap_cases as mc
import matmap_path_cases as pc
import scan_cases as sc
import scan_source_cases as ssc
import transitions_cases as tc
from scan_cases import DX, rel_linf

pytestmark = pytest.mark.gpu

KEY = ('eight', ec.HOLES, 'padded', None, 0.5, 0.3)        # the (20, 18, 35) case with holes, held in a (21, 20, 38) box


@pytest.fixture(scope='module')
def hip():
    import adi_thermal_fields_amd.adi3d_hip_coeff as m
    return m


@pytest.fixture(scope='module')
def cases(hip):
    return {c[0]: c for c in pc.stage_cases(hip)}


_RIGS = {}


def _rig(hip, shape):
    """(grid, map of eight materials at random with 255 off the mask, mask, ids, T0) on the mask of the Goldak tests; one per shape"""
    if shape not in _RIGS:
        mask = ssc.case_mask(shape)
        ids, T0 = pc.ids_and_field(shape, mask)
        grid = hip.Grid3D(*shape, DX, mask)
        mm = hip.MaterialMap(grid, pc.MATERIALS8, ids, robin_h=350.0, neumann={'z-': 2e5})
        T0.setflags(write=False)
        _RIGS[shape] = (grid, mm, mask, ids, T0)
    return _RIGS[shape]


def _inside(shape, box):
    m = np.zeros(shape, dtype=bool)
    m[tuple(slice(lo, hi) for lo, hi in box)] = True
    return m


def _stage_holds(hip, grid, mm, mask, ids, T0, path, t, dt, name, theta=0.5):
    """the stage against the field form (equality) and the host twin (bar_of); returns the window's box"""
    src = path.on_device()
    msrc = hip.MapPathSource(mm, src)
    prm = hip.Params(dt, theta)
    box = msrc.window(t, dt)[2]
    inside = _inside(T0.shape, box)
    got = np.asarray(msrc.explicit_rhs(np.array(T0), prm, t))
    field = np.asarray(mm.explicit_rhs(np.array(T0), prm, S=src.sample_step_device(grid, t, dt)))
    plain = np.asarray(mm.explicit_rhs(np.array(T0), prm))
    changed = got.view(np.int64) != plain.view(np.int64)
    print('%s: box %s = %d cells, %d in the mask, %d written; stage equal to the field form: %s'
          % (name, box, int(inside.sum()), int((inside & mask).sum()), int(changed.sum()), np.array_equal(got, field)))
    assert np.array_equal(got, field)
    assert changed.any() and not changed[~inside].any() and not changed[~mask].any()
    # from a field of zeros the explicit stage gives R0 = 0 exactly, so the result IS the increment (dt * q) / C[id]
    inc = np.asarray(msrc.explicit_rhs(np.zeros(T0.shape), prm, t))
    twin, tbox = pc.host_twin(src, sc.HostGrid(T0.shape, grid.dx, mask), ids, np.zeros(T0.shape), t, dt,
                              C=[m.rho * m.cp for m in mm.materials])
    bar = ssc.bar_of(path, t, dt)
    err = rel_linf(inc, twin)
    print('%s: increment, device against the host twin %.2e (bar %.0e)' % (name, err, bar))
    assert tbox == box and err <= bar
    assert np.array_equal(inc != 0, twin != 0)
    return box


# ---- 1. the stage ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', pc.STAGE_IDS)
def test_stage_is_the_field_form_bit_for_bit(hip, cases, name):
    _, path, shape, t, dt, want = cases[name]
    grid, mm, mask, ids, T0 = _rig(hip, shape)
    pc.check_window(path, shape, t, dt, want, hip.MapPathSource(mm, path).window(t, dt))
    _stage_holds(hip, grid, mm, mask, ids, T0, path, t, dt, name)


def _padded_rig(hip, monkeypatch):
    monkeypatch.setattr(hip, 'recommended_dims', ec.pad_dims)
    c = ec.case(KEY)
    grid = hip.Grid3D(*c['shape'], c['dx'], c['mask'])
    assert grid.layout.padded
    mm = hip.MaterialMap(grid, c['materials'], np.array(c['ids']), **ec.bc_of(c))
    path = hip.ScanPath(eta=0.8, a=3e-3, b=3e-3, c_f=3e-3, c_r=6e-3, power=2000.0, start=(6e-3, 9e-3, 35e-3))
    path.line_to((15e-3, 9e-3, 35e-3), speed=1.0)
    return c, grid, mm, path, hip.Params(c['dt'], c['theta'])


def test_stage_on_the_padded_layout_with_holes_and_all_eight_materials(hip, monkeypatch):
    c, grid, mm, path, prm = _padded_rig(hip, monkeypatch)
    t = 1e-3
    box = _stage_holds(hip, grid, mm, c['mask'], np.array(c['ids']), c['T0'], path, t, prm.dt, 'padded', theta=c['theta'])
    inside = _inside(c['shape'], box)
    q = path.sample_step(sc.HostGrid(c['shape'], c['dx'], c['mask']), t, prm.dt)
    counts = [int(((q > 0) & c['mask'] & (c['ids'] == m)).sum()) for m in range(8)]
    print('in-mask heated cells of each material: %s; holes inside the box: %d' % (counts, int((inside & ~c['mask']).sum())))
    assert min(counts) >= 20 and (inside & ~c['mask']).sum() >= 20


# ---- 2. the step -----------------------------------------------------------------------------------------------------------------
def _hold(X, c, ref, what):
    ok, f = ec.meets_bar(np.asarray(X), c, ref)
    print('%-64s inc %.2e K  err %.2e K = %8.2f ulp  bar %.2e' % (what, f['inc'], f['abs_err'], f['ulp'], ec.bar(f, ec.A_MAP)))
    assert ec.untouched_exact(np.asarray(X), c) and ok, (what, f)


def test_step_is_the_field_form_and_holds_the_bar_of_the_references(hip, monkeypatch):
    from adi_thermal_fields_amd.packs import MaterialMap
    c, grid, mm, path, prm = _padded_rig(hip, monkeypatch)
    src, t = path.on_device(), 1e-3
    msrc = hip.MapPathSource(mm, src)
    step = lambda **kw: np.asarray(hip.adi_step_numba_coeff(np.array(c['T0']), grid, mm.mat, prm, mm.packs, c['Tinf'],
                                                            material_map=mm, **kw))
    X = step(S=msrc, t=t)
    F = step(S=src.sample_step_device(grid, t, prm.dt))
    plain = step()
    print('step: path form equal to the field form: %s' % np.array_equal(X, F))
    assert np.array_equal(X, F) and not np.array_equal(X, plain)
    Sh = path.sample_step(sc.HostGrid(c['shape'], c['dx'], c['mask']), t, prm.dt)
    _hold(X, c, ec.reference_of(c, S=Sh), 'step with MapPathSource vs the long-double reference')
    W = ec.run(MaterialMap.step_reference, MaterialMap.packs_reference, c, S=Sh)
    dirc = c['mask'] & c['dir_mask']
    ref = (W[c['mask']], float(np.max(np.abs(W - c['T0'])[c['mask'] & ~dirc])), float(np.max(np.abs(W[c['mask']]))))
    _hold(X, c, ref, 'step with MapPathSource vs MaterialMap.step_reference')
    # a window without a powered piece: the step without S, and no launch
    for tt in (-5.0, path.t_end + 1e-3):
        assert msrc.window(tt, prm.dt)[2] == ((0, 0), (0, 0), (0, 0))
        assert np.array_equal(step(S=msrc, t=tt), plain)


def _full_rig(hip):
    """the rig of tests/test_transitions_gpu.py -- a dense plate under a powder layer with a copper bar through both, at 1300 K
    -- with a surface loss per material and a monitor, under a beam that turns a corner on the powder"""
    shape = (24, 20, 16)
    mask = np.zeros(shape, bool)
    mask[:, :, :12] = True
    ids = np.full(shape, 1, np.uint8)
    ids[:, :, 8:] = 0
    ids[:3, :, :] = 2
    grid = hip.Grid3D(*shape, tc.DX, mask)
    mm = hip.MaterialMap(grid, tc.MATERIALS, ids, robin_h=None)
    T0 = np.where(mask, 1300.0, tc.TINF)
    mph = hip.MapPhaseField(mm, tc.LAWS, T=hip.to_device(T0))
    tr = hip.MaterialTransitions(mm, tc.RULES['powder'], phase=mph)
    lp = hip.MapLossPacks(mm, xc.LOSSES8[:len(tc.MATERIALS)], tc.TINF)
    mon = hip.FieldMonitor(grid, probes=[(12, 10, 11), (6, 10, 9)], regions=[((0, 24), (0, 20), (0, 8)), ((0, 24), (0, 20), (8, 12))],
                           capacity=8, material_map=mm)
    path = hip.ScanPath(power=30000.0, eta=0.8, a=4e-3, b=4e-3, c_f=4e-3, c_r=6.4e-3, f_f=0.6, start=(7e-3, 8e-3, 12e-3))
    path.line_to((7.9e-3, 8e-3, 12e-3), 0.08).line_to((7.9e-3, 9.2e-3, 12e-3), 0.08)
    return dict(grid=grid, mm=mm, mph=mph, tr=tr, lp=lp, mon=mon, src=path.on_device(), T=hip.to_device(T0), ids=ids)


def _same(a, b, what='result'):
    if isinstance(a, dict):
        assert set(a) == set(b), what
        for k in a:
            _same(a[k], b[k], '%s[%s]' % (what, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, '%s[%d]' % (what, i))
    else:
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=what)


def test_step_with_loss_phase_transitions_and_a_monitor_all_together(hip):
    from adi_thermal_fields_amd import waam
    a, b = _full_rig(hip), _full_rig(hip)
    prm = hip.Params(4e-3, 0.5)
    msrc = hip.MapPathSource(a['mm'], a['src'])
    for n in range(6):                                      # the corner is in the third step
        t = n * prm.dt
        kw = lambda r: dict(material_map=r['mm'], surface_loss=r['lp'], phase=r['mph'], transitions=r['tr'], monitor=r['mon'], t=t)
        a['T'] = hip.adi_step_numba_coeff(a['T'], a['grid'], a['mm'].mat, prm, a['mm'].packs, tc.TINF, S=msrc, **kw(a))
        b['T'] = hip.adi_step_numba_coeff(b['T'], b['grid'], b['mm'].mat, prm, b['mm'].packs, tc.TINF,
                                          S=b['src'].sample_step_device(b['grid'], t, prm.dt), **kw(b))
        assert np.array_equal(np.asarray(a['T']), np.asarray(b['T'])), n
        assert np.array_equal(a['mm'].ids, b['mm'].ids) and a['tr'].changed == b['tr'].changed, n
        assert np.array_equal(np.asarray(a['mph'].liquid_fraction), np.asarray(b['mph'].liquid_fraction)), n
    print('cells that changed their material in six steps: %d; liquid cells: %d'
          % (a['tr'].changed, int((np.asarray(a['mph'].liquid_fraction) > 0).sum())))
    assert a['tr'].changed > 0 and (a['mm'].ids != a['ids']).any() and np.asarray(a['mph'].liquid_fraction).max() > 0
    ra, rb = waam.monitor_result(a['mon'], a['mm'].mat), waam.monitor_result(b['mon'], b['mm'].mat)
    assert len(ra[0]['t']) == 6
    _same(ra, rb, 'monitor')


# ---- 3. the driver ---------------------------------------------------------------------------------------------------------------
def test_run_path_deposition_heated_is_its_loop_with_the_field(hip):
    from adi_thermal_fields_amd import waam
    from bead_cases import DX as BDX, TS
    path, bead, plate, dt, steps = dc.raster()
    ids = dc.plate_ids(plate)
    got_T, got_mask, n = waam.run_path_deposition(hip, plate, path, bead, BDX, mc.STEEL, dc.H, dc.TINF, TS, dc.THETA, dt, heat=True,
                                                  material_map=dict(materials=dc.MATERIALS, ids=ids, wire=dc.WIRE))
    grid = hip.Grid3D(*dc.SHAPE, BDX, plate)
    mm = hip.MaterialMap(grid, dc.MATERIALS, ids, robin_h={f: dc.H for f in dc.ROBIN})
    prm = hip.Params(dt, dc.THETA)
    T = hip.to_device(np.full(dc.SHAPE, dc.TINF))
    src = path.on_device()
    dep = hip.PathDeposit(grid, src, bead, TS, material_map=mm, material_id=dc.WIRE)
    for t, d in steps:
        rng = dep.deposit(T, t, d)
        if rng is not None:
            mm.update(*rng)
        prm.dt = d
        T = hip.adi_step_numba_coeff(T, grid, mm.mat, prm, mm.packs, Tinf=dc.TINF, S=src.sample_step_device(grid, t, d), t=t,
                                     material_map=mm)
    assert n == len(steps) == 12 and max(dc.SHAPE) <= 48
    np.testing.assert_array_equal(got_T, np.asarray(T))
    np.testing.assert_array_equal(got_mask, grid.d_mask.cpu().numpy().astype(bool))
    cold_T, cold_mask, _ = waam.run_path_deposition(hip, plate, path, bead, BDX, mc.STEEL, dc.H, dc.TINF, TS, dc.THETA, dt,
                                                    material_map=dict(materials=dc.MATERIALS, ids=ids, wire=dc.WIRE))
    print('two beads: %d cells born; the heated run is up to %.1f K above the unheated one' % (got_mask.sum() - plate.sum(),
                                                                                               (got_T - cold_T).max()))
    assert got_mask.sum() > plate.sum() and np.array_equal(got_mask, cold_mask) and (got_T - cold_T).max() > 10.0


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(hip):
    shape = ssc.AXIS_SHAPE
    grid, mm, mask, ids, T0 = _rig(hip, shape)
    path = ssc.oblique(hip, 2)
    msrc = hip.MapPathSource(mm, path)
    prm = hip.Params(sc.DT, 0.5)
    with pytest.raises(TypeError, match='does not ride a captured graph.*adi_step_numba_coeff'):
        hip.StagedStepper(grid, mm.mat, prm, mm.packs, 20.0, material_map=mm, source=msrc)
    plain_packs = hip.precompute_coeff_packs_unified(grid, mm.mat, robin_h={'z+': 350.0})
    for bare in (path, path.on_device()):                   # today's messages, with and without a map
        with pytest.raises(TypeError, match='source must be a GoldakSource'):
            hip.StagedStepper(grid, mm.mat, prm, plain_packs, 20.0, source=bare)
        with pytest.raises(ValueError, match='a GoldakSource object cannot be combined'):
            hip.StagedStepper(grid, mm.mat, prm, mm.packs, 20.0, material_map=mm, source=bare)
        with pytest.raises(TypeError, match='a scan path enters the step as its field'):
            hip.adi_step_numba_coeff(np.array(T0), grid, mm.mat, prm, mm.packs, 20.0, material_map=mm, S=bare)
        with pytest.raises(TypeError, match='a scan path enters the step as its field'):
            hip.adi_step_numba_coeff(np.array(T0), grid, mm.mat, prm, plain_packs, 20.0, S=bare)
    with pytest.raises(ValueError, match='needs material_map='):
        hip.adi_step_numba_coeff(np.array(T0), grid, mm.mat, prm, plain_packs, 20.0, S=msrc)
    other = hip.MaterialMap(grid, pc.MATERIALS8, ids, robin_h=350.0)
    with pytest.raises(ValueError, match='belongs to another MaterialMap'):
        hip.adi_step_numba_coeff(np.array(T0), grid, mm.mat, prm, mm.packs, 20.0, material_map=mm, S=hip.MapPathSource(other, path))
    with pytest.raises(TypeError, match='src must be a GoldakSource, got object'):
        hip.MapSource(mm, object())
