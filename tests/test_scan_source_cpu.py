"""CPU: the library's evaluator of a scan path, run on the host (adi_scan_sample_host: the code the kernels compile, no HIP call),
against the host definition ScanPath.sample_step; its argument checks; the frozen ScanPathSource."""
import ctypes

import numpy as np
import pytest

import scan_cases as sc
import scan_source_cases as ssc
from scan_cases import DT, DX, rel_linf


@pytest.fixture(scope='module')
def hip():
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    return hip


@pytest.fixture(scope='module')
def all_cases(hip):
    return {c[0]: c for c in ssc.cases(hip)}


def test_the_case_list_is_what_its_names_say(all_cases):
    """every case is there and sits on the branch its name says; the idle windows are the three of the existing test"""
    assert list(all_cases) == ssc.CASE_IDS
    d = lambda name: ssc.deltas(*[all_cases[name][i] for i in (1, 4, 5)])
    assert d('simpson_delta_5e-4') == pytest.approx([5e-4]) and all_cases['simpson_delta_5e-4'][6] == ssc.BAR
    assert d('erf_delta_2e-3') == pytest.approx([2e-3]) and all_cases['erf_delta_2e-3'][6] == ssc.BAR_SMALL_DELTA
    assert 0.0 in d('dwell_with_power') and len(d('dwell_with_power')) == 2
    assert min(d('corner')) >= 0.1 and len(d('corner')) == 2 and all_cases['corner'][6] == ssc.BAR
    assert [n for n, c in all_cases.items() if not c[7]] == ['window_before_t_start', 'window_after_t_end',
                                                              'window_inside_an_idle_dwell']
    for w, (name, when, segs) in zip(range(6), ssc.WINDOWS):
        assert all_cases['window_' + name][7] == (segs is not None)


@pytest.mark.parametrize('name', ssc.CASE_IDS)
def test_host_evaluator_vs_sample_step(all_cases, name):
    _, path, shape, mask, t, dt, bar, deposits = all_cases[name]
    g = sc.HostGrid(shape, DX, mask)
    want = path.sample_step(g, t, dt)
    got = path.on_device().sample_step_host(g, t, dt)
    if not deposits:
        assert not want.any()
        np.testing.assert_array_equal(got, 0.0)              # nothing deposits: a field of exact zeros
        return
    assert want.max() > 0
    err = rel_linf(got, want)
    print('%s: library evaluator on the host vs sample_step %.2e (bar %.0e)' % (name, err, bar))
    assert err <= bar
    np.testing.assert_array_equal(got[~g.mask], 0.0)
    np.testing.assert_array_equal(got[~ssc.support_boxes(path, shape, t, dt)], 0.0)
    if mask is not None:
        assert (want[g.mask] > 0).any() and not g.mask.all()


def _call(hip, shape, tab, K, t_end, dt=DT, table_ptr=True):
    from adi_thermal_fields_amd import _lib
    tab = np.ascontiguousarray(tab, dtype=np.float64)
    out = np.empty((4, 4, 4))
    return _lib.lib.adi_scan_sample_host(ctypes.byref(shape), tab.ctypes.data if table_ptr else None, K, t_end, None, 4, 4, 4,
                                         DX, 0.0, dt, out.ctypes.data)


def test_argument_errors_without_gpu(hip):
    """each is refused before any HIP call (this machine may have no GPU at all)"""
    from adi_thermal_fields_amd import _lib
    shape = _lib.ScanShape(0.8, 3e-4, 2.5e-4, 3e-4, 6e-4, 0.6, 2, 0)
    good = np.array([[0.0, 0, 0, 0, 1.0, 0.0, 0.1, 800.0], [1.0, 0.1, 0, 0, 0.0, 1.0, 0.1, 800.0]])
    assert _call(hip, shape, good, 2, 2.0) == _lib.ADI_OK
    bad = {}
    bad['null segment table'] = lambda: _call(hip, shape, good, 2, 2.0, table_ptr=False)
    bad['at least one segment'] = lambda: _call(hip, shape, good, 0, 2.0)
    desc = good.copy(); desc[1, 0] = -1.0
    bad['t_begin does not ascend'] = lambda: _call(hip, shape, desc, 2, 2.0)
    bad['t_end is not after'] = lambda: _call(hip, shape, good, 2, 1.0)
    nonunit = good.copy(); nonunit[0, 4:6] = (0.8, 0.7)
    bad['not a unit vector'] = lambda: _call(hip, shape, nonunit, 2, 2.0)
    neg = good.copy(); neg[1, 7] = -1.0
    bad['power < 0'] = lambda: _call(hip, shape, neg, 2, 2.0)
    slow = good.copy(); slow[0, 6] = -0.1
    bad['speed < 0'] = lambda: _call(hip, shape, slow, 2, 2.0)
    bad['dt must be > 0'] = lambda: _call(hip, shape, good, 2, 2.0, dt=0.0)
    nan = good.copy(); nan[0, 2] = np.nan
    bad['non-finite entry'] = lambda: _call(hip, shape, nan, 2, 2.0)
    for text, fn in bad.items():
        with pytest.raises(ValueError, match=text):
            _lib.check(fn())
    with pytest.raises(ValueError, match='dt must be > 0'):
        _lib.check(_call(hip, shape, good, 2, 2.0, dt=-DT))
    with pytest.raises(ValueError, match='non-positive length'):
        _lib.check(_call(hip, _lib.ScanShape(0.8, 0.0, 2.5e-4, 3e-4, 6e-4, 0.6, 2, 0), good, 2, 2.0))
    # the device entry point checks what it can see of a path before it launches anything
    p8 = ctypes.c_void_p(8)
    with pytest.raises(ValueError, match='at least one segment'):
        _lib.check(_lib.lib.adi_scan_sample(ctypes.byref(shape), p8, 0, 2.0, p8, 4, 4, 4, 0, DX, 0.0, DT, p8, None))
    with pytest.raises(ValueError, match='adi_scan_sample: null argument'):
        _lib.check(_lib.lib.adi_scan_sample(ctypes.byref(shape), None, 2, 2.0, p8, 4, 4, 4, 0, DX, 0.0, DT, p8, None))
    with pytest.raises(ValueError, match='bad dx / t / dt'):
        _lib.check(_lib.lib.adi_scan_sample(ctypes.byref(shape), p8, 2, 2.0, p8, 4, 4, 4, 0, DX, 0.0, 0.0, p8, None))


def test_a_snapshot_is_frozen(hip):
    path = sc.leg_path(hip, sc.SMALL, (4 * DX, 5 * DX, 5 * DX), 0.0, 6 * DX, 0.4)
    src = path.on_device()
    assert isinstance(src, hip.ScanPathSource) and src.K == 1
    g = sc.HostGrid((16, 12, 10), DX)
    t_end, tab, key = src.t_end, src.table().copy(), src.graph_key()
    before = src.sample_step(g, 0.0, 2 * path.t_end)
    path.line_to((4 * DX, 9 * DX, 5 * DX), 0.4).dwell(1e-3, power=100.0)
    path.power = 5.0
    assert path.n_segments == 3 and path.t_end > t_end
    assert src.K == 1 and src.t_end == t_end and src.graph_key() == key
    np.testing.assert_array_equal(src.table(), tab)
    np.testing.assert_array_equal(src.sample_step(g, 0.0, 2 * t_end), before)
    np.testing.assert_array_equal(src.sample_step_host(g, 0.0, 2 * t_end) != 0, before != 0)
    assert rel_linf(src.sample_step_host(g, 0.0, 2 * t_end), before) <= ssc.BAR
    assert rel_linf(path.sample_step(g, 0.0, 2 * t_end), before) > 1e-3       # the builder itself has moved on
    with pytest.raises(ValueError):
        src.table()[0, 7] = 1.0                                               # read-only
    assert hip.ScanPathSource(path).K == 3


def test_an_empty_path_is_refused(hip):
    with pytest.raises(ValueError, match='no segment'):
        hip.ScanPath(power=100.0, **sc.SMALL).on_device()
    with pytest.raises(TypeError):
        hip.ScanPathSource(hip.GoldakSource(100.0, 0.8, 1e-4, 1e-4, 1e-4, 1e-4))


def test_a_bad_table_is_refused_at_construction(hip):
    """the library's checks run when the snapshot is made: a direction that is no unit vector never reaches a launch"""
    path = sc.leg_path(hip, sc.SMALL, (4 * DX, 5 * DX, 5 * DX), 0.0, 6 * DX, 0.4)
    tb, p0, p1, d, vel, P = path._seg[0]
    path._seg[0] = (tb, p0, p1, (0.8, 0.7), vel, P)
    with pytest.raises(ValueError, match='not a unit vector'):
        path.on_device()
