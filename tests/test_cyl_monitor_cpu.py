"""CPU: the cylindrical field monitor without a GPU -- the host twin adi_cyl_monitor_record_host against the NumPy definition
CylFieldMonitor.record_reference bit for bit on every case of cyl_monitor_cases.py, the definition's rounding bound against
math.fsum, what a cyclic roll along phi leaves unchanged, the argument rules, cells_of, the identities of region_log, the guard
words and the spill row."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import cyl_monitor_cases as mc  # noqa: E402
from adi_thermal_fields_amd import _lib  # noqa: E402
from adi_thermal_fields_amd.cyl_monitor import CylFieldMonitor  # noqa: E402
from adi_thermal_fields_amd.cyl_extras import CylThermalHistory  # noqa: E402

CASES = mc.case_ids()


class _Grid:
    """what the host-side methods of CylFieldMonitor read of a GridCyl"""

    def __init__(self, shape, r_in, dr=mc.DR, dz=1.2e-3):
        self.nr, self.nphi, self.nz = shape
        self.shape = tuple(shape)
        self.R_in, self.dr, self.dphi, self.dz = r_in, dr, 2.0 * math.pi / shape[1], dz
        self.r = r_in + (np.arange(shape[0], dtype=np.float64) + 0.5) * dr


@pytest.mark.parametrize('c', CASES, ids=mc.case_name)
def test_host_twin_is_the_definition_bit_for_bit(c):
    shape, mode, r_in = c
    case, refs = mc.reference(shape, mode, r_in)
    store, rows, blk = mc.host_rows(case, r_in)
    want = mc.reference_rows(refs)
    assert mc.same_rows(rows[:mc.NREC], want)
    npr = len(case['probes'])
    assert np.array_equal(rows[:mc.NREC, npr::mc.REGION_WORDS], want[:, npr::mc.REGION_WORDS])          # cells, to the integer
    assert np.array_equal(rows[:mc.NREC, npr + 1::mc.REGION_WORDS], want[:, npr + 1::mc.REGION_WORDS])  # sum_i
    assert np.isnan(rows[mc.NREC].view(np.float64)).all()                                               # the spill row: untouched
    assert (store[:mc.GUARD] == mc.GUARD_WORD).all() and (store[-mc.GUARD:] == mc.GUARD_WORD).all()
    assert blk[3] == mc.NREC
    # what the cases promise: an inactive probe and a region without an active cell log NaN, zeros of both signs are extrema
    if mode != 'all':
        for ref in refs:
            assert np.isnan(ref['probes'][-1]) and ref['cells'][-1] == 0
            assert np.isnan(ref['T_min'][-1]) and np.isnan(ref['T_max'][-1]) and ref['sum_T'][-1] == 0.0
    else:
        assert np.signbit(refs[0]['T_min'][1]) and np.signbit(refs[0]['T_max'][1]) and refs[0]['T_max'][1] == 0.0
        assert not np.signbit(refs[1]['T_min'][1]) and refs[1]['T_min'][1] == 0.0
    assert np.isfinite(np.concatenate([r[k] for r in refs for k in ('sum_T', 'sum_rT', 'sum_extra', 'sum_rextra')])).all()


@pytest.mark.parametrize('c', CASES[::3] + CASES[1::3], ids=mc.case_name)
def test_without_extra_the_extra_sums_are_plus_zero(c):
    shape, mode, r_in = c
    case, refs = mc.reference(shape, mode, r_in, False)
    _, rows, _ = mc.host_rows(case, r_in, with_extra=False)
    assert mc.same_rows(rows[:mc.NREC], mc.reference_rows(refs))
    _, with_x = mc.reference(shape, mode, r_in)
    for a, b in zip(refs, with_x):
        for k in ('sum_extra', 'sum_rextra'):
            assert (a[k] == 0.0).all() and not np.signbit(a[k]).any()
        for k in ('cells', 'sum_i', 'T_min', 'T_max', 'sum_T', 'sum_rT', 'probes'):
            assert mc.same_rows(a[k].view(np.int64), b[k].view(np.int64))


@pytest.mark.parametrize('c', CASES, ids=mc.case_name)
def test_rounding_bound_against_fsum(c):
    """|sum - exact| <= d eps sum|terms| with d = rounding_depth (d + 1 for the r-weighted sums, whose exact value is the sum
    over the radii of r_i times the correctly rounded plane sum, in rational arithmetic)"""
    shape, mode, r_in = c
    case, refs = mc.reference(shape, mode, r_in)
    regions = CylFieldMonitor.checked_regions(shape, case['regions'])
    r = _Grid(shape, r_in).r
    worst = 0.0
    for n in (0, mc.NREC - 1):
        act = case['acts'][n]
        X = np.nan_to_num(case['extras'][n], nan=0.0)
        for q, box in enumerate(regions):
            d = CylFieldMonitor.rounding_depth(shape, box)
            for F, name, rname in ((case['fields'][n], 'sum_T', 'sum_rT'), (X, 'sum_extra', 'sum_rextra')):
                terms = mc.region_terms(F, act, shape, box)
                mag = math.fsum(np.abs(terms))
                err = abs(refs[n][name][q] - math.fsum(terms))
                assert err <= d * mc.EPS * mag, (n, q, name)
                exact, rmag = Fraction(0), 0.0
                for i in range(box[0][0], box[0][1]):
                    one = (box[0], box[1], box[2])
                    ti = mc.region_terms(F, act, shape, ((i, i + 1), one[1], one[2]))
                    exact += Fraction(float(r[i])) * Fraction(math.fsum(ti))
                    rmag += float(r[i]) * math.fsum(np.abs(ti))
                rerr = abs(Fraction(float(refs[n][rname][q])) - exact)
                assert rerr <= (d + 1) * mc.EPS * rmag, (n, q, rname)
                if mag > 0.0:
                    worst = max(worst, err / (mc.EPS * mag))
    print('worst error: %.3f eps sum|terms|' % worst)


def test_rounding_depth_and_chunks():
    assert [CylFieldMonitor.chunks(s)[1] for s in mc.SHAPES] == [1, 1, 2, 3, 7, 257]
    assert CylFieldMonitor.rounding_depth((2, 2, 65540), ((0, 2), (0, 2), (0, 65540))) == 19 + 2 + 2
    assert CylFieldMonitor.rounding_depth((5, 8, 129), ((1, 4), (6, 10), (0, 3))) == 19 + 1 + 3


@pytest.mark.parametrize('shape', [(3, 5, 7), (5, 8, 129), (1, 4, 130)])
def test_a_roll_along_phi(shape):
    """A wrapped region after a cyclic roll of the field along phi holds the same cells at other pair positions, so the
    definition implies: the integer words and the extrema are equal on every field (they depend on no order); the sums are
    equal to the bit on a field of small integers, where every addition of the definition is exact, R_in = 0 and dr = 1
    included for the r-weighted ones; on a general field they agree only within the two rounding bounds, which is asserted as
    that and no more."""
    nr, nphi, nz = shape
    rng = np.random.default_rng(11)
    act = rng.random(shape) < 0.7
    box = ((0, nr), (nphi - 2, nphi + 2), (1, nz))
    for shift in (1, 2, nphi - 1):
        rolled = ((0, nr), ((nphi - 2 + shift) % nphi, (nphi - 2 + shift) % nphi + 4), (1, nz))
        for exact in (True, False):
            T = rng.integers(-40, 41, shape).astype(np.float64) if exact else rng.uniform(-500.0, 1700.0, shape)
            grid = (0.0, 1.0) if exact else (0.03, mc.DR)
            a = CylFieldMonitor.record_reference(T, act, (), [box], grid, extra=T)
            b = CylFieldMonitor.record_reference(np.roll(T, shift, axis=1), np.roll(act, shift, axis=1), (), [rolled], grid,
                                                 extra=np.roll(T, shift, axis=1))
            for k in ('cells', 'sum_i', 'T_min', 'T_max'):
                assert mc.same_rows(a[k].view(np.int64), b[k].view(np.int64)), (shift, k)
            d = CylFieldMonitor.rounding_depth(shape, box)
            r = grid[0] + (np.arange(nr) + 0.5) * grid[1]
            for k, w, dd in (('sum_T', None, d), ('sum_rT', r, d + 1), ('sum_extra', None, d), ('sum_rextra', r, d + 1)):
                if exact:
                    assert mc.same_rows(a[k].view(np.int64), b[k].view(np.int64)), (shift, k)
                else:
                    mag = math.fsum(np.abs(mc.region_terms(T, act, shape, box, w)))
                    assert abs(a[k][0] - b[k][0]) <= 2 * dd * mc.EPS * mag, (shift, k)


def test_checked_regions_and_probes():
    shape = (4, 12, 9)
    whole = ((0, 4), (0, 12), (0, 9))
    assert CylFieldMonitor.checked_regions(shape, None) == (whole,)
    assert CylFieldMonitor.checked_regions(shape, ()) == (whole,)
    assert CylFieldMonitor.checked_regions(shape, [None, ((1, 2), (10, 14), (0, 9))]) == (whole, ((1, 2), (10, 14), (0, 9)))
    inc = CylFieldMonitor.region_cells(shape, ((1, 2), (10, 14), (0, 9)))
    assert sorted(set(np.argwhere(inc)[:, 1])) == [0, 1, 10, 11] and inc.sum() == 4 * 9
    assert CylFieldMonitor.checked_regions(shape, [((0, 4), (11, 23), (0, 9))])            # j1 = j0 + nphi
    for bad in ([((0, 4), (12, 13), (0, 9))], [((0, 4), (-1, 3), (0, 9))], [((0, 4), (3, 16), (0, 9))], [((0, 4), (3, 3), (0, 9))],
                [((2, 2), (0, 1), (0, 1))], [((0, 5), (0, 1), (0, 1))], [((0, 4), (0, 1), (-1, 1))], [((0, 4), (0, 1), (0, 10))],
                [((0, 4), (0, 1))], [((0, 4), (0, 1.5), (0, 1))], [None] * 9):
        with pytest.raises(ValueError):
            CylFieldMonitor.checked_regions(shape, bad)
    assert CylFieldMonitor.checked_probes(shape, [(3, 11, 8)]) == ((3, 11, 8),)
    for bad in ([(4, 0, 0)], [(0, 12, 0)], [(0, 0, -1)], [(0, 0)], [(0.5, 0, 0)], [(0, 0, 0)] * 257):
        with pytest.raises(ValueError):
            CylFieldMonitor.checked_probes(shape, bad)
    assert len(CylFieldMonitor.checked_probes(shape, [(0, 0, 0)] * 256)) == 256


def test_cells_of():
    g = _Grid((4, 12, 9), 0.03, dr=2.0e-3, dz=1.0e-3)
    dphi = g.dphi
    pts = [(0.03, 0.0, 0.0), (0.0379, 0.5 * dphi, 0.0089), (0.031, -0.5 * dphi, 0.001), (0.031, 2.0 * math.pi + 1.5 * dphi, 0.0),
           (0.031, -2.0 * math.pi - 0.5 * dphi, 0.0)]
    assert CylFieldMonitor.cells_of(g, pts) == ((0, 0, 0), (3, 0, 8), (0, 11, 1), (0, 1, 0), (0, 11, 0))
    for bad in ((0.0299, 0.0, 0.0), (0.0381, 0.0, 0.0), (0.031, 0.0, -1e-6), (0.031, 0.0, 0.0091)):
        with pytest.raises(ValueError):
            CylFieldMonitor.cells_of(g, [bad])


def _call(blk, T, rows, capacity, regions, probes=(), extra=None, act=None, r_in=0.0, dr=1.0, shape=None, stride=0):
    mc.host_record(blk, T, extra, act, r_in, dr, regions, probes, rows, capacity, plane_stride=stride, shape=shape)


def test_argument_errors_of_the_c_abi():
    shape = (3, 5, 7)
    T = np.zeros(shape)
    whole = CylFieldMonitor.checked_regions(shape, None)
    store, rows = mc.host_log(2, mc.REGION_WORDS)
    blk = mc.host_block(0.0, 0.1, 2)
    before = store.copy()
    bad_regions = [[((0, 3), (5, 6), (0, 7))], [((0, 3), (2, 8), (0, 7))], [((0, 3), (1, 1), (0, 7))], [((0, 4), (0, 5), (0, 7))],
                   [((0, 3), (0, 5), (0, 8))], [((-1, 3), (0, 5), (0, 7))], list(whole) * 9, []]
    for reg in bad_regions:
        with pytest.raises(ValueError):
            _call(blk, T, rows, 2, reg)
    for kw in (dict(probes=[(3, 0, 0)]), dict(probes=[(0, 0, 7)]), dict(probes=[(0, -1, 0)]), dict(dr=0.0), dict(r_in=-1.0),
               dict(r_in=float('nan')), dict(shape=(3, 5, 0)), dict(shape=(65536, 1, 1)), dict(stride=34), dict(extra=rows)):
        with pytest.raises(ValueError):
            _call(blk, T, rows, 2, whole, **kw)
    with pytest.raises(ValueError):
        _call(blk, T, rows, 0, whole)
    with pytest.raises(ValueError):
        _call(blk, T, T, 2, whole)                                    # the log aliases T
    for args in ((None, T, rows), (blk, None, rows), (blk, T, None)):
        with pytest.raises(ValueError):
            _call(args[0], args[1], args[2], 2, whole, shape=shape)
    assert np.array_equal(store, before) and blk[3] == 0              # refused before anything is touched
    assert _lib.lib.adi_cyl_monitor_reset_log(None, None, 2, 8, None) == _lib.ADI_ERR_ARG
    assert _lib.lib.adi_cyl_monitor_record(None, None, None, None, 3, 5, 7, 0, 0.0, 1.0, 1, None, 0, None, None, None, 0, None,
                                           2, None) == _lib.ADI_ERR_ARG
    assert _lib.lib.adi_abi_version() == 18


def test_padded_plane_stride_on_the_host():
    """a plane stride above nphi*nz (odd, so never the pair form): the same bits as the dense array"""
    shape, r_in = (5, 8, 129), 0.03
    case, refs = mc.reference(shape, 'random', r_in)
    regions = CylFieldMonitor.checked_regions(shape, case['regions'])
    sx = shape[1] * shape[2] + 3
    n_el = (shape[0] - 1) * sx + shape[1] * shape[2]                  # what the header promises is touched, and no more
    def padded(a, dtype, fill):
        flat = np.full(n_el, fill, dtype=dtype)
        np.lib.stride_tricks.as_strided(flat, shape, (sx * flat.itemsize, shape[2] * flat.itemsize, flat.itemsize))[:] = a
        return flat
    store, rows = mc.host_log(1, len(case['probes']) + mc.REGION_WORDS * len(regions))
    blk = mc.host_block(0.0, 0.1, 1)
    mc.host_record(blk, padded(case['fields'][0], np.float64, mc.SENTINEL_T), padded(case['extras'][0], np.float64, 0.5),
                   padded(case['acts'][0], np.bool_, True), r_in, mc.DR, regions, case['probes'], rows, 1, plane_stride=sx,
                   shape=shape)
    assert mc.same_rows(rows[0], CylFieldMonitor.row_of(refs[0]))


def test_capacity_2_spill_row_on_the_host():
    """past the capacity every record lands in the spill row, which so holds the last one; the block's slot counts them all"""
    shape, r_in = (3, 5, 7), 0.0
    case, refs = mc.reference(shape, 'births', r_in)
    store, rows, blk = mc.host_rows(case, r_in, capacity=2)
    want = mc.reference_rows(refs)
    assert mc.same_rows(rows[:2], want[:2]) and mc.same_rows(rows[2], want[2])
    regions = CylFieldMonitor.checked_regions(shape, case['regions'])
    mc.host_record(blk, np.ascontiguousarray(case['fields'][0]), np.ascontiguousarray(case['extras'][0]), case['acts'][0], r_in,
                   mc.DR, regions, case['probes'], rows, 2)
    assert mc.same_rows(rows[2], want[0]) and mc.same_rows(rows[:2], want[:2])
    assert blk[3] == 4 and max(0, int(blk[3]) - 2) == 2                                    # dropped, as rows() counts them
    assert (store[:mc.GUARD] == mc.GUARD_WORD).all() and (store[-mc.GUARD:] == mc.GUARD_WORD).all()


class _HostMonitor(CylFieldMonitor):
    """region_log and traces over rows made on the host: the accessors' arithmetic without a device"""

    def __init__(self, grid, case, rows, times):
        self.grid = grid
        self.probes = CylFieldMonitor.checked_probes(grid.shape, case['probes'])
        self.regions = CylFieldMonitor.checked_regions(grid.shape, case['regions'])
        self._d_extra = object()
        self._rows, self._times = rows, list(times)

    def rows(self):
        return self._rows.copy(), 0


def test_region_log_identities():
    shape, r_in = (5, 8, 129), 0.03
    case, refs = mc.reference(shape, 'random', r_in)
    _, rows, _ = mc.host_rows(case, r_in)
    g = _Grid(shape, r_in)
    mon = _HostMonitor(g, case, rows[:mc.NREC], [mc.T0_CLOCK + (n + 1) * mc.DT for n in range(mc.NREC)])

    class Mat:
        rho, cp = 7800.0, 500.0
    log = mon.region_log(Mat)
    tr = mon.traces()
    nreg = len(mon.regions)
    assert log['cells'].shape == (nreg, mc.NREC) and tr['T'].shape == (len(mon.probes), mc.NREC) and log['dropped'] == 0
    assert mc.same_rows(log['volume'].view(np.int64), CylThermalHistory.pool_volume(g, log['cells'], log['sum_i']).view(np.int64))
    assert mc.same_rows(log['heat'].view(np.int64), ((Mat.rho * Mat.cp) * (g.dr * g.dphi * g.dz) * log['sum_rT']).view(np.int64))
    assert mc.same_rows(log['extra_volume'].view(np.int64), ((g.dr * g.dphi * g.dz) * log['sum_rextra']).view(np.int64))
    for n, ref in enumerate(refs):
        assert np.array_equal(log['cells'][:, n], ref['cells']) and np.array_equal(log['sum_i'][:, n], ref['sum_i'])
        assert mc.same_rows(tr['T'][:, n].view(np.int64), ref['probes'].view(np.int64))
        for k in ('T_min', 'T_max', 'sum_T', 'sum_rT', 'sum_extra', 'sum_rextra'):
            assert mc.same_rows(log[k][:, n].copy().view(np.int64), ref[k].view(np.int64))
        act = case['acts'][n]
        for q, box in enumerate(mon.regions):
            cells = CylFieldMonitor.region_cells(shape, box) & act
            vol = float(np.sum(np.broadcast_to(g.r[:, None, None], shape)[cells].astype(np.longdouble))
                        * np.longdouble(g.dr) * np.longdouble(g.dphi) * np.longdouble(g.dz))
            assert abs(log['volume'][q, n] - vol) <= 4 * mc.EPS * vol
            if ref['cells'][q]:
                assert log['T_mean'][q, n] == ref['sum_T'][q] / ref['cells'][q]
                assert ref['T_min'][q] <= log['T_vmean'][q, n] <= ref['T_max'][q]
            else:
                assert np.isnan(log['T_mean'][q, n]) and np.isnan(log['T_vmean'][q, n])
    assert 'heat' not in mon.region_log()
    assert list(log['t']) == [mc.T0_CLOCK + (n + 1) * mc.DT for n in range(mc.NREC)]


def test_exported_and_documented():
    import adi_thermal_fields_amd.adi3d_hip_cyl as hipcyl
    assert 'CylFieldMonitor' in hipcyl.__all__ and hipcyl.CylFieldMonitor is CylFieldMonitor
    assert CylFieldMonitor._keyword == 'monitor'
    for name in ('adi_cyl_monitor_record', 'adi_cyl_monitor_record_host', 'adi_cyl_monitor_reset_log'):
        assert name in _lib.SIGNATURES
