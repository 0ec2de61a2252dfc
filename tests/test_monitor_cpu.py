"""CPU: the FieldMonitor without a device -- its definition (FieldMonitor.record_reference) against math.fsum and the plain
NumPy statements, the census of tests/monitor_cases.py (every case holds what it is there for), and the argument rules of the
C ABI and of the Python side that are checked before anything is launched.

The bound on a sum: the definition adds along a tree whose longest path from a cell to the result holds d rounding operations
(FieldMonitor.rounding_depth: 17 in the brick, ceil(bricks / 256) + 9 in the region), so |sum - exact| <= d eps sum|terms| to
first order; eps = 2^-52 is twice the unit roundoff, which covers the higher orders.  d + 1 for sum_wT: its product rounds
first."""
import ctypes
import math
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import monitor_cases as mc  # noqa: E402


@pytest.fixture(scope='module')
def FM():
    from adi_thermal_fields_amd.monitor import FieldMonitor
    return FieldMonitor


_refs = {}


def _ref(FM, n):
    if n not in _refs:
        c = mc.case(n)
        _refs[n] = (c, mc.reference(FM, c, c['T0']))
    return _refs[n]


def _within(got, terms, d):
    exact = math.fsum(terms)
    bound = d * mc.EPS * math.fsum(abs(t) for t in terms)
    print('sum %r fsum %r |diff| %.3e bound %.3e' % (got, exact, abs(got - exact), bound))
    assert abs(got - exact) <= bound, (got, exact, bound)


# ---- the definition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', mc.CASES)
def test_sums_against_fsum(FM, n):
    c, ref = _ref(FM, n)
    T, m = c['T0'], c['mask']
    w = None
    if 'ids' in c:
        w = np.array(FM.weights_of([mc._Mat(*x) for x in mc.MATERIALS], mc.DX))
    for r, box in enumerate(mc.boxes(c)):
        sl = tuple(slice(lo, hi) for lo, hi in box)
        sel = m[sl]
        d = FM.rounding_depth(box)
        assert d == 17 + -(-FM.brick_count(box) // 256) + 9
        _within(float(ref['sum_T'][r]), T[sl][sel].tolist(), d)
        if w is not None:
            _within(float(ref['sum_wT'][r]), (w[c['ids'][sl][sel]] * T[sl][sel]).tolist(), d + 1)
            _within(float(ref['sum_extra'][r]), c['extra'][sl][sel].tolist(), d)
        else:
            assert ref['sum_wT'][r] == 0.0 and ref['sum_extra'][r] == 0.0


@pytest.mark.parametrize('n', mc.CASES)
def test_counts_extrema_and_probes_are_the_numpy_statements(FM, n):
    c, ref = _ref(FM, n)
    T, m = c['T0'], c['mask']
    for r, box in enumerate(mc.boxes(c)):
        sl = tuple(slice(lo, hi) for lo, hi in box)
        vals = T[sl][m[sl]]
        assert ref['cells'][r] == vals.size == int(m[sl].sum())
        if vals.size:
            assert ref['T_min'][r] == vals.min() and ref['T_max'][r] == vals.max()
        else:
            assert np.isnan(ref['T_min'][r]) and np.isnan(ref['T_max'][r])
    for q, p in enumerate(c['probes']):
        if m[p]:
            assert ref['probes'][q] == T[p]
        else:
            assert np.isnan(ref['probes'][q])
    assert ref['cells'].dtype == np.int64


def test_the_signed_zero_rule_and_the_directed_values(FM):
    d = mc.directed()
    ref = FM.record_reference(d['T'], d['mask'], d['probes'], d['regions'])
    for r, (lo, hi) in enumerate(d['want']):
        assert mc.bits(ref['T_min'][r]) == mc.bits(lo), (r, ref['T_min'][r], lo)
        assert mc.bits(ref['T_max'][r]) == mc.bits(hi), (r, ref['T_max'][r], hi)
    assert ref['cells'][-1] == 1 and ref['sum_T'][-1] == 123.25
    assert mc.bits(ref['probes'][0]) == mc.bits(123.25) and mc.bits(ref['probes'][1]) == mc.bits(-0.0)
    assert np.isnan(ref['probes'][2])
    # regions of zeros alone: the sum of +0.0 and -0.0 terms in the defined order is +0.0 unless every term of a pair chain is -0.0
    assert ref['sum_T'][0] == 0.0 and ref['sum_T'][3] == 0.0 and not np.signbit(ref['sum_T'][3])


def test_the_order_is_the_bricks_and_the_box_alone(FM):
    """the same cells in a region that is given alone or next to others, in a field shifted by whole bricks: the same bits; and
    a sum whose order matters (terms over 16 decades) differs from a plainly ordered one, so the comparison can fail"""
    rng = np.random.default_rng(11)
    shape = (40, 40, 40)
    V = rng.standard_normal(shape) * 10.0 ** rng.integers(-8, 8, shape)
    box = ((3, 37), (5, 33), (7, 39))
    a = FM.ordered_sum(V, box)
    W = np.zeros((56, 40, 40))
    W[16:] = V
    b = FM.ordered_sum(W, ((19, 53),) + box[1:])
    assert mc.bits(a) == mc.bits(b)
    sl = tuple(slice(lo, hi) for lo, hi in box)
    assert any(mc.bits(a) != mc.bits(s) for s in (float(np.cumsum(V[sl].ravel())[-1]), float(V[sl].sum())))


def test_row_of_lays_the_words_out_as_the_header_says(FM):
    c, ref = _ref(FM, 1)
    row = FM.row_of(ref)
    npr, nreg = len(c['probes']), len(c['regions'])
    assert row.dtype == np.int64 and row.size == npr + 6 * nreg
    assert np.array_equal(row[:npr], mc.bits(ref['probes']))
    for r in range(nreg):
        w = row[npr + 6 * r:npr + 6 * r + 6]
        assert w[0] == ref['cells'][r]
        assert np.array_equal(w[1:], mc.bits([ref[k][r] for k in ('T_min', 'T_max', 'sum_T', 'sum_wT', 'sum_extra')]))


# ---- the census ---------------------------------------------------------------------------------------------------------------
def _brick_kinds(c, phys, box):
    """(all-solid bricks, flag-reading bricks with in-mask cells) among the bricks the region meets"""
    solid = mc.solid_bricks(c, phys)[mc.region_bricks(box)]
    return int(solid.sum()), int((~solid).sum())


def test_census_case_1():
    c = mc.case(1)
    assert not mc.vec_form(c)                                       # odd rows: the cell-by-cell loads
    assert mc.vec_form(c, mc.PADDED[1])                             # ... and the padded variant the 16-byte ones
    assert 0.5 < c['mask'].mean() < 0.7
    whole, cut, one, empty = mc.boxes(c)
    assert cut[2][0] % 2 == 1 and cut[2][1] % 2 == 1                # a pair split by the region's edge at both ends
    assert all(lo % 16 and hi % 16 for lo, hi in cut)               # bricks cut on every axis
    m = c['mask']
    assert m[cut[0][0]:cut[0][1], cut[1][0]:cut[1][1], cut[2][0] - 1].any()     # the split pairs hold in-mask cells outside
    assert m[cut[0][0]:cut[0][1], cut[1][0]:cut[1][1], cut[2][1]].any()
    assert all(lo // 16 == (hi - 1) // 16 for lo, hi in one)        # inside one brick
    assert not m[tuple(slice(lo, hi) for lo, hi in empty)].any()    # no in-mask cell
    assert m[tuple(slice(lo, hi) for lo, hi in one)].any()
    p_in, p_off, p_last, _ = c['probes']
    assert m[p_in] and not m[p_off] and m[p_last] and p_last[2] == c['shape'][2] - 1 and c['shape'][2] % 2 == 1


def test_census_case_2():
    c = mc.case(2)
    for phys in (None, mc.PADDED[2]):
        assert mc.vec_form(c, phys)
        for box in mc.boxes(c):
            n_solid, n_flags = _brick_kinds(c, phys, box)
            assert n_solid >= 1 and n_flags >= 1, (phys, box)       # all-solid bricks next to flag-reading ones
    a, b = mc.boxes(c)
    assert all(max(x[0], y[0]) < min(x[1], y[1]) for x, y in zip(a, b))          # the regions overlap
    assert c['T0'][~c['mask']].min() > c['T0'][c['mask']].max()     # off-mask values above every in-mask value


def test_census_case_3():
    c = mc.case(3)
    phys = mc.phys_of(c)
    assert (phys[0] + 15) // 16 > 32                                # a second summary word per brick row
    solid = mc.solid_bricks(c)
    assert solid[32:].any() and not solid[32:].all()                # ... with set and unset bits in it
    _, box = mc.boxes(c)
    assert box[0][0] < 512 < box[0][1]                              # a region across the word boundary
    assert phys != c['shape']                                       # a padded layout of the library's own choice


def test_census_case_4():
    c = mc.case(4)
    m = c['mask']
    assert set(np.unique(c['ids'][m])) == {0, 1} and len(mc.MATERIALS) == 2
    assert 0.0 <= c['extra'][m].min() and c['extra'][m].max() <= 1.0


# ---- the argument rules of the C ABI --------------------------------------------------------------------------------------------
def test_argument_errors_without_gpu():
    """every rule is checked before any HIP call"""
    from adi_thermal_fields_amd import _lib
    lib, P = _lib.lib, ctypes.c_void_p
    assert _lib.MONITOR_MAX_REGIONS == 8 and _lib.MONITOR_MAX_PROBES == 256 and _lib.MONITOR_REGION_WORDS == 6
    reg = (ctypes.c_int * 6)(0, 20, 0, 20, 0, 40)
    prb = (ctypes.c_int * 3)(1, 2, 3)
    w = (ctypes.c_double * 2)(1.0, 2.0)
    #      0      1      2     3     4      5     6   7   8   9  10  11   12  13   14   15 16    17     18    19    20  21
    ok = [P(8), P(16), None, None, P(24), None, 20, 20, 40, 0, 1, reg, 1, prb, P(32), 0, None, P(40), 1000, P(48), 16, None]

    def rec(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.adi_monitor_record(*a)
    for i in (0, 1, 4, 17, 19, 11, 13, 14):
        with pytest.raises(ValueError, match='null argument'):
            _lib.check(rec(**{'a%d' % i: None}))
    with pytest.raises(ValueError, match='aliases T'):
        _lib.check(rec(a19=P(16)))
    with pytest.raises(ValueError, match='aliases T'):
        _lib.check(rec(a17=P(16)))
    with pytest.raises(ValueError, match='aliases the extra field'):
        _lib.check(rec(a2=P(48)))
    with pytest.raises(ValueError, match='log aliases the partial'):
        _lib.check(rec(a19=P(40)))
    for nreg in (0, 9, -1):
        with pytest.raises(ValueError, match='regions'):
            _lib.check(rec(a10=nreg))
    for npr in (257, -1):
        with pytest.raises(ValueError, match='probes'):
            _lib.check(rec(a12=npr))
    for bad, what in (((5, 5, 0, 20, 0, 40), 'empty'), ((0, 20, 7, 3, 0, 40), 'empty'), ((0, 21, 0, 20, 0, 40), 'leaves the box'),
                      ((0, 20, 0, 20, -1, 40), 'leaves the box'), ((0, 20, 0, 20, 0, 41), 'leaves the box')):
        with pytest.raises(ValueError, match=what):
            _lib.check(rec(a11=(ctypes.c_int * 6)(*bad)))
    for bad in ((20, 0, 0), (0, -1, 0), (0, 0, 40)):
        with pytest.raises(ValueError, match='outside the box'):
            _lib.check(rec(a13=(ctypes.c_int * 3)(*bad)))
    for cap in (0, -5):
        with pytest.raises(ValueError, match='capacity'):
            _lib.check(rec(a20=cap))
    with pytest.raises(ValueError, match='words of partials'):      # 2 x 2 x 3 bricks x 6 words = 72
        _lib.check(rec(a18=71))
    with pytest.raises(ValueError, match='bad grid'):
        _lib.check(rec(a6=0))
    with pytest.raises(ValueError, match='too large'):
        _lib.check(rec(a8=16 * 65535 + 1, a6=1, a7=1, a11=(ctypes.c_int * 6)(0, 1, 0, 1, 0, 1), a12=0))
    with pytest.raises(ValueError, match='ids without weights'):
        _lib.check(rec(a3=P(56)))
    for nmat in (0, 9):
        with pytest.raises(ValueError, match='materials'):
            _lib.check(rec(a3=P(56), a15=nmat, a16=w))
    with pytest.raises(ValueError, match='not finite'):
        _lib.check(rec(a3=P(56), a15=2, a16=(ctypes.c_double * 2)(1.0, float('inf'))))
    # the log
    with pytest.raises(ValueError, match='null argument'):
        _lib.check(lib.adi_monitor_reset_log(None, P(8), 4, 7, None))
    with pytest.raises(ValueError, match='null argument'):
        _lib.check(lib.adi_monitor_reset_log(P(8), None, 4, 7, None))
    with pytest.raises(ValueError, match='capacity'):
        _lib.check(lib.adi_monitor_reset_log(P(8), P(16), 0, 7, None))
    for rw in (5, 256 + 48 + 1):
        with pytest.raises(ValueError, match='a row of'):
            _lib.check(lib.adi_monitor_reset_log(P(8), P(16), 4, rw, None))


# ---- the argument rules of the Python side --------------------------------------------------------------------------------------
def test_python_argument_errors_without_gpu(FM):
    shape = (20, 20, 40)
    grid = types.SimpleNamespace(shape=shape, dx=1e-3)
    with pytest.raises(ValueError, match='outside the grid'):
        FM(grid, probes=[(20, 0, 0)])
    with pytest.raises(ValueError, match='outside the grid'):
        FM(grid, probes=[(0, 0, -1)])
    with pytest.raises(ValueError, match='a probe is a cell'):
        FM(grid, probes=[(0, 0)])
    with pytest.raises(ValueError, match='at most 256'):
        FM(grid, probes=[(0, 0, 0)] * 257)
    with pytest.raises(ValueError, match='is empty'):
        FM(grid, regions=[((3, 3), (0, 20), (0, 40))])
    with pytest.raises(ValueError, match='leaves the grid'):
        FM(grid, regions=[((0, 21), (0, 20), (0, 40))])
    with pytest.raises(ValueError, match='a region is'):
        FM(grid, regions=[((0, 20), (0, 20))])
    with pytest.raises(ValueError, match='1 to 8'):
        FM(grid, regions=[None] * 9)
    with pytest.raises(ValueError, match='capacity'):
        FM(grid, capacity=0)
    with pytest.raises(TypeError, match='must be a MaterialMap'):
        FM(grid, material_map=object())
    assert FM.checked_regions(shape, ()) == (((0, 20), (0, 20), (0, 40)),) == FM.checked_regions(shape, [None])
    # metres -> cells
    assert FM.cells_of(grid, [(0.0, 0.0199, 0.0395)]) == ((0, 19, 39),)
    assert FM.cells_of(grid, [(0.0105, 0.0115, 0.0125)], origin=(0.01, 0.01, 0.01)) == ((0, 1, 2),)
    for pt in ((-1e-9, 0.0, 0.0), (0.02, 0.0, 0.0), (0.0, 0.0, 0.04)):
        with pytest.raises(ValueError, match='outside the grid'):
            FM.cells_of(grid, [pt])


def test_check_extras_refuses_a_foreign_monitor(FM):
    from adi_thermal_fields_amd import step
    g1, g2 = object(), object()
    mon = FM.__new__(FM)
    mon.grid, mon.material_map = g1, None
    prm = types.SimpleNamespace(dt=0.1, theta=0.5)
    args = (None, prm, ())
    step._check_extras(g1, *args, step.StepExtras(monitor=mon))
    with pytest.raises(ValueError, match='belongs to another grid'):
        step._check_extras(g2, *args, step.StepExtras(monitor=mon))
    with pytest.raises(TypeError, match='must be a FieldMonitor'):
        step._check_extras(g1, *args, step.StepExtras(monitor=object()))
    mon.material_map = object()
    with pytest.raises(ValueError, match="material_map is not the step's"):
        step._check_extras(g1, *args, step.StepExtras(monitor=mon))


def test_the_waam_loops_refuse_a_monitor_on_other_backends():
    """the ValueError they raise for history="""
    from adi_thermal_fields_amd import waam
    from oracle import adi_oracle as orc
    plate = np.zeros((8, 8, 8), dtype=bool)
    plate[:, :, :3] = True
    with pytest.raises(ValueError, match='monitor needs the device loop'):
        waam.run_single_track(orc, plate, (2, 6, 3, 5, 2), 1e-3, (mc.RHO, mc.CP, mc.K), mc.H, 25.0, 1500.0, 0.5, 0.01, 0.02,
                              monitor=dict(probes=[(3, 0, 3)]))
