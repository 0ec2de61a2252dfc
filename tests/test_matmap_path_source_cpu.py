"""CPU: a ScanPath inside the step of a MaterialMap without a source field (MapPathSource) -- the library's twin of
the kernel on the host (adi_matmap_scan_add_r0_host: the code the kernel compiles, no HIP call) against the NumPy statement
R0 + dt * path.sample_step(grid, t, dt) / C[ids]; the window's box and segment range; the cells that stay as they were; the
windows without a powered piece; every refusal, of the Python classes and of the C entries, before any HIP call.

How the increment is measured: the twin is run once on R0 = 0, where r + v is v exactly, so `inc` below IS (dt * q) / C[id] as
the library rounds it, held to the NumPy statement's at the bar of scan_source_cases (the rounding of erf and exp only).  On a
random R0 the result is then R0 + inc bit for bit -- the same addition -- which no subtraction of two large numbers blurs."""
import ctypes

import numpy as np
import pytest

import matmap_path_cases as pc
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


def _setup(case):
    """(path, src, grid, ids, R0) of a case of scan_source_cases: eight materials at random, 255 off the mask"""
    name, path, shape, mask, t, dt, bar, deposits = case
    g = sc.HostGrid(shape, DX, mask)
    ids, R0 = pc.ids_and_field(shape, g.mask, seed=len(name))
    return path, path.on_device(), g, ids, R0


@pytest.mark.parametrize('name', ssc.CASE_IDS)
def test_host_twin_vs_the_numpy_statement(all_cases, name):
    _, path, shape, mask, t, dt, bar, deposits = all_cases[name]
    path, src, g, ids, R0 = _setup(all_cases[name])
    q = path.sample_step(g, t, dt)
    inc, box = pc.host_twin(src, g, ids, np.zeros(shape), t, dt)
    got, box2 = pc.host_twin(src, g, ids, R0, t, dt)
    assert box == box2
    if not deposits:
        assert not q.any() and box == ((0, 0), (0, 0), (0, 0))
        assert np.array_equal(got, R0) and not inc.any()
        return
    want = np.where(g.mask, dt * q / pc.C8[np.where(g.mask, ids, 0)], 0.0)
    heated = ids[(q != 0) & g.mask]
    assert want.max() > 0 and (heated.size < 200 or len(np.unique(heated)) == 8)   # every material takes heat
    err = rel_linf(inc, want)
    print('%s: increment of the host twin vs the NumPy statement %.2e (bar %.0e)' % (name, err, bar))
    assert err <= bar
    # the same addition on a random field, bit for bit; a cell whose q_step is 0 keeps its R0, every cell outside the box too
    assert np.array_equal(got, R0 + inc)
    same = got.view(np.int64) == R0.view(np.int64)
    assert same[q == 0.0].all() and same[~g.mask].all()
    inside = np.zeros(shape, dtype=bool)
    inside[tuple(slice(lo, hi) for lo, hi in box)] = True
    assert same[~inside].all() and not same[inside].all()
    if mask is not None:
        assert (~g.mask & inside).any()                                        # off-mask cells inside the box


@pytest.mark.parametrize('name', ssc.CASE_IDS)
def test_window_is_the_union_of_the_index_boxes(hip, all_cases, name):
    _, path, shape, mask, t, dt, bar, deposits = all_cases[name]
    msrc = hip.MapPathSource(pc.bare_map(sc.HostGrid(shape, DX, mask)), path)
    k0, k1, box = msrc.window(t, dt)
    pieces = [(k, p) for k in range(path.n_segments) for p in [path._piece(k, t, t + dt)] if p is not None]
    assert bool(pieces) == deposits
    assert 0 <= k0 <= k1 <= path.n_segments and all(k0 <= k < k1 for k, _ in pieces)
    if not pieces:
        assert box == ((0, 0), (0, 0), (0, 0))
        return
    sl = [path._index_box(k, p, shape, DX) for k, p in pieces]
    assert box == tuple((min(s[a].start for s in sl), max(s[a].stop for s in sl)) for a in range(3))
    inside = ssc.support_boxes(path, shape, t, dt)
    idx = np.nonzero(inside)
    assert box == tuple((int(i.min()), int(i.max()) + 1) for i in idx)
    if len(pieces) == 1:                                    # one piece: the box, cell for cell
        mine = np.zeros(shape, dtype=bool)
        mine[tuple(slice(lo, hi) for lo, hi in box)] = True
        assert np.array_equal(mine, inside)


@pytest.mark.parametrize('when,t,dt', [('before t_start', 0.5 * DT, DT), ('after t_end', None, DT), ('inside the jump', 5.1 * DT, 0.3 * DT),
                                       ('inside the idle dwell', 9.0 * DT, DT)])
def test_a_window_without_a_powered_piece_leaves_r0_alone(hip, when, t, dt):
    from test_scan_path_gpu import _window_path
    shape = ssc.CORNER_SHAPE
    path = _window_path(hip, shape)
    t = path.t_end + 0.25 * DT if t is None else t
    assert not ssc.deltas(path, t, dt)
    if when == 'inside the jump':
        tab = path.table()
        assert tab[1, 7] == 0.0 and tab[1, 0] < t and t + dt < tab[2, 0]
    g = sc.HostGrid(shape, DX, ssc.case_mask(shape))
    ids, R0 = pc.ids_and_field(shape, g.mask, seed=3)
    got, box = pc.host_twin(path.on_device(), g, ids, R0, t, dt)
    assert box == ((0, 0), (0, 0), (0, 0))
    assert np.array_equal(got.view(np.int64), R0.view(np.int64))
    assert hip.MapPathSource(pc.bare_map(g), path).window(t, dt)[2] == box


def test_the_device_tests_windows_are_what_their_names_say(hip):
    """the cases of test_matmap_path_source_gpu.py, checked here where no launch depends on them; the host twin holds the bar on
    each of them too"""
    cases = pc.stage_cases(hip)
    assert [c[0] for c in cases] == pc.STAGE_IDS
    for name, path, shape, t, dt, want in cases:
        g = sc.HostGrid(shape, DX, ssc.case_mask(shape))
        pc.check_window(path, shape, t, dt, want, hip.MapPathSource(pc.bare_map(g), path).window(t, dt))
        ids, _ = pc.ids_and_field(shape, g.mask)
        inc, _ = pc.host_twin(path.on_device(), g, ids, np.zeros(shape), t, dt)
        want_inc = np.where(g.mask, dt * path.sample_step(g, t, dt) / pc.C8[np.where(g.mask, ids, 0)], 0.0)
        assert want_inc.max() > 0 and rel_linf(inc, want_inc) <= ssc.bar_of(path, t, dt), name


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _leg(hip):
    return sc.leg_path(hip, sc.SMALL, (4 * DX, 5 * DX, 5 * DX), 0.0, 6 * DX, 0.4)


def test_constructor_and_exports(hip):
    from adi_thermal_fields_amd.matmap_extras import MapPathSource, MapSource
    assert hip.MapPathSource is MapPathSource and 'MapPathSource' not in hip.__all__
    g = sc.HostGrid((16, 12, 10), DX)
    path = _leg(hip)
    with pytest.raises(TypeError, match='mm must be a MaterialMap'):
        MapPathSource(object(), path)
    for bad in (object(), hip.GoldakSource(100.0, 0.8, 1e-4, 1e-4, 1e-4, 1e-4), None):
        with pytest.raises(TypeError, match='src must be a ScanPath or a ScanPathSource'):
            MapPathSource(pc.bare_map(g), bad)
    with pytest.raises(TypeError, match='src must be a GoldakSource, got object'):      # (today's message)
        MapSource(pc.bare_map(g), object())
    with pytest.raises(TypeError, match='src must be a GoldakSource, got ScanPath'):
        MapSource(pc.bare_map(g), path)
    src = path.on_device()
    assert MapPathSource(pc.bare_map(g), src).src is src
    frozen = MapPathSource(pc.bare_map(g), path)            # a ScanPath is frozen for the caller
    assert isinstance(frozen.src, hip.ScanPathSource) and frozen.src.K == 1
    path.line_to((4 * DX, 9 * DX, 5 * DX), 0.4)
    assert frozen.src.K == 1 and not isinstance(frozen, (hip.GoldakSource, MapSource))


def test_step_refusals_come_before_any_launch(hip):
    """_check_extras runs before the first launch of adi_step_hip_coeff and in StagedStepper.__init__ (no device is here)"""
    from adi_thermal_fields_amd import step
    from adi_thermal_fields_amd.packs import Params
    g = sc.HostGrid((16, 12, 10), DX)
    path = _leg(hip)
    mm, other = pc.bare_map(g), pc.bare_map(g)
    msrc = hip.MapPathSource(mm, path)
    prm = Params(1e-3)
    check = lambda source, m=None, **kw: step._check_extras(g, mm.mat, prm, mm.packs, step.StepExtras(source=source, material_map=m), **kw)
    with pytest.raises(ValueError, match='needs material_map='):
        check(msrc)
    with pytest.raises(ValueError, match='belongs to another MaterialMap'):
        check(hip.MapPathSource(other, path), mm)
    with pytest.raises(TypeError, match='does not ride a captured graph.*adi_step_numba_coeff'):
        check(msrc, mm, stepper=True)
    with pytest.raises(TypeError, match='does not ride a captured graph'):
        check(msrc, None, stepper=True)
    # a bare path keeps today's messages, in both places
    for bare in (path, path.on_device()):
        with pytest.raises(TypeError, match='a scan path enters the step as its field'):
            hip.adi_step_numba_coeff(None, g, mm.mat, prm, mm.packs, S=bare)
        with pytest.raises(TypeError, match='a scan path enters the step as its field'):
            hip.adi_step_numba_coeff(None, g, mm.mat, prm, mm.packs, material_map=mm, S=bare)
        with pytest.raises(TypeError, match=r'source must be a GoldakSource \(pass a source field'):
            check(bare, None, stepper=True)


def test_c_entries_validate_before_any_hip_call(hip):
    from adi_thermal_fields_amd import _lib
    lib, chk = _lib.lib, _lib.check
    shape = _lib.ScanShape(0.8, 3e-4, 2.5e-4, 3e-4, 6e-4, 0.6, 2, 0)
    tab = np.array([[0.0, 0, 0, 0, 1.0, 0.0, 0.1, 800.0], [1.0, 0.1, 0, 0, 0.0, 1.0, 0.1, 800.0]])
    p8 = ctypes.c_void_p(64)                                # a non-null "device" pointer no check may follow
    R0, ids = np.zeros((4, 4, 4)), np.zeros((4, 4, 4), np.uint8)

    def dev(sh=ctypes.byref(shape), h_tab=tab.ctypes.data, d_tab=p8, K=2, R=p8, fl=p8, idp=p8, n=(4, 4, 4), dx=DX, t=0.0, dt=DT,
            nmat=2, C=(3.8e6, 3.4e6)):
        Cv = None if C is None else (ctypes.c_double * len(C))(*C)
        return lib.adi_matmap_scan_add_r0(sh, h_tab, d_tab, K, 2.0, R, fl, idp, *n, 0, dx, t, dt, nmat, Cv, None, None)

    def host(sh=ctypes.byref(shape), h_tab=tab.ctypes.data, K=2, R=R0.ctypes.data, idp=ids.ctypes.data, n=(4, 4, 4), dx=DX, t=0.0,
             dt=DT, nmat=2, C=(3.8e6, 3.4e6)):
        Cv = None if C is None else (ctypes.c_double * len(C))(*C)
        return lib.adi_matmap_scan_add_r0_host(sh, h_tab, K, 2.0, R, None, idp, *n, dx, t, dt, nmat, Cv, None)

    assert host() == _lib.ADI_OK                            # (the good call of the twin; the device entry has no good call here)
    for fn, who in ((dev, 'adi_matmap_scan_add_r0'), (host, 'adi_matmap_scan_add_r0_host')):
        bad = {'null shape': dict(sh=None), 'null segment table': dict(h_tab=None), who + ': null argument': dict(R=None),
               'at least one segment': dict(K=0), 'K = -1': dict(K=-1), 'at most': dict(K=(1 << 24) + 1),
               'dt must be > 0': dict(dt=0.0), r'9 materials \(1 to 8\)': dict(nmat=9, C=(1.0,) * 9),
               r'0 materials \(1 to 8\)': dict(nmat=0), 'C of material 1 must be finite and > 0': dict(C=(1.0, -2.0)),
               'bad dx': dict(dx=0.0), 'bad grid': dict(n=(4, 0, 4)), 'bad t / dt': dict(t=np.nan)}
        for text, kw in bad.items():
            with pytest.raises(ValueError, match=text):
                chk(fn(**kw))
        with pytest.raises(ValueError, match=who + ': null argument'):
            chk(fn(idp=None))
        with pytest.raises(ValueError, match=who + ': null argument'):
            chk(fn(C=None))
        with pytest.raises(ValueError, match='dt must be > 0'):
            chk(fn(dt=-DT))
    for kw in (dict(d_tab=None), dict(fl=None)):
        with pytest.raises(ValueError, match='adi_matmap_scan_add_r0: null argument'):
            chk(dev(**kw))
    seg, box = (ctypes.c_int * 2)(), (ctypes.c_int * 6)()
    with pytest.raises(ValueError, match='adi_scan_window_box: null output'):
        chk(lib.adi_scan_window_box(ctypes.byref(shape), tab.ctypes.data, 2, 2.0, 4, 4, 4, DX, 0.0, DT, None, box))
    with pytest.raises(ValueError, match='adi_scan_window_box: bad t / dt'):
        chk(lib.adi_scan_window_box(ctypes.byref(shape), tab.ctypes.data, 2, 2.0, 4, 4, 4, DX, 0.0, 0.0, seg, box))
    # h_box_out is optional and receives the six ints of the window
    out = (ctypes.c_int * 6)(*[-1] * 6)
    Cv = (ctypes.c_double * 2)(3.8e6, 3.4e6)
    chk(lib.adi_matmap_scan_add_r0_host(ctypes.byref(shape), tab.ctypes.data, 2, 2.0, R0.ctypes.data, None, ids.ctypes.data, 4, 4, 4,
                                        DX, 0.0, DT, 2, Cv, out))
    chk(lib.adi_scan_window_box(ctypes.byref(shape), tab.ctypes.data, 2, 2.0, 4, 4, 4, DX, 0.0, DT, seg, box))
    assert list(out) == list(box) and list(seg) == [0, 1]
    assert all(0 <= out[2 * a] < out[2 * a + 1] <= 4 for a in range(3))


def test_new_kernel_needs_no_scratch():
    """the footprint DESIGN.md 6l5 reports, from the code object"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts'))
    import kernel_meta
    if not os.path.isdir(kernel_meta.LLVM):
        pytest.skip('no ROCm LLVM tools')
    m = {k['short']: k for k in kernel_meta.all_kernels()}['adi::k_mapscan_add_r0']
    assert m['scratch'] == 0 and m.get('vgpr_spill_count', 0) == 0 and m['vgpr_count'] <= 128
