"""GPU: the thermal-history recorder where it records -- k_history_record / k_history_seed on grids whose 16 x 16 x 16 bricks are
partly all-solid, in both load forms, with the flags summary's second word in use (there also k_phase_apply / k_phase_seed and
k_surface_loss), on every comparison of the kernel at equality and one ulp either side, through the C ABI with arrays that are
only 8-byte aligned, through births that cross the planes 15 | 16 and 31 | 32, and through 401 steps of one graph.
tests/history_seam_cases.py builds the inputs; tests/test_history_seams_cpu.py shows that they hold what they are there to catch.

Expected values: ThermalHistory.record_reference / seed_reference fed with the same fields, PhaseChange.correct, and the pinned C
oracle's packs.  Bars: bit for bit everywhere (np.array_equal with NaN in the same places; in part 3 the bit patterns, so that
-0.0 is not 0.0).  Off-mask cells of T_peak, t_hi and t_lo -- those of the physical box outside the logical one included --
hold markers before every record launch and are read back over the whole physical box."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import history_cases as hc  # noqa: E402
import history_seam_cases as hs  # noqa: E402
import seam_cases as sc  # noqa: E402
from history_seam_cases import CP, DX, FACES, K, MARKS, RHO, TINF  # noqa: E402
from test_history_gpu import _assert_result, _assert_state, _guards_intact, _log_rows, _same, _state  # noqa: E402
from test_phase_gpu import _assert_summary, _f_phys  # noqa: E402

pytestmark = pytest.mark.gpu

HOT_OUTSIDE = 1750.0      # what the fields hold in the cells of the physical box outside the logical one: above every level


@pytest.fixture(scope='module')
def mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    return hip


@pytest.fixture(scope='module')
def orc():
    from oracle import adi_oracle
    return adi_oracle


def _force(monkeypatch, hip, phys):
    if phys is not None:
        monkeypatch.setattr(hip, 'recommended_dims', lambda nx, ny, nz: phys)


def _phys_t(t, L):
    """a field over the whole physical box as a view of the device tensor"""
    import torch
    px, py, pz, sx = L.pd
    return torch.as_strided(t, (px, py, pz), (sx, pz, 1))


def _phys(t, L):
    return _phys_t(t, L).cpu().numpy()


def _off_phys(mask, L):
    """the off-mask cells of the physical box"""
    return ~hs.embed(np.asarray(mask, dtype=bool), L.pd[:3])


def _field(hip, grid, a, outside=HOT_OUTSIDE):
    """a device field in the grid's layout; the cells of the physical box outside the logical one hold `outside`"""
    import torch
    L = grid.layout
    d = hip.to_device(np.asarray(a, dtype=np.float64))
    assert L.is_native(d.t)
    if L.padded:
        out = torch.from_numpy(_off_phys(np.ones(L.shape, dtype=bool), L)).to(d.t.device)
        _phys_t(d.t, L)[out] = outside
    return d


def _mark(h, off):
    """markers on every off-mask cell of the three fields, over the physical box"""
    import torch
    L = h.grid.layout
    o = torch.from_numpy(off).to(h.d_peak.device)
    for f, v in zip((h.d_peak, h.d_t_hi, h.d_t_lo), MARKS):
        _phys_t(f, L)[o] = v


def _assert_recorded(h, want, mask, off, what):
    """the in-mask cells equal the definition's, the markers are intact"""
    L = h.grid.layout
    for name, f, w, v in zip(('T_peak', 't_hi', 't_lo'), (h.d_peak, h.d_t_hi, h.d_t_lo), want, MARKS):
        got = _phys(f, L)
        assert (got[off] == v).all(), (what, name, 'markers overwritten', int((got[off] != v).sum()))
        g = got[:mask.shape[0], :mask.shape[1], :mask.shape[2]][mask]
        assert _same(g, w[mask]), (what, name, int((~((g == w[mask]) | (np.isnan(g) & np.isnan(w[mask])))).sum()))


def _summary(grid):
    return hs.summary_bits(grid.d_bricks.cpu().numpy(), grid.layout.pd[:3])


# ---- 1. mixed bricks, both load forms -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', hs.MIXED)
def test_mixed_bricks_in_both_load_forms(mods, monkeypatch, name):
    """three synthetic steps and a selective seed on S1, S1p, S2 (16-byte loads; set bricks next to clear ones on S1 and S2) and
    S3 (odd rows: cell by cell), the pool across the brick seams of every axis"""
    hip = mods
    shape, phys = sc.BOXES[name]
    _force(monkeypatch, hip, phys)
    mask = sc.mask_of(name)
    grid = hip.Grid3D(*shape, DX, mask)
    L = grid.layout
    sc.assert_layout(name, L)
    bits = _summary(grid)
    assert np.array_equal(bits, hs.predicted_bricks(mask, L.pd[:3])), np.argwhere(bits).tolist()
    if name in ('S1', 'S2'):
        assert bits.any() and not bits.all()                        # all-solid workgroups next to ones that read the flags
    else:
        assert not bits.any()
    lv = hip.HistoryLevels(*hs.LEVELS)
    F = hs.mixed_fields(name)
    states, pools, times = hs.definition_steps(hip.ThermalHistory, lv, mask, F, hs.MIXED_T0, hs.MIXED_DT)
    assert any(hs.spans_two_bricks(p, shape) for p in pools) and min(p['cells'] for p in pools) == 0
    d = [_field(hip, grid, f) for f in F]
    h = hip.ThermalHistory(grid, lv, capacity=4, T=d[0], t=hs.MIXED_T0)
    ptrs = [t.t.data_ptr() for t in d] + [h.d_peak.data_ptr()]
    assert hs.vector_form(L.pd, grid.d_flags.data_ptr(), *ptrs) == (name != 'S3')
    _assert_state(h, states[0], 'seed')
    off = _off_phys(mask, L)
    assert all(np.isnan(_phys(f, L)[off]).all() for f in (h.d_peak, h.d_t_hi, h.d_t_lo))
    _mark(h, off)
    for n in range(3):
        h.record(d[n], d[n + 1], hs.MIXED_DT)
        _assert_recorded(h, states[n + 1], mask, off, (name, 'step', n))
        assert np.array_equal(_log_rows(h, n + 1), hc.pool_rows(pools[:n + 1])), (name, n)
        assert h.t == times[n] and _guards_intact(h)
    assert h.slot == 3 and np.array_equal(h.melt_pool()['t'], np.array(times))
    # a seed that selects single cells either side of the seams: they restart, every other in-mask cell keeps its state
    sel = hs.seam_sel(shape)
    h.seed(d[3], sel=sel)
    want = hip.ThermalHistory.seed_reference(states[3], F[3], mask, sel)
    _assert_state(h, want, 'selective seed')
    assert all(np.isnan(_phys(f, L)[off]).all() for f in (h.d_peak, h.d_t_hi, h.d_t_lo))
    assert (want[0][sel & mask] == F[3][sel & mask]).all() and not _same(want[0], states[3][0])


# ---- 2. rows past 512 -----------------------------------------------------------------------------------------------------------
def _long_grid(hip, cavity):
    """the 560 x 48 x 48 box on the physical box the library picks, with the facts the tests rely on read from the layout and
    the downloaded summary: more than 32 bricks along axis 0, the far brick inside the box and clear in the SECOND word, its
    counterpart in the first word set"""
    mask = hs.long_mask(cavity)
    grid = hip.Grid3D(*hs.LONG_SHAPE, DX, mask)
    L = grid.layout
    px, py, pz, sx = L.pd
    nbx, nbz = (px + 15) // 16, (pz + 15) // 16
    bwx = (nbx + 31) // 32
    far, near = hs.LONG_FAR, hs.LONG_NEAR
    assert nbx > 32 and bwx == 2
    assert 16 * (far[0] + 1) < px and 16 * (far[1] + 1) < py and 16 * (far[2] + 1) < pz and min(far) > 0
    assert pz % 2 == 0 and sx % 2 == 0                                   # the 16-byte loads
    words = grid.d_bricks.cpu().numpy().view(np.uint32)
    assert len(words) == ((py + 15) // 16) * nbz * bwx
    wf, bf = hs.summary_word(*far, L.pd[:3])
    wn, bn = hs.summary_word(*near, L.pd[:3])
    assert wf == (far[1] * nbz + far[2]) * bwx + 1 and wn == wf - 1 and bf == bn
    assert not (int(words[wf]) >> bf) & 1 and (int(words[wn]) >> bn) & 1
    assert np.array_equal(hs.summary_bits(words, L.pd[:3]), hs.predicted_bricks(mask, L.pd[:3]))
    return grid, mask


@pytest.mark.parametrize('cavity', [False, True], ids=['hole', 'cavity'])
def test_history_in_the_second_summary_word(mods, cavity):
    hip = mods
    grid, mask = _long_grid(hip, cavity)
    L = grid.layout
    lv = hip.HistoryLevels(*hs.LEVELS)
    F = hs.long_fields()
    states, pools, times = hs.definition_steps(hip.ThermalHistory, lv, mask, F, hs.LONG_T0, hs.LONG_DT)
    assert pools[0]['lo'][0] < 32 and pools[0]['hi'][0] >= 528 and pools[1]['cells'] == 0
    d = [_field(hip, grid, f) for f in F]
    h = hip.ThermalHistory(grid, lv, capacity=2, T=d[0], t=hs.LONG_T0)
    assert hs.vector_form(L.pd, grid.d_flags.data_ptr(), *[t.t.data_ptr() for t in d], h.d_peak.data_ptr())
    _assert_state(h, states[0], 'seed')
    off = _off_phys(mask, L)
    assert off[hs.LONG_HOLE] and all(np.isnan(_phys(f, L)[off]).all() for f in (h.d_peak, h.d_t_hi, h.d_t_lo))
    _mark(h, off)
    for n in range(2):
        h.record(d[n], d[n + 1], hs.LONG_DT)
        _assert_recorded(h, states[n + 1], mask, off, ('step', n))
    assert h.slot == 2 and np.array_equal(_log_rows(h, 2), hc.pool_rows(pools)) and _guards_intact(h)
    mp = h.melt_pool()
    assert np.array_equal(mp['lo'][0], pools[0]['lo']) and np.array_equal(mp['hi'][0], pools[0]['hi']) and mp['dropped'] == 0
    assert np.array_equal(mp['t'], np.array(times))
    for b in (hs.LONG_FAR, hs.LONG_NEAR):                                # both bricks were recorded
        cells = hs.brick_cells(b, hs.LONG_SHAPE) & mask
        assert np.isfinite(np.asarray(h.t_hi)[cells]).any() and np.isfinite(np.asarray(h.t_lo)[cells]).any()


def test_latent_heat_in_the_second_summary_word(mods):
    """the seed, one step with phase= and one direct correction on the box with the single-cell hole: f and T against
    PhaseChange.correct fed with the same step without the correction; the hole's f and the f of the cells of the physical box
    outside the logical one stay as they were"""
    hip = mods
    grid, mask = _long_grid(hip, False)
    L = grid.layout
    shape = hs.LONG_SHAPE
    mat, law = hip.Material(RHO, CP, K), hip.PhaseChange(*hs.LONG_LAW)
    prm = hip.Params(2.0 * DX * DX / hs.KAPPA, 0.5)
    packs = hip.precompute_coeff_packs_unified(grid, mat, robin_h={f: 200.0 for f in FACES})
    T0 = hs.long_melt_field()
    Tstar = np.asarray(hip.StagedStepper(grid, mat, prm, packs, TINF).step(_field(hip, grid, T0, outside=1700.0)))
    ph = hip.PhaseField(grid, mat, law)
    ph.seed(_field(hip, grid, T0, outside=1700.0))
    f0 = law.f_eq(T0) * mask
    want_phys = hs.embed(f0, L.pd[:3], 0.0)                              # 0 off the mask, outside the logical box too
    assert np.array_equal(_f_phys(ph), want_phys)
    _assert_summary(ph, 'seed')
    _phys_t(ph.f, L)[hs.LONG_HOLE] = sc.MARKER                           # (the brick of the hole holds liquid: its entry is set)
    want_phys[hs.LONG_HOLE] = sc.MARKER
    st = hip.StagedStepper(grid, mat, prm, packs, TINF, phase=ph)
    T1 = st.step(_field(hip, grid, T0, outside=1700.0))
    want_T, want_f = law.correct(Tstar, f0, mask, None, CP)
    assert ((want_f > 0) & (want_f < 1)).any() and (want_f == 1.0).any() and not np.array_equal(want_T, Tstar)
    for b in (hs.LONG_FAR, hs.LONG_NEAR):
        assert (want_f[hs.brick_cells(b, shape) & mask] == 1.0).all()
    assert np.array_equal(np.asarray(T1), want_T)
    want_phys[:shape[0], :shape[1], :shape[2]][mask] = want_f[mask]
    got = _f_phys(ph)
    assert np.array_equal(got, want_phys), int((got != want_phys).sum())
    _assert_summary(ph, 'step')
    # a correction of a field of our own, hot outside the logical box as well
    T2 = np.where(want_f > 0, 1380.0, 1500.0) + sc.field_of(shape, seed=3) * 0.05
    d_T2 = _field(hip, grid, T2, outside=1700.0)
    ph.apply(d_T2)
    want_T2, want_f2 = law.correct(T2, want_f, mask, None, CP)
    assert not np.array_equal(want_f2, want_f)
    assert np.array_equal(np.asarray(d_T2)[mask], want_T2[mask]) and np.asarray(d_T2)[hs.LONG_HOLE] == T2[hs.LONG_HOLE]
    assert (_phys(d_T2.t, L)[_off_phys(np.ones(shape, dtype=bool), L)] == 1700.0).all()
    want_phys[:shape[0], :shape[1], :shape[2]][mask] = want_f2[mask]
    got = _f_phys(ph)
    assert np.array_equal(got, want_phys), int((got != want_phys).sum())
    _assert_summary(ph, 'apply')


def test_surface_loss_in_the_second_summary_word(mods, orc):
    """LossPacks.update (the per-step mode) on the box with the cavity: the inner-brick skip leaves brick (33, 1, 1) in, and the
    three coefficient arrays are the oracle's on every exposed cell and untouched elsewhere"""
    hip = mods
    grid, mask = _long_grid(hip, True)
    L = grid.layout
    shape = hs.LONG_SHAPE
    mat, loss = hip.Material(RHO, CP, K), sc.loss5(hip.SurfaceLoss)
    T = sc.field_of(shape)
    lp = hip.LossPacks(grid, mat, loss, TINF)
    import torch
    for p in lp.packs:
        torch.as_strided(p.d_coeff, (L.numel_padded,), (1,)).fill_(sc.MARKER)
    lp.update(hip.to_device(T))
    want = sc.expected_packs(orc, shape, mask, loss, T)
    far, near = hs.brick_cells(hs.LONG_FAR, shape), hs.brick_cells(hs.LONG_NEAR, shape)
    for a, p in enumerate(lp.packs):
        ex = sc.exposed_along(mask, a)
        assert (ex & far).any() and not (ex & near).any()
        got = _phys(p.d_coeff, L)
        w = np.where(hs.embed(ex, L.pd[:3]), hs.embed(want[a].coeff, L.pd[:3], 0.0), sc.MARKER)
        bad = np.argwhere(got != w)
        assert len(bad) == 0, ('axis', a, 'differing cells', len(bad), 'first', bad[0].tolist())
        assert (got[:shape[0], :shape[1], :shape[2]][ex & far] != sc.MARKER).all()
        assert (got[:shape[0], :shape[1], :shape[2]][near] == sc.MARKER).all()


# ---- 3. every comparison at its edge --------------------------------------------------------------------------------------------
def _edge_grid(hip):
    mask = np.ones(hs.EDGE_SHAPE, dtype=bool)
    grid = hip.Grid3D(*hs.EDGE_SHAPE, DX, mask)
    L = grid.layout
    assert not L.padded and L.pd[2] % 2 == 0 and L.pd[3] % 2 == 0
    assert _summary(grid).tolist() == [[[True, True]]]                   # two bricks, both all solid
    return grid, mask


@pytest.mark.parametrize('which', list(hs.EDGE_LEVELS))
def test_every_comparison_at_its_edge(mods, which):
    """the directed (A, B) pairs of tests/history_seam_cases.py in both bricks: one step against the definition, bit patterns
    compared, with the levels (800, 500, 1400) and with (0, -5, 0), where B = -0.0 sits on T_hi and on T_melt"""
    hip = mods
    grid, mask = _edge_grid(hip)
    levels = hs.EDGE_LEVELS[which]
    lv = hip.HistoryLevels(*levels)
    A, B = hs.edge_fields(which)
    c = hs.edge_classes(A, B, levels)
    for nm in ('A_on_hi', 'B_on_hi', 'A_on_lo', 'B_on_lo', 'B_on_peak', 'B_on_melt', 'fraction_one', 'both_crossings', 'A_inf',
               'B_nan', 'A_nan') + (('B_neg_zero', 'A_neg_zero') if which == 'zero' else ()):
        assert c[nm][:, :, :16].any() and c[nm][:, :, 16:].any(), nm
    TH = hip.ThermalHistory
    seed = TH.seed_reference(hc.empty_state(hs.EDGE_SHAPE), A, mask)
    with np.errstate(all='ignore'):
        want, pool = TH.record_reference(seed, A, B, mask, hs.EDGE_T0, hs.EDGE_DT, lv)
    dA, dB = hip.to_device(A), hip.to_device(B)
    assert hs.same_bits(np.asarray(dA), A) and hs.same_bits(np.asarray(dB), B)
    h = TH(grid, lv, capacity=2, T=dA, t=hs.EDGE_T0)
    assert hs.vector_form(grid.layout.pd, grid.d_flags.data_ptr(), dA.t.data_ptr(), dB.t.data_ptr(), h.d_peak.data_ptr())
    for name, got, w in zip(('T_peak', 't_hi', 't_lo'), _state(h), seed):
        assert hs.same_bits(got, w), ('seed', name)
    h.record(dA, dB, hs.EDGE_DT)
    for name, got, w in zip(('T_peak', 't_hi', 't_lo'), _state(h), want):
        bad = ~((hs.bits(got) == hs.bits(w)) | (np.isnan(got) & np.isnan(w)))
        first = tuple(np.argwhere(bad)[0]) if bad.any() else None
        assert hs.same_bits(got, w), (which, name, int(bad.sum()), first, None if first is None else (A[first], B[first], got[first], w[first]))
    assert np.array_equal(_log_rows(h, 1), hc.pool_rows([pool])) and pool['cells'] == int((B >= levels[2]).sum())
    assert h.t == hs.EDGE_T0 + hs.EDGE_DT and _guards_intact(h)


def test_the_vote_of_a_brick_next_to_one_that_does_not_vote(mods):
    """brick 0 entirely at a peak of exactly T_lo records nothing; brick 1 with one cell a hair above records that cell alone"""
    hip = mods
    grid, mask = _edge_grid(hip)
    lv = hip.HistoryLevels(*hs.LEVELS)
    TH = hip.ThermalHistory
    for bump in (False, True):
        A, B = hs.vote_fields(bump)
        h = TH(grid, lv, capacity=2, T=hip.to_device(A))
        h.record(hip.to_device(A), hip.to_device(B), 0.5)
        seed = TH.seed_reference(hc.empty_state(hs.EDGE_SHAPE), A, mask)
        want, _ = TH.record_reference(seed, A, B, mask, 0.0, 0.5, lv)
        _assert_state(h, want, bump)
        got = np.asarray(h.t_lo)
        assert np.argwhere(np.isfinite(got)).tolist() == ([list(hs.VOTE_CELL)] if bump else [])
        assert not np.isfinite(got[:, :, :16]).any() and h.t == 0.5


# ---- 4. pointer alignment through the C ABI -----------------------------------------------------------------------------------------
ABI_VARIANTS = ('aligned', 'T_in', 'T_out', 'T_peak', 'flags', 'no_bricks')


def _abi_buffers(hip, grid, lv, A, B, variant):
    """the arrays of one call sequence as views of buffers one element larger: `variant` names the one that starts 8 bytes (the
    flags: 1 byte) past its buffer"""
    import torch
    L = grid.layout
    n = L.numel_padded
    dev = grid.d_flags.device
    flat = lambda t: torch.as_strided(t, (n,), (1,))

    def view(buf, shifted):
        v = buf[1:n + 1] if shifted else buf[:n]
        assert v.data_ptr() % 16 == (buf.element_size() if shifted else 0)
        return v
    b = {}
    for key, src in (('T_in', A), ('T_out', B), ('T_peak', None), ('t_hi', None), ('t_lo', None)):
        buf = torch.full((n + 2,), float('nan'), dtype=torch.float64, device=dev)
        b[key] = view(buf, variant == key)
        if src is not None:
            b[key].copy_(flat(_field(hip, grid, src).t))
    fl = torch.zeros(n + 2, dtype=torch.uint8, device=dev)
    b['flags'] = view(fl, variant == 'flags')
    b['flags'].copy_(flat(grid.d_flags))
    b['bricks'] = None if variant == 'no_bricks' else grid.d_bricks
    return b


def _abi_phys(v, L):
    import torch
    px, py, pz, sx = L.pd
    return torch.as_strided(v, (px, py, pz), (sx, pz, 1), v.storage_offset())


def _cp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize('name', ['S1p', 'S2'])
def test_arrays_that_are_only_8_byte_aligned(mods, monkeypatch, name):
    """adi_history_seed and adi_history_record called directly: each of T_in, T_out, T_peak shifted by 8 bytes and the flags by
    1 byte (each takes the kernels to the cell-by-cell form), then without the flags summary -- the bits of the aligned call and
    of the definition every time.  On S1p every brick is clear; on S2 all but one are set, so there the summary matters"""
    hip = mods
    import torch
    from adi_thermal_fields_amd import _lib
    lib = _lib.lib
    shape, phys = sc.BOXES[name]
    _force(monkeypatch, hip, phys)
    mask = sc.mask_of(name)
    grid = hip.Grid3D(*shape, DX, mask)
    L = grid.layout
    sc.assert_layout(name, L)
    assert _summary(grid).any() == (name == 'S2')
    lv = hip.HistoryLevels(*hs.LEVELS)
    F = hs.mixed_fields(name)
    A, B = F[0], F[2]                                                     # the step from hot to cold: crossings of both levels
    TH = hip.ThermalHistory
    seed = TH.seed_reference(hc.empty_state(shape), A, mask)
    want, pool = TH.record_reference(seed, A, B, mask, hs.MIXED_T0, hs.MIXED_DT, lv)
    assert np.isfinite(want[1]).any() and np.isfinite(want[2]).any()
    off = _off_phys(mask, L)
    o = torch.from_numpy(off).to(grid.d_flags.device)
    inside = (slice(0, shape[0]), slice(0, shape[1]), slice(0, shape[2]))
    res = {}
    for variant in ABI_VARIANTS:
        b = _abi_buffers(hip, grid, lv, A, B, variant)
        vec = hs.vector_form(L.pd, b['flags'].data_ptr(), b['T_in'].data_ptr(), b['T_out'].data_ptr(), b['T_peak'].data_ptr())
        assert vec == (variant in ('aligned', 'no_bricks')), variant
        hobj = TH(grid, lv, capacity=2, t=hs.MIXED_T0)                    # its block and its log; nothing seeded
        st = [b['T_peak'], b['t_hi'], b['t_lo']]
        _lib.check(lib.adi_history_seed(_cp(b['T_in']), *[_cp(s) for s in st], _cp(b['flags']), _cp(b['bricks']), None, *L.pd,
                                        hip._stream()))
        got = [_abi_phys(s, L).cpu().numpy() for s in st]
        for nm, g, w in zip(('T_peak', 't_hi', 't_lo'), got, seed):
            assert _same(g[inside], w) and np.isnan(g[off]).all(), (variant, 'seed', nm)
        for s, v in zip(st, MARKS):
            _abi_phys(s, L)[o] = v
        hobj.set_clock(hs.MIXED_DT)
        _lib.check(lib.adi_history_record(ctypes.byref(lv.as_c()), _cp(hobj.d_block), _cp(b['T_in']), _cp(b['T_out']),
                                          *[_cp(s) for s in st], _cp(hobj.d_log), _cp(b['flags']), _cp(b['bricks']), *L.pd,
                                          hip._stream()))
        got = [_abi_phys(s, L).cpu().numpy() for s in st]
        for nm, g, w, v in zip(('T_peak', 't_hi', 't_lo'), got, want, MARKS):
            assert (g[off] == v).all(), (variant, nm, 'markers overwritten')
            assert _same(g[inside][mask], w[mask]), (variant, nm)
        row = _log_rows(hobj, 1).copy()
        assert np.array_equal(row, hc.pool_rows([pool])) and _guards_intact(hobj), variant
        res[variant] = got + [row]
    for variant in ABI_VARIANTS[1:]:
        for x, y in zip(res['aligned'], res[variant]):
            assert _same(x, y), variant


def test_what_the_c_abi_refuses_launches_nothing(mods, monkeypatch):
    """ADI_ERR_ARG for aliased arrays, levels out of order or not finite and a capacity of 0 or 2^31 -- and the state arrays, the
    log and the block hold afterwards what they held before"""
    hip = mods
    import torch
    from adi_thermal_fields_amd import _lib
    lib = _lib.lib
    shape, phys = sc.BOXES['S1p']
    _force(monkeypatch, hip, phys)
    mask = sc.mask_of('S1p')
    grid = hip.Grid3D(*shape, DX, mask)
    L = grid.layout
    lv = hip.HistoryLevels(*hs.LEVELS)
    F = hs.mixed_fields('S1p')
    b = _abi_buffers(hip, grid, lv, F[0], F[2], 'aligned')
    hobj = hip.ThermalHistory(grid, lv, capacity=2, t=hs.MIXED_T0)
    hobj.set_clock(hs.MIXED_DT)
    for key, v in zip(('T_peak', 't_hi', 't_lo'), MARKS):
        b[key].fill_(v)
    held = {k: b[k].clone() for k in ('T_in', 'T_out', 'T_peak', 't_hi', 't_lo')}
    held_log, held_blk = hobj._log_store.clone(), hobj.d_block.clone()

    def record(levels=hs.LEVELS, **swap):
        a = dict(b, **{k: b[v] for k, v in swap.items()})
        return lib.adi_history_record(ctypes.byref(_lib.HistoryLevelsC(*levels)), _cp(hobj.d_block), _cp(a['T_in']), _cp(a['T_out']),
                                      _cp(a['T_peak']), _cp(a['t_hi']), _cp(a['t_lo']), _cp(hobj.d_log), _cp(a['flags']),
                                      _cp(a['bricks']), *L.pd, hip._stream())

    def seed(**swap):
        a = dict(b, **{k: b[v] for k, v in swap.items()})
        return lib.adi_history_seed(_cp(a['T_in']), _cp(a['T_peak']), _cp(a['t_hi']), _cp(a['t_lo']), _cp(a['flags']),
                                    _cp(a['bricks']), None, *L.pd, hip._stream())
    inf, nan = float('inf'), float('nan')
    calls = [('T_out aliases T_in', lambda: record(T_out='T_in')),
             ('T_peak aliases T_in', lambda: record(T_peak='T_in')), ('t_hi aliases T_out', lambda: record(t_hi='T_out')),
             ('t_lo aliases T_in', lambda: record(t_lo='T_in')), ('seed: T_peak aliases T', lambda: seed(T_peak='T_in')),
             ('seed: t_lo aliases T', lambda: seed(t_lo='T_in')),
             ('T_hi below T_lo', lambda: record(levels=(500.0, 800.0, 1400.0))), ('T_hi equals T_lo', lambda: record(levels=(800.0, 800.0, 1400.0))),
             ('T_hi infinite', lambda: record(levels=(inf, 500.0, 1400.0))), ('T_lo NaN', lambda: record(levels=(800.0, nan, 1400.0))),
             ('T_melt infinite', lambda: record(levels=(800.0, 500.0, -inf))),
             ('capacity 0', lambda: lib.adi_history_reset_log(_cp(hobj.d_block), _cp(hobj.d_log), 0, hip._stream())),
             ('capacity 2^31', lambda: lib.adi_history_reset_log(_cp(hobj.d_block), _cp(hobj.d_log), 2 ** 31, hip._stream()))]
    for what, call in calls:
        assert call() == _lib.ADI_ERR_ARG, what
        assert _lib.last_error(), what
    torch.cuda.synchronize()
    as_int = lambda t: t.view(torch.int64)
    for k, v in held.items():
        assert torch.equal(as_int(b[k]), as_int(v)), k
    assert torch.equal(hobj._log_store, held_log) and torch.equal(hobj.d_block, held_blk)
    # ... and the same arrays in order are accepted
    assert record() == _lib.ADI_OK
    assert lib.adi_history_reset_log(_cp(hobj.d_block), _cp(hobj.d_log), 2, hip._stream()) == _lib.ADI_OK
    torch.cuda.synchronize()
    assert not torch.equal(as_int(b['T_peak']), as_int(held['T_peak']))


# ---- 5. births across the seams with a recorder -------------------------------------------------------------------------------------
def test_births_across_the_seams(mods, monkeypatch):
    """the device calls of the layer-birth loop on the padded 20 x 18 x 40 box, one recorded step per layer: planes [0, 14),
    then 14..17 across 15 | 16, then layers of two planes across 31 | 32 to the top.  After every birth the summary (rebuilt on
    the layer's plane range only) is the predicted one and sync_mask seeds exactly the newborn cells; after every step the state
    and the log are the definition's.  Two bricks turn all-solid on the way"""
    hip = mods
    import torch
    TH = hip.ThermalHistory
    c = hs.BIRTH
    shape, phys = sc.BOXES[c['box']]
    _force(monkeypatch, hip, phys)
    nz = shape[2]
    full = np.ones(shape, dtype=bool)
    grid = hip.Grid3D(*shape, DX, np.zeros(shape, dtype=bool))
    L = grid.layout
    sc.assert_layout(c['box'], L)
    mat, prm, lv = hip.Material(RHO, CP, K), hip.Params(hs.birth_dt(), c['theta']), hip.HistoryLevels(*c['levels'])
    d_full, d_act = L.to_layout(full, torch.uint8), L.empty(torch.uint8, zero=True)
    grid.set_mask_device(d_act, all_solid=False)
    bpacks = hip.BirthPacks(grid, mat, robin_h={f: c['h'] for f in FACES})
    T = hip.to_device(np.full(shape, TINF))
    layers, masks = hs.birth_layers(), hs.birth_masks()
    h, state, mask, t, pools = None, None, np.zeros(shape, dtype=bool), 0.0, []
    bits_old = _summary(grid)
    assert not bits_old.any()
    flips, steps_after_flip = 0, 0
    for n, ((k0, k1), m) in enumerate(zip(layers, masks)):
        hip.birth_planes(T, d_act, d_full, grid, k0, k1, c['Ts'])
        grid.set_mask_device(d_act, max(k0 - 1, 0), min(nz, k1 + 1), all_solid=False)      # the range form
        packs = bpacks.update(k0 - 1, k1 + 1)
        assert np.array_equal(grid.mask, m), n
        bits = _summary(grid)
        assert np.array_equal(bits, hs.predicted_bricks(m, L.pd[:3])), (n, np.argwhere(bits).tolist())
        flips += int((bits & ~bits_old).sum())
        bits_old = bits
        newborn = m & ~mask
        Th = np.asarray(T)
        assert newborn.any() and (Th[newborn] == c['Ts']).all()
        if h is None:
            h = TH(grid, lv, capacity=len(layers) + 1, T=T)
            state = TH.seed_reference(hc.empty_state(shape), Th, m)
        else:
            with pytest.raises(ValueError, match='sync_mask'):
                h.record(T, T.copy(), prm.dt)
            h.sync_mask(T)
            kept = tuple(np.where(mask, s, v) for s, v in zip(state, MARKS))               # (what the device holds off the old mask)
            state = TH.seed_reference(kept, Th, m, newborn)
        _assert_state(h, state, ('birth', n))
        assert (np.asarray(h.T_peak)[newborn] == c['Ts']).all()
        mask = m
        off = _off_phys(mask, L)
        assert all(np.isnan(_phys(f, L)[off]).all() for f in (h.d_peak, h.d_t_hi, h.d_t_lo))
        _mark(h, off)
        Tn = hip.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=TINF, history=h)
        state, pool = TH.record_reference(state, Th, np.asarray(Tn), mask, t, prm.dt, lv)
        t = t + prm.dt
        pools.append(pool)
        _assert_recorded(h, state, mask, off, ('step', n))
        assert np.array_equal(_log_rows(h, n + 1), hc.pool_rows(pools)) and h.t == t, n
        steps_after_flip += int(flips > 0)
        T = Tn
    assert mask.all() and flips == 2 and bits_old[0, 0, 0] and bits_old[0, 0, 1]           # bits went 0 -> 1 during the run
    assert steps_after_flip == len(layers) - 1
    assert np.isfinite(state[1]).any() and np.isfinite(state[2]).any() and max(p['cells'] for p in pools) > 0
    assert h.slot == len(layers) and _guards_intact(h)


def test_run_layer_birth_on_a_head_of_three_bricks_with_history(mods):
    """waam.run_layer_birth(history=) on the 20 x 18 x 40 head in layers of two planes against the same event loop with single
    steps and the definition (tests/history_seam_cases.py: layer_birth_by_single_steps)"""
    hip = mods
    import torch
    from adi_thermal_fields_amd import waam
    c = hs.HEAD
    full, layers, tb, t_out, sched, dt_cap, nsubs = hs.head_plan(waam)
    assert max(nsubs) < waam.GRAPH_MIN_NSUB and (14, 15) in layers and (16, 17) in layers and (32, 33) in layers
    lv = hip.HistoryLevels(*c['levels'])
    got, nsteps, res = waam.run_layer_birth(hip, full, DX, (RHO, CP, K), c['h'], TINF, c['Ts'], c['theta'], c['cfl'], layers, tb,
                                            t_out, history=lv)
    seen = []

    def summary(grid, mask):
        bits = _summary(grid)
        assert np.array_equal(bits, hs.predicted_bricks(mask, grid.layout.pd[:3])), len(seen)
        seen.append(bits)
    T, steps, state, pools, times, mask = hs.layer_birth_by_single_steps(hip, waam, full, DX, (RHO, CP, K), c['h'], TINF, c['Ts'],
                                                                         c['theta'], dt_cap, layers, sched, lv, uint8=torch.uint8,
                                                                         summary=summary)
    assert nsteps == steps == len(pools) == sum(nsubs[1:]) and np.array_equal(mask, full) and len(seen) == len(layers)
    assert np.array_equal(got, T)
    assert np.isfinite(state[1]).any() and np.isfinite(state[2]).any() and max(p['cells'] for p in pools) > 0
    third = np.zeros(full.shape, dtype=bool)
    third[:, :, 32:] = full[:, :, 32:]
    assert np.isfinite(state[1][third]).any()                            # crossings in the third brick along axis 2
    _assert_result(res, state, pools, times, 'layer birth')
    assert times[0] > tb[0]


# ---- 6. a long run through the graph ----------------------------------------------------------------------------------------------
def test_401_steps_through_the_graph_and_a_log_that_fills(mods):
    """StagedStepper.run(T, 401) -- 200 replays and a tail step -- against 401 single steps without a recorder and the
    definition with the clock of a run (t_n = t0 + n*dt); then a log of 402 rows that a recorded step, a run of 399 and a fresh
    capture's run of 2 fill to the brim: the four warm-up steps of that capture spill past the last row and are taken back"""
    hip = mods
    TH = hip.ThermalHistory
    c = hs.LONG_RUN
    mask, T0, dt = hs.long_run_inputs()
    nst = c['steps']
    grid, mat, prm = hip.Grid3D(*c['shape'], DX, mask), hip.Material(RHO, CP, K), hip.Params(dt, c['theta'])
    packs = hip.precompute_coeff_packs_unified(grid, mat, robin_h={f: c['h'] for f in FACES})
    lv = hip.HistoryLevels(*hs.LEVELS)
    plain = hip.StagedStepper(grid, mat, prm, packs, TINF)
    traj, T = [T0], hip.to_device(T0)
    for _ in range(nst + 1):
        T = plain.step(T)
        traj.append(np.asarray(T))
    case = dict(shape=c['shape'], mask=mask)
    states, pools, times, t_end = hc.record_trajectory(TH, lv, case, traj[:nst + 1], t=c['t0'], clock='run', segments=[(dt, nst, None)])
    late = hs.late_crossings(states, c['late'])
    print('crossings after step %d: T_hi %d, T_lo %d' % ((c['late'],) + late))
    assert min(late) > 0
    h = TH(grid, lv, capacity=nst, T=hip.to_device(T0), t=c['t0'])
    st = hip.StagedStepper(grid, mat, prm, packs, TINF, history=h)
    out = st.run(hip.to_device(T0), nst)
    assert st.captures == 1 and np.array_equal(np.asarray(out), traj[nst])
    _assert_state(h, states[nst], 'run of 401')
    assert np.array_equal(_log_rows(h, nst), hc.pool_rows(pools))
    mp = h.melt_pool()
    assert h.t == t_end and h.slot == nst and mp['dropped'] == 0 and np.array_equal(mp['t'], np.array(times)) and _guards_intact(h)
    empty = np.array([0] + [2 ** 31 - 1] * 3 + [-1] * 3 + [0], dtype=np.int32)
    assert np.array_equal(h.d_log.cpu().numpy().reshape(nst + 1, 8)[nst], empty)            # nothing spilled
    # a recorded step, then a second stepper's run of 401 on a log of 402 rows: a fresh capture with the log in use
    segs = [(dt, 1, None), (dt, nst, None)]
    states2, pools2, times2, t_end2 = hc.record_trajectory(TH, lv, case, traj, t=c['t0'], clock='run', segments=segs)
    h2 = TH(grid, lv, capacity=nst + 1, T=hip.to_device(T0), t=c['t0'])
    first = hip.StagedStepper(grid, mat, prm, packs, TINF, history=h2)
    T1 = first.step(hip.to_device(T0))
    assert h2.slot == 1 and np.array_equal(np.asarray(T1), traj[1])
    second = hip.StagedStepper(grid, mat, prm, packs, TINF, history=h2)
    out = second.run(T1, nst)
    assert second.captures == 1 and np.array_equal(np.asarray(out), traj[nst + 1])
    _assert_state(h2, states2[nst + 1], 'step and run of 401')
    mp = h2.melt_pool()
    assert h2.slot == nst + 1 and mp['dropped'] == 0 and h2.t == t_end2 and np.array_equal(mp['t'], np.array(times2))
    assert np.array_equal(_log_rows(h2, nst + 1), hc.pool_rows(pools2)) and _guards_intact(h2)
    assert np.array_equal(h2.d_log.cpu().numpy().reshape(nst + 2, 8)[nst + 1], empty)
    # the warm-up of a fresh capture two rows from the end of the log: its four steps run past the capacity
    segs = [(dt, 1, None), (dt, nst - 2, None), (dt, 2, None)]
    states3, pools3, times3, t_end3 = hc.record_trajectory(TH, lv, case, traj, t=c['t0'], clock='run', segments=segs)
    h2.reset(hip.to_device(T0), t=c['t0'])
    T1 = first.step(hip.to_device(T0))
    Tm = second.run(T1, nst - 2)
    assert second.captures == 1 and h2.slot == nst - 1
    third = hip.StagedStepper(grid, mat, prm, packs, TINF, history=h2)
    out = third.run(Tm, 2)
    assert third.captures == 1 and np.array_equal(np.asarray(out), traj[nst + 1])
    _assert_state(h2, states3[nst + 1], 'warm-up at the end of the log')
    mp = h2.melt_pool()
    assert h2.slot == nst + 1 and mp['dropped'] == 0 and h2.t == t_end3 and np.array_equal(mp['t'], np.array(times3))
    assert np.array_equal(_log_rows(h2, nst + 1), hc.pool_rows(pools3)) and _guards_intact(h2)
    assert np.array_equal(h2.d_log.cpu().numpy().reshape(nst + 2, 8)[nst + 1], empty)
