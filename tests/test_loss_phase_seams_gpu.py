"""GPU: k_surface_loss and k_phase_apply / k_phase_seed where their 16 x 16 x 16 bricks meet -- plane ranges that begin, end and
turn inside bricks (both modes of adi_surface_loss_update), the inner-brick skip of the per-step mode next to a cavity, births on
planes 15 and 30 of a head with three bricks along axis 2 with surface loss, latent heat and a moving source on, and directed
inputs on every comparison of the two laws.  tests/seam_cases.py builds the inputs; tests/test_loss_phase_seams_cpu.py shows that
they hold what they are there to catch.

Expected values: the pinned C oracle fed with SurfaceLoss.h_of fields, and PhaseChange.correct / f_eq.  Bars: np.array_equal
wherever both sides perform the header's fixed sequence of IEEE operations (coefficient arrays, one correction, the seed, graph
replay against plain launches); whole runs T <= 1e-10 relative L-inf and |f - f_oracle| <= 1e-10 * T_birth / (Tl - Ts), the
project's bars.  Cells that must not be written hold a marker before the call and are read back over the whole physical box."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import seam_cases as sc  # noqa: E402
from seam_cases import CP, DX, K, KAPPA, MARKER, RHO, TINF, rel_linf  # noqa: E402
from test_phase_gpu import _assert_summary  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from oracle import adi_oracle as orc
    return hip, orc


def _force(monkeypatch, hip, phys):
    if phys is not None:
        monkeypatch.setattr(hip, 'recommended_dims', lambda nx, ny, nz: phys)


def _grid(monkeypatch, hip, name, mask=None):
    """the box `name` with its mask, on the physical box the table of tests/seam_cases.py names -- asserted, not assumed"""
    shape, phys = sc.BOXES[name]
    _force(monkeypatch, hip, phys)
    grid = hip.Grid3D(*shape, DX, sc.mask_of(name) if mask is None else mask)
    sc.assert_layout(name, grid.layout)
    return grid


def _phys(t, layout):
    """a field over the whole physical box, as it is in memory"""
    import torch
    px, py, pz, sx = layout.pd
    return torch.as_strided(t, (px, py, pz), (sx, pz, 1)).cpu().numpy()


def _fill(t, layout, value):
    """every element of the buffer, the cells outside the logical box and the plane padding included"""
    import torch
    torch.as_strided(t, (layout.numel_padded,), (1,)).fill_(value)


def _embed(a, layout, fill=0.0):
    out = np.full(layout.pd[:3], fill, dtype=a.dtype)
    out[:a.shape[0], :a.shape[1], :a.shape[2]] = a
    return out


def _same(got, want, what):
    """bit equality with a message that carries the count of differing cells and the first of them"""
    if got.shape == want.shape and np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    first = tuple(int(v) for v in bad[0])
    raise AssertionError((what, 'differing cells', len(bad), 'first', first, 'got', float(got[first]), 'want', float(want[first])))


def _brick_bit(grid, bi, bj, bk):
    px, py, pz, _ = grid.layout.pd
    nbz, nwx = (pz + 15) // 16, ((px + 15) // 16 + 31) // 32
    w = grid.d_bricks.cpu().numpy().view(np.uint32)
    return bool((int(w[(bj * nbz + bk) * nwx + bi // 32]) >> (bi % 32)) & 1)


def _update_range(hip, lp, d_T, k0, k1, bricks):
    """adi_surface_loss_update in the per-step mode (full = 0) on the planes [k0, k1): no host code passes a range there"""
    from adi_thermal_fields_amd import _lib
    g, m = lp.grid, lp.mat
    law = lp.loss.as_c(lp.Tinf)
    coeff = _lib.ptr_array([p.d_coeff.data_ptr() for p in lp.packs])
    d_bricks = ctypes.c_void_p(g.d_bricks.data_ptr()) if bricks else None
    _lib.check(_lib.lib.adi_surface_loss_update(ctypes.byref(law), float(lp.Tinf), ctypes.c_void_p(d_T.t.data_ptr()),
                                                ctypes.c_void_p(g.d_flags.data_ptr()), d_bricks, *g.layout.pd, g.dx, m.rho, m.cp,
                                                coeff, int(k0), int(k1), 0, hip._stream()))


# ---- 1. coefficient arrays on plane ranges ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['S1', 'S1p', 'S3'])
def test_plane_ranges_in_both_modes(mods, monkeypatch, name):
    hip, orc = mods
    grid = _grid(monkeypatch, hip, name)
    L = grid.layout
    shape, mask = sc.BOXES[name][0], sc.mask_of(name)
    nz = shape[2]
    mat, loss = hip.Material(RHO, CP, K), sc.loss5(hip.SurfaceLoss)
    T = sc.field_of(shape)
    d_T = hip.to_device(T)
    assert L.is_native(d_T.t)
    lp = hip.LossPacks(grid, mat, loss, TINF)
    want = [_embed(p.coeff, L) for p in sc.expected_packs(orc, shape, mask, loss, T)]
    exposed = [_embed(sc.exposed_along(mask, a), L, False) for a in range(3)]
    for k0, k1 in sc.plane_ranges(name):
        # full = 1 through rebuild: every cell of the planes, zeros where nothing is exposed; nothing outside them
        for p in lp.packs:
            _fill(p.d_coeff, L, MARKER)
        lp.rebuild(d_T, k0, k1)
        for a, p in enumerate(lp.packs):
            got = _phys(p.d_coeff, L)
            _same(got[:, :, k0:k1], want[a][:, :, k0:k1], ('full', name, 'axis', a, 'range', (k0, k1)))
            out = np.ones(got.shape, dtype=bool)
            out[:, :, k0:k1] = False
            assert out[:, :, nz:].all()                                    # (S1p: the planes beyond the logical box)
            _same(got[out], np.full(int(out.sum()), MARKER), ('full, outside', name, 'axis', a, 'range', (k0, k1)))
        # full = 0: the cells exposed along the axis inside the range, nothing else; with and without the flags summary
        res = {}
        for bricks in (True, False):
            for p in lp.packs:
                _fill(p.d_coeff, L, MARKER)
            _update_range(hip, lp, d_T, k0, k1, bricks)
            res[bricks] = [_phys(p.d_coeff, L) for p in lp.packs]
            for a, got in enumerate(res[bricks]):
                sel = exposed[a].copy()
                sel[:, :, :k0] = False
                sel[:, :, k1:] = False
                assert sel.any() or k0 == k1
                _same(got, np.where(sel, want[a], MARKER), ('step', name, 'bricks', bricks, 'axis', a, 'range', (k0, k1)))
        for a in range(3):
            _same(res[True][a], res[False][a], ('step, bricks against none', name, 'axis', a, 'range', (k0, k1)))


def test_neumann_packs_through_a_birth_across_plane_16(mods, monkeypatch):
    """LossPacks(neumann=) on the padded box: planes [14, 18) are born, rebuild(T, 13, 19) rewrites the coefficients and the
    fluxes of those planes, and all six arrays are the oracle's for the new mask at every cell"""
    hip, orc = mods
    import torch
    shape = sc.BOXES['S1p'][0]
    full = sc.mask_of('S1p')
    k0, k1 = sc.BIRTH_PLANES
    old = full.copy()
    old[:, :, k0:k1] = False
    grid = _grid(monkeypatch, hip, 'S1p', mask=old)
    L = grid.layout
    mat, loss, q = hip.Material(RHO, CP, K), sc.loss5(hip.SurfaceLoss), sc.neumann_of(shape)
    T = sc.field_of(shape)
    d_T = hip.to_device(T)
    d_full, d_act = L.to_layout(full, torch.uint8), L.to_layout(old, torch.uint8)
    grid.set_mask_device(d_act, all_solid=False)
    lp = hip.LossPacks(grid, mat, loss, TINF, neumann=q, T=d_T)
    before = sc.expected_packs(orc, shape, old, loss, T, neumann=q)
    for a, (p, w) in enumerate(zip(lp.packs, before)):
        _same(p.coeff, w.coeff, ('before the birth, coeff', a))
        _same(p.qflux, w.qflux, ('before the birth, qflux', a))
    hip.birth_planes(d_T, d_act, d_full, grid, k0, k1, sc.T_BIRTH)
    grid.set_mask_device(d_act, k0 - 1, k1 + 1, all_solid=False)
    assert np.array_equal(grid.mask, full)
    Tn = np.where(full & ~old, sc.T_BIRTH, T)
    assert np.array_equal(np.asarray(d_T), Tn)
    lp.rebuild(d_T, k0 - 1, k1 + 1)
    after = sc.expected_packs(orc, shape, full, loss, Tn, neumann=q)
    for a, (p, w) in enumerate(zip(lp.packs, after)):
        _same(p.coeff, w.coeff, ('after the birth, coeff', a))
        _same(p.qflux, w.qflux, ('after the birth, qflux', a))
        assert p.mask_version == grid.mask_version
    # the cells of the physical box outside the logical one carry neither a coefficient nor a flux
    for p in lp.packs:
        for t in (p.d_coeff, p.d_qflux):
            got = _phys(t, L)
            assert not got[shape[0]:].any() and not got[:, shape[1]:].any() and not got[:, :, shape[2]:].any()


# ---- 2. the inner-brick skip ----------------------------------------------------------------------------------------------
def test_inner_brick_skip_next_to_a_cavity(mods, monkeypatch):
    hip, orc = mods
    shape = sc.BOXES['S2'][0]
    mat, loss = hip.Material(RHO, CP, K), sc.loss5(hip.SurfaceLoss)
    T = sc.field_of(shape)
    T2 = T.copy()
    T2[16:32, 16:32, 16:32] += 55.0                                         # another field inside brick (1, 1, 1) only
    for cavity in (True, False):
        mask = sc.mask_of('S2', cavity=cavity)
        grid = _grid(monkeypatch, hip, 'S2', mask=mask)
        L = grid.layout
        assert L.pd[:3] == shape                                             # bricks (1, 1, 1) and (1, 1, 2) are inner bricks
        assert _brick_bit(grid, 1, 1, 2) and _brick_bit(grid, 1, 1, 1) == (not cavity)
        lp = hip.LossPacks(grid, mat, loss, TINF)
        exposed = [sc.exposed_along(mask, a) for a in range(3)]
        near = np.zeros(shape, dtype=bool)
        near[16:32, 16:32, 16:32] = True
        for field in (T, T2):
            for p in lp.packs:
                _fill(p.d_coeff, L, MARKER)
            lp.update(hip.to_device(field))
            want = sc.expected_packs(orc, shape, mask, loss, field)
            for a, p in enumerate(lp.packs):
                got = _phys(p.d_coeff, L)
                assert (exposed[a] & near).any() == cavity
                _same(got, np.where(exposed[a], want[a].coeff, MARKER), ('update', 'cavity', cavity, 'axis', a))
                assert (got[16:32, 16:32, 32:48] == MARKER).all()            # the whole of brick (1, 1, 2)
        if cavity:                                                           # the cavity's neighbours followed the field
            old = sc.expected_packs(orc, shape, mask, loss, T)
            assert all((old[a].coeff[exposed[a] & near] != want[a].coeff[exposed[a] & near]).all() for a in range(3))


# ---- 3. deposition on a multi-brick head with everything on -----------------------------------------------------------------
F_BAR = 1e-10 * sc.HEAD['Ts'] / (sc.HEAD['law'][2] - sc.HEAD['law'][1])


@pytest.mark.parametrize('phys', [None, (32, 32, 48)], ids=['picked', 'padded'])
def test_run_layer_birth_on_a_head_of_three_bricks(mods, monkeypatch, phys):
    """waam.run_layer_birth, births on planes 15 and 30 among them, surface loss and latent heat on, segments on the graph
    path and on the step-by-step one, against the same event loop over the oracle (tests/seam_cases.py: head_oracle)"""
    hip, orc = mods
    from adi_thermal_fields_amd import waam
    _force(monkeypatch, hip, phys)
    c = sc.HEAD
    full, layers, tb, t_out, nsubs = sc.head_plan(waam)
    assert hip.Layout(*c['shape']).padded == (phys is not None)
    assert max(nsubs) >= waam.GRAPH_MIN_NSUB and min(nsubs) < waam.GRAPH_MIN_NSUB, nsubs
    assert (15, 17) in layers and (30, 32) in layers
    want = sc.head_oracle(orc, waam, hip.SurfaceLoss, hip.PhaseChange)
    loss, law = hip.SurfaceLoss(h=c['h'], emissivity=c['emissivity']), hip.PhaseChange(*c['law'])
    got, nsteps, got_f = waam.run_layer_birth(hip, full, DX, (RHO, CP, K), 0.0, TINF, c['Ts'], c['theta'], c['cfl'], layers, tb,
                                              t_out, surface_loss=loss, phase_change=law)
    eT, ef = rel_linf(got, want['T']), float(np.abs(got_f - want['f']).max())
    print('run_layer_birth on 20 x 18 x 40 (%s): %d steps, T rel L-inf %.3e, |df| %.3e (bar %.3e)'
          % ('padded' if phys else 'picked', nsteps, eT, ef, F_BAR))
    assert nsteps == want['steps']
    assert eT <= 1e-10 and ef <= F_BAR, (eT, ef)
    assert not got_f[~full].any()


@pytest.mark.parametrize('phys', [None, (32, 32, 48)], ids=['picked', 'padded'])
def test_phase_summary_through_births(mods, monkeypatch, phys):
    """the loop of run_layer_birth written out with adi_step_numba_coeff(surface_loss=, phase=) and sync_mask, two steps per
    layer: after every birth the newborn cells hold f_eq(T_birth) and every other cell its f, bit for bit, and after every
    birth and every step an entry of the summary is 0 exactly when its brick holds no f"""
    hip, _ = mods
    import torch
    from adi_thermal_fields_amd import waam
    _force(monkeypatch, hip, phys)
    c = sc.HEAD
    shape = c['shape']
    full, layers, _, _, _ = sc.head_plan(waam)
    grid = hip.Grid3D(*shape, DX, np.zeros(shape, dtype=bool))
    L = grid.layout
    assert L.padded == (phys is not None) and L.pd[2] % 2 == 0 and (L.pd[2] + 15) // 16 == 3
    mat, prm = hip.Material(RHO, CP, K), hip.Params(c['cfl'] * DX * DX / KAPPA, c['theta'])
    loss, law = hip.SurfaceLoss(h=c['h'], emissivity=c['emissivity']), hip.PhaseChange(*c['law'])
    d_full, d_act = L.to_layout(full, torch.uint8), L.empty(torch.uint8, zero=True)
    grid.set_mask_device(d_act, all_solid=False)
    lp = hip.LossPacks(grid, mat, loss, TINF)
    ph = hip.PhaseField(grid, mat, law)
    T = hip.to_device(np.full(shape, TINF))
    mask = np.zeros(shape, dtype=bool)
    mixed = 0
    for n, (ks, ke) in enumerate(layers[:12]):                              # up to plane 35: all three bricks along axis 2
        f_old = np.asarray(ph.liquid_fraction)
        hip.birth_planes(T, d_act, d_full, grid, ks, ke + 1, c['Ts'])
        grid.set_mask_device(d_act, max(ks - 1, 0), min(shape[2], ke + 2), all_solid=False)
        lp.rebuild(T, ks - 1, ke + 2)
        ph.sync_mask(T)
        born = np.zeros(shape, dtype=bool)
        born[:, :, ks:ke + 1] = full[:, :, ks:ke + 1]
        born &= ~mask
        mask |= born
        assert born.any() and np.array_equal(grid.mask, mask)
        got_f = np.asarray(ph.liquid_fraction)
        assert np.array_equal(got_f, np.where(born, 1.0, f_old)), ('birth', n, int((got_f != np.where(born, 1.0, f_old)).sum()))
        s = _assert_summary(ph, 'birth %d' % n)
        for i in range(2):
            T = hip.adi_step_numba_coeff(T, grid, mat, prm, lp.packs, Tinf=TINF, surface_loss=lp, phase=ph)
            s = _assert_summary(ph, 'layer %d step %d' % (n, i))
        along = s.any(axis=(0, 1))
        mixed += int(along.any() and not along.all())
        assert not np.asarray(ph.liquid_fraction)[~mask].any()
    assert mixed > 0                                                         # zero and non-zero entries along axis 2
    assert s.any(axis=(0, 1))[2]                                             # the third brick along axis 2 holds liquid


def test_moving_source_across_plane_32_graph_and_launches(mods, monkeypatch):
    """8 steps on the padded box with the Goldak source travelling from plane 30 to plane 33, surface loss and latent heat on:
    StagedStepper.run (graph) against the lagged, corrected loop over the oracle, and bit for bit against plain launches"""
    hip, orc = mods
    want = sc.segment_oracle(orc, hip.SurfaceLoss, hip.PhaseChange, hip.GoldakSource)
    grid = _grid(monkeypatch, hip, 'S1p')
    c = sc.SEGMENT
    mat, prm = hip.Material(RHO, CP, K), hip.Params(want['dt'], c['theta'])
    loss, law = hip.SurfaceLoss(h=sc.HEAD['h'], emissivity=sc.HEAD['emissivity']), hip.PhaseChange(*sc.HEAD['law'])
    src = sc.segment_source(hip.GoldakSource)
    lp = hip.LossPacks(grid, mat, loss, TINF)
    ph = hip.PhaseField(grid, mat, law, T=hip.to_device(want['T0']))
    st = hip.StagedStepper(grid, mat, prm, lp.packs, TINF, source=src, surface_loss=lp, phase=ph)
    res = {}
    for graph in (True, False):
        ph.seed(hip.to_device(want['T0']))
        T = st.run(hip.to_device(want['T0']), c['nsteps'], graph=graph, t0=0.0)
        res[graph] = (np.asarray(T), np.asarray(ph.liquid_fraction))
        _assert_summary(ph, 'graph' if graph else 'launches')
    assert st.captures == 1
    eT, ef = rel_linf(res[True][0], want['T']), float(np.abs(res[True][1] - want['f']).max())
    print('source across plane 32: T rel L-inf %.3e, |df| %.3e (bar %.3e)' % (eT, ef, F_BAR))
    assert eT <= 1e-10 and ef <= F_BAR, (eT, ef)
    _same(res[True][0], res[False][0], 'T, graph against launches')
    _same(res[True][1], res[False][1], 'f, graph against launches')
    assert np.array_equal(res[True][0][~want['mask']], want['T0'][~want['mask']])


# ---- 4. the laws at their branch points -----------------------------------------------------------------------------------
@pytest.mark.parametrize('lawname', ['usual', 'narrow', 'ratio'])
@pytest.mark.parametrize('box', ['S3', 'solid'])
def test_latent_heat_on_every_comparison(mods, lawname, box):
    """(T*, f) pairs on H == Hs, H == Hl, T* == Ts, T* == Tl and one and two ulp either side, with f = -0.0, a denormal, values
    outside [0, 1]: one correction and the seed against PhaseChange.correct / f_eq, bit for bit, signs of zeros included"""
    hip, _ = mods
    law = dict(sc.branch_laws(hip.PhaseChange))[lawname]
    cp = sc.CP_BRANCH
    mask, dm, Tstar, f = sc.branch_inputs(law, box)
    shape = mask.shape
    grid = hip.Grid3D(*shape, DX, mask)
    L = grid.layout
    if box == 'S3':
        sc.assert_layout('S3', L)                                            # odd nz: scalar loads
    else:                                                                    # 16-byte loads, both bricks all solid
        assert not L.padded and L.pd[2] % 2 == 0 and L.pd[3] % 2 == 0 and _brick_bit(grid, 0, 0, 0) and _brick_bit(grid, 0, 0, 1)
    mat = hip.Material(RHO, cp, K)
    ph = hip.PhaseField(grid, mat, law, dir_mask=dm)
    ph.set_liquid_fraction(f)
    loaded = np.asarray(ph.liquid_fraction)
    assert np.array_equal(loaded, f) and np.array_equal(np.signbit(loaded), np.signbit(f))
    _assert_summary(ph, 'load')
    T = hip.to_device(Tstar)
    ph.apply(T)
    want_T, want_f = law.correct(Tstar, f, mask, dm, cp)
    got_T, got_f = np.asarray(T), np.asarray(ph.liquid_fraction)
    what = (lawname, box, sc.branch_census(law, mask, dm, Tstar, f))
    _same(got_T, want_T, ('T',) + what)
    _same(got_f, want_f, ('f',) + what)
    _same(np.signbit(got_f), np.signbit(want_f), ('sign of f',) + what)
    _same(np.signbit(got_T), np.signbit(want_T), ('sign of T',) + what)
    _assert_summary(ph, 'apply')
    ph.seed(hip.to_device(Tstar))
    want_f = law.f_eq(Tstar) * mask
    got_f = np.asarray(ph.liquid_fraction)
    _same(got_f, want_f, ('seed',) + what)
    _same(np.signbit(got_f), np.signbit(want_f), ('sign of the seed',) + what)
    _assert_summary(ph, 'seed')


@pytest.mark.parametrize('name,table,T_offset', sc.KNOT_CASES, ids=[c[0] for c in sc.KNOT_CASES])
def test_surface_loss_on_every_knot(mods, monkeypatch, name, table, T_offset):
    """temperatures on every knot of a 2-knot and a 16-knot table, one ulp either side and beyond both ends; the table off on
    'x-' and on elsewhere: both modes against the oracle fed with h_of, bit for bit"""
    hip, orc = mods
    grid = _grid(monkeypatch, hip, 'S3')
    L = grid.layout
    shape, mask = sc.BOXES['S3'][0], sc.mask_of('S3')
    mat, loss = hip.Material(RHO, CP, K), sc.knot_loss(hip.SurfaceLoss, table, T_offset)
    T = sc.tile(sc.knot_temperatures(table), shape)
    d_T = hip.to_device(T)
    lp = hip.LossPacks(grid, mat, loss, TINF, T=d_T)
    want = sc.expected_packs(orc, shape, mask, loss, T)
    for a, p in enumerate(lp.packs):
        _same(p.coeff, want[a].coeff, (name, 'rebuild', 'axis', a))
        _fill(p.d_coeff, L, MARKER)
    lp.update(d_T)
    for a, p in enumerate(lp.packs):
        _same(_phys(p.d_coeff, L), np.where(sc.exposed_along(mask, a), want[a].coeff, MARKER), (name, 'update', 'axis', a))
