"""CPU: the preconditions of tests/test_loss_phase_seams_gpu.py, from the pinned C oracle and the NumPy definitions alone.  The GPU
tests compare the device with expected arrays on masks, plane ranges, fields and directed inputs built in tests/seam_cases.py;
here those inputs are shown to hold what they are there to catch -- a cavity on each brick border, arrays that differ from plane
to plane, a run that melts and refreezes, a table of (T*, f) pairs on every comparison of the latent-heat law, knot tables whose
clamp is observable -- so that none of the GPU tests can pass vacuously."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import adi_thermal_fields_amd.adi3d_hip_coeff as hip  # noqa: E402
from adi_thermal_fields_amd import waam  # noqa: E402
from oracle import adi_oracle as orc  # noqa: E402
import seam_cases as sc  # noqa: E402
from seam_cases import FACES  # noqa: E402


def _brick_of(cells):
    return {tuple(int(v) // 16 for v in c) for c in cells}


def test_masks_hold_cavities_on_the_brick_borders():
    m = sc.mask_of('S1')
    assert m.shape == (20, 18, 40) and np.array_equal(m, sc.mask_of('S1p'))
    holes = ~m
    for k in (0, 14, 15, 16, 17, 30, 31, 32, 39):
        assert holes[:, :, k].any(), k
    # single cells on 15 / 16 / 31 / 32 (all six neighbours in the mask) and cavities that span 15|16 and 31|32
    pad = np.pad(m, 1)
    lone = holes & np.all([pad[1 + d[0]:21 + d[0], 1 + d[1]:19 + d[1], 1 + d[2]:41 + d[2]]
                           for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))], axis=0)
    for k in (15, 16, 31, 32):
        assert lone[:, :, k].any(), k
    assert (holes[:, :, 15] & holes[:, :, 16]).any() and (holes[:, :, 31] & holes[:, :, 32]).any()
    assert holes[15, 15, 20] and holes[16, 16, 20]                         # through the brick corner of axes 0 and 1
    # every axis has cells exposed on the minus side only, the plus side only, both and neither
    for a in range(3):
        sl = lambda d: tuple(slice(1 + (d if i == a else 0), 1 + (d if i == a else 0) + m.shape[i]) for i in range(3))
        lo, hi = ~pad[sl(-1)] & m, ~pad[sl(+1)] & m
        for want in (lo & ~hi, hi & ~lo, lo & hi, m & ~lo & ~hi):
            assert want.any(), a
        assert np.array_equal(sc.exposed_along(m, a), lo | hi)
    # S2: one cavity, wholly inside brick (1, 1, 1); its exposed neighbours too
    m2 = sc.mask_of('S2')
    assert (~m2).sum() == 27 and _brick_of(np.argwhere(~m2)) == {(1, 1, 1)}
    inner = np.zeros_like(m2)
    inner[1:-1, 1:-1, 1:-1] = True
    for a in range(3):
        assert _brick_of(np.argwhere(sc.exposed_along(m2, a) & inner)) == {(1, 1, 1)}, a
    assert sc.mask_of('S2', cavity=False).all()
    # S3: a quarter of the cells are holes, in every brick that is more than one row (brick (1, 1, 1) has three cells)
    m3 = sc.mask_of('S3')
    assert 0.2 < (~m3).mean() < 0.3
    assert _brick_of(np.argwhere(~m3)) >= {(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)} - {(1, 1, 1)}


@pytest.mark.parametrize('name', ['S1', 'S3'])
def test_expected_arrays_make_a_shifted_range_visible(name):
    """the coefficient arrays differ from plane to plane and between exposed neighbours along every axis, never hold the
    marker, and every plane range of part 1 holds exposed cells of every axis (the empty one apart)"""
    shape = sc.BOXES[name][0]
    mask, T = sc.mask_of(name), sc.field_of(shape)
    loss = sc.loss5(hip.SurfaceLoss)
    xp = np.array(sc.TABLE5[0])
    assert (T[mask] < xp[0]).any() and (T[mask] > xp[-1]).any() and all(((T > a) & (T < b) & mask).any() for a, b in zip(xp, xp[1:]))
    packs = sc.expected_packs(orc, shape, mask, loss, T)
    for a, p in enumerate(packs):
        ex = sc.exposed_along(mask, a)
        c = p.coeff
        assert np.array_equal(c != 0.0, ex), a                             # zeros exactly where nothing is exposed
        assert not (c == sc.MARKER).any()
        for k in range(shape[2] - 1):
            both = ex[:, :, k] & ex[:, :, k + 1]
            assert (both.any() or a == 2) and (c[:, :, k][both] != c[:, :, k + 1][both]).all(), (a, k)
        for ax in range(3):
            n = shape[ax]
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[ax], hi[ax] = slice(0, n - 1), slice(1, n)
            both = ex[tuple(lo)] & ex[tuple(hi)]
            assert (both.any() or ax == a) and (c[tuple(lo)][both] != c[tuple(hi)][both]).all(), (a, ax)
        for k0, k1 in sc.plane_ranges(name):
            assert (k1 == k0) or ex[:, :, k0:k1].any(), (a, k0, k1)
            for k in (k0, k1):                                              # the planes either side of a range's end differ
                assert k0 == k1 or k in (0, shape[2]) or not np.array_equal(c[:, :, k - 1], c[:, :, k]), (a, k0, k1)
    ranges = sc.plane_ranges(name)
    assert (5, 5) in ranges and (0, shape[2]) in ranges and any(k0 % 16 and k1 % 16 and k0 // 16 != (k1 - 1) // 16 for k0, k1 in ranges)
    assert any(k0 >= 16 for k0, _ in ranges)                                # a range whose first brick is not brick 0


def test_births_of_part_1_change_the_exposure_and_the_fluxes():
    shape = sc.BOXES['S1p'][0]
    full = sc.mask_of('S1p')
    k0, k1 = sc.BIRTH_PLANES
    old = full.copy()
    old[:, :, k0:k1] = False
    assert old[:, :, k0 - 1].any() and full[:, :, k0:k1].any() and k0 < 16 < k1
    T = sc.field_of(shape)
    Tn = np.where(full & ~old, sc.T_BIRTH, T)
    loss, q = sc.loss5(hip.SurfaceLoss), sc.neumann_of(shape)
    before = sc.expected_packs(orc, shape, old, loss, T, neumann=q)
    after = sc.expected_packs(orc, shape, full, loss, Tn, neumann=q)
    # the rebuilt range [k0 - 1, k1 + 1) holds every change, in the coefficients and in the fluxes
    for a in range(3):
        for name in ('coeff', 'qflux'):
            b, c = getattr(before[a], name), getattr(after[a], name)
            diff = b != c
            assert not diff[:, :, :k0 - 1].any() and not diff[:, :, k1 + 1:].any(), (a, name)
    assert (before[2].coeff[:, :, k0 - 1] != after[2].coeff[:, :, k0 - 1]).any()           # the plane below was covered
    assert ((before[2].coeff != 0) & (after[2].coeff == 0)).any()                            # a stale exposure falls to zero
    assert (before[2].qflux != after[2].qflux).any() and (before[0].qflux != after[0].qflux).any()
    assert len(np.unique(after[0].qflux[after[0].qflux != 0])) > 100                         # the per-cell 'x-' array is at work


def test_deposition_run_melts_refreezes_and_is_born_on_the_brick_borders():
    full, layers, tb, t_out, nsubs = sc.head_plan(waam)
    assert full.shape == (20, 18, 40) and full.any(axis=(0, 1)).all()
    starts = [ks for ks, _ in layers]
    assert 15 in starts and 30 in starts and (15, 17) in layers and (30, 32) in layers, layers
    assert max(nsubs) >= waam.GRAPH_MIN_NSUB and min(nsubs) < waam.GRAPH_MIN_NSUB, nsubs
    r = sc.head_oracle(orc, waam, hip.SurfaceLoss, hip.PhaseChange)
    assert r['steps'] == sum(nsubs)
    assert r['f_max'] == 1.0 and r['mushy'] > 0 and r['refroze'] > 0, {k: r[k] for k in ('f_max', 'mushy', 'refroze')}
    assert r['birth_starts'] == starts
    f = r['f']
    assert ((f > 0) & (f < 1)).any()                                        # the last layers are still freezing at the end
    # the 8-step segment: the source's centre crosses plane 32, a pool with a mushy rim forms
    s = sc.segment_oracle(orc, hip.SurfaceLoss, hip.PhaseChange, hip.GoldakSource)
    assert s['centres'][0] < 32.0 < s['centres'][-1], s['centres']
    assert s['f'].max() == 1.0 and ((s['f'] > 0) & (s['f'] < 1)).any()
    assert _brick_of(np.argwhere(s['f'] > 0)) >= {(1, 0, 1), (1, 0, 2)}     # liquid on both sides of plane 32


@pytest.mark.parametrize('lawname', ['usual', 'narrow', 'ratio'])
@pytest.mark.parametrize('box', ['S3', 'solid'])
def test_branch_table_hits_every_path_of_the_correction(lawname, box):
    law = dict(sc.branch_laws(hip.PhaseChange))[lawname]
    L, Ts, Tl = law.validate()
    cp = sc.CP_BRANCH
    dT, Hs, Hl, cm = law.constants(cp)
    if lawname == 'narrow':
        assert Tl == np.nextafter(np.nextafter(Ts, np.inf), np.inf)
    if lawname == 'ratio':
        assert L == 1e9 and abs(dT - 1e-3) < 1e-12
    Tt, ft = sc.branch_table(law)
    assert set(ft.tolist()) >= {0.0, 1.0, 0.5, 5e-324} and np.signbit(ft).sum() >= 2 * len(Tt) // len(sc.F_VALUES)
    for t in (Ts, Tl):
        for n in range(-2, 3):
            v = t
            for _ in range(abs(n)):
                v = np.nextafter(v, np.inf if n > 0 else -np.inf)
            assert (Tt == v).any(), (t, n)
    mask, dm, T, f = sc.branch_inputs(law, box)
    n = sc.branch_census(law, mask, dm, T, f)
    for key in ('rest_solid', 'rest_liquid', 'solid', 'liquid', 'mushy', 'on_Hs', 'on_Hl', 'rest_on_Ts', 'rest_on_Tl',
                'neg_zero', 'outside', 'dirichlet'):
        assert n[key] > 0, (lawname, box, n)
    assert (n['off_mask'] > 0) == (box == 'S3'), n
    # every pair of the table lands on a cell the correction acts on
    act = (mask & ~dm).ravel()
    idx = np.arange(T.size) % len(Tt)
    assert len(np.unique(idx[act])) == len(Tt), (lawname, box, len(np.unique(idx[act])), len(Tt))
    # the definition leaves the cells at rest, the Dirichlet cells and the holes alone, and moves the others
    Tn, fn = law.correct(T, f, mask, dm, cp)
    keep = ~mask | dm | ((f == 0) & (T <= Ts)) | ((f == 1) & (T >= Tl))
    assert np.array_equal(Tn[keep], T[keep]) and np.array_equal(fn[keep], f[keep])
    assert np.array_equal(np.signbit(fn[keep]), np.signbit(f[keep]))
    assert (fn[~keep] >= 0).all() and (fn[~keep] <= 1).all() and not np.signbit(fn[~keep]).any()
    assert not np.isnan(Tn).any() and not np.isnan(fn).any()
    # on H == Hs the solid branch gives H / cp, the mushy one Ts + 0 / cm: different doubles where Ts is ours to choose
    on = mask & ~dm & ~keep & (cp * T + L * f == Hs)
    assert on.any() and (Tn[on] == Hs / cp).all()
    assert (Hs / cp != Ts) == (lawname != 'usual'), (lawname, Hs / cp, Ts)
    # on H == Hl the liquid branch gives (H - L) / cp and f = 1
    on = mask & ~dm & ~keep & (cp * T + L * f == Hl)
    assert on.any() and (Tn[on] == (Hl - L) / cp).all() and (fn[on] == 1.0).all()


@pytest.mark.parametrize('name,table,T_offset', sc.KNOT_CASES, ids=[c[0] for c in sc.KNOT_CASES])
def test_knot_inputs_make_the_clamp_observable(name, table, T_offset):
    loss = sc.knot_loss(hip.SurfaceLoss, table, T_offset)
    xp, fp = np.array(table[0]), np.array(table[1])
    assert len(xp) == (2 if 'knots2' in name else hip.SurfaceLoss.MAX_KNOTS)
    slopes = np.diff(fp) / np.diff(xp)
    if 'knots2' in name:
        assert abs(slopes[0] / 1e6 - 1.0) < 1e-3, slopes
    else:
        assert (slopes < 0).any() and (slopes > 0).any()
    # at the last knot the clamp and the last segment's formula are different doubles ...
    interior = fp[-2] + slopes[-1] * (xp[-1] - xp[-2])
    assert interior != fp[-1], (interior, fp[-1])
    # ... and stay different through h_f and the coefficient on at least one face that carries the table
    A, C = sc.DX * sc.DX, sc.RHO * sc.CP * sc.DX ** 3
    seen = [f for f in FACES if (sc.last_knot_doubles(loss, f, sc.TINF, False) * A / C)
            != (sc.last_knot_doubles(loss, f, sc.TINF, True) * A / C)]
    assert 'y+' in seen and 'x-' not in seen, seen
    for f in FACES:
        assert sc.last_knot_doubles(loss, f, sc.TINF, False) == loss.h_of(np.array([xp[-1]]), f, sc.TINF)[0], f
    # the table is off on 'x-' and on everywhere else; 'y-' is a black body without convection
    hs, es = loss.validate(sc.TINF)[:2]
    assert (hs[0], es[0]) == (0.0, 0.0) and all(h != 0 or e != 0 for h, e in zip(hs[1:], es[1:])) and (hs[2], es[2]) == (0.0, 1.0)
    assert np.array_equal(loss.h_of(xp, 'x-', sc.TINF), np.zeros_like(xp))
    # the tiled temperatures put every knot and both its neighbours on a cell exposed on 'y+' alone along axis 1
    shape = sc.BOXES['S3'][0]
    mask = sc.mask_of('S3')
    vals = sc.knot_temperatures(table)
    T = sc.tile(vals, shape)
    assert (vals < xp[0]).any() and (vals > xp[-1]).any() and len(np.unique(vals)) == len(vals) == 3 * len(xp) + 3
    pad = np.pad(mask, 1)
    only_plus = mask & pad[1:-1, :-2, 1:-1] & ~pad[1:-1, 2:, 1:-1]
    for a in range(3):
        ex = sc.exposed_along(mask, a)
        assert set(np.unique(T[ex]).tolist()) == set(vals.tolist()), a
    assert (T[only_plus] == xp[-1]).any()
    assert float(sc.TINF) + T_offset > 0 and (vals + T_offset > 0).all()
