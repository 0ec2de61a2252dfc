"""CPU: the preconditions of tests/test_history_seams_gpu.py, from the definition (ThermalHistory.record_reference /
seed_reference), the pinned C oracle and the layout rules of the library alone.  The GPU tests compare the recorder with the
definition on inputs built in tests/history_seam_cases.py; here those inputs are shown to reach what they are aimed at -- grids
with set and clear bricks side by side, a clear brick in the second summary word next to a set one in the first, a non-empty
class of cells for every comparison of the kernel, a summary bit that goes 0 -> 1 during the births, crossings after step 300 --
so that none of the GPU tests can pass vacuously.  Also here: the precondition waam.run_single_track now enforces."""
import math
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
import history_cases as hc  # noqa: E402
import history_seam_cases as hs  # noqa: E402
import seam_cases as sc  # noqa: E402
from history_seam_cases import CP, DX, FACES, K, RHO, TINF  # noqa: E402

TH = hip.ThermalHistory


def _layout(name):
    shape, phys = sc.BOXES[name]
    L = hip.Layout(*shape) if phys is None else hip.Layout(*shape, phys=phys)
    sc.assert_layout(name, L)
    return L


def _bricks_of(cells):
    return {tuple(int(v) // 16 for v in c) for c in cells}


# ---- the summary predictor ------------------------------------------------------------------------------------------------------
def test_predicted_summary_on_hand_made_masks():
    """the rule the GPU tests hold the downloaded summary to, on masks whose answer is plain"""
    ones = np.ones((32, 16, 32), dtype=bool)
    assert hs.predicted_bricks(ones, (32, 16, 32)).all()
    assert not hs.predicted_bricks(ones, (32, 16, 48)).any(axis=(0, 1))[1:].any()      # plane 32 of the physical box is off the mask
    m = ones.copy()
    m[16, 3, 3] = False                                 # a hole on the first plane of brick (1, 0, 0): its neighbour in brick 0
    assert np.array_equal(hs.predicted_bricks(m, (32, 16, 32)), np.array([[[False, True]], [[False, True]]]))
    m = ones.copy()
    m[17, 3, 3] = False                                 # one plane further in: brick 0 no longer sees it
    assert np.array_equal(hs.predicted_bricks(m, (32, 16, 32)), np.array([[[True, True]], [[False, True]]]))
    # the word and the bit: 35 x 3 x 4 bricks, two words per (j, k)
    assert hs.summary_word(33, 1, 1, (560, 48, 64)) == ((1 * 4 + 1) * 2 + 1, 1)
    assert hs.summary_word(1, 1, 1, (560, 48, 64)) == ((1 * 4 + 1) * 2, 1)
    w = np.zeros(24, dtype=np.uint32)
    w[11] = 2
    got = hs.summary_bits(w, (560, 48, 64))
    assert got.sum() == 1 and got[33, 1, 1]


# ---- 1. mixed bricks ------------------------------------------------------------------------------------------------------------
MIXED_SET = {'S1': 4, 'S1p': 0, 'S2': 35, 'S3': 0}     # set bricks of each box


@pytest.mark.parametrize('name', hs.MIXED)
def test_mixed_boxes_hold_set_and_clear_bricks_and_a_pool_across_them(name):
    L = _layout(name)
    shape = sc.BOXES[name][0]
    mask = sc.mask_of(name)
    bits = hs.predicted_bricks(mask, L.pd[:3])
    assert int(bits.sum()) == MIXED_SET[name], (name, np.argwhere(bits).tolist())
    if name in ('S1', 'S2'):
        # a set brick with a clear neighbour along every axis that has two bricks of the logical box
        assert bits.any() and not bits.all()
        for a in range(3):
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[a], hi[a] = slice(0, -1), slice(1, None)
            assert (bits[tuple(lo)] != bits[tuple(hi)]).any(), (name, a)
    if name == 'S2':
        assert not bits[1, 1, 1] and bits[1, 1, 2] and bits[0, 1, 1] and bits[2, 2, 3]
    if name == 'S1':
        assert np.argwhere(bits).tolist() == [[0, 1, 0], [0, 1, 2], [1, 0, 0], [1, 1, 0]]
    # the load form: S3 alone has an odd row length
    assert hs.vector_form(L.pd, 0, 0, 0, 0) == (name != 'S3')
    assert not hs.vector_form(L.pd, 1, 0, 0, 0) and not hs.vector_form(L.pd, 0, 0, 8, 0)
    # the three steps: a pool across two bricks on every axis that has two, an empty pool, crossings of both kinds
    F = hs.mixed_fields(name)
    lv = hip.HistoryLevels(*hs.LEVELS)
    states, pools, _ = hs.definition_steps(TH, lv, mask, F, hs.MIXED_T0, hs.MIXED_DT)
    assert any(hs.spans_two_bricks(p, shape) for p in pools), [hs.pool_bricks(p) for p in pools]
    assert min(p['cells'] for p in pools) == 0
    _, t_hi, t_lo = states[-1]
    assert (np.isfinite(t_hi) & np.isnan(t_lo)).any() and np.isfinite(t_lo).any() and np.isnan(t_hi[mask]).any()
    for s in states:
        assert all(np.isnan(a[~mask]).all() for a in s)
    # the precondition of the definition: every A is at most the peak
    for n, A in enumerate(F[:-1]):
        assert (A[mask] <= states[n][0][mask]).all(), n
    # the selection of the last seed: single cells on the seam planes, on both sides of i = 16 and j = 16, in the mask
    sel = hs.seam_sel(shape) & mask
    idx = np.argwhere(sel)
    planes = [k for k in (15, 16, 31, 32) if k < shape[2]]
    assert set(idx[:, 2].tolist()) == set(planes)
    for k in planes:
        on = idx[idx[:, 2] == k]
        assert (on[:, 0] == 15).any() and (on[:, 0] == 16).any() and (on[:, 1] == 15).any() and (on[:, 1] == 16).any(), (name, k)
    seeded = TH.seed_reference(states[-1], F[-1], mask, hs.seam_sel(shape))
    assert (seeded[0][sel] == F[-1][sel]).all() and (seeded[0][sel] != states[-1][0][sel]).any()
    assert np.array_equal(seeded[1][~sel], states[-1][1][~sel], equal_nan=True) and np.isnan(seeded[1][sel]).all()


# ---- 2. rows past 512 -----------------------------------------------------------------------------------------------------------
def test_long_box_puts_a_clear_brick_in_the_second_summary_word():
    L = hip.Layout(*hs.LONG_SHAPE)
    px, py, pz, sx = L.pd
    nbx, nbz = (px + 15) // 16, (pz + 15) // 16
    assert nbx > 32 and (nbx + 31) // 32 == 2
    far, near = hs.LONG_FAR, hs.LONG_NEAR
    # the far brick lies inside the physical box and is an inner brick of it (the skip of k_surface_loss applies)
    assert 16 * (far[0] + 1) < px and 16 * (far[1] + 1) < py and 16 * (far[2] + 1) < pz and min(far) > 0
    assert pz % 2 == 0 and sx % 2 == 0
    for cavity in (False, True):
        mask = hs.long_mask(cavity)
        holes = np.argwhere(~mask)
        assert len(holes) == (27 if cavity else 1) and _bricks_of(holes) == {far}
        assert 528 <= holes[:, 0].min() and holes[:, 0].max() <= 543
        bits = hs.predicted_bricks(mask, L.pd[:3])
        assert not bits[far] and bits[near]
        assert hs.summary_word(*far, L.pd[:3]) == ((far[1] * nbz + far[2]) * 2 + 1, far[0] - 32)
        assert hs.summary_word(*near, L.pd[:3]) == ((far[1] * nbz + far[2]) * 2, near[0])
        assert far[0] - 32 == near[0]                   # the same bit of neighbouring words: a lookup without i / 512 hits `near`
        # every other brick that lies inside the logical box and off its faces is set
        inner = bits[:, :, :hs.LONG_SHAPE[2] // 16 - 1]
        assert int((~inner).sum()) == 1
    # the recorded steps: a pool in both bricks in the first, none in the second, crossings of one level and of both
    mask = hs.long_mask(False)
    F = hs.long_fields()
    lv = hip.HistoryLevels(*hs.LEVELS)
    states, pools, _ = hs.definition_steps(TH, lv, mask, F, hs.LONG_T0, hs.LONG_DT)
    for b in (far, near):
        cells = hs.brick_cells(b, hs.LONG_SHAPE)
        assert (F[1][cells & mask] >= hs.LEVELS[2]).all()
        assert np.isfinite(states[-1][1][cells & mask]).any() and np.isfinite(states[-1][2][cells]).any()
        assert (np.isfinite(states[-1][1]) & np.isnan(states[-1][2]) & cells).any()
    assert pools[0]['cells'] > 0 and pools[0]['lo'][0] // 16 < 1 < 33 < pools[0]['hi'][0] // 16 + 1 and pools[1]['cells'] == 0
    assert all(np.isnan(s[hs.LONG_HOLE]) for s in states[-1])
    # the latent-heat step starts above the liquidus in both bricks and solid elsewhere
    law = hip.PhaseChange(*hs.LONG_LAW)
    f0 = law.f_eq(hs.long_melt_field())
    assert (f0[hs.brick_cells(far, hs.LONG_SHAPE)] == 1.0).all() and (f0[hs.brick_cells(near, hs.LONG_SHAPE)] == 1.0).all()
    assert (f0 == 0.0).any()


def test_long_box_cavity_exposes_cells_of_the_far_brick_only():
    """the oracle's packs for the cavity variant: the cells the cavity exposes exist, lie in brick (33, 1, 1), and carry
    coefficients that follow the field"""
    shape = hs.LONG_SHAPE
    mask = hs.long_mask(True)
    loss = sc.loss5(hip.SurfaceLoss)
    T = sc.field_of(shape)
    packs = sc.expected_packs(orc, shape, mask, loss, T)
    inner = np.zeros(shape, dtype=bool)
    inner[1:-1, 1:-1, 1:-1] = True
    for a, p in enumerate(packs):
        ex = sc.exposed_along(mask, a)
        assert np.array_equal(p.coeff != 0.0, ex), a
        assert not (p.coeff == sc.MARKER).any()
        near_cavity = ex & inner
        assert int(near_cavity.sum()) == 18 and _bricks_of(np.argwhere(near_cavity)) == {hs.LONG_FAR}, a
        assert len(np.unique(p.coeff[near_cavity])) > 1
        assert not ex[hs.brick_cells(hs.LONG_NEAR, shape)].any()


# ---- 3. every comparison at its edge --------------------------------------------------------------------------------------------
EDGE_CLASSES = ['A_below_hi', 'A_on_hi', 'A_above_hi', 'B_below_hi', 'B_on_hi', 'B_above_hi', 'A_below_lo', 'A_on_lo',
                'A_above_lo', 'B_below_lo', 'B_on_lo', 'B_above_lo', 'B_below_peak', 'B_on_peak', 'B_above_peak', 'B_below_melt',
                'B_on_melt', 'B_above_melt', 'fraction_one', 'both_crossings', 'A_inf', 'B_nan', 'A_nan']


def _edge_run(which):
    levels = hs.EDGE_LEVELS[which]
    lv = hip.HistoryLevels(*levels)
    A, B = hs.edge_fields(which)
    mask = np.ones(hs.EDGE_SHAPE, dtype=bool)
    seed = TH.seed_reference(hc.empty_state(hs.EDGE_SHAPE), A, mask)
    with np.errstate(all='ignore'):
        state, pool = TH.record_reference(seed, A, B, mask, hs.EDGE_T0, hs.EDGE_DT, lv)
    return levels, A, B, seed, state, pool


@pytest.mark.parametrize('which', list(hs.EDGE_LEVELS))
def test_edge_table_holds_every_class_in_both_bricks(which):
    levels, A, B, seed, state, pool = _edge_run(which)
    hi, lo, melt = levels
    c = hs.edge_classes(A, B, levels)
    names = EDGE_CLASSES + (['B_neg_zero', 'A_neg_zero'] if which == 'zero' else [])
    for nm in names:
        for b in (0, 1):
            part = c[nm][:, :, 16 * b:16 * b + 16]
            assert part[:, :, 0::2].any() and part[:, :, 1::2].any(), (which, nm, b)      # both cells of a thread's pair
    peak, t_hi, t_lo = state
    t_n, dt = hs.EDGE_T0, hs.EDGE_DT
    # what the definition makes of them: `<=` and `>` as written, one comparison each
    assert np.isnan(t_hi[c['A_on_hi']]).all() and np.isnan(t_hi[c['A_below_hi']]).all()
    on = c['A_above_hi'] & (B <= hi)
    assert on.any() and np.isfinite(t_hi[on]).all()
    assert np.isfinite(t_hi[c['B_on_hi']]).all() and np.isfinite(t_hi[c['B_below_hi']]).all() and np.isnan(t_hi[c['B_above_hi']]).all()
    assert np.isfinite(t_lo[c['B_on_lo']]).all() and np.isfinite(t_lo[c['B_below_lo']]).all() and np.isnan(t_lo[c['B_above_lo']]).all()
    assert np.isnan(t_lo[c['A_on_lo']]).all() and np.isnan(t_lo[c['A_below_lo']]).all()
    assert (t_hi[c['fraction_one']] == t_n + dt).all()
    both = c['both_crossings'] & np.isfinite(A)
    assert np.isfinite(t_hi[both]).all() and np.isfinite(t_lo[both]).all() and (t_lo[both] >= t_hi[both]).all()
    assert (t_lo[both] > t_hi[both]).any()
    assert np.isnan(t_hi[c['A_inf']]).all() and np.isinf(peak[c['A_inf']]).all()       # inf / inf: a crossing at an unknown time
    assert hs.same_bits(peak[c['B_nan']], A[c['B_nan']]) and np.isnan(t_hi[c['B_nan']]).all()
    assert np.isnan(peak[c['A_nan']]).all() and np.isnan(t_hi[c['A_nan']]).all() and np.isnan(t_lo[c['A_nan']]).all()
    assert (peak[c['B_above_peak']] == B[c['B_above_peak']]).all() and (peak[c['B_on_peak']] == A[c['B_on_peak']]).all()
    assert (peak[c['B_below_peak']] == A[c['B_below_peak']]).all()
    # the pool: `>=`
    want = int((B >= melt).sum())
    assert pool['cells'] == want and c['B_on_melt'].sum() > 0 and want < int((B >= hs.dn(melt)).sum())
    assert want > int((B > melt).sum())
    assert pool['lo'][2] < 16 <= pool['hi'][2]
    # every cell keeps the precondition (the seed is A)
    assert hs.same_bits(seed[0], A)


def test_the_two_edge_runs_differ_where_they_are_meant_to():
    _, A1, B1, _, s1, p1 = _edge_run('usual')
    levels, A2, B2, _, s2, p2 = _edge_run('zero')
    assert levels[0] == 0.0 and levels[2] == 0.0
    c1, c2 = hs.edge_classes(A1, B1, hs.EDGE_LEVELS['usual']), hs.edge_classes(A2, B2, levels)
    # -0.0 meets T_hi = 0.0 and T_melt = 0.0 in the second run only: it is a crossing (B <= T_hi) and a pool cell (B >= T_melt)
    nz = c2['B_neg_zero'] & (A2 > 0.0)
    assert nz.any() and np.isfinite(s2[1][nz]).all() and (s2[1][nz] == hs.EDGE_T0 + hs.EDGE_DT).all()
    assert (B2[nz] >= levels[2]).all() and p2['cells'] >= int(nz.sum())
    nz1 = c1['B_neg_zero'] & (A1 > 0.0)
    assert nz1.any() and np.isnan(s1[1][nz1]).all()
    # the sign of a zero peak is the seed's: B = 0.0 is not above a peak of -0.0, nor -0.0 above 0.0
    for s, A, B in ((s1, A1, B1), (s2, A2, B2)):
        z = (A == 0.0) & (B == 0.0)
        assert (np.signbit(A[z]) != np.signbit(B[z])).any()
        assert np.array_equal(np.signbit(s[0][z]), np.signbit(A[z]))
    assert not hs.same_bits(np.array([0.0]), np.array([-0.0])) and hs.same_bits(np.array([np.nan, 1.0]), np.array([-np.nan, 1.0]))
    assert p1['cells'] != p2['cells']


def test_vote_inputs_hold_one_crossing_in_the_second_brick():
    lv = hip.HistoryLevels(*hs.LEVELS)
    mask = np.ones(hs.EDGE_SHAPE, dtype=bool)
    for bump in (False, True):
        A, B = hs.vote_fields(bump)
        seed = TH.seed_reference(hc.empty_state(hs.EDGE_SHAPE), A, mask)
        state, _ = TH.record_reference(seed, A, B, mask, 0.0, 0.5, lv)
        found = np.argwhere(np.isfinite(state[2]))
        assert found.tolist() == ([list(hs.VOTE_CELL)] if bump else [])
        assert not (seed[0][:, :, :16] > hs.LEVELS[1]).any() and (seed[0][:, :, 16:] > hs.LEVELS[1]).sum() == int(bump)
    assert hs.VOTE_CELL[2] >= 16


# ---- 5. births across the seams -------------------------------------------------------------------------------------------------
def test_births_flip_summary_bits_and_cool_through_the_levels():
    c = hs.BIRTH
    shape, phys = sc.BOXES[c['box']]
    L = _layout(c['box'])
    layers, masks = hs.birth_layers(), hs.birth_masks()
    assert layers[0] == (0, 14) and layers[1] == (14, 18) and (30, 32) in layers and (32, 34) in layers and layers[-1][1] == shape[2]
    assert masks[-1].all()
    bits = [hs.predicted_bricks(m, L.pd[:3]) for m in masks]
    assert not bits[0].any()
    flips = [n for n in range(1, len(bits)) if (bits[n] & ~bits[n - 1]).any()]
    assert flips == [1, layers.index((32, 34))], flips                 # brick (0, 0, 0) after planes 14..17, (0, 0, 1) after 32..33
    assert bits[1][0, 0, 0] and bits[-1][0, 0, 1] and int(bits[-1].sum()) == 2
    assert flips[-1] < len(layers) - 1                                  # steps are recorded after the last flip
    # the loop over the oracle, one step per layer: cells cross both levels and the pool is never empty nor the whole body
    lv = hip.HistoryLevels(*c['levels'])
    grid, mat = orc.Grid3D(*shape, DX, np.zeros(shape, dtype=bool)), orc.Material(RHO, CP, K)
    prm = orc.Params(hs.birth_dt(), c['theta'])
    T, mask, state, t = np.full(shape, TINF), np.zeros(shape, dtype=bool), hc.empty_state(shape), 0.0
    for n, m in enumerate(masks):
        newborn = m & ~mask
        T = np.where(newborn, c['Ts'], T)
        state = TH.seed_reference(state, T, m, newborn)
        mask = m
        grid.mask = mask.copy()
        packs = orc.precompute_coeff_packs_unified(grid, mat, robin_h={f: c['h'] for f in FACES})
        Tn = orc.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=TINF)
        state, pool = TH.record_reference(state, T, Tn, mask, t, prm.dt, lv)
        t, T = t + prm.dt, Tn
        assert 0 < pool['cells'] < int(mask.sum()), n
    assert np.isfinite(state[2]).sum() > 1000 and (np.isfinite(state[1]) & np.isnan(state[2])).any()


def test_head_plan_of_the_layer_birth_run():
    full, layers, tb, t_out, sched, dt_cap, nsubs = hs.head_plan(waam)
    assert full.shape == (20, 18, 40) and all(ke - ks == 1 for ks, ke in layers) and len(layers) == 20
    assert (14, 15) in layers and (16, 17) in layers and (30, 31) in layers and (32, 33) in layers
    assert max(nsubs) < waam.GRAPH_MIN_NSUB and sum(nsubs) <= 64, nsubs       # few sub-steps: every segment step by step
    assert not hip.Layout(*full.shape).padded
    # the event loop over the oracle: a pool, crossings of both levels in the third brick along axis 2, cells that never cross
    c = hs.HEAD
    shape = full.shape
    lv = hip.HistoryLevels(*c['levels'])
    mask = np.zeros(shape, dtype=bool)
    grid, mat = orc.Grid3D(*shape, DX, mask.copy()), orc.Material(RHO, CP, K)
    T, state, t, pools = np.full(shape, TINF), hc.empty_state(shape), 0.0, []
    for what, arg in sched:
        if what == 'advance' and mask.any():
            nsub = max(1, int(math.ceil(arg / dt_cap)))
            prm = orc.Params(arg / nsub, c['theta'])
            packs = orc.precompute_coeff_packs_unified(grid, mat, robin_h={f: c['h'] for f in FACES})
            for _ in range(nsub):
                Tn = orc.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=TINF)
                state, pool = TH.record_reference(state, T, Tn, mask, t, prm.dt, lv)
                t, T = t + prm.dt, Tn
                pools.append(pool)
        elif what == 'birth':
            ks, ke = layers[arg]
            old = mask.copy()
            mask[:, :, ks:ke + 1] |= full[:, :, ks:ke + 1]
            T = np.where(mask & ~old, c['Ts'], T)
            state = TH.seed_reference(state, T, mask, mask & ~old)
            grid.mask = mask.copy()
    assert len(pools) == sum(nsubs[1:]) and max(p['cells'] for p in pools) > 100 and min(p['cells'] for p in pools) == 0
    third = full.copy()
    third[:, :, :32] = False
    assert np.isfinite(state[1][third]).sum() > 100 and np.isfinite(state[2][third]).any()
    assert np.isnan(state[1][full]).any() and (np.isfinite(state[1]) & np.isnan(state[2])).any()


# ---- 6. a long run through the graph ----------------------------------------------------------------------------------------------
def test_long_run_still_crosses_both_levels_after_step_300():
    c = hs.LONG_RUN
    mask, T0, dt = hs.long_run_inputs()
    assert c['steps'] % 2 == 1 and c['steps'] // 2 == 200                  # 200 replays of the two-step graph and a tail step
    grid, mat, prm = orc.Grid3D(*c['shape'], DX, mask), orc.Material(RHO, CP, K), orc.Params(dt, c['theta'])
    packs = orc.precompute_coeff_packs_unified(grid, mat, robin_h={f: c['h'] for f in FACES})
    traj = [T0]
    for _ in range(c['steps']):
        traj.append(orc.adi_step_numba_coeff(traj[-1], grid, mat, prm, packs, Tinf=TINF))
    lv = hip.HistoryLevels(*hs.LEVELS)
    case = dict(shape=c['shape'], mask=mask, segments=[(dt, c['steps'], None)])
    states, pools, times, t_end = hc.record_trajectory(TH, lv, case, traj, t=c['t0'], clock='run')
    late_hi, late_lo = hs.late_crossings(states, c['late'])
    assert late_hi > 100 and late_lo > 100, (late_hi, late_lo)
    assert pools[0]['cells'] > 0 and pools[-1]['cells'] == 0 and pools[0]['lo'][2] < 16 <= pools[0]['hi'][2]
    # the clock of a run is t0 + n*dt, not a running sum: the two differ in the last bits by step 401
    run, acc = c['t0'] + 400 * dt, c['t0']
    for _ in range(400):
        acc = acc + dt
    assert times[-1] == c['t0'] + 401 * dt and run != acc


# ---- 7. the precondition in run_single_track --------------------------------------------------------------------------------------
def test_run_single_track_refuses_a_recorder_when_the_track_dips_into_the_plate():
    shape, dx = (10, 9, 8), 1e-3
    plate = np.zeros(shape, dtype=bool)
    plate[:, :, :4] = True
    lv = hip.HistoryLevels(*hs.LEVELS)
    args = (dx, (RHO, CP, K), 10.0, 25.0, 1500.0, 0.5, 0.02, 0.4)
    for box in ((3, 7, 3, 7, 3), (3, 7, 0, 2, 1)):                       # one plane into the plate; wholly inside it
        with pytest.raises(ValueError, match='overlaps the plate.*recorder would miss'):
            waam.run_single_track(hip, plate, box, *args, history=lv)
    # columns beyond the track's length do not count, nor does a plate outside the box; without a recorder nothing changes
    class Reached(Exception):
        pass

    class Backend:
        @staticmethod
        def Grid3D(*a):
            raise Reached

    far = plate.copy()
    far[3:7, 5:, 4:7] = True
    for p, box, h in ((plate, (3, 7, 4, 7, 3), lv), (far, (3, 7, 4, 7, 3), lv), (plate, (3, 7, 3, 7, 3), None)):
        with pytest.raises(Reached):
            waam.run_single_track(Backend, p, box, *args, history=h)
