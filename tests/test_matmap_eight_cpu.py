"""CPU: the conditions that keep tests/test_matmap_eight_gpu.py honest, each checked from the definition (MaterialMap.step_reference /
packs_reference / pair_table_of, NumPy fp64) and the extended-precision reference tests/matmap_ref_ld.py alone: the eight materials
are told apart by every table entry, the definition meets the bar on every case, every ordered pair of ids occurs where a kernel
could lose it, the mistakes an eight-wide table invites miss the bar by orders of magnitude, and the id pattern of the latent-heat
test reaches every branch of every law.  Cases, metric and bar: tests/matmap_eight_cases.py.  No GPU."""
import numpy as np
import pytest

import matmap_eight_cases as ec
import matmap_extras_cases as xc
from adi_thermal_fields_amd.packs import MaterialMap

UNIQUE = ec.unique_cases(ec.keys())
UNIQUE_EIGHT = ec.unique_cases(ec.eight_keys())


def _definition(c, **kw):
    return ec.run(MaterialMap.step_reference, MaterialMap.packs_reference, c, **kw)


# ---- the materials ------------------------------------------------------------------------------------------------------------------
def _min_gap(values):
    v = np.sort(np.asarray(values, dtype=np.float64).ravel())
    return float(np.min(np.diff(v) / v[1:]))


def test_every_table_entry_tells_the_eight_materials_apart():
    assert ec.MATERIALS8[:3] == ec.mc.MATERIALS and ec.ALPHA_MAX == ec.mc.ALPHA_MAX
    assert ec.ALPHA_MAX == ec.mc.COPPER[2] / (ec.mc.COPPER[0] * ec.mc.COPPER[1])
    for dt in (1e-3, ec.case(ec.eight_keys()[0])['dt'], ec.case(ec.eight_keys()[3])['dt']):
        G = MaterialMap.pair_table_of(ec.MATERIALS8, ec.DX, dt)
        assert G.shape == (8, 8) and (G > 0).all()
        print('dt %.3e: smallest relative gap among the 64 pair-table entries %.2e' % (dt, _min_gap(G)))
        assert _min_gap(G) >= ec.MIN_GAP
    C = [rho * cp for rho, cp, _ in ec.MATERIALS8]
    print('smallest relative gap among the eight C %.2e' % _min_gap(C))
    assert _min_gap(C) >= ec.MIN_GAP


def test_the_case_lists_are_the_ones_the_kernels_switches_ask_for():
    assert len(ec.eight_keys()) == 8 + 12 + 6 and len(ec.switch_keys()) == 66
    for fam, shape, layout, axis, theta, cfl in ec.switch_keys():
        n = shape[axis]
        others = [s for a, s in enumerate(shape) if a != axis]
        assert all(s % 2 == 1 and s % 8 != 0 and s <= 21 for s in others), shape
        if n <= 33:
            assert others[0] * others[1] >= 300, shape
        # the lines a tile or a wave takes together: adjacent lines along the contiguous direction (axes 0 and 1), lines of the
        # box (axis 2); an odd count is a multiple of no tile (8 .. 256 lines) and of no 64 / Lp > 1
        lines = others[0] * others[1] if axis != 1 else shape[2]
        assert lines % 2 == 1, shape
    assert {k[1][k[3]] for k in ec.switch_keys() if k[3] < 2} == set(ec.SWITCH_LENGTHS[0])
    assert {k[1][2] for k in ec.switch_keys() if k[3] == 2} == set(ec.SWITCH_LENGTHS[2])
    for key in UNIQUE:
        c = ec.case(key)
        assert c['ids'].max() == 7 or c['ids'].size < 64
        assert c['materials'] is ec.MATERIALS8 and c['mask'].shape == key[1]


# ---- the definition meets the bar ------------------------------------------------------------------------------------------------------
def test_definition_meets_the_bar_on_every_case():
    worst = 0.0
    for key in UNIQUE:
        c = ec.case(key)
        ok, f = ec.meets_bar(_definition(c), c, ec.reference(key))
        share = f['abs_err'] / ec.bar(f, ec.A_MAP)
        print('%-60s err %.2e K = %6.2f ulp = %.1e of the bar' % (ec.tag(key), f['abs_err'], f['ulp'], share))
        worst = max(worst, share)
        assert ok, (ec.tag(key), f)
    print('worst: %.2e of the bar' % worst)


# ---- pair coverage ----------------------------------------------------------------------------------------------------------------------
def test_every_ordered_pair_of_ids_occurs_along_each_axis():
    keys = [k for k in UNIQUE if k[0] == 'eight' or max(k[1]) >= 128]
    assert len(keys) >= 20 + 24
    for key in keys:
        c = ec.case(key)
        counts = [ec.pair_counts(c, axis) for axis in range(3)]
        print('%-60s fewest occurrences of a pair along axis 0, 1, 2: %s' % (ec.tag(key), [int(n.min()) for n in counts]))
        for axis in range(3):
            assert counts[axis].shape == (64,) and counts[axis].min() >= 8, (ec.tag(key), axis)


def test_every_ordered_pair_occurs_in_both_halves_of_a_16_row_segment():
    keys = [k for k in UNIQUE if k[1] in ec.mc.ROWS16 or (k[0] == 'switch' and k[1][k[3]] in (513, 1024))]
    assert len(keys) == 6 + 12
    for key in keys:
        c = ec.case(key)
        axis = int(np.argmax(key[1]))
        halves = [ec.pair_counts(c, axis, half) for half in (0, 1)]
        print('%-60s fewest in rows r %% 16 < 8: %d, >= 8: %d' % (ec.tag(key), halves[0].min(), halves[1].min()))
        assert halves[0].min() >= 1 and halves[1].min() >= 1, ec.tag(key)
        assert np.array_equal(halves[0] + halves[1], ec.pair_counts(c, axis))


# ---- mutants ----------------------------------------------------------------------------------------------------------------------------
LOW2 = np.arange(8) & 3


def _rows_and_3(G):
    return G[LOW2, :]


def _columns_and_3(G):
    return G[:, LOW2]


def _both_and_3(G):
    return G[np.ix_(LOW2, LOW2)]


def _transposed(G):
    return G.T.copy()


@pytest.mark.parametrize('mutant', [_rows_and_3, _columns_and_3, _both_and_3, _transposed],
                         ids=['G[m&3][n]', 'G[m][n&3]', 'G[m&3][n&3]', 'G[n][m]'])
def test_mutants_of_the_pair_table_exceed_the_bar(monkeypatch, mutant):
    real = MaterialMap.pair_table_of
    worst = np.inf
    for key in UNIQUE_EIGHT:
        c = ec.case(key)
        monkeypatch.setattr(MaterialMap, 'pair_table_of', staticmethod(lambda *a: mutant(real(*a))))
        ok, f = ec.meets_bar(_definition(c), c, ec.reference(key))
        monkeypatch.setattr(MaterialMap, 'pair_table_of', staticmethod(real))
        times = f['abs_err'] / ec.bar(f, ec.A_MAP)
        print('%-12s %-55s %.2e K = %.1e times the bar' % (mutant.__name__, ec.tag(key), f['abs_err'], times))
        worst = min(worst, times)
        assert not ok and times >= 100.0, (ec.tag(key), f)
    print('the mildest: %.1e times the bar' % worst)


def test_a_source_divided_by_the_wrong_materials_C_exceeds_the_bar():
    """S / C[id & 3] in place of S / C[id]: the definition run on the field S C[id] / C[id & 3], which it divides by C[id]"""
    C = np.array([rho * cp for rho, cp, _ in ec.MATERIALS8])
    worst = np.inf
    for key in UNIQUE_EIGHT:
        c = ec.case(key)
        S = ec.source_field(key)
        ref = ec.reference_of(c, S=S)
        ok, f = ec.meets_bar(_definition(c, S=S), c, ref)
        assert ok, (ec.tag(key), f)
        ids = c['ids'].astype(np.intp)
        ok, f = ec.meets_bar(_definition(c, S=S * (C[ids] / C[ids & 3])), c, ref)
        times = f['abs_err'] / ec.bar(f, ec.A_MAP)
        print('S / C[id & 3]  %-55s %.2e K = %.1e times the bar' % (ec.tag(key), f['abs_err'], times))
        worst = min(worst, times)
        assert not ok and times >= 100.0, (ec.tag(key), f)
    print('the mildest: %.1e times the bar' % worst)


# ---- bricks8 ----------------------------------------------------------------------------------------------------------------------------
def test_bricks8_reaches_every_branch_of_every_law_and_every_kind_of_brick():
    mask, ids = ec.bricks8()
    laws = xc.laws_of(ec.MATERIALS8)
    assert len(laws) == 8 and laws[:3] == xc.LAWS
    without = [m for m, law in enumerate(laws) if law is None]
    assert len(without) >= 2 and max(m for m in range(8) if laws[m] is not None) == 7
    fl = xc.fields(mask, ids, laws)
    xc.assert_covered(fl['T_star'], fl['f0'], mask, ids, fl['dir_mask'], ec.MATERIALS8, 'bricks8')
    assert set(xc.coverage(fl['T_star'], fl['f0'], mask, ids, fl['dir_mask'], ec.MATERIALS8)) == set(range(8)) - set(without)
    words = xc.brick_words(mask, ids, ec.BRICKS_SHAPE).tolist()
    print('brick words: %s' % words)
    assert len(words) == 16 and words[:8] == [1 << b for b in range(8)]
    assert any(words[m] == 1 << m for m in without)                    # a single-material brick of a material without a law
    assert words.count(0) == 1 and words[11] == 0
    assert max(bin(w).count('1') for w in words) >= 5
    holes = [int((~mask[16 * (b // 8):16 * (b // 8) + 16, 16 * ((b // 4) % 2):16 * ((b // 4) % 2) + 16,
                        16 * (b % 4):16 * (b % 4) + 16]).sum()) for b in range(8)]
    assert sum(h == 0 for h in holes) == 4 and sum(h > 0.2 * 4096 for h in holes) == 4
    losses = xc.losses_of(ec.MATERIALS8)
    assert len(losses) == 8 and losses[:3] == xc.LOSSES and len({w.key() for w in losses}) == 8
    vals = [w.validate(xc.TINF) for w in losses]
    assert any(v[2].size and max(v[1]) > 0 for v in vals)                           # a table
    assert any(max(v[0]) == 0.0 and min(v[1]) > 0.0 and not v[2].size for v in vals)    # emissivity alone
    assert any(min(v[0]) == 0.0 for v in vals)                                      # no h on a face
