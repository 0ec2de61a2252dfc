"""CPU: the cases of tests/transitions_eight_cases.py (MaterialTransitions with eight materials, changed cells placed at the brick
seams and at the ends of the box, values at the edge of `>=`).  The coverage of the cases, counted from the
definition; the conditions every shape was built for; and, for every shape, that each way the kernel could go wrong with ids 4 to 7
or at a seam -- a mutant of the definition written here -- gives another result than the definition.  No GPU (the built library is
needed for the imports)."""
import types

import numpy as np
import pytest

import transitions_eight_cases as ec
from adi_thermal_fields_amd.matmap_extras import MapPhaseField, MaterialTransitions
from adi_thermal_fields_amd.packs import MaterialMap

MUTANTS = ('target_read_at_m_and_3', 'target_cut_to_two_bits', 'ruled_cut_to_four_bits', 'threshold_read_at_m_and_3',
           'C_of_the_old_material', 'C_read_at_n_and_3', 'f_from_the_old_law', 'greater_not_greater_equal', 'dirichlet_cells_changed',
           'both_hops_in_one_pass', 'word_loses_no_bit', 'word_gains_no_bit')


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def state_after(c, rules, mutant=None):
    """ids, f, words, count and the six pack arrays after one pass, written out with the kernel's tables (target, threshold and
    `ruled` per material; 0 where there is no rule) so that each can be read wrongly: mutant None is the definition"""
    T, f0, mask, ids, dirc = c['T'], c['f0'], c['mask'], c['ids'], c['dir_mask']
    to = np.array([0 if r is None else r[0] for r in rules])
    T_at = np.array([0.0 if r is None else r[1] for r in rules])
    ruled = np.array([r is not None for r in rules])
    if mutant == 'ruled_cut_to_four_bits':
        ruled[4:] = False
    m = ids.astype(np.intp)
    target = to[m & 3 if mutant == 'target_read_at_m_and_3' else m]
    if mutant == 'target_cut_to_two_bits':
        target = target & 3
    thr = T_at[m & 3 if mutant == 'threshold_read_at_m_and_3' else m]
    hot = T > thr if mutant == 'greater_not_greater_equal' else T >= thr
    free = mask if mutant == 'dirichlet_cells_changed' else mask & ~dirc
    cells = free & ruled[m] & hot
    ids_new = np.where(cells, target, m)
    if mutant == 'both_hops_in_one_pass':
        again = cells & ruled[ids_new] & (T >= T_at[ids_new])
        ids_new = np.where(again, to[ids_new], ids_new)
    ids_new = ids_new.astype(np.uint8)
    law_ids = ids if mutant == 'f_from_the_old_law' else ids_new
    f = np.where(cells, MapPhaseField.f_eq_of(ec.LAWS, T, cells, law_ids), f0)
    C_ids = ids_new
    if mutant == 'C_of_the_old_material':
        C_ids = np.where(cells, ids, ids_new)
    if mutant == 'C_read_at_n_and_3':
        C_ids = np.where(cells, ids_new & 3, ids_new)
    packs = MaterialMap.packs_reference(mask, C_ids, ec.MATERIALS, ec.DX, **ec.bc_of(c))
    w0, w1 = ec.brick_words(mask, ids, c['shape']), ec.brick_words(mask, ids_new, c['shape'])
    words = w0 | w1 if mutant == 'word_loses_no_bit' else w0 & w1 if mutant == 'word_gains_no_bit' else w1
    return types.SimpleNamespace(ids=ids_new, f=f, words=words, count=int(cells.sum()), packs=packs)


def differs(a, b):
    """the parts of the state in which a and b differ"""
    out = [k for k in ('ids', 'words') if not np.array_equal(getattr(a, k), getattr(b, k))]
    if not _bits(a.f, b.f):
        out.append('f')
    if a.count != b.count:
        out.append('count')
    if any(not _bits(p.coeff, q.coeff) or not _bits(p.qflux, q.qflux) for p, q in zip(a.packs, b.packs)):
        out.append('packs')
    return out


def test_the_rules_are_what_the_cases_say():
    r = MaterialTransitions._checked_rules(ec.RULES8, 8)
    ruled = [m for m, x in enumerate(r) if x is not None]
    to = {m: r[m][0] for m in ruled}
    at = {m: r[m][1] for m in ruled}
    assert any(m < 4 for m in ruled) and any(m >= 4 for m in ruled)
    assert any(n < 4 for n in to.values()) and any(n >= 4 for n in to.values())
    assert any(m >= 4 and n >= 4 and m & 3 != n & 3 for m, n in to.items())
    # a two-hop chain across the halves whose first hop leaves the cell hot enough for the second
    assert any(n in to and (m < 4) != (n < 4) and to[n] != m and at[m] >= at[n] for m, n in to.items())
    # a two-cycle a -> b, b -> a with the way back at the higher threshold
    assert any(to.get(n) == m and at[n] > at[m] for m, n in to.items())
    assert any(x is None for x in r[:4]) and any(x is None for x in r[4:])
    assert len(set(at.values())) == len(at)
    assert any(ec.LAWS[n] is None for n in to.values()) and any(ec.LAWS[n] is not None for n in to.values())
    # the threshold of a material above 3 lies below that of the material its id is cut to: reading T_at[m & 3] loses cells
    assert any(m >= 4 and (m & 3) in at and at[m & 3] > at[m] for m in ruled)
    e = MaterialTransitions._checked_rules(ec.RULES8_EDGE, 8)
    assert e[0][1] == 0.0 and np.signbit(e[0][1]) and e[5][1] < 0.0


@pytest.mark.parametrize('name', list(ec.SHAPES))
def test_the_cases_cover_what_they_were_built_for(name):
    c = ec.case(name)
    assert c['mask'].shape == ec.SHAPES[name] and c['ids'].max() <= 7 and not c['T'].flags.writeable
    cov = ec.assert_covered(name)
    ec.assert_conditions(name)
    ids1, f1, n1 = ec.reference(ec.RULES8, c['T'], c['f0'], c['mask'], c['ids'], c['dir_mask'])
    assert n1 == sum(cov['changed_from'].values()) == sum(cov['pairs'].values())
    # the passes that follow: the second hop of the chain, the way back of the cycle; after a few nothing but the cycle moves
    ids, f, counts = ids1, f1, [n1]
    for _ in range(4):
        ids, f, n = ec.reference(ec.RULES8, c['T'], f, c['mask'], ids, c['dir_mask'])
        counts.append(n)
    print('%s: cells changed in five passes: %s' % (name, counts))
    assert counts[1] > 0 and counts[2] > 0
    free = c['mask'] & ~c['dir_mask']
    chain = free & (c['ids'] == 1) & (c['T'] >= 1380.0)
    cycle = free & (c['ids'] == 3) & (c['T'] >= 1510.0)
    assert chain.any() and (ids1[chain] == 5).all() and cycle.any() and (ids1[cycle] == 7).all()
    ids2 = ec.reference(ec.RULES8, c['T'], f1, c['mask'], ids1, c['dir_mask'])[0]
    assert (ids2[chain] == 6).all() and (ids2[cycle] == 3).all()
    assert counts[3] == counts[4] > 0                       # (3 <-> 7 above 1510, for ever)


def test_every_class_is_met_with_eight_materials():
    total = {}
    for name in ('seams',) + ec.BODIES:
        cov = ec.coverage(ec.case(name))
        for cls in ec.CLASSES:
            total[cls] = total.get(cls, 0) + cov[cls]
    print('  '.join('%s %d' % kv for kv in total.items()))
    assert all(total[cls] >= 1 for cls in ec.CLASSES)
    for name in ec.BODIES:                                  # each random body meets every class by itself
        ec.assert_covered(name, every_class=True)


@pytest.mark.parametrize('name', list(ec.SHAPES))
def test_every_mutant_is_separated(name):
    c = ec.case(name)
    want = state_after(c, ec.RULES8)
    ids1, f1, n1 = ec.reference(ec.RULES8, c['T'], c['f0'], c['mask'], c['ids'], c['dir_mask'])
    ref = types.SimpleNamespace(ids=ids1, f=f1, words=ec.brick_words(c['mask'], ids1, c['shape']), count=n1,
                                packs=MaterialMap.packs_reference(c['mask'], ids1, ec.MATERIALS, ec.DX, **ec.bc_of(c)))
    assert differs(want, ref) == [] and want.ids.dtype == ref.ids.dtype
    missed = []
    for mutant in MUTANTS:
        d = differs(state_after(c, ec.RULES8, mutant), want)
        print('%s: %s %s' % (name, mutant, 'separated in ' + ', '.join(d) if d else 'NOT SEPARATED'))
        if not d:
            missed.append(mutant)
    assert not missed, (name, missed)


def test_the_edge_values_by_the_definition():
    c = ec.case('odd_row')
    T, cells = ec.edge_field(c)
    ids1, f1, n1 = ec.reference(ec.RULES8_EDGE, T, c['f0'], c['mask'], c['ids'], c['dir_mask'])
    got = {what: (int(ids1[p]), float(f1[p])) for what, p in cells.items()}
    print(got)
    for what in ('zero_plus', 'zero_minus', 'inf_no_law'):
        assert got[what] == (4, 0.0), what
    for what in ('tiny_minus', 'minus_inf_0', 'nan_0'):
        assert got[what][0] == 0, what
    assert got['at_negative'][0] == 6 and got['inf_5'] == (6, 1.0) and got['inf_law'] == (7, 1.0)
    for what in ('below_negative', 'minus_inf_5', 'nan_5'):
        assert got[what][0] == 5, what
    for what in ('minus_inf_3', 'nan_3'):
        assert got[what][0] == 3, what
    p = cells['inf_off_mask']
    assert ids1[p] == c['ids'][p] and not np.isnan(f1).any()
    unchanged = ids1 == c['ids']
    assert _bits(f1[unchanged], c['f0'][unchanged])


def test_a_replay_marks_the_host_ids_stale():
    """a replayed graph runs the pass without a call of apply(): StagedStepper.run tells the object, which marks the map's host
    copy of the id field stale -- nothing is launched, the download waits for `mm.ids`"""
    mm = types.SimpleNamespace(_ids_stamped=False)
    tr = MaterialTransitions.__new__(MaterialTransitions)
    tr.mm = mm
    tr.after_replay()
    assert mm._ids_stamped is True
