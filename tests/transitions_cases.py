"""Inputs of tests/test_transitions_cpu.py and tests/test_transitions_gpu.py: cells of a MaterialMap that change their material
when they get hot enough (MaterialTransitions).  Built from NumPy alone (no device), read-only, a function of
the case's name.

Materials: 0 loose POWDER, 1 DENSE metal, 2 a COPPER bar (no rule, no law), 3 a FLUX coating.
    RULES['powder']   powder -> dense at the liquidus 1450; flux -> copper at 930 (it burns off: the new material has no law)
    RULES['chain']    the same and dense -> copper at 1500: 0 -> 1 -> 2, with powder cells hot enough for both hops
    LAWS              powder and dense melt over 1400 - 1450, flux over 900 - 960, copper never

A case is a random body (25 % holes, ids uniform over the four materials, T uniform on [800, 1700], 5 % Dirichlet cells, f0 the
equilibrium fraction of ANOTHER random field) with six bricks of 16 x 16 x 16 cells overwritten so that every path of the
kernel is met whatever the random part holds:
    brick (0,0,0)   powder alone, no hole: cold but for a few interior cells, one at exactly T_at, one an ulp below it
    brick (0,0,1)   powder and dense, every cell below every threshold: the early return on T
    brick (0,0,2)   copper alone, hot: no ruled material in the set word
    brick (1,0,0)   dense but for three hot powder cells: the powder bit leaves the set word
    brick (0,1,0)   copper but for hot flux cells with f > 0: they become copper, f -> 0, the summary goes 1 -> 0
    brick (1,1,0)   powder and dense with f = 0 throughout, some powder cells above the liquidus: the summary goes 0 -> 1
Shapes: 32 x 32 x 48 (whole bricks, pair loads), 37 x 21 x 50 (held in a padded box: ragged edge bricks), 20 x 18 x 35 (held
unpadded: an odd row length, the cell-by-cell instantiation).  `assert_covered` counts every class from the definition alone and
fails where one is empty."""
import functools
import zlib

import numpy as np

from adi_thermal_fields_amd.matmap_extras import MapPhaseField, MaterialTransitions
from adi_thermal_fields_amd.packs import _nbr_in_mask
from adi_thermal_fields_amd.phase import PhaseChange
import matmap_extras_cases as xc

POWDER = (4000.0, 490.0, 0.3)
DENSE = (7800.0, 490.0, 25.0)
COPPER = (8900.0, 385.0, 390.0)
FLUX = (2200.0, 1100.0, 1.2)
MATERIALS = (POWDER, DENSE, COPPER, FLUX)
DX = 1e-3
TINF = 20.0
T_LIQ, T_FLUX, T_DENSE = 1450.0, 930.0, 1500.0
RULES = {'powder': ((1, T_LIQ), None, None, (2, T_FLUX)),
         'chain': ((1, T_LIQ), (2, T_DENSE), None, (2, T_FLUX))}
LAWS = (PhaseChange(2.7e5, 1400.0, 1450.0), PhaseChange(2.7e5, 1400.0, 1450.0), None, PhaseChange(9.0e4, 900.0, 960.0))
SHAPES = {'bricks': (32, 32, 48), 'padded': (37, 21, 50), 'odd': (20, 18, 35)}
BELOW = float(np.nextafter(T_LIQ, 0.0))
B = xc.BRICK
CLASSES = ('changed_in_uniform_brick', 'changed_in_mixed_brick', 'cold_ruled_brick', 'brick_without_rule', 'hot_dirichlet',
           'hot_off_mask', 'changed_exposed_h_and_q', 'changed_interior', 'exactly_T_at', 'one_ulp_below', 'bit_leaves_set',
           'new_material_without_law', 'summary_1_to_0', 'summary_0_to_1')


def _brick(bi, bj, bk):
    return (slice(B * bi, B * bi + B), slice(B * bj, B * bj + B), slice(B * bk, B * bk + B))


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(shape, mask, ids, T, f0, dir_mask, dir_value, robin_h, neumann) of the shape called `name`"""
    shape = SHAPES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    mask = rng.random(shape) > 0.25
    ids = rng.integers(0, 4, shape).astype(np.uint8)
    T = rng.uniform(800.0, 1700.0, shape)
    T_prev = rng.uniform(800.0, 1700.0, shape)
    dir_mask = mask & (rng.random(shape) < 0.05)
    special = np.zeros(shape, bool)
    zero_f = np.zeros(shape, bool)
    # (0,0,0): powder alone, solid; hot cells in its interior, one at T_at exactly, one an ulp below
    b = _brick(0, 0, 0)
    special[b] = True
    mask[b] = True
    ids[b] = 0
    T[b] = rng.uniform(800.0, 1390.0, T[b].shape)
    T[5:8, 5:8, 5:8] = rng.uniform(1460.0, 1700.0, (3, 3, 3))
    T[9, 9, 9] = T_LIQ
    T[9, 9, 11] = BELOW
    # (0,0,1): powder and dense, cold (flux's threshold is lower, but no flux is here)
    b = _brick(0, 0, 1)
    special[b] = True
    ids[b] = rng.integers(0, 2, ids[b].shape).astype(np.uint8)
    T[b] = rng.uniform(800.0, 1440.0, T[b].shape)
    # (0,0,2): copper alone, hot
    b = _brick(0, 0, 2)
    special[b] = True
    ids[b] = 2
    T[b] = rng.uniform(1500.0, 1700.0, T[b].shape)
    # (1,0,0): dense but for three hot powder cells (in the mask)
    b = _brick(1, 0, 0)
    special[b] = True
    ids[b] = 1
    T[b] = rng.uniform(800.0, 1390.0, T[b].shape)
    for c in ((17, 3, 4), (18, 9, 9), (19, 15, 15)):
        ids[c] = 0
        mask[c] = True
        T[c] = 1600.0
    # (0,1,0): copper but for hot flux cells, all of them in the mushy range of their law: f0 > 0 there and nowhere else
    b = _brick(0, 1, 0)
    special[b] = True
    ids[b] = 2
    sub = ids[b]
    sub[rng.random(sub.shape) < 0.3] = 3
    sub[0, 0, 0] = 3
    ids[b] = sub
    mask[0, B, 0] = True
    T[b] = np.where(ids[b] == 3, rng.uniform(935.0, 955.0, T[b].shape), T[b])
    T_prev[b] = T[b]
    # (1,1,0): powder and dense with f0 = 0, some powder above the liquidus
    b = _brick(1, 1, 0)
    special[b] = True
    zero_f[b] = True
    ids[b] = rng.integers(0, 2, ids[b].shape).astype(np.uint8)
    T[b] = rng.uniform(800.0, 1440.0, T[b].shape)
    sub_T, sub_ids = T[b], ids[b]
    sub_T[sub_ids == 0] = np.where(rng.random(int((sub_ids == 0).sum())) < 0.3, 1470.0, sub_T[sub_ids == 0])
    sub_ids[0, 0, 1] = 0
    sub_T[0, 0, 1] = 1470.0
    T[b], ids[b] = sub_T, sub_ids
    mask[B, B, 1] = True
    dir_mask = dir_mask & ~special & mask
    f0 = MapPhaseField.f_eq_of(LAWS, T_prev, mask, ids)
    f0 = np.where(zero_f, 0.0, f0)
    c = dict(shape=shape, mask=mask, ids=ids, T=T, f0=f0, dir_mask=dir_mask, dir_value=rng.uniform(30.0, 60.0, shape),
             robin_h={'x-': 350.0, 'x+': rng.uniform(20.0, 400.0, shape), 'y-': 120.0, 'y+': rng.uniform(20.0, 400.0, shape),
                      'z-': 350.0, 'z+': 80.0},
             neumann={'z-': 2e5, 'y+': rng.uniform(1e3, 1e5, shape)})
    for v in list(c.values()) + list(c['robin_h'].values()) + list(c['neumann'].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def bc_of(c, loss=False):
    """the MaterialMap's boundary keywords; loss: robin_h=None, what a MapLossPacks asks for"""
    return dict(dir_mask=c['dir_mask'], dir_value=c['dir_value'], neumann=c['neumann'], robin_h=None if loss else c['robin_h'])


def reference(rules, T, f, mask, ids, dir_mask):
    """MaterialTransitions.apply_reference under LAWS (f None: without a phase)"""
    return MaterialTransitions.apply_reference(rules, T, f, mask, ids, dir_mask, None if f is None else LAWS)


def _popcount(w):
    return np.array([bin(int(v)).count('1') for v in w])


def coverage(rules, T, f0, mask, ids, dir_mask, robin_h, neumann):
    """{class: count} from the definition alone; the brick words are those of the logical box (the padding holds no cell)"""
    shape = mask.shape
    ids_new, f_new, n = reference(rules, T, f0, mask, ids, dir_mask)
    changed = ids_new != ids
    assert int(changed.sum()) == n
    ruled = sum(1 << m for m, r in enumerate(rules) if r is not None)
    T_at = np.array([np.inf if r is None else r[1] for r in rules])
    w0, w1 = xc.brick_words(mask, ids, shape), xc.brick_words(mask, ids_new, shape)
    s0, s1 = xc.brick_any(f0, shape), xc.brick_any(f_new, shape)
    nb = [(n_ + B - 1) // B for n_ in shape]
    brick_of = np.ravel_multi_index(tuple(np.indices(shape)[a] // B for a in range(3)), nb)
    # per brick: the smallest threshold among the set's ruled materials, and the hottest in-mask cell
    t_min = np.array([min([T_at[m] for m in range(len(rules)) if (int(w) & ruled) >> m & 1] or [np.inf]) for w in w0])
    hottest = np.full(len(w0), -np.inf)
    np.maximum.at(hottest, brick_of[mask], T[mask])
    interior = mask.copy()
    for axis in range(3):
        for plus in (False, True):
            interior &= _nbr_in_mask(mask, axis, plus)
    exposed_yp = mask & ~_nbr_in_mask(mask, 1, True)
    own_rule = ruled >> ids.astype(np.int64) & 1 != 0
    at = T_at[ids]
    out = dict(
        changed_in_uniform_brick=int((changed & (_popcount(w0)[brick_of] == 1)).sum()),
        changed_in_mixed_brick=int((changed & (_popcount(w0)[brick_of] > 1)).sum()),
        cold_ruled_brick=int((((w0 & ruled) != 0) & (hottest < t_min)).sum()),
        brick_without_rule=int(((w0 != 0) & ((w0 & ruled) == 0)).sum()),
        hot_dirichlet=int((mask & dir_mask & own_rule & (T >= at)).sum()),
        hot_off_mask=int((~mask & own_rule & (T >= at)).sum()),
        changed_exposed_h_and_q=int((changed & exposed_yp & (robin_h['y+'] != 0.0) & (neumann['y+'] != 0.0)).sum()),
        changed_interior=int((changed & interior).sum()),
        exactly_T_at=int((changed & (T == at)).sum()),
        one_ulp_below=int((mask & ~dir_mask & own_rule & (T == np.nextafter(at, -np.inf))).sum()),
        bit_leaves_set=int(((w0 & ~w1) != 0).sum()),
        new_material_without_law=int((changed & (f0 != 0.0) & np.array([w is None for w in LAWS])[ids_new]).sum()),
        summary_1_to_0=int(((s0 == 1) & (s1 == 0)).sum()),
        summary_0_to_1=int(((s0 == 0) & (s1 == 1)).sum()))
    # a cell hot enough for the rule of its new material too: it waits for the next step
    new_rule = ruled >> ids_new.astype(np.int64) & 1 != 0
    out['second_hop_waits'] = int((changed & new_rule & (T >= T_at[ids_new])).sum())
    return out


def assert_covered(c, rules, what=''):
    cov = coverage(rules, c['T'], c['f0'], c['mask'], c['ids'], c['dir_mask'], c['robin_h'], c['neumann'])
    print('%s: %s' % (what, '  '.join('%s %d' % kv for kv in cov.items())))
    for name in CLASSES:
        assert cov[name] >= 1, (what, name)
    if rules is RULES['chain']:
        assert cov['second_hop_waits'] >= 1, what
    return cov
