"""Inputs of tests/test_transitions_eight_cpu.py and tests/test_transitions_eight_gpu.py: MaterialTransitions with
all eight materials a MaterialMap serves, with the changed cells placed by where they sit, and at the edges of the comparison
T >= T_at.  Built from NumPy alone (no device), read-only, a function of the case's name.  Materials: matmap_eight_cases.MATERIALS8;
laws: matmap_extras_cases.LAWS8 (ids 2 and 4 have none).

RULES8 (material -> new material at T_at; ids 2 and 4, one in each half of 0 .. 7, have no rule):
    0 -> 4 at 1450   into the upper half, the new material has no law
    1 -> 5 at 1380   into the upper half; 1 -> 5 -> 6 is the two-hop chain (a cell of 1 that changes is hot enough for 5's rule)
    3 -> 7 at 1210   the two-cycle: 3 -> 7, and 7 -> 3 at the higher 1510: a cell above 1510 alternates, one hop per pass
    5 -> 6 at 1120   both ids above 3, and 5 & 3 != 6 & 3; the threshold lies BELOW that of material 5 & 3 = 1
    6 -> 2 at 1600   into the lower half, the new material has no law (a third hop of the chain)
    7 -> 3 at 1510
All thresholds are distinct; targets 5, 6, 7 and 3 have a law, 4 and 2 have none.
RULES8_EDGE: 0 -> 4 at -0.0 (T = +0.0 is at the threshold: both zeros compare equal), 5 -> 6 at -250, 3 -> 7 at 1210.

Shapes (SHAPES; every one but `padded` is held in its own box, `padded` in nx + 1, ny + 3, nz + 2):
    seams    33 x 33 x 34: two bricks of 16 and one cell on every axis.  Ruled hot cells on the product SEAM_IJ x SEAM_IJ x SEAM_K,
             holes next to two of them, a pair whose odd cell alone changes, the 16 cells of one thread, one brick that changes whole
    odd_row  20 x 18 x 35: rows of 35 cells, the cell-by-cell instantiation; changed cells at k = 34
    padded   37 x 21 x 50: changed cells on the last logical plane of every axis
    thin_<axis>_<n>   the axis `axis` n = 1, 2, 3 cells long, the other two 5 and 6: one ragged brick, every in-mask ruled cell hot
odd_row and padded are random bodies (25 % holes, ids uniform on 0 .. 7, T uniform on [900, 1700], 5 % Dirichlet cells, f0 the
equilibrium fraction of ANOTHER field) with six bricks overwritten as in transitions_cases.case, so that every class of
transitions_cases.CLASSES is met; `coverage` counts the classes from the definition alone."""
import functools
import zlib

import numpy as np

from adi_thermal_fields_amd.matmap_extras import MapPhaseField, MaterialTransitions
from adi_thermal_fields_amd.packs import _nbr_in_mask
import matmap_extras_cases as xc
from matmap_eight_cases import MATERIALS8
from matmap_extras_cases import LAWS8, BRICK, brick_words, brick_any
from solidification_cases import neighbour_class
from transitions_cases import CLASSES

MATERIALS = MATERIALS8
LAWS = LAWS8
DX = 1e-3
TINF = 20.0
RULES8 = ((4, 1450.0), (5, 1380.0), None, (7, 1210.0), None, (6, 1120.0), (2, 1600.0), (3, 1510.0))
RULES8_EDGE = ((4, -0.0), None, None, (7, 1210.0), None, (6, -250.0), None, None)
RULED = tuple(m for m, r in enumerate(RULES8) if r is not None)
T_AT = np.array([np.inf if r is None else r[1] for r in RULES8])
B = BRICK
SEAM_IJ = (0, 15, 16, 31, 32)
SEAM_K = (0, 1, 15, 16, 17, 32, 33)
SEAM_HOLES = ((14, 15, 15), (15, 14, 15), (15, 15, 14), (17, 16, 17), (16, 17, 17), (16, 16, 18))
SEAM_PLUS_ONLY, SEAM_MINUS_ONLY = (15, 15, 15), (16, 16, 17)       # the planted cells the holes leave with one neighbour per axis
ODD_PAIR = (5, 5, 6)                                               # cell (5, 5, 7) changes, (5, 5, 6) does not
THREAD = 8 * 21 + 3                                                # the thread of brick (1, 1, 1) whose 16 cells all change
WHOLE_BRICK = (0, 1, 1)
THIN = tuple('thin_%d_%d' % (a, n) for a in range(3) for n in (1, 2, 3))
SHAPES = dict(seams=(33, 33, 34), odd_row=(20, 18, 35), padded=(37, 21, 50))
for _name in THIN:
    _a, _n = int(_name[5]), int(_name[7])
    _s = [5, 6]
    _s.insert(_a, _n)
    SHAPES[_name] = tuple(_s)
BODIES = ('odd_row', 'padded')                                     # the shapes on which every class of CLASSES is met


def pad_dims(nx, ny, nz):
    return nx + 1, ny + 3, nz + 2


def exact_dims(nx, ny, nz):
    return nx, ny, nz


def dims_of(name):
    return pad_dims if name == 'padded' else exact_dims


def _brick(bi, bj, bk):
    return (slice(B * bi, B * bi + B), slice(B * bj, B * bj + B), slice(B * bk, B * bk + B))


def thread_cells(tid, brick):
    """the 16 cells thread `tid` of a brick's workgroup owns (adi_brick_dev.hpp: row it * 32 + tid / 8, cells 2 (tid % 8) + 0, 1)"""
    out = []
    for it in range(8):
        row = it * 32 + (tid >> 3)
        for s in (0, 1):
            out.append((B * brick[0] + (row >> 4), B * brick[1] + (row & 15), B * brick[2] + 2 * (tid & 7) + s))
    return out


def _random_body(rng, shape):
    mask = rng.random(shape) > 0.25
    ids = rng.integers(0, 8, shape).astype(np.uint8)
    T = rng.uniform(900.0, 1700.0, shape)
    T_prev = rng.uniform(900.0, 1700.0, shape)
    dir_mask = mask & (rng.random(shape) < 0.05)
    return mask, ids, T, T_prev, dir_mask


def _hot(rng, m, n=None):
    """temperatures at or above the threshold of material m, below 1700"""
    return rng.uniform(T_AT[m] + 1.0, max(T_AT[m] + 2.0, 1700.0), n)


def _body(name, rng):
    """odd_row, padded: transitions_cases.case's six bricks with eight materials"""
    shape = SHAPES[name]
    mask, ids, T, T_prev, dir_mask = _random_body(rng, shape)
    special = np.zeros(shape, bool)
    zero_f = np.zeros(shape, bool)
    # (0,0,0): material 5 alone, solid; cold but for a few interior cells, one at T_at exactly, one an ulp below
    b = _brick(0, 0, 0)
    special[b] = True
    mask[b] = True
    ids[b] = 5
    T[b] = rng.uniform(900.0, 1100.0, T[b].shape)
    T[5:8, 5:8, 5:8] = rng.uniform(1130.0, 1700.0, (3, 3, 3))
    T[9, 9, 9] = T_AT[5]
    T[9, 9, 11] = np.nextafter(T_AT[5], 0.0)
    # (0,0,1): materials 0 and 6, every cell below both thresholds
    b = _brick(0, 0, 1)
    special[b] = True
    ids[b] = np.where(rng.random(ids[b].shape) < 0.5, 0, 6).astype(np.uint8)
    T[b] = rng.uniform(900.0, 1440.0, T[b].shape)
    # (0,0,2): materials 2 and 4, hot: no ruled material in the set word
    b = _brick(0, 0, 2)
    special[b] = True
    ids[b] = np.where(rng.random(ids[b].shape) < 0.5, 2, 4).astype(np.uint8)
    T[b] = rng.uniform(1600.0, 1700.0, T[b].shape)
    # (1,0,0): material 4 but for three hot cells of 7: bit 7 leaves the set word, bit 3 joins it
    b = _brick(1, 0, 0)
    special[b] = True
    ids[b] = 4
    T[b] = rng.uniform(900.0, 1100.0, T[b].shape)
    for c in ((17, 3, 4), (18, 9, 9), (19, 15, 15)):
        ids[c] = 7
        mask[c] = True
        T[c] = 1650.0
    # (0,1,0): material 2 but for cells of 0 that were mushy (f0 > 0 there and nowhere else in the brick) and are at or above
    # 1450 now: they become 4, which has no law: f -> 0, the summary goes 1 -> 0
    b = _brick(0, 1, 0)
    special[b] = True
    sub = np.full(ids[b].shape, 2, np.uint8)
    sub[rng.random(sub.shape) < 0.3] = 0
    sub[0, 0, 0] = 0
    ids[b] = sub
    mask[0, B, 0] = True
    T[b] = np.where(sub == 0, rng.uniform(1455.0, 1500.0, sub.shape), T[b])
    T_prev[b] = rng.uniform(1410.0, 1440.0, sub.shape)
    # (1,1,0): materials 3 and 4 with f0 = 0 throughout, some cells of 3 above 1210: they become 7, mushy at that T: 0 -> 1
    b = _brick(1, 1, 0)
    special[b] = True
    zero_f[b] = True
    sub_ids = np.where(rng.random(ids[b].shape) < 0.5, 3, 4).astype(np.uint8)
    sub_T = rng.uniform(900.0, 1200.0, sub_ids.shape)
    sub_T[sub_ids == 3] = np.where(rng.random(int((sub_ids == 3).sum())) < 0.3, 1250.0, sub_T[sub_ids == 3])
    sub_ids[0, 0, 1] = 3
    sub_T[0, 0, 1] = 1250.0
    T[b], ids[b] = sub_T, sub_ids
    mask[B, B, 1] = True
    # changed cells where the box ends: the last cell of the odd rows (odd_row), the last logical plane of every axis (padded)
    nx, ny, nz = shape
    last = [(3, ny - 1, nz - 1), (nx - 1, ny - 1, nz - 1), (nx - 1, 5, 20), (nx - 1, ny - 1, 21), (7, ny - 1, 22)]
    for n, c in enumerate(last):
        ids[c] = RULED[n % len(RULED)]
        mask[c] = True
        special[c] = True
        T[c] = 1690.0
    dir_mask = dir_mask & ~special & mask
    f0 = MapPhaseField.f_eq_of(LAWS, T_prev, mask, ids)
    f0 = np.where(zero_f, 0.0, f0)
    return dict(mask=mask, ids=ids, T=T, f0=f0, dir_mask=dir_mask, last=last)


def _seams(rng):
    shape = SHAPES['seams']
    mask, ids, T, T_prev, dir_mask = _random_body(rng, shape)
    special = np.zeros(shape, bool)
    # one brick that changes whole: ruled materials alone, no hole, above every threshold
    b = _brick(*WHOLE_BRICK)
    special[b] = True
    mask[b] = True
    ids[b] = np.array(RULED, np.uint8)[rng.integers(0, len(RULED), ids[b].shape)]
    T[b] = rng.uniform(1610.0, 1700.0, T[b].shape)
    # the product: in the mask with all their neighbours, of a ruled material, hot; one of them at its threshold exactly
    planted = [(i, j, k) for i in SEAM_IJ for j in SEAM_IJ for k in SEAM_K]
    planted += thread_cells(THREAD, (1, 1, 1))
    planted.append((ODD_PAIR[0], ODD_PAIR[1], ODD_PAIR[2] + 1))
    for n, c in enumerate(planted):
        for axis in range(3):
            for d in (-1, 1):
                q = list(c)
                q[axis] += d
                if 0 <= q[axis] < shape[axis]:
                    mask[tuple(q)] = True
        mask[c] = True
        special[c] = True
        if T_AT[ids[c]] == np.inf:
            ids[c] = RULED[n % len(RULED)]
        T[c] = rng.uniform(T_AT[ids[c]] + 1.0, max(T_AT[ids[c]] + 2.0, 1700.0))
    T[16, 15, 16] = T_AT[ids[16, 15, 16]]
    for c in SEAM_HOLES:
        assert not special[c]
        mask[c] = False
    # the even cell of the pair stays: material 4, which has no rule
    ids[ODD_PAIR] = 4
    mask[ODD_PAIR] = True
    special[ODD_PAIR] = True
    dir_mask = dir_mask & ~special & mask
    f0 = MapPhaseField.f_eq_of(LAWS, T_prev, mask, ids)
    return dict(mask=mask, ids=ids, T=T, f0=f0, dir_mask=dir_mask, planted=planted)


def _thin(name, rng):
    """one ragged brick: ids among 0, 1, 3, 4, 5, 6, 7 (2 joins the set by 6 -> 2), every ruled cell in the mask hot, one cell of
    every ruled material in the mask and free; one Dirichlet cell (of material 0, hot), one cell at its threshold exactly"""
    shape = SHAPES[name]
    n = int(np.prod(shape))
    pool = np.array([0, 1, 3, 4, 5, 6, 7], np.uint8)
    ids = pool[np.arange(n) % len(pool)]
    ids = ids[rng.permutation(n)].reshape(shape)
    mask = rng.random(shape) > 0.2
    flat = [tuple(p) for p in np.argwhere(np.ones(shape, bool))]
    for m in RULED:                                              # the first cell of every ruled material is in the mask
        mask[next(p for p in flat if ids[p] == m)] = True
    T = rng.uniform(900.0, 1700.0, shape)
    T_prev = rng.uniform(900.0, 1700.0, shape)
    for m in RULED:
        T = np.where(ids == m, _hot(rng, m, shape), T)
    dir_mask = np.zeros(shape, bool)
    zeros = [p for p in flat if ids[p] == 0]
    mask[zeros[1]] = True
    dir_mask[zeros[1]] = True
    at = next(p for p in flat if ids[p] == 3)
    T[at] = T_AT[3]
    again = [p for p in flat if ids[p] == 3][1]                  # a cell of 3 above the threshold of 7 too: the cycle
    mask[again] = True
    T[again] = 1600.0
    T[next(p for p in flat if ids[p] == 5)] = 1200.0          # between the thresholds of 5 (1120) and of 5 & 3 = 1 (1380)
    f0 = MapPhaseField.f_eq_of(LAWS, T_prev, mask, ids)
    return dict(mask=mask, ids=ids, T=T, f0=f0, dir_mask=dir_mask)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(shape, mask, ids, T, f0, dir_mask, dir_value, robin_h, neumann, ...) of the shape called `name`"""
    shape = SHAPES[name]
    rng = np.random.default_rng(zlib.crc32(('eight/' + name).encode()))
    c = _seams(rng) if name == 'seams' else _body(name, rng) if name in BODIES else _thin(name, rng)
    c.update(shape=shape, name=name, dir_value=rng.uniform(30.0, 60.0, shape),
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
    """MaterialTransitions.apply_reference under LAWS8 (f None: without a phase)"""
    return MaterialTransitions.apply_reference(rules, T, f, mask, ids, dir_mask, None if f is None else LAWS)


def edge_field(c):
    """(T, cells) for RULES8_EDGE on a case: the case's T with the values at the edge of `>=` planted in free in-mask cells of
    materials 0 (threshold -0.0), 5 (-250) and 3 (1210; the new material 7 has a law).  cells: {what: cell}"""
    T = np.array(c['T'])
    free = c['mask'] & ~c['dir_mask']
    of = {m: [tuple(p) for p in np.argwhere(free & (c['ids'] == m))] for m in (0, 3, 5)}
    below = float(np.nextafter(-250.0, -np.inf))
    plan = [('zero_plus', 0, 0.0), ('zero_minus', 0, -0.0), ('tiny_minus', 0, -5e-324), ('inf_no_law', 0, np.inf),
            ('minus_inf_0', 0, -np.inf), ('nan_0', 0, np.nan),
            ('at_negative', 5, -250.0), ('below_negative', 5, below), ('minus_inf_5', 5, -np.inf), ('nan_5', 5, np.nan),
            ('inf_5', 5, np.inf),
            ('inf_law', 3, np.inf), ('minus_inf_3', 3, -np.inf), ('nan_3', 3, np.nan)]
    cells = {}
    for what, m, v in plan:
        p = of[m].pop(len(of[m]) // 2)
        T[p] = v
        cells[what] = p
    p = tuple(np.argwhere(~c['mask'])[0])
    T[p] = np.inf                                           # off the mask: nothing changes there
    cells['inf_off_mask'] = p
    return T, cells


def _popcount(w):
    return np.array([bin(int(v)).count('1') for v in w])


def coverage(c, rules=RULES8):
    """{class: count} of transitions_cases.CLASSES from the definition alone, and what the eight materials add: `changed_from`
    (per material, the cells that change), `pairs` ({(old, new): cells}), `second_hop_waits`"""
    T, f0, mask, ids, dir_mask = c['T'], c['f0'], c['mask'], c['ids'], c['dir_mask']
    shape = mask.shape
    ids_new, f_new, n = reference(rules, T, f0, mask, ids, dir_mask)
    changed = ids_new != ids
    assert int(changed.sum()) == n
    ruled = sum(1 << m for m, r in enumerate(rules) if r is not None)
    T_at = np.array([np.inf if r is None else r[1] for r in rules])
    w0, w1 = brick_words(mask, ids, shape), brick_words(mask, ids_new, shape)
    s0, s1 = brick_any(f0, shape), brick_any(f_new, shape)
    nb = [(n_ + B - 1) // B for n_ in shape]
    brick_of = np.ravel_multi_index(tuple(np.indices(shape)[a] // B for a in range(3)), nb)
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
        changed_exposed_h_and_q=int((changed & exposed_yp & (c['robin_h']['y+'] != 0.0) & (c['neumann']['y+'] != 0.0)).sum()),
        changed_interior=int((changed & interior).sum()),
        exactly_T_at=int((changed & (T == at)).sum()),
        one_ulp_below=int((mask & ~dir_mask & own_rule & (T == np.nextafter(at, -np.inf))).sum()),
        bit_leaves_set=int(((w0 & ~w1) != 0).sum()),
        new_material_without_law=int((changed & (f0 != 0.0) & np.array([w is None for w in LAWS])[ids_new]).sum()),
        summary_1_to_0=int(((s0 == 1) & (s1 == 0)).sum()),
        summary_0_to_1=int(((s0 == 0) & (s1 == 1)).sum()))
    new_rule = ruled >> ids_new.astype(np.int64) & 1 != 0
    out['second_hop_waits'] = int((changed & new_rule & (T >= T_at[ids_new])).sum())
    out['bit_joins_set'] = int(((w1 & ~w0) != 0).sum())
    out['changed_from'] = {m: int((changed & (ids == m)).sum()) for m, r in enumerate(rules) if r is not None}
    out['pairs'] = {(m, r[0]): int((changed & (ids == m) & (ids_new == r[0])).sum()) for m, r in enumerate(rules) if r is not None}
    return out


def assert_covered(name, every_class=None):
    """print the counts of the case; every ruled material changes a cell and every pair the rules allow occurs; on the random
    bodies (every_class None: decided by the name) every class of transitions_cases.CLASSES is met"""
    c = case(name)
    cov = coverage(c)
    print('%s: %s' % (name, '  '.join('%s %s' % kv for kv in cov.items())))
    for m, n in cov['changed_from'].items():
        assert n >= 1, (name, 'no cell of material %d changes' % m)
    for pair, n in cov['pairs'].items():
        assert n >= 1, (name, pair)
    assert cov['second_hop_waits'] >= 1 and cov['bit_joins_set'] >= 1, name
    if name in BODIES if every_class is None else every_class:
        for cls in CLASSES:
            assert cov[cls] >= 1, (name, cls)
    return cov


def conditions(name):
    """what the shape was built for, counted from the definition -> dict"""
    c = case(name)
    mask, ids = c['mask'], c['ids']
    ids1, _, n = reference(RULES8, c['T'], c['f0'], mask, ids, c['dir_mask'])
    changed = ids1 != ids
    out = dict(changed=n)
    if name == 'seams':
        cls = neighbour_class(mask)
        combos = {tuple((int(v) >> (2 * a)) & 3 for a in range(3)) for v in cls[changed]}
        out['combos'] = len([t for t in combos if 0 not in t])                          # 1 minus only, 2 plus only, 3 both
        out['planted_changed'] = int(sum(changed[p] for p in c['planted']))
        out['planted'] = len(c['planted'])
        out['seam_sides'] = [(int(changed[tuple(slice(15, 16) if a == ax else slice(None) for a in range(3))].sum()),
                              int(changed[tuple(slice(16, 17) if a == ax else slice(None) for a in range(3))].sum()))
                             for ax in range(3)]
        out['plus_only'] = int(cls[SEAM_PLUS_ONLY]) if changed[SEAM_PLUS_ONLY] else -1
        out['minus_only'] = int(cls[SEAM_MINUS_ONLY]) if changed[SEAM_MINUS_ONLY] else -1
        out['both_of_a_pair'] = int((changed[:, :, 0::2] & changed[:, :, 1::2]).sum())
        i, j, k = ODD_PAIR
        out['odd_alone'] = bool(changed[i, j, k + 1] and not changed[i, j, k] and mask[i, j, k])
        out['thread'] = int(sum(changed[p] for p in thread_cells(THREAD, (1, 1, 1))))
        out['whole_brick'] = int(changed[_brick(*WHOLE_BRICK)].sum())
    elif name in BODIES:
        nx, ny, nz = c['shape']
        out['last_planes'] = [int(changed[nx - 1].sum()), int(changed[:, ny - 1].sum()), int(changed[:, :, nz - 1].sum())]
        out['last_planted'] = int(sum(changed[p] for p in c['last']))
    else:
        free = mask & ~c['dir_mask']
        own = np.isfinite(T_AT[ids])
        out['ruled_free'] = int((free & own).sum())
        out['hot_dirichlet'] = int((mask & c['dir_mask'] & own & (c['T'] >= T_AT[ids])).sum())
    return out


def assert_conditions(name):
    k = conditions(name)
    print('%s: %s' % (name, k))
    if name == 'seams':
        assert k['combos'] == 27 and k['planted_changed'] == k['planted'] == 5 * 5 * 7 + 16 + 1
        assert all(a >= 35 and b >= 35 for a, b in k['seam_sides'])
        assert k['plus_only'] == 0b101010 and k['minus_only'] == 0b010101
        assert k['both_of_a_pair'] >= 3 * 25 and k['odd_alone'] and k['thread'] == 16 and k['whole_brick'] == B ** 3
    elif name in BODIES:
        assert all(n >= 1 for n in k['last_planes']) and k['last_planted'] == 5
    else:
        assert k['changed'] == k['ruled_free'] >= 6 and k['hot_dirichlet'] == 1
    return k
