"""CPU: cells of a MaterialMap that change their material when they get hot enough (MaterialTransitions): the
definition against a per-cell loop, the coverage of the shared cases, what the class, the C entries and the step refuse, and the
new kernels' footprint.  Inputs: tests/transitions_cases.py.  No GPU (the built library is needed for the imports)."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest

import transitions_cases as tc
from adi_thermal_fields_amd import _lib, step
from adi_thermal_fields_amd.matmap_extras import MapPhaseField, MaterialTransitions
from adi_thermal_fields_amd.packs import MaterialMap, Material, Params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _loop(rules, T, f, mask, ids, dir_mask, laws):
    """the definition again, cell by cell, written from the issue's words and sharing nothing with apply_reference"""
    ids_new = ids.copy()
    f_new = None if f is None else f.copy()
    n = 0
    for p in zip(*np.nonzero(mask)):
        m = int(ids[p])
        if rules[m] is None or (dir_mask is not None and dir_mask[p]):
            continue
        to, T_at = rules[m]
        if not T[p] >= T_at:
            continue
        ids_new[p] = to
        n += 1
        if f is not None:
            if laws[to] is None:
                f_new[p] = 0.0
            else:
                Ts, Tl = laws[to].T_solidus, laws[to].T_liquidus
                f_new[p] = min(max((T[p] - Ts) / (Tl - Ts), 0.0), 1.0)
    return ids_new, f_new, n


@pytest.mark.parametrize('rules', ['powder', 'chain'])
@pytest.mark.parametrize('name', list(tc.SHAPES))
def test_the_cases_cover_every_class_and_the_definition_is_the_per_cell_loop(name, rules):
    c, r = tc.case(name), tc.RULES[rules]
    cov = tc.assert_covered(c, r, '%s/%s' % (name, rules))
    T = np.array(c['T'])
    T[6, 6, 6] = np.nan                                     # (a powder cell of brick (0,0,0) that was hot: a NaN never is)
    T[tuple(np.argwhere(~c['mask'])[0])] = np.nan
    got = MaterialTransitions.apply_reference(r, T, c['f0'], c['mask'], c['ids'], c['dir_mask'], tc.LAWS)
    want = _loop(r, T, c['f0'], c['mask'], c['ids'], c['dir_mask'], tc.LAWS)
    assert np.array_equal(got[0], want[0]) and got[0].dtype == np.uint8 and _bits(got[1], want[1]) and got[2] == want[2]
    assert got[2] >= cov['changed_interior'] > 0
    # f_eq of a changed cell is MapPhaseField.f_eq_of's under the new ids; every other f is untouched
    changed = got[0] != c['ids']
    assert _bits(got[1][changed], MapPhaseField.f_eq_of(tc.LAWS, T, c['mask'], got[0])[changed])
    assert _bits(got[1][~changed], c['f0'][~changed])
    # without a phase and without Dirichlet cells
    ids2, f2, n2 = MaterialTransitions.apply_reference(r, T, None, c['mask'], c['ids'], None, None)
    w2 = _loop(r, T, None, c['mask'], c['ids'], None, None)
    assert f2 is None and np.array_equal(ids2, w2[0]) and n2 == w2[2] and n2 > got[2]
    # nothing changes off the mask, in Dirichlet cells, or without rules
    assert np.array_equal(got[0][~c['mask'] | c['dir_mask']], c['ids'][~c['mask'] | c['dir_mask']])
    none = MaterialTransitions.apply_reference((None,) * 4, T, c['f0'], c['mask'], c['ids'], c['dir_mask'], tc.LAWS)
    assert np.array_equal(none[0], c['ids']) and _bits(none[1], c['f0']) and none[2] == 0


def test_a_chain_takes_one_hop_per_pass():
    c, r = tc.case('odd'), tc.RULES['chain']
    ids1, f1, n1 = tc.reference(r, c['T'], c['f0'], c['mask'], c['ids'], c['dir_mask'])
    both = c['mask'] & ~c['dir_mask'] & (c['ids'] == 0) & (c['T'] >= tc.T_DENSE)
    assert both.sum() > 10 and (ids1[both] == 1).all()
    ids2, f2, n2 = tc.reference(r, c['T'], f1, c['mask'], ids1, c['dir_mask'])
    assert (ids2[both] == 2).all() and (f2[both] == 0.0).all() and n2 >= both.sum()
    ids3, _, n3 = tc.reference(r, c['T'], f2, c['mask'], ids2, c['dir_mask'])
    assert n3 == 0 and np.array_equal(ids3, ids2)


# ---- what the class refuses, before anything is launched -------------------------------------------------------------------------
def _bare_map(n=4, valid=True):
    mm = MaterialMap.__new__(MaterialMap)                  # (no device here: the attributes the checks read)
    mm.grid = types.SimpleNamespace(mask_version=3)
    mm.materials = tuple(Material(*m) for m in tc.MATERIALS[:n])
    mm.mat = mm.materials[0]
    mm.packs = tuple(types.SimpleNamespace(mask_version=3) for _ in range(3))
    mm.ids_all_valid, mm._ids_version = valid, 0
    return mm


def _bare_tr(mm, phase=None):
    tr = MaterialTransitions.__new__(MaterialTransitions)
    tr.mm, tr.grid, tr.phase = mm, mm.grid, phase
    tr._mask_version, tr._ids_version = mm.grid.mask_version, mm._ids_version
    return tr


def _bare_phase(mm):
    ph = MapPhaseField.__new__(MapPhaseField)
    ph.mm, ph.grid = mm, mm.grid
    ph._mask_version, ph._ids_version = mm.grid.mask_version, mm._ids_version
    return ph


def test_rules_are_checked():
    chk = MaterialTransitions._checked_rules
    assert chk(tc.RULES['chain'], 4) == ((1, 1450.0), (2, 1500.0), None, (2, 930.0))
    assert chk([(np.uint8(1), np.float32(5.0)), None], 2) == ((1, 5.0), None)
    with pytest.raises(TypeError, match='rules must be a sequence'):
        chk(5, 4)
    with pytest.raises(ValueError, match='3 rules for 4 materials'):
        chk(tc.RULES['powder'][:3], 4)
    with pytest.raises(TypeError, match=r'\(to, T_at\) or None'):
        chk((1450.0, None, None, None), 4)
    with pytest.raises(TypeError, match='must be an int'):
        chk(((1.0, 1450.0), None, None, None), 4)
    with pytest.raises(TypeError, match='must be an int'):
        chk(((True, 1450.0), None, None, None), 4)
    with pytest.raises(ValueError, match='turns into 4'):
        chk(((4, 1450.0), None, None, None), 4)
    with pytest.raises(ValueError, match='turns into -1'):
        chk(((-1, 1450.0), None, None, None), 4)
    with pytest.raises(ValueError, match='turns into itself'):
        chk((None, (1, 1450.0), None, None), 4)
    with pytest.raises(TypeError, match='real number'):
        chk(((1, 'hot'), None, None, None), 4)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match='not finite'):
            chk(((1, bad), None, None, None), 4)


def test_the_constructor_checks_come_before_any_launch():
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    assert hip.MaterialTransitions is MaterialTransitions and 'MaterialTransitions' not in hip.__all__
    mm = _bare_map()
    with pytest.raises(TypeError, match='mm must be a MaterialMap'):
        MaterialTransitions(object(), tc.RULES['powder'])
    with pytest.raises(ValueError, match='3 rules for 4 materials'):
        MaterialTransitions(mm, tc.RULES['powder'][:3])
    with pytest.raises(TypeError, match='phase must be a MapPhaseField'):
        MaterialTransitions(mm, tc.RULES['powder'], phase=object())
    with pytest.raises(ValueError, match='another MaterialMap'):
        MaterialTransitions(mm, tc.RULES['powder'], phase=_bare_phase(_bare_map()))
    with pytest.raises(ValueError, match='names no material'):
        MaterialTransitions(_bare_map(valid=False), tc.RULES['powder'])


def test_the_step_refuses_what_does_not_fit():
    mm = _bare_map()
    g, prm = mm.grid, Params(1e-3)
    args = (g, mm.mat, prm, mm.packs)
    tr = _bare_tr(mm)
    step._check_extras(*args, step.StepExtras(material_map=mm, transitions=tr))
    with pytest.raises(ValueError, match='needs material_map='):
        step._check_extras(*args, step.StepExtras(transitions=tr))
    with pytest.raises(TypeError, match='must be a MaterialTransitions'):
        step._check_extras(*args, step.StepExtras(material_map=mm, transitions=object()))
    with pytest.raises(ValueError, match='another MaterialMap'):
        step._check_extras(*args, step.StepExtras(material_map=mm, transitions=_bare_tr(_bare_map())))
    ph = _bare_phase(mm)
    # the phase, in both directions, and another phase of the same map
    with pytest.raises(ValueError, match="is not the step's phase="):
        step._check_extras(*args, step.StepExtras(material_map=mm, phase=ph, transitions=tr))
    with pytest.raises(ValueError, match="is not the step's phase="):
        step._check_extras(*args, step.StepExtras(material_map=mm, transitions=_bare_tr(mm, ph)))
    with pytest.raises(ValueError, match="is not the step's phase="):
        step._check_extras(*args, step.StepExtras(material_map=mm, phase=_bare_phase(mm), transitions=_bare_tr(mm, ph)))
    step._check_extras(*args, step.StepExtras(material_map=mm, phase=ph, transitions=_bare_tr(mm, ph)))
    # stale: the mask or the ids moved on since the words were built; with a phase, the phase's staleness too
    g.mask_version = 4
    for p in mm.packs:
        p.mask_version = 4
    with pytest.raises(ValueError, match=r'MaterialTransitions: .*call sync_mask\(\)'):
        step._check_extras(*args, step.StepExtras(material_map=mm, transitions=tr))
    tr._mask_version = 4
    step._check_extras(*args, step.StepExtras(material_map=mm, transitions=tr))
    mm._ids_version = 1
    with pytest.raises(ValueError, match=r'MaterialTransitions: .*call sync_mask\(\)'):
        step._check_extras(*args, step.StepExtras(material_map=mm, transitions=tr))
    # the graph key: nothing is appended without transitions
    assert step.StepExtras().graph_key() == (None,) * 7
    k = types.SimpleNamespace(graph_key=lambda: ('k',))
    assert step.StepExtras(transitions=k).graph_key() == (None,) * 7 + (('transitions', ('k',)),)
    x = step.StepExtras(phase=k, transitions=k, history=k)
    assert x.stateful == [k, k, k] and x.recorders == [k]


# ---- the C entries: every argument is checked before any HIP call ----------------------------------------------------------------
def test_argument_errors_of_the_c_entries():
    lib, check = _lib.lib, _lib.check
    p8, p16 = ctypes.c_void_p(8), ctypes.c_void_p(16)
    n = 4
    to = (ctypes.c_int * n)(1, -1, -1, 2)
    T_at = (ctypes.c_double * n)(1450.0, 0.0, 0.0, 930.0)
    laws = (_lib.PhaseChangeLaw * n)(*[_lib.PhaseChangeLaw(2.7e5, 1400.0, 1450.0)] * n)
    on = (ctypes.c_int * n)(1, 1, 0, 1)
    C = (ctypes.c_double * n)(*[rho * cp for rho, cp, _ in tc.MATERIALS])
    modes, scal = (ctypes.c_int * 6)(*[1] * 6), (ctypes.c_double * 6)(*[5.0] * 6)
    out = _lib.ptr_array([8, 8, 8])

    def call(nmat=n, to=to, T_at=T_at, laws=laws, on=on, T=p8, ids=p8, f=p16, summary=p8, words=p8, count=p8, dims=(4, 4, 4, 0),
             dx=tc.DX, C=C, modes=modes, coeff=out):
        check(lib.adi_matmap_transition(nmat, to, T_at, laws, on, T, ids, p8, None, p8, None, f, summary, words, count, *dims, dx,
                                        C, modes, scal, None, modes, scal, None, coeff, out, None))
    for kw in (dict(T=None), dict(ids=None), dict(words=None), dict(count=None), dict(to=None)):
        with pytest.raises(ValueError, match='adi_matmap_transition: null argument'):
            call(**kw)
    for kw in (dict(f=None), dict(summary=None), dict(laws=None), dict(on=None)):
        with pytest.raises(ValueError, match='go together'):
            call(**kw)
    with pytest.raises(ValueError, match='aliases'):
        call(f=p8)
    with pytest.raises(ValueError, match='9 materials'):
        call(nmat=9)
    with pytest.raises(ValueError, match='material 0 turns into 4'):
        call(to=(ctypes.c_int * n)(4, -1, -1, 2))
    with pytest.raises(ValueError, match='material 3 turns into 3'):
        call(to=(ctypes.c_int * n)(1, -1, -1, 3))
    with pytest.raises(ValueError, match='threshold of material 3 is not finite'):
        call(T_at=(ctypes.c_double * n)(1450.0, 0.0, 0.0, float('nan')))
    call_ok_T = (ctypes.c_double * n)(1450.0, float('nan'), float('inf'), 930.0)     # (read only where there is a rule)
    with pytest.raises(ValueError, match='bad grid'):
        call(T_at=call_ok_T, dims=(0, 4, 4, 0))
    bad = (_lib.PhaseChangeLaw * n)(*[_lib.PhaseChangeLaw(2.7e5, 1450.0, 1400.0)] * n)
    with pytest.raises(ValueError, match='T_liquidus'):
        call(laws=bad)
    with pytest.raises(ValueError, match='dx must be finite'):
        call(dx=0.0)
    with pytest.raises(ValueError, match='C of material 0'):
        call(C=(ctypes.c_double * n)(0.0, 1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match='bad face mode'):
        call(modes=(ctypes.c_int * 6)(1, 1, 7, 1, 1, 1))
    with pytest.raises(ValueError, match='missing h field'):
        call(modes=(ctypes.c_int * 6)(1, 2, 1, 1, 1, 1))
    with pytest.raises(ValueError, match='null output'):
        call(coeff=_lib.ptr_array([8, None, 8]))
    with pytest.raises(ValueError, match='adi_matmap_brick_sets: null argument'):
        check(lib.adi_matmap_brick_sets(p8, None, None, p8, 4, 4, 4, 0, None))
    with pytest.raises(ValueError, match='adi_matmap_brick_sets: null argument'):
        check(lib.adi_matmap_brick_sets(p8, None, p8, None, 4, 4, 4, 0, None))
    with pytest.raises(ValueError, match='bad grid'):
        check(lib.adi_matmap_brick_sets(p8, None, p8, p8, 4, 0, 4, 0, None))
    with pytest.raises(ValueError, match='plane_stride'):
        check(lib.adi_matmap_brick_sets(p8, None, p8, p8, 4, 4, 4, 15, None))
    assert lib.adi_abi_version() == 18


# ---- the kernels' footprint ----------------------------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_meta
    if not os.path.isdir(kernel_meta.LLVM):
        pytest.skip('no ROCm LLVM tools at %s' % kernel_meta.LLVM)
    ks = [k for k in kernel_meta.all_kernels() if k['obj'] == 'adi_matmap_transition.o']
    names = {re.match(r'adi::(\w+)', k['short']).group(1) for k in ks}
    assert names == {'k_maptransition', 'k_mapbricksets'} and len(ks) == 4 + 2
    for k in ks:
        print('%-36s %3d VGPRs %3d SGPRs %4d B LDS %d B scratch' % (k['short'], k['vgpr_count'], k['sgpr_count'], k['lds'],
                                                                    k['scratch']))
    bad = ['%s: %d B scratch, %d spilled VGPRs' % (k['short'], k['scratch'], k.get('vgpr_spill_count', 0))
           for k in ks if k['scratch'] != 0 or k.get('vgpr_spill_count', 0) != 0]
    assert not bad, '\n'.join(bad)
    # the body the coefficient builds and the transition pass share is one: adi_matmap.hip holds no copy of it
    src = open(os.path.join(ROOT, 'adi_thermal_fields_amd', 'csrc', 'adi_matmap.hip')).read()
    assert 'void map_coeffs_cell' not in src
