"""GPU: which entry points of the library a step calls, how often and in which order -- for every combination of the step's
optional parts and every form of the step.

A pass-through recorder stands in for `lib` in every module of the package that holds it (`_install`): it appends the entry
point's name and calls through.  Entry points that launch nothing (a workspace size, say) are recorded like every other.

Combinations: nothing; a GoldakSource; a source field; surface loss + phase + history + solidification + monitor; `material=`
with a source field and the three recorders; `material_map=` with MapLossPacks, MapPhaseField, a source field and the three
recorders.  Forms: adi_step_numba_coeff (NST calls), StagedStepper.step with events (NST calls), run(graph=False) of NST steps, and
run through the graph with nsteps=2, where the four warm-up steps and the two captured ones pass the recorder and the replay does
not.  A stepper takes no source field, so its three forms run the field combinations without the field (and the combination that
is a field alone has the first form only).

Shapes, the small ones of tests/test_step_forms_gpu.py that take every branch: (20, 18, 35), fused explicit stage + sweep 0
through the general kernel; (72, 12, 20) with the physical box pinned to the logical one, where there is no fused kernel.  The
two-material map runs on (20, 18, 35).

EXPECTED holds the lists as literals.  They were recorded with this same recorder (`trace`) on an MI355X from the PARENT of the
commit that added this file, 2e88301e2567be602d8d446673439a432aa5374a, not from the code under test: the commit folded the
step's optional parts into one record and the two branches of the launch sequence into one, and this is the statement that no
launch moved."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import history_cases as hc  # noqa: E402
import matlaw_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

NST = 3
SHAPES = {'general': (20, 18, 35), 'no_fused_kernel': (72, 12, 20)}
COMBOS = ('nothing', 'goldak', 'field', 'recorders', 'material', 'material_map')
FORMS = ('call', 'step', 'run_plain', 'run_graph')
CASES = [(c, s) for c in COMBOS for s in SHAPES if not (c == 'material_map' and s != 'general')]
# entry points that launch nothing, they answer a question on the host: whether the grid has a fused kernel (once per
# adi_step_numba_coeff call) and the size of the sweeps' workspace (three times, when a grid's scratch is first made)
QUERIES = {'adi_explicit_fused_supported', 'adi_sweep_workspace_bytes'}

# the step's own launches
FUSED = ['adi_explicit_sweep0_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks']
UNFUSED = ['adi_explicit_rhs', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks']
# EXPECTED, (combination, shape name) -> {form: [entry point, ...]}, stands at the end of the file


@pytest.fixture(scope='module')
def hip():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    return hip


class _Recorder:
    """stands in for `lib`: every entry point looked up on it appends its name to `names` when called, and calls through"""

    def __init__(self, lib, names):
        self._lib, self.names = lib, names

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def through(*args):
            self.names.append(name)
            return fn(*args)
        return through


def _install(monkeypatch, names):
    """the recorder in place of `lib` in every module of the package whose `lib` is _lib.lib (_lib itself keeps its own: a
    module imported later must find the library there)"""
    from adi_thermal_fields_amd import _lib
    rec = _Recorder(_lib.lib, names)
    mods = [m for n, m in sorted(sys.modules.items())
            if n.startswith('adi_thermal_fields_amd.') and m is not _lib and getattr(m, '__dict__', {}).get('lib') is _lib.lib]
    assert len(mods) >= 8
    for m in mods:
        monkeypatch.setattr(m, 'lib', rec)


def _inputs(shape):
    """mask with holes, a hot blob in a cold body, two materials split along axis 0"""
    rng = np.random.default_rng(11)
    blob = hc._blob(shape)
    mask = rng.random(shape) > 0.07
    mask[blob] = True
    T0 = np.full(shape, hc.TINF)
    T0[blob] = 1900.0
    ids = np.zeros(shape, dtype=np.uint8)
    ids[shape[0] // 2:] = 1
    return mask, np.where(mask, T0, hc.TINF), blob, ids


def _rig(hip, combo, shape):
    """-> dict(grid, mat, prm, packs, S, source, kw): the arguments of the step for a combination; S is what
    adi_step_numba_coeff takes, source what a stepper takes, kw the other optional parts"""
    mask, T0, blob, ids = _inputs(shape)
    grid = hip.Grid3D(*shape, hc.DX, mask.copy())
    assert not grid.layout.padded
    mat, prm = hip.Material(hc.RHO, hc.CP, hc.K), hip.Params(hc.DT_A, hc.THETA)
    T0d = hip.to_device(T0)
    ctr = [0.5 * (s.start + s.stop) * hc.DX for s in blob]
    src = hip.GoldakSource(power=900.0, eta=0.8, a=1.5e-3, b=1.5e-3, c_f=1.5e-3, c_r=3e-3, f_f=0.6,
                           origin=(ctr[0] - 2 * hc.DX, ctr[1], ctr[2]), velocity=0.02, travel_axis=0, travel_sign=1, depth_axis=2)
    field = hip.to_device(src.sample(grid, 0.5 * hc.DT_A))
    robin = {f: hc.H for f in hc.FACES}
    r = dict(grid=grid, mat=mat, prm=prm, T0=T0d, S=None, source=None, kw={})

    def recorders(mm=None):
        return dict(history=hip.ThermalHistory(grid, hip.HistoryLevels(*hc.LEVELS), capacity=32, T=T0d),
                    solidification=hip.SolidificationRecord(grid, 1425.0, T=T0d),
                    monitor=hip.FieldMonitor(grid, probes=((3, 4, 5),), regions=(None, ((2, 19), (0, 12), (3, 20))), capacity=32,
                                             material_map=mm))

    if combo in ('nothing', 'goldak', 'field'):
        r['packs'] = hip.precompute_coeff_packs_unified(grid, mat, robin_h=robin, robin_Tinf=hc.TINF)
        if combo == 'goldak':
            r['S'] = r['source'] = src
        elif combo == 'field':
            r['S'] = field
    elif combo == 'recorders':
        lp = hip.LossPacks(grid, mat, hip.SurfaceLoss(h=hc.H, emissivity=0.8), hc.TINF)
        r['packs'] = lp.packs
        r['kw'] = dict(surface_loss=lp, phase=hip.PhaseField(grid, mat, hip.PhaseChange(2.7e5, 1400.0, 1450.0), T=T0d),
                       **recorders())
    elif combo == 'material':
        nm = hip.NonlinearPacks(grid, hc.RHO, mc.steel(hip.MaterialLaw), hc.TINF, loss=hip.SurfaceLoss(h=hc.H), T=T0d)
        r.update(mat=nm.mat, packs=nm.packs, S=field)
        r['kw'] = dict(material=nm, **recorders())
    else:
        mats = ((hc.RHO, hc.CP, hc.K), (8900.0, 385.0, 390.0))
        mm = hip.MaterialMap(grid, mats, ids)
        laws = (hip.PhaseChange(2.7e5, 1400.0, 1450.0), None)
        r.update(mat=mm.mat, packs=mm.packs, S=field)
        r['kw'] = dict(material_map=mm, surface_loss=hip.MapLossPacks(mm, hip.SurfaceLoss(h=hc.H, emissivity=0.8), hc.TINF),
                       phase=hip.MapPhaseField(mm, laws, T=T0d), **recorders(mm))
    return r


def trace(hip, monkeypatch, combo, name):
    """{form: the entry points it called, in order}; everything is built before the recorder goes in, one rig per form"""
    import torch
    if name == 'no_fused_kernel':
        monkeypatch.setattr(hip, 'recommended_dims', lambda nx, ny, nz: (nx, ny, nz))
    out = {}
    for form in FORMS:
        if form != 'call' and combo == 'field':
            continue
        r = _rig(hip, combo, SHAPES[name])
        g, mat, prm, packs = r['grid'], r['mat'], r['prm'], r['packs']
        assert hip.fused_supported(g) == (name != 'no_fused_kernel')
        st = None if form == 'call' else hip.StagedStepper(g, mat, prm, packs, hc.TINF, source=r['source'], **r['kw'])
        events = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        T = r['T0']
        names = []
        with monkeypatch.context() as mp:
            _install(mp, names)
            if form == 'call':
                for i in range(NST):
                    T = hip.adi_step_numba_coeff(T, g, mat, prm, packs, Tinf=hc.TINF, S=r['S'], t=i * prm.dt, **r['kw'])
            elif form == 'step':
                for i in range(NST):
                    T = st.step(T, events=events, t=i * prm.dt)
            elif form == 'run_plain':
                T = st.run(T, NST, graph=False)
            else:
                T = st.run(T, 2, graph=True)
                assert st.captures == 1
        torch.cuda.synchronize()
        assert np.isfinite(np.asarray(T)[np.asarray(g.mask, dtype=bool)]).all()
        out[form] = names
    return out


@pytest.mark.parametrize('combo,name', CASES, ids=['%s-%s' % c for c in CASES])
def test_the_entry_points_of_every_form_are_the_parents(hip, monkeypatch, combo, name):
    got = trace(hip, monkeypatch, combo, name)
    want = EXPECTED[combo, name]
    assert sorted(got) == sorted(want)
    for form in FORMS:
        if form in want:
            assert got[form] == want[form], (combo, name, form)


@pytest.mark.parametrize('name', list(SHAPES))
def test_with_every_optional_part_none_only_the_steps_own_launches(hip, monkeypatch, name):
    """the three launches (fused) or four of a step and nothing before, between or after them, in every form; the two QUERIES
    launch nothing and are left out here (EXPECTED holds them too)"""
    own = FUSED if name == 'general' else UNFUSED
    got = trace(hip, monkeypatch, 'nothing', name)
    for form, steps in (('call', NST), ('step', NST), ('run_plain', NST), ('run_graph', 6)):
        assert [n for n in got[form] if n not in QUERIES] == own * steps, (name, form)


# recorded from the parent commit (see the module docstring); repeats are written as list * n
EXPECTED = {
    ('nothing', 'general'): {
        'call': ['adi_explicit_fused_supported', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes',
            'adi_sweep_workspace_bytes'] + ['adi_explicit_sweep0_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks',
            'adi_explicit_fused_supported'] * 2 + ['adi_explicit_sweep0_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks'],
        'step': ['adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes'] +
            ['adi_explicit_sweep0_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks'] * 3,
        'run_plain': ['adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes'] +
            ['adi_explicit_sweep0_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks'] * 3,
        'run_graph': ['adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes'] +
            ['adi_explicit_sweep0_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks'] * 6,
    },
    ('nothing', 'no_fused_kernel'): {
        'call': ['adi_explicit_fused_supported', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes',
            'adi_sweep_workspace_bytes'] + ['adi_explicit_rhs', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks',
            'adi_explicit_fused_supported'] * 2 + ['adi_explicit_rhs', 'adi_sweep_bricks', 'adi_sweep_bricks',
            'adi_sweep_bricks'],
        'step': ['adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes'] + ['adi_explicit_rhs',
            'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks'] * 3,
        'run_plain': ['adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes'] +
            ['adi_explicit_rhs', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks'] * 3,
        'run_graph': ['adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes'] +
            ['adi_explicit_rhs', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks'] * 6,
    },
    ('goldak', 'general'): {
        'call': ['adi_explicit_fused_supported', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes',
            'adi_sweep_workspace_bytes'] + ['adi_explicit_sweep0_bricks', 'adi_source_set', 'adi_source_workspace_bytes',
            'adi_source_lines0', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_explicit_fused_supported'] * 2 +
            ['adi_explicit_sweep0_bricks', 'adi_source_set', 'adi_source_workspace_bytes', 'adi_source_lines0',
            'adi_sweep_bricks', 'adi_sweep_bricks'],
        'step': ['adi_source_set', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes'] +
            ['adi_explicit_sweep0_bricks', 'adi_source_workspace_bytes', 'adi_source_lines0', 'adi_sweep_bricks',
            'adi_sweep_bricks', 'adi_source_set'] * 2 + ['adi_explicit_sweep0_bricks', 'adi_source_workspace_bytes',
            'adi_source_lines0', 'adi_sweep_bricks', 'adi_sweep_bricks'],
        'run_plain': ['adi_source_set', 'adi_source_set', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes',
            'adi_sweep_workspace_bytes'] + ['adi_explicit_sweep0_bricks', 'adi_source_workspace_bytes', 'adi_source_lines0',
            'adi_source_tick', 'adi_sweep_bricks', 'adi_sweep_bricks'] * 3,
        'run_graph': ['adi_source_set', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes']
            + ['adi_explicit_sweep0_bricks', 'adi_source_workspace_bytes', 'adi_source_lines0', 'adi_source_tick',
            'adi_sweep_bricks', 'adi_sweep_bricks'] * 6 + ['adi_source_set'],
    },
    ('goldak', 'no_fused_kernel'): {
        'call': ['adi_explicit_fused_supported', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes',
            'adi_sweep_workspace_bytes'] + ['adi_explicit_rhs', 'adi_sweep_bricks', 'adi_source_set',
            'adi_source_workspace_bytes', 'adi_source_lines0', 'adi_sweep_bricks', 'adi_sweep_bricks',
            'adi_explicit_fused_supported'] * 2 + ['adi_explicit_rhs', 'adi_sweep_bricks', 'adi_source_set',
            'adi_source_workspace_bytes', 'adi_source_lines0', 'adi_sweep_bricks', 'adi_sweep_bricks'],
        'step': ['adi_source_set', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes'] +
            ['adi_explicit_rhs', 'adi_sweep_bricks', 'adi_source_workspace_bytes', 'adi_source_lines0', 'adi_sweep_bricks',
            'adi_sweep_bricks', 'adi_source_set'] * 2 + ['adi_explicit_rhs', 'adi_sweep_bricks', 'adi_source_workspace_bytes',
            'adi_source_lines0', 'adi_sweep_bricks', 'adi_sweep_bricks'],
        'run_plain': ['adi_source_set', 'adi_source_set', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes',
            'adi_sweep_workspace_bytes'] + ['adi_explicit_rhs', 'adi_sweep_bricks', 'adi_source_workspace_bytes',
            'adi_source_lines0', 'adi_source_tick', 'adi_sweep_bricks', 'adi_sweep_bricks'] * 3,
        'run_graph': ['adi_source_set', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes']
            + ['adi_explicit_rhs', 'adi_sweep_bricks', 'adi_source_workspace_bytes', 'adi_source_lines0', 'adi_source_tick',
            'adi_sweep_bricks', 'adi_sweep_bricks'] * 6 + ['adi_source_set'],
    },
    ('field', 'general'): {
        'call': ['adi_explicit_fused_supported', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes',
            'adi_sweep_workspace_bytes'] + ['adi_explicit_rhs_src', 'adi_sweep_bricks', 'adi_sweep_bricks',
            'adi_sweep_bricks', 'adi_explicit_fused_supported'] * 2 + ['adi_explicit_rhs_src', 'adi_sweep_bricks',
            'adi_sweep_bricks', 'adi_sweep_bricks'],
    },
    ('field', 'no_fused_kernel'): {
        'call': ['adi_explicit_fused_supported', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes',
            'adi_sweep_workspace_bytes'] + ['adi_explicit_rhs_src', 'adi_sweep_bricks', 'adi_sweep_bricks',
            'adi_sweep_bricks', 'adi_explicit_fused_supported'] * 2 + ['adi_explicit_rhs_src', 'adi_sweep_bricks',
            'adi_sweep_bricks', 'adi_sweep_bricks'],
    },
    ('recorders', 'general'): {
        'call': ['adi_explicit_fused_supported', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes',
            'adi_sweep_workspace_bytes'] + ['adi_surface_loss_update', 'adi_explicit_sweep0_bricks', 'adi_sweep_bricks',
            'adi_sweep_bricks', 'adi_phase_summary_words', 'adi_phase_apply', 'adi_history_set_clock', 'adi_history_record',
            'adi_history_tick', 'adi_history_set_clock', 'adi_solid_record', 'adi_history_tick', 'adi_monitor_record',
            'adi_history_tick', 'adi_explicit_fused_supported'] * 2 + ['adi_surface_loss_update',
            'adi_explicit_sweep0_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_phase_summary_words',
            'adi_phase_apply', 'adi_history_set_clock', 'adi_history_record', 'adi_history_tick', 'adi_history_set_clock',
            'adi_solid_record', 'adi_history_tick', 'adi_monitor_record', 'adi_history_tick'],
        'step': ['adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes'] +
            ['adi_surface_loss_update', 'adi_explicit_sweep0_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks',
            'adi_phase_summary_words', 'adi_phase_apply', 'adi_history_set_clock', 'adi_history_record', 'adi_history_tick',
            'adi_history_set_clock', 'adi_solid_record', 'adi_history_tick', 'adi_monitor_record', 'adi_history_tick'] * 3,
        'run_plain': ['adi_history_set_clock', 'adi_history_set_clock', 'adi_history_set_clock', 'adi_sweep_workspace_bytes',
            'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes'] + ['adi_surface_loss_update',
            'adi_explicit_sweep0_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_phase_summary_words',
            'adi_phase_apply', 'adi_history_record', 'adi_history_tick', 'adi_solid_record', 'adi_history_tick',
            'adi_monitor_record', 'adi_history_tick'] * 3,
        'run_graph': ['adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes',
            'adi_history_set_clock', 'adi_history_set_clock', 'adi_history_set_clock'] + ['adi_surface_loss_update',
            'adi_explicit_sweep0_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_phase_summary_words',
            'adi_phase_apply', 'adi_history_record', 'adi_history_tick', 'adi_solid_record', 'adi_history_tick',
            'adi_monitor_record', 'adi_history_tick'] * 6 + ['adi_history_set_clock', 'adi_history_set_clock',
            'adi_history_set_clock'],
    },
    ('recorders', 'no_fused_kernel'): {
        'call': ['adi_explicit_fused_supported', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes',
            'adi_sweep_workspace_bytes'] + ['adi_surface_loss_update', 'adi_explicit_rhs', 'adi_sweep_bricks',
            'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_phase_summary_words', 'adi_phase_apply', 'adi_history_set_clock',
            'adi_history_record', 'adi_history_tick', 'adi_history_set_clock', 'adi_solid_record', 'adi_history_tick',
            'adi_monitor_record', 'adi_history_tick', 'adi_explicit_fused_supported'] * 2 + ['adi_surface_loss_update',
            'adi_explicit_rhs', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_phase_summary_words',
            'adi_phase_apply', 'adi_history_set_clock', 'adi_history_record', 'adi_history_tick', 'adi_history_set_clock',
            'adi_solid_record', 'adi_history_tick', 'adi_monitor_record', 'adi_history_tick'],
        'step': ['adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes'] +
            ['adi_surface_loss_update', 'adi_explicit_rhs', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks',
            'adi_phase_summary_words', 'adi_phase_apply', 'adi_history_set_clock', 'adi_history_record', 'adi_history_tick',
            'adi_history_set_clock', 'adi_solid_record', 'adi_history_tick', 'adi_monitor_record', 'adi_history_tick'] * 3,
        'run_plain': ['adi_history_set_clock', 'adi_history_set_clock', 'adi_history_set_clock', 'adi_sweep_workspace_bytes',
            'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes'] + ['adi_surface_loss_update', 'adi_explicit_rhs',
            'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_phase_summary_words', 'adi_phase_apply',
            'adi_history_record', 'adi_history_tick', 'adi_solid_record', 'adi_history_tick', 'adi_monitor_record',
            'adi_history_tick'] * 3,
        'run_graph': ['adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes',
            'adi_history_set_clock', 'adi_history_set_clock', 'adi_history_set_clock'] + ['adi_surface_loss_update',
            'adi_explicit_rhs', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_phase_summary_words',
            'adi_phase_apply', 'adi_history_record', 'adi_history_tick', 'adi_solid_record', 'adi_history_tick',
            'adi_monitor_record', 'adi_history_tick'] * 6 + ['adi_history_set_clock', 'adi_history_set_clock',
            'adi_history_set_clock'],
    },
    ('material', 'general'): {
        'call': ['adi_explicit_fused_supported', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes',
            'adi_sweep_workspace_bytes'] + ['adi_matlaw_loss_update', 'adi_matlaw_theta', 'adi_explicit_rhs_src',
            'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_matlaw_recover', 'adi_history_set_clock',
            'adi_history_record', 'adi_history_tick', 'adi_history_set_clock', 'adi_solid_record', 'adi_history_tick',
            'adi_monitor_record', 'adi_history_tick', 'adi_explicit_fused_supported'] * 2 + ['adi_matlaw_loss_update',
            'adi_matlaw_theta', 'adi_explicit_rhs_src', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks',
            'adi_matlaw_recover', 'adi_history_set_clock', 'adi_history_record', 'adi_history_tick', 'adi_history_set_clock',
            'adi_solid_record', 'adi_history_tick', 'adi_monitor_record', 'adi_history_tick'],
        'step': ['adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes'] +
            ['adi_matlaw_loss_update', 'adi_matlaw_theta', 'adi_explicit_sweep0_bricks', 'adi_sweep_bricks',
            'adi_sweep_bricks', 'adi_matlaw_recover', 'adi_history_set_clock', 'adi_history_record', 'adi_history_tick',
            'adi_history_set_clock', 'adi_solid_record', 'adi_history_tick', 'adi_monitor_record', 'adi_history_tick'] * 3,
        'run_plain': ['adi_history_set_clock', 'adi_history_set_clock', 'adi_history_set_clock', 'adi_sweep_workspace_bytes',
            'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes'] + ['adi_matlaw_loss_update', 'adi_matlaw_theta',
            'adi_explicit_sweep0_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_matlaw_recover', 'adi_history_record',
            'adi_history_tick', 'adi_solid_record', 'adi_history_tick', 'adi_monitor_record', 'adi_history_tick'] * 3,
        'run_graph': ['adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes',
            'adi_history_set_clock', 'adi_history_set_clock', 'adi_history_set_clock'] + ['adi_matlaw_loss_update',
            'adi_matlaw_theta', 'adi_explicit_sweep0_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_matlaw_recover',
            'adi_history_record', 'adi_history_tick', 'adi_solid_record', 'adi_history_tick', 'adi_monitor_record',
            'adi_history_tick'] * 6 + ['adi_history_set_clock', 'adi_history_set_clock', 'adi_history_set_clock'],
    },
    ('material', 'no_fused_kernel'): {
        'call': ['adi_explicit_fused_supported', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes',
            'adi_sweep_workspace_bytes'] + ['adi_matlaw_loss_update', 'adi_matlaw_theta', 'adi_explicit_rhs_src',
            'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_matlaw_recover', 'adi_history_set_clock',
            'adi_history_record', 'adi_history_tick', 'adi_history_set_clock', 'adi_solid_record', 'adi_history_tick',
            'adi_monitor_record', 'adi_history_tick', 'adi_explicit_fused_supported'] * 2 + ['adi_matlaw_loss_update',
            'adi_matlaw_theta', 'adi_explicit_rhs_src', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks',
            'adi_matlaw_recover', 'adi_history_set_clock', 'adi_history_record', 'adi_history_tick', 'adi_history_set_clock',
            'adi_solid_record', 'adi_history_tick', 'adi_monitor_record', 'adi_history_tick'],
        'step': ['adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes'] +
            ['adi_matlaw_loss_update', 'adi_matlaw_theta', 'adi_explicit_rhs', 'adi_sweep_bricks', 'adi_sweep_bricks',
            'adi_sweep_bricks', 'adi_matlaw_recover', 'adi_history_set_clock', 'adi_history_record', 'adi_history_tick',
            'adi_history_set_clock', 'adi_solid_record', 'adi_history_tick', 'adi_monitor_record', 'adi_history_tick'] * 3,
        'run_plain': ['adi_history_set_clock', 'adi_history_set_clock', 'adi_history_set_clock', 'adi_sweep_workspace_bytes',
            'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes'] + ['adi_matlaw_loss_update', 'adi_matlaw_theta',
            'adi_explicit_rhs', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_matlaw_recover',
            'adi_history_record', 'adi_history_tick', 'adi_solid_record', 'adi_history_tick', 'adi_monitor_record',
            'adi_history_tick'] * 3,
        'run_graph': ['adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes',
            'adi_history_set_clock', 'adi_history_set_clock', 'adi_history_set_clock'] + ['adi_matlaw_loss_update',
            'adi_matlaw_theta', 'adi_explicit_rhs', 'adi_sweep_bricks', 'adi_sweep_bricks', 'adi_sweep_bricks',
            'adi_matlaw_recover', 'adi_history_record', 'adi_history_tick', 'adi_solid_record', 'adi_history_tick',
            'adi_monitor_record', 'adi_history_tick'] * 6 + ['adi_history_set_clock', 'adi_history_set_clock',
            'adi_history_set_clock'],
    },
    ('material_map', 'general'): {
        'call': ['adi_explicit_fused_supported', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes',
            'adi_sweep_workspace_bytes'] + ['adi_matmap_loss_update', 'adi_matmap_explicit', 'adi_matmap_sweep',
            'adi_matmap_sweep', 'adi_matmap_sweep', 'adi_phase_summary_words', 'adi_matmap_phase_apply',
            'adi_history_set_clock', 'adi_history_record', 'adi_history_tick', 'adi_history_set_clock', 'adi_solid_record',
            'adi_history_tick', 'adi_monitor_record', 'adi_history_tick', 'adi_explicit_fused_supported'] * 2 +
            ['adi_matmap_loss_update', 'adi_matmap_explicit', 'adi_matmap_sweep', 'adi_matmap_sweep', 'adi_matmap_sweep',
            'adi_phase_summary_words', 'adi_matmap_phase_apply', 'adi_history_set_clock', 'adi_history_record',
            'adi_history_tick', 'adi_history_set_clock', 'adi_solid_record', 'adi_history_tick', 'adi_monitor_record',
            'adi_history_tick'],
        'step': ['adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes'] +
            ['adi_matmap_loss_update', 'adi_matmap_explicit', 'adi_matmap_sweep', 'adi_matmap_sweep', 'adi_matmap_sweep',
            'adi_phase_summary_words', 'adi_matmap_phase_apply', 'adi_history_set_clock', 'adi_history_record',
            'adi_history_tick', 'adi_history_set_clock', 'adi_solid_record', 'adi_history_tick', 'adi_monitor_record',
            'adi_history_tick'] * 3,
        'run_plain': ['adi_history_set_clock', 'adi_history_set_clock', 'adi_history_set_clock', 'adi_sweep_workspace_bytes',
            'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes'] + ['adi_matmap_loss_update', 'adi_matmap_explicit',
            'adi_matmap_sweep', 'adi_matmap_sweep', 'adi_matmap_sweep', 'adi_phase_summary_words', 'adi_matmap_phase_apply',
            'adi_history_record', 'adi_history_tick', 'adi_solid_record', 'adi_history_tick', 'adi_monitor_record',
            'adi_history_tick'] * 3,
        'run_graph': ['adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes', 'adi_sweep_workspace_bytes',
            'adi_history_set_clock', 'adi_history_set_clock', 'adi_history_set_clock'] + ['adi_matmap_loss_update',
            'adi_matmap_explicit', 'adi_matmap_sweep', 'adi_matmap_sweep', 'adi_matmap_sweep', 'adi_phase_summary_words',
            'adi_matmap_phase_apply', 'adi_history_record', 'adi_history_tick', 'adi_solid_record', 'adi_history_tick',
            'adi_monitor_record', 'adi_history_tick'] * 6 + ['adi_history_set_clock', 'adi_history_set_clock',
            'adi_history_set_clock'],
    },
}
