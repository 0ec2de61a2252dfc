"""The Cartesian backend is one module per concern behind the facade adi3d_hip_coeff: what the facade exports and from where,
that every module imports on its own, that none of them leans on the facade, and that the facade defines nothing.  No GPU."""
import ast
import importlib
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PKG = 'adi_thermal_fields_amd'
# in import order: a module imports only from those before it (and _lib, _ledger)
MODULES = ['fields', 'packs', 'heat_source', 'deposition', 'surface_loss', 'phase', 'history', 'step']
# the slab decomposition: dist_slab (SlabStepper) re-exports the comms of slab_comm and the HipEngine of slab_engine
SLAB_MODULES = ['slab_comm', 'slab_engine', 'dist_slab']

ALL = ['Grid3D', 'Material', 'Params', 'AxisCoeffPack', 'exposed_mask', 'precompute_coeff_packs_unified',
       'adi_step_hip_coeff', 'adi_step_numba_coeff', 'adi_step_gpu_coeff', 'DeviceField', 'to_device',
       'adi_explicit_rhs', 'adi_sweep_axis', 'StagedStepper', 'Layout', 'apply_surface_impulse_Q',
       'exposed_faces_per_layer', 'count_exposed_faces', 'perimeter_ratio', 'birth_planes', 'BirthPacks',
       'GoldakSource', 'ScanPath', 'SurfaceLoss', 'LossPacks', 'PhaseChange', 'PhaseField', 'HistoryLevels',
       'ThermalHistory']

# every name the facade hands out -> the module that owns it
HOME = {
    '_lib': ['lib', 'check', 'ptr_array'],
    'fields': ['_MASK_VERSIONS', '_device', '_stream', '_p', '_sweep_workspace_bytes', 'recommended_dims', 'Layout',
               'DeviceField', 'to_device', 'Grid3D', '_wrap'],
    'packs': ['Material', 'Params', 'AxisCoeffPack', 'exposed_mask', '_fc_arg', 'precompute_coeff_packs_unified'],
    'heat_source': ['GoldakSource', 'ScanPath', '_source_block', '_source_work'],
    'deposition': ['apply_surface_impulse_Q', 'exposed_faces_per_layer', 'count_exposed_faces', 'perimeter_ratio',
                   'birth_planes', 'BirthPacks'],
    'surface_loss': ['SurfaceLoss', 'LossPacks'],
    'phase': ['PhaseChange', 'PhaseField'],
    'history': ['HistoryLevels', 'ThermalHistory'],
    'step': ['adi_explicit_rhs', 'adi_sweep_axis', 'adi_explicit_sweep_axis0', 'adi_step_hip_coeff', 'adi_step_numba_coeff',
             'adi_step_gpu_coeff', 'StagedStepper', 'fused_supported', 'valid_range', '_sparse_arg', '_sweep_into',
             '_explicit_sweep0_into', '_explicit_src_into', '_source_lines0_into'],
}


@pytest.fixture(scope='module')
def hip():
    return importlib.import_module(PKG + '.adi3d_hip_coeff')


def test_all_is_unchanged(hip):
    assert hip.__all__ == ALL


def test_every_exported_name_is_its_home_modules_object(hip):
    listed = [n for names in HOME.values() for n in names]
    assert len(listed) == len(set(listed))
    assert set(ALL) <= set(listed)
    for mod, names in HOME.items():
        home = importlib.import_module('%s.%s' % (PKG, mod))
        for n in names:
            assert getattr(hip, n) is getattr(home, n), (mod, n)


@pytest.fixture(scope='module')
def fresh_imports():
    """one fresh interpreter per module, all started at once (an interpreter spends its time importing torch)"""
    procs = {m: subprocess.Popen([sys.executable, '-c', 'import %s.%s' % (PKG, m)], cwd=ROOT, stdout=subprocess.DEVNULL,
                                 stderr=subprocess.PIPE, text=True) for m in MODULES + SLAB_MODULES}
    return {m: (p.communicate()[1], p.returncode) for m, p in procs.items()}


@pytest.mark.parametrize('mod', MODULES + SLAB_MODULES)
def test_module_imports_on_its_own(fresh_imports, mod):
    """(a cycle that only works once the facade has imported everything in order shows up here)"""
    err, rc = fresh_imports[mod]
    assert rc == 0, err[-2000:]


def _imports(mod):
    """what a module's source imports from its own package: {module name}, the package itself as ''"""
    with open(os.path.join(ROOT, PKG, mod + '.py')) as f:
        tree = ast.parse(f.read())
    found = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and (node.level == 1 or (node.module or '').split('.')[0] == PKG):
            sub = (node.module or '') if node.level == 1 else '.'.join((node.module or '').split('.')[1:])
            found |= {sub.split('.')[0]} if sub else {a.name for a in node.names}
        elif isinstance(node, ast.Import):
            found |= {a.name.split('.')[1] for a in node.names if a.name.startswith(PKG + '.')}
    return found


@pytest.mark.parametrize('mod', MODULES)
def test_no_module_imports_the_facade_and_the_order_holds(mod):
    found = _imports(mod)
    assert 'adi3d_hip_coeff' not in found
    allowed = set(MODULES[:MODULES.index(mod)]) | {'_lib', '_ledger'}
    assert found <= allowed, (mod, sorted(found - allowed))


@pytest.mark.parametrize('mod', SLAB_MODULES + ['adi3d_hip_cyl', 'frame_io', 'voxel_bc_correction', 'waam'])
def test_the_packages_other_modules_import_from_the_new_homes(mod):
    """(slab_engine.HipEngine alone keeps its one handle on the facade, taken inside its constructor)"""
    with open(os.path.join(ROOT, PKG, mod + '.py')) as f:
        tree = ast.parse(f.read())
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert not any('adi3d_hip_coeff' in ast.dump(n) for n in top)
    if mod != 'slab_engine':
        assert 'adi3d_hip_coeff' not in _imports(mod)


def test_the_facade_defines_nothing(hip):
    for name, obj in vars(hip).items():
        if name.startswith('_'):
            continue
        owner = getattr(obj, '__module__', None)
        if owner is not None:
            assert owner != hip.__name__, name
    with open(hip.__file__) as f:
        tree = ast.parse(f.read())
    assert not [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef))]


def test_module_state_exists_once_and_assignment_reaches_the_home(hip):
    fields = importlib.import_module(PKG + '.fields')
    assert hip._MASK_VERSIONS is fields._MASK_VERSIONS
    assert hip.Grid3D is fields.Grid3D
    # what the GPU tests do to force a padded box: monkeypatch.setattr(hip, 'recommended_dims', ...) must be seen by Layout
    real = fields.recommended_dims
    fake = lambda nx, ny, nz: (nx + 1, ny + 2, nz + 3)      # noqa: E731
    try:
        hip.recommended_dims = fake
        assert fields.recommended_dims is fake
    finally:
        hip.recommended_dims = real
    assert fields.recommended_dims is real and hip.recommended_dims is real


def test_dist_slab_hands_out_the_moved_names_themselves():
    slab, comm, engine = (importlib.import_module('%s.%s' % (PKG, m)) for m in ('dist_slab', 'slab_comm', 'slab_engine'))
    assert slab.__all__ == ['SlabStepper', 'TorchDistComm', 'HostStagedDistComm', 'LocalComm', 'LoopbackComm', 'SelfLoopDistComm',
                            'HipEngine', 'split_planes', 'rccl_env_defaults', 'gather_slabs']
    for n in comm.__all__:
        assert getattr(slab, n) is getattr(comm, n), n
    assert slab.HipEngine is engine.HipEngine and engine.__all__ == ['HipEngine']
    assert set(comm.__all__) | {'HipEngine', 'SlabStepper'} == set(slab.__all__)
