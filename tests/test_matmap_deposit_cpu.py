"""CPU: a MaterialMap carried through births, deposits and a moving source -- the argument checks of the three new
C entries (before any HIP call), the keyword checks of PathDeposit and MapSource (no device), the footprint of the new kernels,
and the NumPy definition of the driver loop (matmap_deposit_cases.definition_loop) under a partition of its steps."""
import ctypes
import os
import sys

import numpy as np
import pytest

import bead_cases as bc
import matmap_cases as mc
import matmap_deposit_cases as dc
from adi_thermal_fields_amd import _lib
from adi_thermal_fields_amd._lib import lib, check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('adi_matmap_build_coeffs_planes', 'adi_bead_deposit_ids', 'adi_matmap_source_add_r0')
P8 = ctypes.c_void_p(64)                                   # a non-null "device" pointer no check may follow
I6, D6 = ctypes.c_int * 6, ctypes.c_double * 6


def test_new_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, 'include', 'adi_hip.h')).read()
    for n in NEW:
        assert n + '(' in hdr and hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert lib.adi_abi_version() == 18


def _planes(k0, k1, nmat=2, C=(3.8e6, 3.4e6), ids=P8, nz=6):
    out3 = _lib.ptr_array([64, 64, 64])
    Cv = (ctypes.c_double * len(C))(*C)
    return lib.adi_matmap_build_coeffs_planes(P8, ids, 4, 5, nz, 0, 1e-3, nmat, Cv, I6(*[1] * 6), D6(*[10.0] * 6), None, I6(*[0] * 6),
                                              D6(*[0.0] * 6), None, out3, out3, k0, k1, None)


@pytest.mark.parametrize('k0,k1', [(2, 2), (3, 2), (-1, 2), (0, 7), (6, 6)])
def test_plane_build_refuses_an_empty_or_out_of_box_range(k0, k1):
    with pytest.raises(ValueError, match=r'adi_matmap_build_coeffs_planes: bad plane range'):
        check(_planes(k0, k1))


def test_plane_build_checks_tables_and_pointers_like_the_full_build():
    with pytest.raises(ValueError, match='null argument'):
        check(_planes(0, 1, ids=None))
    with pytest.raises(ValueError, match=r'9 materials \(1 to 8\)'):
        check(_planes(0, 1, nmat=9, C=(1.0,) * 9))
    with pytest.raises(ValueError, match='C of material 1 must be finite and > 0'):
        check(_planes(0, 1, C=(3.8e6, 0.0)))
    with pytest.raises(ValueError, match='C of material 0 must be finite and > 0'):
        check(_planes(0, 1, C=(-1.0, 1.0)))


def _deposit_ids(ids=P8, mid=1, active=P8):
    shape = _lib.BeadShape(2e-3, 2e-3, 0, 2)
    path = bc.BY_NAME['leg_plus_u'].path
    table = np.ascontiguousarray(path.table())
    return lib.adi_bead_deposit_ids(ctypes.byref(shape), table.ctypes.data, P8, len(table), float(path.t_end), P8, active, None, ids,
                                    mid, 8, 8, 8, 8, 8, 8, 0, 1e-3, 0.0, 0.1, 1700.0, P8, None)


def test_stamping_deposit_checks_the_id_field_and_the_id():
    with pytest.raises(ValueError, match='adi_bead_deposit_ids: null id field'):
        check(_deposit_ids(ids=None))
    for bad in (-1, _lib.MATMAP_MAX, 255):                 # the entry knows no table: an id beyond ADI_MATMAP_MAX names no material
        with pytest.raises(ValueError, match='adi_bead_deposit_ids: material id'):
            check(_deposit_ids(mid=bad))
    with pytest.raises(ValueError, match='aliases a mask'):
        check(_deposit_ids(ids=P8, active=P8))


def _source_add(nmat=2, C=(3.8e6, 3.4e6), ids=P8, dt=1e-3, blk=P8):
    from adi_thermal_fields_amd.heat_source import GoldakSource
    src = GoldakSource(origin=(4e-3, 4e-3, 8e-3), **dc.SRC_KW)
    Cv = (ctypes.c_double * len(C))(*C)
    return lib.adi_matmap_source_add_r0(blk, ctypes.byref(src.as_c()), P8, P8, ids, 8, 8, 8, 0, 1e-3, dt, nmat, Cv, None)


def test_map_source_entry_validates_before_any_hip_call():
    with pytest.raises(ValueError, match='adi_matmap_source_add_r0: null argument'):
        check(_source_add(ids=None))
    with pytest.raises(ValueError, match='adi_matmap_source_add_r0: null argument'):
        check(_source_add(blk=None))
    with pytest.raises(ValueError, match=r'9 materials \(1 to 8\)'):
        check(_source_add(nmat=9, C=(1.0,) * 9))
    with pytest.raises(ValueError, match='C of material 1 must be finite and > 0'):
        check(_source_add(C=(1.0, -2.0)))
    with pytest.raises(ValueError, match='bad dx / dt'):
        check(_source_add(dt=0.0))
    with pytest.raises(ValueError, match='adi_matmap_source_add_r0'):
        check(lib.adi_matmap_source_add_r0(P8, None, P8, P8, P8, 8, 8, 8, 0, 1e-3, 1e-3, 1, (ctypes.c_double * 1)(1.0), None))


# ---- the Python keyword checks, without a device ---------------------------------------------------------------------------
class _FakeMap:
    """stands where a MaterialMap would, for the checks that come before its type is looked at"""


def _bare_map(grid, n=3):
    from adi_thermal_fields_amd.packs import MaterialMap, Material
    mm = MaterialMap.__new__(MaterialMap)                  # (no device here: the attributes the checks read)
    mm.grid, mm.materials = grid, tuple(Material(*m) for m in mc.MATERIALS[:n])
    return mm


def test_path_deposit_keyword_checks():
    from adi_thermal_fields_amd.deposition import PathDeposit
    case = bc.BY_NAME['leg_plus_u']
    g = bc.HostGrid(case.shape, bc.DX, case.active)
    with pytest.raises(ValueError, match='material_map and material_id go together'):
        PathDeposit(g, case.path, case.bead, bc.TS, material_id=1)
    with pytest.raises(ValueError, match='material_map and material_id go together'):
        PathDeposit(g, case.path, case.bead, bc.TS, material_map=_bare_map(g))
    with pytest.raises(TypeError, match='must be a MaterialMap'):
        PathDeposit(g, case.path, case.bead, bc.TS, material_map=_FakeMap(), material_id=0)
    with pytest.raises(ValueError, match='another grid'):
        PathDeposit(g, case.path, case.bead, bc.TS, material_map=_bare_map(bc.HostGrid(case.shape, bc.DX, case.active)), material_id=0)
    for bad in (3, -1, 1.0, True):
        with pytest.raises(ValueError, match='material_id must be an integer from 0 to 2'):
            PathDeposit(g, case.path, case.bead, bc.TS, material_map=_bare_map(g), material_id=bad)
    dep = PathDeposit(g, case.path, case.bead, bc.TS, material_map=_bare_map(g), material_id=np.uint8(2))
    assert dep.material_id == 2 and isinstance(dep.material_id, int)
    assert PathDeposit(g, case.path, case.bead, bc.TS).material_map is None


def test_map_source_checks_and_is_no_goldak_source():
    from adi_thermal_fields_amd.heat_source import GoldakSource
    from adi_thermal_fields_amd.matmap_extras import MapSource
    from adi_thermal_fields_amd.packs import Params
    from adi_thermal_fields_amd import step
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    assert hip.MapSource is MapSource and 'MapSource' not in hip.__all__
    case = bc.BY_NAME['leg_plus_u']
    g = bc.HostGrid(case.shape, bc.DX, case.active)
    src = GoldakSource(origin=(4e-3, 4e-3, 8e-3), **dc.SRC_KW)
    with pytest.raises(TypeError, match='mm must be a MaterialMap'):
        MapSource(_FakeMap(), src)
    with pytest.raises(TypeError, match='src must be a GoldakSource'):
        MapSource(_bare_map(g), object())
    ms = MapSource(_bare_map(g), src)
    assert not isinstance(ms, GoldakSource) and ms.mm.grid is g and ms.shape_key() == ('map',) + src.shape_key()
    # without material_map= it is refused, before anything is launched (no device is there to launch on)
    with pytest.raises(ValueError, match='a MapSource needs material_map='):
        step._check_extras(g, ms.mm.materials[0], Params(1e-3), (None, None, None), step.StepExtras(source=ms))


# ---- the definition of the driver loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['jump_whole', 'corner', 'ragged_raster', 'corner_depth_axis_0'])
def test_births_and_ids_of_a_partition_equal_those_of_one_step(name):
    case = bc.BY_NAME[name]
    ids0 = dc.random_ids(case.shape, 3)
    ids0[case.active] = 0
    t0, span = case.whole()
    one_mask, one_ids = dc.births_and_ids(case, [(t0, span)], ids0)
    assert (one_mask & ~case.active).any()
    born = one_mask & ~case.active
    assert np.array_equal(one_ids, np.where(born, dc.WIRE, ids0)) and np.array_equal(one_ids[~born], ids0[~born])
    for cuts in ((0.5,), (0.21, 0.22, 0.8), tuple(np.linspace(0.05, 0.95, 13))):
        mask, ids = dc.births_and_ids(case, dc.partition(t0, t0 + span, cuts), ids0)
        assert np.array_equal(mask, one_mask) and np.array_equal(ids, one_ids), cuts


def test_a_second_wire_stamps_only_its_own_newborn_cells_in_the_definition():
    a, b = bc.BY_NAME['leg_plus_u'], bc.BY_NAME['leg_plus_v']
    ids0 = np.zeros(a.shape, np.uint8)
    mask, ids = dc.births_and_ids(a, [a.whole()], ids0, 1)
    born_a = mask & ~a.active
    born_b = b.reference(*b.whole(), active=mask)
    ids2 = dc.stamp(ids, born_b, 2)
    assert born_a.any() and born_b.any() and not (born_a & born_b).any()
    assert (ids2[born_a] == 1).all() and (ids2[born_b] == 2).all() and (ids2[~(born_a | born_b)] == 0).all()


def test_definition_loop_splits_at_a_step_boundary():
    """the loop over 12 steps is the loop over the first 5 continued over the other 7: nothing of it depends on what came
    before but (T, mask, ids)"""
    from adi_thermal_fields_amd.heat_source import ScanPath
    from adi_thermal_fields_amd.deposition import BeadProfile, PathDeposit
    from adi_thermal_fields_amd.packs import MaterialMap
    shape, dx = bc.SHAPES[0], bc.DX
    P = lambda u, v: (u * dx, v * dx, 6.3 * dx)            # noqa: E731
    path = ScanPath(power=200.0, start=P(4.37, 6.21), t_start=0.125, **bc.GOLDAK)
    path.line_to(P(18.13, 6.21), 40 * dx).line_to(P(18.13, 10.47), 120 * dx, power=0.0).line_to(P(4.37, 10.47), 40 * dx)
    bead = BeadProfile(3.3 * dx, 2.4 * dx, 'parabola')
    plate = np.zeros(shape, bool)
    plate[:, :, :4] = True
    ids0 = dc.random_ids(shape, 5)
    ids0[plate] = 0
    from adi_thermal_fields_amd.waam import path_steps
    steps = path_steps(path.t_start, path.t_end, (path.t_end - path.t_start) / 11.5)
    assert len(steps) == 12
    robin = {f: 35.0 for f in dc.ROBIN}
    T, mask, ids = dc.definition_loop(path, bead, plate, ids0, dc.MATERIALS, dc.WIRE, steps, dx, 300.0, bc.TS, 0.5, robin, heat=True)
    assert mask.sum() > plate.sum() and (ids[mask & ~plate] == dc.WIRE).all() and np.array_equal(ids[~(mask & ~plate)], ids0[~(mask & ~plate)])
    assert np.isfinite(T).all() and T.max() > 1000.0 and np.array_equal(T[~mask], np.full((~mask).sum(), 300.0))
    # continued by hand from the state after 5 steps
    T5, m5, i5 = dc.definition_loop(path, bead, plate, ids0, dc.MATERIALS, dc.WIRE, steps[:5], dx, 300.0, bc.TS, 0.5, robin, heat=True)
    Tc, mc_, ic = T5, m5, i5
    for t, d in steps[5:]:
        born = PathDeposit.reference(path, bead, shape, dx, t, d, active=mc_)
        ic = dc.stamp(ic, born, dc.WIRE)
        Tc = np.where(born, bc.TS, Tc)
        mc_ = mc_ | born
        pk = MaterialMap.packs_reference(mc_, ic, dc.MATERIALS, dx, robin_h=robin)
        Tc = MaterialMap.step_reference(Tc, mc_, ic, dc.MATERIALS, dx, d, 0.5, pk, 300.0, S=path.sample_step(bc.HostGrid(shape, dx, mc_), t, d))
    assert np.array_equal(Tc, T) and np.array_equal(mc_, mask) and np.array_equal(ic, ids)


def test_long_double_source_field_agrees_with_the_host_evaluator():
    from adi_thermal_fields_amd.heat_source import GoldakSource
    shape = mc.HOLES
    src = GoldakSource(origin=(8.4e-3, 9.2e-3, 35e-3), **dc.SRC_KW)
    mask = np.ones(shape, bool)
    q64 = src.sample(bc.HostGrid(shape, mc.DX, mask), 0.07)
    qld = dc.source_field_ld(src, shape, mc.DX, mask, 0.07)
    assert qld.dtype == np.longdouble and q64.max() > 0
    inside = (q64 > 0) & (qld > 0)
    assert inside.sum() > 100 and np.max(np.abs(qld[inside].astype(np.float64) - q64[inside]) / q64[inside]) <= 1e-13


# ---- footprint ----------------------------------------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_meta
    if not os.path.isdir(kernel_meta.LLVM):
        pytest.skip('no ROCm LLVM tools at %s' % kernel_meta.LLVM)
    ks = {k['short']: k for k in kernel_meta.all_kernels()}
    for name in ('adi::k_mapcoeffs_planes', 'adi::k_mapsource_add_r0', 'adi::k_bead_deposit'):
        assert name in ks, name
        assert ks[name]['scratch'] == 0 and ks[name].get('vgpr_spill_count', 0) == 0, ks[name]
