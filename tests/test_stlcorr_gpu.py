"""GPU: the STL correction of voxel Robin coefficients (adi_thermal_fields_amd.voxel_bc_correction, csrc/adi_stlcorr.hip)
against the reference's fields (tests/golden/stlcorr_*.npz, written by tests/golden/make_golden_stlcorr.py).

Bounds.  The set of non-zero cells of every field must be the reference's exactly: that is the binning, and the fixtures
keep every centroid at least 1e-9 dx away from a voxel boundary.  A value may differ by n_max * 2^-52 relative, the bound
for sums of n_max positive terms taken in another order, n_max read from the fixture; the device adds in the
reference's order, so the differences measured so far are zero.  At scale there is no reference: for an
all-true mask that contains the mesh every sub-triangle lands, so each projected-area field sums to
sum(area * max(+-n_c, 0)) over the triangles, within N * 2^-52 relative for N sub-triangles.
"""
import math
import os

import numpy as np
import pytest

import cases
from helpers import GOLDEN, rel_linf
from stlcorr_meshes import subdivisions, tube_triangles

pytestmark = pytest.mark.gpu

FACES = ('x-', 'x+', 'y-', 'y+', 'z-', 'z+')
CASES = ['cyl64', 'cyl700', 'frustum', 'offgrid_sub1', 'offgrid_sub3', 'empty', 'small']
EPS = 2.0 ** -52


class Mesh:
    """the fixture's arrays as the mesh object the reference was given"""

    def __init__(self, g):
        self.triangles, self.face_normals, self.area_faces = g['triangles'], g['normals'], g['areas']
        self.triangles_center = g['triangles'].mean(axis=1)


def _load(name):
    g = np.load(os.path.join(GOLDEN, 'stlcorr_%s.npz' % name))
    base_h = {str(f): float(v) for f, v in zip(g['base_faces'], g['base_vals'])}
    return g, base_h


def _corrector(g, mask=None):
    from adi_thermal_fields_amd.voxel_bc_correction import STLBoundaryCorrector
    return STLBoundaryCorrector(Mesh(g), g['mask'] if mask is None else mask, g['origin'], float(g['dx']),
                                max_subdiv=int(g['max_subdiv']), area_epsilon=float(g['area_epsilon']))


def _compare(what, got, want, n_max):
    """same non-zero cells, values within n_max * 2^-52 relative; -> largest relative difference"""
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == want.shape, what
    assert np.array_equal(got != 0.0, want != 0.0), '%s: %d cells differ in being zero' % (
        what, int(np.count_nonzero((got != 0.0) != (want != 0.0))))
    nz = want != 0.0
    worst = float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0
    assert worst <= n_max * EPS, '%s: relative difference %.3e above %d * 2^-52' % (what, worst, n_max)
    return worst


@pytest.mark.parametrize('fallback', [True, False], ids=['fallback', 'nofallback'])
@pytest.mark.parametrize('name', CASES)
def test_fields_equal_the_reference(name, fallback):
    g, base_h = _load(name)
    n_max, tag = int(g['n_max']), 'on' if fallback else 'off'
    robin, scale = _corrector(g).build_corrected_fields(base_h, fallback_to_base=fallback)
    assert list(robin) == list(base_h) and list(scale) == list(base_h)          # the reference's keys, in its order
    worst = 0.0
    for f in base_h:
        worst = max(worst, _compare('robin ' + f, robin[f], g['robin_%s_%s' % (tag, f)], n_max),
                    _compare('scale ' + f, scale[f], g['scale_%s_%s' % (tag, f)], n_max))
        if fallback and base_h[f] != 0.0:
            fell = (g['count'][FACES.index(f)] == 0) & (g['robin_on_' + f] != 0.0)   # no contribution, yet a value
            assert np.all(robin[f][fell] == base_h[f]) and np.all(scale[f][fell] == 1.0), f
        if base_h[f] == 0.0:
            assert not robin[f].any() and not scale[f].any(), f
    print('STLCORR %s %s: %d sub-triangles, n_max %d, largest relative difference %.3e (bound %.3e)'
          % (name, tag, int(g['n_sub']), n_max, worst, n_max * EPS))


@pytest.mark.parametrize('name', CASES)
def test_projected_area_fields_equal_the_reference(name):
    g, _ = _load(name)
    area = _corrector(g).projected_area_fields()
    assert list(area) == list(FACES)
    worst = max(_compare('area ' + f, area[f], g['area_' + f], int(g['n_max'])) for f in FACES)
    assert all(np.array_equal(area[f] != 0.0, g['count'][i] != 0) for i, f in enumerate(FACES))
    print('STLCORR area %s: largest relative difference %.3e' % (name, worst))


def test_wrapper_and_device_mask_give_the_same_fields():
    """build_corrected_robin_fields (the reference's helper) on a NumPy mask, and the corrector on a device mask: tensor,
    bool tensor and DeviceField"""
    import torch
    from adi_thermal_fields_amd.adi3d_hip_coeff import DeviceField
    from adi_thermal_fields_amd.voxel_bc_correction import build_corrected_robin_fields
    g, base_h = _load('cyl64')
    robin, scale = build_corrected_robin_fields(Mesh(g), g['mask'], g['origin'], float(g['dx']), base_h)
    for f in base_h:
        _compare('robin ' + f, robin[f], g['robin_on_' + f], int(g['n_max']))
        _compare('scale ' + f, scale[f], g['scale_on_' + f], int(g['n_max']))
    d_bool = torch.from_numpy(g['mask']).cuda()
    for m in (d_bool, d_bool.to(torch.uint8), DeviceField(d_bool.to(torch.float64))):
        r2, s2 = _corrector(g, mask=m).build_corrected_fields(base_h)
        for f in base_h:
            assert isinstance(r2[f], torch.Tensor) and r2[f].is_cuda and r2[f].dtype == torch.float64
            assert np.array_equal(r2[f].cpu().numpy(), robin[f]) and np.array_equal(s2[f].cpu().numpy(), scale[f]), f


def test_two_runs_give_the_same_bits():
    import torch
    g, base_h = _load('cyl700')
    d_mask = torch.from_numpy(g['mask']).cuda()
    a = _corrector(g, mask=d_mask).build_corrected_fields(base_h)
    b = _corrector(g, mask=d_mask).build_corrected_fields(base_h)
    for x, y in zip(a, b):
        for f in base_h:
            assert torch.equal(x[f], y[f]), f
    pa, pb = _corrector(g, mask=d_mask).projected_area_fields(), _corrector(g, mask=d_mask).projected_area_fields()
    assert all(torch.equal(pa[f], pb[f]) for f in FACES)


@pytest.mark.parametrize('name', ['cyl64', 'frustum'])
def test_packs_from_device_fields_step_like_the_oracle(name):
    """mask and fields never leave HBM: Grid3D's device mask -> corrector -> robin_h of precompute_coeff_packs_unified ->
    three Cartesian steps, against the pinned oracle fed with the reference's (golden) fields"""
    import adi_thermal_fields_amd.adi3d_hip_coeff as hip
    from oracle import adi_oracle as orc
    g, base_h = _load(name)
    shape, dx, mask = g['mask'].shape, float(g['dx']), g['mask']
    mat = dict(cases.STEEL)
    rng = np.random.default_rng(11)
    T0 = np.where(mask, rng.uniform(20.0, 1000.0, shape), 20.0)
    dt = 40.0 * dx * dx / (mat['k'] / (mat['rho'] * mat['cp']))

    grid = hip.Grid3D(*shape, dx, mask)
    robin, _ = _corrector(g, mask=grid.d_mask).build_corrected_fields(base_h)
    for f in base_h:
        assert grid.layout.is_native(robin[f]), f                                 # taken as it is: no copy, no host trip
    packs = hip.precompute_coeff_packs_unified(grid, hip.Material(**mat), robin_h=robin)
    T = hip.to_device(T0)
    for _ in range(3):
        T = hip.adi_step_hip_coeff(T, grid, hip.Material(**mat), hip.Params(dt, 0.5), packs, Tinf=20.0)
    got = np.asarray(T)

    ogrid = orc.Grid3D(*shape, dx, mask)
    opacks = orc.precompute_coeff_packs_unified(ogrid, orc.Material(**mat),
                                                robin_h={f: g['robin_on_' + f] for f in base_h})
    for a in range(3):
        assert rel_linf(np.asarray(packs[a].coeff), opacks[a].coeff) <= 1e-10, a
    Tw = T0
    for _ in range(3):
        Tw = orc.adi_step_numba_coeff(Tw, ogrid, orc.Material(**mat), orc.Params(dt, 0.5), opacks, Tinf=20.0)
    e = rel_linf(got, Tw)
    print('STLCORR end to end %s: rel_linf %.3e after three steps' % (name, e))
    assert e <= 1e-10, e
    assert np.abs(Tw - T0).max() > 1.0                                           # the steps did something


def _expected_sums(mesh):
    """per face: fsum(area * max(+-n_c, 0)) over triangles with |n_c| > 1e-12"""
    out = {}
    for ax in range(3):
        c = mesh.face_normals[:, ax]
        out[FACES[2 * ax + 1]] = math.fsum((mesh.area_faces * c)[c > 1e-12].tolist())
        out[FACES[2 * ax]] = math.fsum((mesh.area_faces * -c)[c < -1e-12].tolist())
    return out


def _fsum_field(t):
    """exact sum of a device field's non-zero cells (there are few), and the flat index of the first of them"""
    import torch
    flat = t.reshape(-1) if t.is_contiguous() else t.contiguous().reshape(-1)
    idx = torch.nonzero(flat).reshape(-1)
    return math.fsum(flat[idx].cpu().tolist()), idx


def test_a_million_triangles_in_512_cubed():
    """no reference at this size (tens of minutes of CPython): conservation of the projected area, and two runs alike"""
    import torch
    from adi_thermal_fields_amd.voxel_bc_correction import STLBoundaryCorrector, TriangleMesh
    dx, n = 1e-3, 512
    mesh = TriangleMesh(tube_triangles((0.256, 0.256, 0.256), (0.3, 0.2, 1.0), 0.2, 0.18, 1000, 500, phase=0.01))
    assert len(mesh) == 1000000 and mesh.triangles.min() > dx and mesh.triangles.max() < (n - 1) * dx
    N = int((subdivisions(mesh.triangles, dx, 6) ** 2).sum())
    mask = torch.ones((n, n, n), dtype=torch.uint8, device='cuda')
    corr = STLBoundaryCorrector(mesh, mask, (0.0, 0.0, 0.0), dx)
    want = _expected_sums(mesh)
    area = corr.projected_area_fields()
    worst = 0.0
    for f in FACES:
        got, _ = _fsum_field(area[f])
        rel = abs(got - want[f]) / want[f]
        worst = max(worst, rel)
        assert rel <= N * EPS, (f, got, want[f], rel, N * EPS)
    print('STLCORR scale: %d triangles, %d sub-triangles, largest relative difference of a face sum %.3e (bound %.3e)'
          % (len(mesh), N, worst, N * EPS))
    again = corr.projected_area_fields()
    assert all(torch.equal(area[f], again[f]) for f in FACES)


@pytest.mark.parametrize('shape', [(1100, 512, 512), (2100, 1024, 1024)], ids=['past_2GiB', 'past_2^31_cells'])
def test_keys_past_32_bits(shape):
    """a mesh in the far corner of a grid whose fp64 fields pass 2 GiB, and of one with more than 2^31 cells: keys, cell
    offsets and the fallback's thread numbers are 64-bit"""
    import torch
    from adi_thermal_fields_amd.voxel_bc_correction import STLBoundaryCorrector, TriangleMesh
    dx = 1e-3
    far = np.array(shape, dtype=np.float64) * dx
    mesh = TriangleMesh(tube_triangles(far - 0.02, (0.3, 0.2, 1.0), 0.012, 0.011, 240, 60, phase=0.01))
    assert np.all(mesh.triangles.min(axis=(0, 1)) > far - 0.04) and np.all(mesh.triangles.max(axis=(0, 1)) < far - dx)
    N = int((subdivisions(mesh.triangles, dx, 6) ** 2).sum())
    mask = torch.ones(shape, dtype=torch.uint8, device='cuda')
    base = 250.0
    robin, scale = STLBoundaryCorrector(mesh, mask, (0.0, 0.0, 0.0), dx).build_corrected_fields({'x+': base})
    del mask
    want = _expected_sums(mesh)['x+'] / (dx * dx)
    # with the fallback the last plane (exposed on x+, never reached by the mesh) holds scale 1 and nothing else does
    assert torch.all(scale['x+'][-1] == 1.0) and torch.all(robin['x+'][-1] == base)
    body = scale['x+'][:-1]
    assert body.stride(0) * (shape[0] - 40) * 8 > 1 << 31
    got, idx = _fsum_field(body[shape[0] - 41:])
    assert not body[:shape[0] - 41].any()
    first = int(idx[0]) + (shape[0] - 41) * shape[1] * shape[2]
    assert first * 8 > 1 << 31 and (shape[0] < 2100 or first > 1 << 31), first
    rel = abs(got - want) / want
    print('STLCORR far corner %s: first cell %d, relative difference of the scale sum %.3e (bound %.3e)'
          % (shape, first, rel, N * EPS))
    assert rel <= N * EPS, (got, want, rel)
