"""CPU: the pieces of the STL correction of voxel Robin coefficients that need no GPU -- the NumPy mesh
(`TriangleMesh`, `load_stl`), argument validation of the adi_stlcorr_* entry points (before any HIP call) and the
scratch-free footprint of their kernels.  The fixtures tests/golden/stlcorr_*.npz come from the reference
(tests/golden/make_golden_stlcorr.py)."""
import ctypes
import glob
import os
import struct
import sys

import numpy as np
import pytest

from helpers import GOLDEN
from stlcorr_meshes import BOUNDARY_CASES, HAND_SET_CASES, MARGIN_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = MARGIN_CASES + BOUNDARY_CASES


def test_every_fixture_is_there():
    have = sorted(os.path.basename(p)[8:-4] for p in glob.glob(os.path.join(GOLDEN, 'stlcorr_*.npz')))
    assert have == sorted(CASES)
    for name in CASES:
        assert os.path.getsize(os.path.join(GOLDEN, 'stlcorr_%s.npz' % name)) < 800000


def _ulps(got, want):
    """|got - want| in units of the spacing of the stored value (of the smallest normal number at zero)"""
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got) - want) / np.spacing(np.maximum(np.abs(want), np.finfo(np.float64).tiny))


@pytest.mark.parametrize('name', [c for c in CASES if c not in HAND_SET_CASES])
def test_triangle_mesh_reproduces_the_stored_normals_and_areas(name):
    from adi_thermal_fields_amd.voxel_bc_correction import TriangleMesh
    g = np.load(os.path.join(GOLDEN, 'stlcorr_%s.npz' % name))
    m = TriangleMesh(g['triangles'])
    n = len(g['triangles'])
    assert m.triangles.shape == (n, 3, 3) and m.triangles_center.shape == (n, 3)
    assert m.face_normals.shape == (n, 3) and m.area_faces.shape == (n,)
    if n == 0:
        return
    ua, un = _ulps(m.area_faces, g['areas']).max(), _ulps(m.face_normals, g['normals']).max()
    print('%s: areas within %.1f ulp, normals within %.1f ulp' % (name, ua, un))
    assert ua <= 4.0, ua
    assert un <= 4.0, un
    assert np.array_equal(m.triangles_center, g['triangles'].mean(axis=1))


def _write_binary(path, tri):
    with open(path, 'wb') as f:
        f.write(b'solid looks like ASCII but is not'.ljust(80, b' '))
        f.write(struct.pack('<I', len(tri)))
        for t in tri:
            f.write(struct.pack('<12fH', 0.0, 0.0, 0.0, *[float(v) for v in t.reshape(-1)], 0))


def _write_ascii(path, tri):
    with open(path, 'w') as f:
        f.write('solid part\n')
        for t in tri:
            f.write(' facet normal 0 0 0\n  outer loop\n')
            for v in t:
                f.write('   vertex %.17e %.17e %.17e\n' % tuple(float(c) for c in v))
            f.write('  endloop\n endfacet\n')
        f.write('endsolid part\n')


def test_load_stl_round_trips_binary_and_ascii(tmp_path):
    from adi_thermal_fields_amd.voxel_bc_correction import TriangleMesh, load_stl
    g = np.load(os.path.join(GOLDEN, 'stlcorr_cyl64.npz'))
    tri = (g['triangles'] * 1e3).astype(np.float32)                  # a file in millimetres, as STL writers store it
    _write_binary(str(tmp_path / 'b.stl'), tri)
    _write_ascii(str(tmp_path / 'a.stl'), tri)
    want = TriangleMesh(tri.astype(np.float64) * 1e-3)
    for fn in ('b.stl', 'a.stl'):
        m = load_stl(str(tmp_path / fn), scale=1e-3)
        assert np.array_equal(m.triangles, want.triangles), fn       # 17 digits print a double exactly
        assert np.array_equal(m.face_normals, want.face_normals) and np.array_equal(m.area_faces, want.area_faces)
    assert np.array_equal(load_stl(str(tmp_path / 'b.stl')).triangles, tri.astype(np.float64))
    (tmp_path / 'bad.stl').write_bytes(b'not an stl file at all' * 10)
    with pytest.raises(ValueError):
        load_stl(str(tmp_path / 'bad.stl'))
    # the winding decides the normal: a right-handed triangle in the plane z = 0 faces +z, area 1/2
    m = TriangleMesh([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
    assert m.face_normals.tolist() == [[0.0, 0.0, 1.0]] and m.area_faces.tolist() == [0.5]
    assert TriangleMesh([[[1, 1, 1]] * 3]).face_normals.tolist() == [[0.0, 0.0, 0.0]]


def test_argument_errors_without_gpu():
    """validation happens before any HIP call"""
    from adi_thermal_fields_amd import _lib
    lib, P, N = _lib.lib, ctypes.c_void_p(8), None
    org = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    D6 = (ctypes.c_double * 6)()
    tab = _lib.ptr_array([None] * 6)
    count = lambda **k: lib.adi_stlcorr_count(*[k.get(a, d) for a, d in (
        ('tri', P), ('area', P), ('ntri', 4), ('dx', 1e-3), ('ms', 6), ('eps', 1e-16), ('out', P), ('stream', N))])
    bin_ = lambda **k: lib.adi_stlcorr_bin(*[k.get(a, d) for a, d in (
        ('tri', P), ('area', P), ('off', P), ('ntri', 4), ('nslot', 16), ('mask', P), ('nx', 4), ('ny', 4), ('nz', 4),
        ('sx', 16), ('sy', 4), ('org', org), ('dx', 1e-3), ('ms', 6), ('key', P), ('sa', P), ('st', P), ('stream', N))])
    acc = lambda **k: lib.adi_stlcorr_accumulate(*[k.get(a, d) for a, d in (
        ('key', P), ('order', P), ('sa', P), ('st', P), ('nrm', P), ('nslot', 16), ('dx', 1e-3), ('base', D6),
        ('area', tab), ('robin', tab), ('scale', tab), ('stream', N))])
    fb = lambda **k: lib.adi_stlcorr_fallback(*[k.get(a, d) for a, d in (
        ('mask', P), ('nx', 4), ('ny', 4), ('nz', 4), ('sx', 16), ('sy', 4), ('face', 0), ('base', 1.0), ('robin', P),
        ('scale', P), ('stream', N))])
    bad = [count(dx=0.0), count(dx=-1.0), count(dx=float('nan')), count(ms=0), count(ms=_lib.STLCORR_MAX_SUBDIV + 1),
           count(ntri=-1), count(tri=N), count(area=N), count(out=N), count(eps=float('nan')),
           bin_(dx=0.0), bin_(ms=0), bin_(ntri=-1), bin_(nslot=-1), bin_(ntri=0), bin_(nx=0), bin_(nz=-3), bin_(sy=3),
           bin_(sx=15), bin_(org=N), bin_(tri=N), bin_(area=N), bin_(off=N), bin_(mask=N), bin_(key=N), bin_(sa=N),
           bin_(st=N),
           acc(dx=0.0), acc(nslot=-1), acc(base=N), acc(area=N), acc(robin=N), acc(scale=N), acc(key=N), acc(order=N),
           acc(sa=N), acc(st=N), acc(nrm=N), acc(robin=_lib.ptr_array([8] + [None] * 5)),
           fb(face=6), fb(face=-1), fb(nx=0), fb(sy=3), fb(sx=15), fb(mask=N), fb(robin=N), fb(scale=N)]
    assert bad == [_lib.ADI_ERR_ARG] * len(bad), bad
    with pytest.raises(ValueError, match='dx must be positive'):
        _lib.check(count(dx=0.0))
    with pytest.raises(ValueError, match='max_subdiv'):
        _lib.check(bin_(ms=0))
    with pytest.raises(ValueError, match='bad face'):
        _lib.check(fb(face=9))
    # nothing to do is not an error, and still no HIP call
    assert count(ntri=0, tri=N, area=N, out=N) == 0 and bin_(ntri=0, nslot=0) == 0 and acc(nslot=0) == 0


def test_corrector_refuses_bad_arguments_and_a_missing_gpu():
    import torch
    from adi_thermal_fields_amd.voxel_bc_correction import STLBoundaryCorrector, TriangleMesh
    mesh, mask = TriangleMesh(np.zeros((0, 3, 3))), np.ones((3, 3, 3), bool)
    with pytest.raises(ValueError):
        STLBoundaryCorrector(mesh, mask, (0, 0, 0), 0.0)
    c = STLBoundaryCorrector(mesh, mask, (0, 0, 0), 1e-3, max_subdiv=0)
    assert c.max_subdiv == 1 and c.shape == (3, 3, 3) and c.area_epsilon == 1e-16      # the reference clamps, :50
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            c.build_corrected_fields({'x-': 1.0})


def test_no_scratch_in_the_stlcorr_kernels():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_meta
    obj = os.path.join(kernel_meta.CSRC, 'adi_stlcorr.o')
    if not os.path.isdir(kernel_meta.LLVM):
        pytest.skip('no ROCm LLVM tools at %s' % kernel_meta.LLVM)
    assert os.path.exists(obj), 'no adi_stlcorr.o under csrc/: run `python -m adi_thermal_fields_amd.build` first'
    ks = {k['short']: k for k in kernel_meta.object_kernels(obj)}
    assert sorted(ks) == ['adi::k_stl_accumulate', 'adi::k_stl_bin', 'adi::k_stl_count', 'adi::k_stl_fallback'], sorted(ks)
    for name, k in ks.items():
        assert k['scratch'] == 0 and k.get('vgpr_spill_count', 0) == 0, (name, k)
        assert k['max_flat_workgroup_size'] == 256, (name, k)


def test_only_divisions_and_the_square_root_fuse_in_the_stlcorr_kernels():
    """A tripwire for the rounding claim of csrc/adi_stlcorr.hip (`#pragma clang fp contract(off)`: every product and sum
    of the binning rounds on its own, as NumPy's do).  The only fused multiply-adds left in the ISA are those of the fp64
    division and square-root expansions: 5 per division (one v_div_fmas_f64 each) and 11 per square root (one v_rsq_f64
    each).  Measured with hipcc of HIP 7.2.26015 (AMD clang 22.0.0git, roc-7.2.0), before this test existed and with it:
    k_stl_count 15 = 5 * 3, k_stl_bin 96 = 5 * 17 + 11 * 1, k_stl_accumulate 30 = 5 * 6, k_stl_fallback 0.
    Not a proof -- the fixtures with centroids on voxel boundaries are (test_stlcorr_gpu.py)."""
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import kernel_meta
    obj = os.path.join(kernel_meta.CSRC, 'adi_stlcorr.o')
    if not os.path.exists(os.path.join(kernel_meta.LLVM, 'llvm-objdump')):
        pytest.skip('no llvm-objdump at %s' % kernel_meta.LLVM)
    assert os.path.exists(obj), 'no adi_stlcorr.o under csrc/: run `python -m adi_thermal_fields_amd.build` first'
    seen = {}
    for name, ops in kernel_meta.object_mnemonics(obj).items():
        if 'k_stl_' not in name:
            continue
        count = lambda *stems: sum(1 for op in ops if op.split('_e32')[0].split('_e64')[0] in stems)
        fused = count('v_fma_f64', 'v_fmac_f64', 'v_pk_fma_f64')
        div, sqrt = count('v_div_fmas_f64'), count('v_rsq_f64')
        short = name[name.index('k_stl_'):].split('E')[0]
        seen[short] = (fused, div, sqrt)
        assert fused == 5 * div + 11 * sqrt, (
            '%s: %d fused fp64 multiply-adds for %d divisions and %d square roots (expected 5 and 11 each).  Either the '
            'compiler expands division / square root differently now -- disassemble the object (llvm-objdump -d on its '
            'gfx950 code object), check that every v_fma_f64 / v_fmac_f64 sits between a v_div_scale_f64 or v_rsq_f64 and '
            'its v_div_fixup_f64 / final v_cndmask, and record the new figures here with the compiler version -- or a '
            'product and a sum of the binning were contracted: then the centroids no longer round as NumPy rounds them'
            % (short, fused, div, sqrt))
    print(seen)
    assert sorted(seen) == ['k_stl_accumulate', 'k_stl_bin', 'k_stl_count', 'k_stl_fallback'], sorted(seen)
    assert seen['k_stl_bin'][1:] == (17, 1) and seen['k_stl_count'][1:] == (3, 0), seen
