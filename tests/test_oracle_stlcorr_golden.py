"""CPU: oracle/stlcorr_oracle.py (the NumPy restatement of the STL correction) against the imported reference's fields,
tests/golden/stlcorr_*.npz -- bit for bit, on the fixtures that keep every centroid away from a voxel boundary and on
the ones that put centroids on boundaries (tests/golden/make_golden_stlcorr.py asserts and stores the share), where
the voxel of a sub-triangle is decided by the last bit of a rounding.  Also here: the conditions on the seeded fuzz of
tests/test_stlcorr_gpu.py, which the oracle alone can check."""
import os

import numpy as np
import pytest

import stlcorr_meshes as sm
from helpers import GOLDEN
from oracle import stlcorr_oracle as orc

FACES = orc.FACES


class Mesh:
    def __init__(self, g):
        self.triangles, self.face_normals, self.area_faces = g['triangles'], g['normals'], g['areas']


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize('name', sm.MARGIN_CASES + sm.BOUNDARY_CASES)
def test_oracle_equals_the_reference(name):
    g = np.load(os.path.join(GOLDEN, 'stlcorr_%s.npz' % name))
    base_h = {str(f): float(v) for f, v in zip(g['base_faces'], g['base_vals'])}
    corr = orc.STLBoundaryCorrector(Mesh(g), g['mask'], g['origin'], float(g['dx']), max_subdiv=int(g['max_subdiv']),
                                    area_epsilon=float(g['area_epsilon']))
    assert int(corr.slots().offset[-1]) == int(g['n_sub'])
    area = corr.projected_area_fields()
    assert list(area) == list(FACES)
    for f in FACES:
        assert _same(area[f], g['area_' + f]), 'area ' + f
    count = corr.contribution_counts()
    assert np.array_equal(count, g['count']) and int(count.max()) == int(g['n_max'])
    for tag, fb in (('on', True), ('off', False)):
        robin, scale = corr.build_corrected_fields(base_h, fallback_to_base=fb)
        assert list(robin) == list(base_h) and list(scale) == list(base_h)
        for f in base_h:
            assert _same(robin[f], g['robin_%s_%s' % (tag, f)]), 'robin %s %s' % (tag, f)
            assert _same(scale[f], g['scale_%s_%s' % (tag, f)]), 'scale %s %s' % (tag, f)
    if name in sm.BOUNDARY_CASES:
        # the generator's number is a share of centroid components within 4 ulp of a boundary; the oracle's is the share
        # of sub-triangles with a component exactly on one
        print('%s: stored share of components at a boundary %.3f, oracle: %.3f of the sub-triangles exactly on one'
              % (name, float(g['boundary_share']), corr.on_boundary_share()))
        assert float(g['boundary_share']) >= float(g['boundary_share_min'])


def test_slot_table_is_the_loop_order():
    """the row-wise table against the two plain loops, for every n up to 9 and one larger"""
    for n in list(range(2, 10)) + [33]:
        want = []
        for i in range(n):
            for j in range(n - i):
                want.append((i, j, False))
                if i + j < n - 1:
                    want.append((i, j, True))
        i, j, up = orc.slot_table(n)
        assert list(zip(i.tolist(), j.tolist(), up.tolist())) == want, n


def test_exposed_mask_by_hand():
    m = np.zeros((3, 2, 2), bool)
    m[0, 0, 0] = m[1, 0, 0] = True
    assert orc.exposed_mask(m, 'x-').nonzero()[0].tolist() == [0]
    assert orc.exposed_mask(m, 'x+').nonzero()[0].tolist() == [1]
    assert orc.exposed_mask(m, 'y+').sum() == 2 and orc.exposed_mask(m, 'z-').sum() == 2
    with pytest.raises(ValueError):
        orc.exposed_mask(m, 'w+')


def test_the_fuzz_stays_on_the_hard_cases():
    """over the 40 seeds of test_stlcorr_gpu.py: at least a quarter of the cases have a centroid component exactly on a
    voxel boundary for at least 1 % of their sub-triangles, and at least 8 use max_subdiv >= 16 with a triangle cut
    that deep; no case is larger than the fuzz can afford"""
    on_boundary, deep, sizes = 0, 0, []
    for seed in range(sm.FUZZ_SEEDS):
        c = sm.fuzz_case(seed)
        corr = orc.STLBoundaryCorrector(c.mesh, c.mask, c.origin, c.dx, max_subdiv=c.max_subdiv,
                                        area_epsilon=c.area_epsilon)
        share, cut = corr.on_boundary_share(), corr.deepest_cut()
        sizes.append(int(corr.slots().offset[-1]))
        on_boundary += share >= 0.01
        deep += c.max_subdiv >= 16 and cut >= 16
        print('seed %2d: %-6s %-12s shape %-15s dx %.4g max_subdiv %2d: %6d sub-triangles, deepest cut %2d, %.3f on a '
              'boundary' % (seed, c.mesh_kind, c.mask_kind, c.mask.shape, c.dx, c.max_subdiv, sizes[-1], cut, share))
    assert on_boundary >= 0.25 * sm.FUZZ_SEEDS, on_boundary
    assert deep >= 8, deep
    assert max(sizes) <= 150000, max(sizes)
