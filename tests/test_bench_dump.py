"""CPU: bench.py --dump-outputs writes what it says -- the 64e6-byte cap on disk for every rank count the bench runs with, and
the sampled cells at the indices dump_sample_cells() names (bench.dump_field on host tensors in the device layout's strides)."""
import os

import numpy as np
import pytest
import torch

import bench


def _disk(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


@pytest.mark.parametrize('world', [1, 2, 4, 8])
@pytest.mark.parametrize('shape_of', ['cart_weak', 'cart_strong', 'cyl'])
def test_all_ranks_together_stay_within_the_cap(tmp_path, world, shape_of):
    shape = {'cart_weak': (512, 512, 512), 'cart_strong': (512 // world, 512, 512), 'cyl': (128, 256, 512)}[shape_of]
    t = torch.zeros(1, dtype=torch.float64).expand(*shape)       # the real extents without the memory
    names = []
    for r in range(world):
        names += bench.dump_field(str(tmp_path), 'T' if world == 1 else 'T_rank%d' % r, t, bench.DUMP_BUDGET // world)
    assert sorted(names) == sorted(os.listdir(str(tmp_path)))
    assert _disk(str(tmp_path)) <= bench.DUMP_BUDGET <= 64 * 2 ** 20
    for f in names:
        a = np.load(os.path.join(str(tmp_path), f))
        assert a.dtype == np.float64 and a.size > 0


def _index_field(shape, padded):
    """a field whose every cell holds its own flat C-order index, in a padded (plane-stride, row-pitch) layout"""
    nx, ny, nz = shape
    px, py, pz = padded
    buf = torch.full((px * py * pz,), -1.0, dtype=torch.float64)
    t = buf.as_strided(shape, (py * pz, pz, 1))
    t.copy_(torch.arange(nx * ny * nz, dtype=torch.float64).reshape(shape))
    return t


def test_sampled_cells_are_the_named_ones(tmp_path):
    shape = (70, 40, 30)
    t = _index_field(shape, (72, 44, 32))
    names = bench.dump_field(str(tmp_path), 'T', t, 200000)
    assert names == ['T_mid_plane.npy', 'T_sample.npy']
    s = np.load(str(tmp_path / 'T_sample.npy'))
    assert s.size == (200000 - 40 * 30 * 8 - 2 * bench.NPY_HEADER_MAX) // 8
    assert np.array_equal(s, bench.dump_sample_cells(t.numel(), s.size).astype(np.float64))
    assert np.all(np.diff(s) > 0)                                 # distinct cells, increasing C order
    assert np.array_equal(np.load(str(tmp_path / 'T_mid_plane.npy')),
                          np.arange(t.numel(), dtype=np.float64).reshape(shape)[35])
    assert _disk(str(tmp_path)) <= 200000


def test_a_field_that_fits_goes_out_whole(tmp_path):
    shape = (20, 12, 10)
    t = _index_field(shape, (24, 16, 16))
    assert bench.dump_field(str(tmp_path), 'T', t, bench.DUMP_BUDGET) == ['T.npy']
    assert np.array_equal(np.load(str(tmp_path / 'T.npy')), np.arange(t.numel(), dtype=np.float64).reshape(shape))


def test_the_sample_size_is_capped(tmp_path):
    t = torch.zeros(1, dtype=torch.float64).expand(512, 512, 512)
    bench.dump_field(str(tmp_path), 'T', t, bench.DUMP_BUDGET)
    assert np.load(str(tmp_path / 'T_sample.npy')).size == bench.DUMP_SAMPLE
