"""CPU: the Goldak heat source of the Cartesian step -- the host evaluator's normalisation, parameter validation in Python and
in the C ABI (every rejection happens before any HIP call), and the register footprint of the new kernels."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

import adi_thermal_fields_amd.adi3d_hip_coeff as hip  # noqa: E402
from adi_thermal_fields_amd import _lib  # noqa: E402
from oracle import adi_oracle as orc  # noqa: E402

P, ETA = 1500.0, 0.8
A, B, CF, CR, FF = 1.0e-3, 1.5e-3, 1.0e-3, 2.0e-3, 0.6


def _fine_grid():
    """a box holding the whole support, the centre on cell faces (the front / rear and depth planes fall between cells)"""
    dx = 1.25e-4
    R = np.sqrt(40.0 / 3.0)
    n = [int(np.ceil(2 * R * L / dx)) + 4 for L in (A, CR, B)]   # axis 0 transverse, 1 travel, 2 depth
    n = [v + (v % 2) for v in n]
    g = orc.Grid3D(n[0], n[1], n[2], dx, np.ones(n, dtype=bool))
    origin = (n[0] // 2 * dx, n[1] // 2 * dx, n[2] // 2 * dx)
    return g, origin


def test_goldak_normalisation_and_front_rear_split():
    g, origin = _fine_grid()
    src = hip.GoldakSource(P, ETA, A, B, CF, CR, f_f=FF, origin=origin, travel_axis=1, travel_sign=+1, depth_axis=2)
    q = src.sample(g, 0.0)
    dv = g.dx ** 3
    total = q.sum() * dv
    assert abs(total - 2 * ETA * P) <= 1e-6 * 2 * ETA * P, total
    k0 = g.nz // 2
    below, above = q[:, :, :k0].sum() * dv, q[:, :, k0:].sum() * dv
    assert abs(below - ETA * P) <= 1e-6 * ETA * P and abs(above - ETA * P) <= 1e-6 * ETA * P, (below, above)
    j0 = g.ny // 2
    front, rear = q[:, j0:, :].sum() * dv, q[:, :j0, :].sum() * dv
    assert abs(front - FF * ETA * P) <= 1e-6 * ETA * P, front
    assert abs(rear - (2 - FF) * ETA * P) <= 1e-6 * ETA * P, rear
    # travel_sign = -1: the front lies towards -axis 1
    src.travel_sign = -1
    q2 = src.sample(g, 0.0)
    assert abs(q2[:, :j0, :].sum() * dv - FF * ETA * P) <= 1e-6 * ETA * P


def test_goldak_support_cut_and_centre():
    src = hip.GoldakSource(P, ETA, A, B, CF, CR, origin=(0.0, 1e-3, 0.0), velocity=0.5)
    assert np.allclose(src.center(2e-3), (0.0, 2e-3, 0.0))
    R = np.sqrt(40.0 / 3.0)
    c = src.center(0.0)
    assert src.q(c[0] + 0.999 * R * A, c[1], c[2], 0.0) > 0.0
    assert src.q(c[0] + 1.001 * R * A, c[1], c[2], 0.0) == 0.0
    assert src.q(c[0], c[1] + 1.001 * R * CF, c[2], 0.0) == 0.0
    assert src.q(c[0], c[1] - 0.999 * R * CR, c[2], 0.0) > 0.0
    assert src.q(c[0], c[1], c[2] + 1.001 * R * B, 0.0) == 0.0
    # off-mask cells receive nothing
    m = np.ones((4, 6, 5), dtype=bool)
    m[1, 2, 3] = False
    g = orc.Grid3D(4, 6, 5, 2e-4, m)
    s = hip.GoldakSource(P, ETA, A, B, CF, CR, origin=(4e-4, 6e-4, 7e-4)).sample(g, 0.0)
    assert s[1, 2, 3] == 0.0 and (s[m] > 0).all()


GOOD = dict(power=P, eta=ETA, a=A, b=B, c_f=CF, c_r=CR, f_f=FF, origin=(0.0, 0.0, 0.0), velocity=0.0, travel_axis=1,
            travel_sign=1, depth_axis=2)
BAD = [dict(power=-1.0), dict(power=np.inf), dict(eta=-0.1), dict(eta=1.5), dict(eta=np.nan), dict(a=0.0), dict(b=-1e-3),
       dict(c_f=0.0), dict(c_r=-2e-3), dict(a=np.inf), dict(f_f=0.0), dict(f_f=2.0), dict(f_f=-0.5), dict(velocity=-1.0),
       dict(velocity=np.nan), dict(origin=(0.0, np.nan, 0.0)), dict(origin=(0.0, 0.0)), dict(travel_axis=3),
       dict(travel_axis=-1), dict(depth_axis=5), dict(travel_axis=2, depth_axis=2), dict(travel_sign=0),
       dict(travel_sign=2), dict(travel_axis=1.5)]


def test_goldak_source_accepts_good_parameters():
    hip.GoldakSource(**GOOD)


@pytest.mark.parametrize('bad', BAD, ids=[','.join('%s=%s' % kv for kv in b.items()) for b in BAD])
def test_goldak_source_rejects(bad):
    with pytest.raises(ValueError):
        hip.GoldakSource(**dict(GOOD, **bad))


def _c_source(**kw):
    d = dict(GOOD, **kw)
    return _lib.HeatSource(d['power'], d['eta'], d['a'], d['b'], d['c_f'], d['c_r'], d['f_f'],
                           (ctypes.c_double * 3)(*d['origin']), d['velocity'], d['travel_axis'], d['travel_sign'],
                           d['depth_axis'], 0)


C_BAD = [dict(power=-1.0), dict(eta=2.0), dict(a=0.0), dict(c_r=-1.0), dict(f_f=2.0), dict(f_f=0.0), dict(b=np.nan),
         dict(velocity=np.inf), dict(travel_axis=3), dict(depth_axis=-1), dict(travel_axis=2, depth_axis=2),
         dict(travel_sign=0)]
FAKE = ctypes.c_void_p(4096)      # never dereferenced: every call below fails its checks before it launches anything


@pytest.mark.parametrize('bad', C_BAD, ids=[','.join('%s=%s' % kv for kv in b.items()) for b in C_BAD])
def test_abi_rejects_bad_sources(bad):
    s = ctypes.byref(_c_source(**bad))
    lib = _lib.lib
    assert lib.adi_source_sample(s, FAKE, 8, 8, 8, 0, 1e-4, 0.0, FAKE, None) == _lib.ADI_ERR_ARG
    assert lib.adi_source_set(FAKE, s, 0.0, 1e-3, 0, None) == _lib.ADI_ERR_ARG
    assert lib.adi_source_lines0(FAKE, s, FAKE, FAKE, FAKE, None, 8, 8, 8, 0, 0, 1e-4, 0.5, 1.0, 1e-3, 7800.0, 500.0,
                                 None, None, 0, None) == _lib.ADI_ERR_ARG
    b = ctypes.c_size_t(0)
    assert lib.adi_source_workspace_bytes(s, 2000, 8, 8, 1e-4, ctypes.byref(b)) == _lib.ADI_ERR_ARG
    assert _lib.last_error()


def test_abi_rejects_bad_arguments():
    lib = _lib.lib
    s = ctypes.byref(_c_source())
    E = _lib.ADI_ERR_ARG
    assert lib.adi_source_sample(None, FAKE, 8, 8, 8, 0, 1e-4, 0.0, FAKE, None) == E
    assert lib.adi_source_sample(s, None, 8, 8, 8, 0, 1e-4, 0.0, FAKE, None) == E
    assert lib.adi_source_sample(s, FAKE, 8, 8, 8, 0, 1e-4, 0.0, None, None) == E
    assert lib.adi_source_sample(s, FAKE, 0, 8, 8, 0, 1e-4, 0.0, FAKE, None) == E
    assert lib.adi_source_sample(s, FAKE, 8, 8, 8, 0, -1e-4, 0.0, FAKE, None) == E
    assert lib.adi_source_sample(s, FAKE, 8, 8, 8, 0, 1e-4, float('nan'), FAKE, None) == E
    assert lib.adi_source_sample(s, FAKE, 8, 8, 8, 10, 1e-4, 0.0, FAKE, None) == E      # plane stride < ny*nz
    assert lib.adi_source_set(None, s, 0.0, 1e-3, 0, None) == E
    assert lib.adi_source_set(FAKE, None, 0.0, 1e-3, 0, None) == E
    assert lib.adi_source_set(FAKE, s, 0.0, 0.0, 0, None) == E
    assert lib.adi_source_set(FAKE, s, float('inf'), 1e-3, 0, None) == E
    assert lib.adi_source_set(FAKE, s, 0.0, 1e-3, -1, None) == E
    assert lib.adi_source_tick(None, None) == E
    args = [FAKE, s, FAKE, FAKE, FAKE, None, 8, 8, 8, 0, 0, 1e-4, 0.5, 1.0, 1e-3, 7800.0, 500.0, None, None, 0, None]

    def lines(**over):
        a = list(args)
        for i, v in over.items():
            a[int(i[1:])] = v
        return lib.adi_source_lines0(*a)
    assert lines(a0=None) == E                      # block
    assert lines(a2=None) == E                      # U
    assert lines(a3=None) == E                      # flags
    assert lines(a4=None) == E                      # no coeff array and no face constants
    assert lines(a6=2000) == E                      # longer than the in-register limit, no workspace
    assert lines(a6=2000, a18=FAKE, a19=1024) == E  # ... too small a workspace
    b = ctypes.c_size_t(1)
    assert lib.adi_source_workspace_bytes(s, 1024, 8, 8, 1e-4, ctypes.byref(b)) == _lib.ADI_OK and b.value == 0
    assert lib.adi_source_workspace_bytes(s, 1040, 8, 16, 1e-4, ctypes.byref(b)) == _lib.ADI_OK
    assert b.value == 2 * 8 * 1040 * (8 + 4) * (16 + 4)          # (a support wider than the grid: the box is clamped)
    assert lib.adi_source_workspace_bytes(s, 0, 8, 8, 1e-4, ctypes.byref(b)) == E
    assert lib.adi_source_workspace_bytes(s, 1040, 8, 8, 0.0, ctypes.byref(b)) == E
    assert lib.adi_source_workspace_bytes(s, 1040, 8, 8, 1e-4, None) == E
    assert lines(a6=-1) == E
    assert lines(a11=0.0) == E                      # dx
    assert lines(a14=-1e-3) == E                    # dt
    assert lines(a15=float('nan')) == E             # rho
    assert lib.adi_explicit_rhs_src(None, FAKE, FAKE, 8, 8, 8, 0, 1e-4, 1e-3, 1e-6, 0.5, 7800.0, 500.0, FAKE, None) == E
    assert lib.adi_explicit_rhs_src(FAKE, None, FAKE, 8, 8, 8, 0, 1e-4, 1e-3, 1e-6, 0.5, 7800.0, 500.0, FAKE, None) == E
    assert lib.adi_explicit_rhs_src(FAKE, FAKE, FAKE, 8, 8, 8, 0, 1e-4, 1e-3, 1e-6, 0.5, 7800.0, 500.0, FAKE, None) == E
    assert lib.adi_explicit_rhs_src(ctypes.c_void_p(8192), FAKE, FAKE, 8, 8, 8, 0, 1e-4, 1e-3, 1e-6, 0.5, 0.0, 500.0,
                                    ctypes.c_void_p(12288), None) == E


def test_block_layout_matches_the_header():
    assert ctypes.sizeof(_lib.HeatSource) + 3 * 8 == _lib.SOURCE_BLOCK_BYTES


def test_new_kernels_have_no_scratch_and_no_spills():
    import kernel_meta
    if not os.path.isdir(kernel_meta.LLVM):
        pytest.skip('no ROCm LLVM tools at %s' % kernel_meta.LLVM)
    obj = os.path.join(kernel_meta.CSRC, 'adi_source.o')
    assert os.path.exists(obj), 'run `python -m adi_thermal_fields_amd.build` first'
    ks = kernel_meta.object_kernels(obj)
    names = {k['short'] for k in ks}
    for want in ('adi::k_source_sample', 'adi::k_explicit_src', 'adi::k_source_lines0<4, 32>', 'adi::k_source_lines0<8, 32>',
                 'adi::k_source_lines0<16, 32>', 'adi::k_source_lines0<16, 64>', 'adi::k_source_lines0_long'):
        assert want in names, sorted(names)
    bad = [(k['short'], k['scratch'], k.get('vgpr_spill_count', 0), k.get('sgpr_spill_count', 0)) for k in ks
           if k['scratch'] or k.get('vgpr_spill_count', 0) or k.get('sgpr_spill_count', 0)]
    assert not bad, bad
