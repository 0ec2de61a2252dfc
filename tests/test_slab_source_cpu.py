"""CPU: the moving heat source on the slab decomposition -- argument checks of adi_source_lines0_slab and adi_source_add_r0
(every rejection happens before any HIP call), the footprint of the new kernel, and SlabStepper's source= / set_source /
step(t=) contract on the reference engine (which has no source kernels)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

import adi_thermal_fields_amd.adi3d_hip_coeff as hip  # noqa: E402
from adi_thermal_fields_amd import _lib, dist_slab  # noqa: E402
from oracle import adi_oracle as orc  # noqa: E402

FAKE = ctypes.c_void_p(4096)      # never dereferenced: every call below fails its checks before it launches anything
E = _lib.ADI_ERR_ARG


def _c_source(**kw):
    d = dict(power=800.0, eta=0.8, a=3e-4, b=2.5e-4, c_f=3e-4, c_r=6e-4, f_f=0.6, origin=(1e-3, 1e-3, 1e-3), velocity=0.1,
             travel_axis=0, travel_sign=1, depth_axis=2)
    d.update(kw)
    return _lib.HeatSource(d['power'], d['eta'], d['a'], d['b'], d['c_f'], d['c_r'], d['f_f'],
                           (ctypes.c_double * 3)(*d['origin']), d['velocity'], d['travel_axis'], d['travel_sign'],
                           d['depth_axis'], 0)


def _lines(s, **over):
    a = [FAKE, s, FAKE, FAKE, FAKE, None, 64, 8, 8, 0, 128, 1, 1e-4, 0.5, 1.0, 1e-3, 7800.0, 500.0, None, None, 0, None]
    for i, v in over.items():
        a[int(i[1:])] = v
    return _lib.lib.adi_source_lines0_slab(*a)


def _add(s, **over):
    a = [FAKE, s, FAKE, FAKE, None, 64, 8, 8, 0, 128, 0, 64, 1e-4, 1e-3, 7800.0, 500.0, None]
    for i, v in over.items():
        a[int(i[1:])] = v
    return _lib.lib.adi_source_add_r0(*a)


@pytest.mark.parametrize('bad', [dict(power=-1.0), dict(eta=2.0), dict(a=0.0), dict(f_f=2.0), dict(travel_axis=3),
                                 dict(travel_axis=2, depth_axis=2), dict(travel_sign=0), dict(velocity=np.nan)],
                         ids=lambda b: ','.join('%s=%s' % kv for kv in b.items()))
def test_slab_entry_points_reject_bad_sources(bad):
    s = ctypes.byref(_c_source(**bad))
    assert _lines(s) == E
    assert _add(s) == E
    assert _lib.last_error()


def test_slab_entry_points_reject_bad_arguments():
    s = ctypes.byref(_c_source())
    assert _lines(None) == E                                  # (a null source)
    assert _lines(s, a0=None) == E                            # null block
    assert _lines(s, a2=None) == E                            # U
    assert _lines(s, a3=None) == E                            # flags
    assert _lines(s, a4=None) == E                            # no coeff array and no face constants
    assert _lines(s, a10=-1) == E                             # plane origin
    assert _lines(s, a6=2000) == E                            # longer than the in-register limit, no workspace
    assert _lines(s, a12=0.0) == E                            # dx
    assert _lines(s, a15=-1e-3) == E                          # dt
    assert _lines(s, a16=float('nan')) == E                   # rho
    assert 'adi_source_lines0_slab' in _lib.last_error()
    assert _add(None) == E
    assert _add(s, a0=None) == E                              # null block
    assert _add(s, a2=None) == E                              # R0
    assert _add(s, a3=None) == E                              # flags
    assert _add(s, a10=40, a11=20) == E                       # i_begin > i_end
    assert _add(s, a10=-1) == E
    assert _add(s, a11=65) == E                               # i_end > nx
    assert _add(s, a9=-1) == E                                # plane origin
    assert _add(s, a12=0.0) == E                              # dx
    assert _add(s, a13=0.0) == E                              # dt
    assert _add(s, a15=float('inf')) == E and 'adi_source_add_r0' in _lib.last_error()   # cp
    assert _add(s, a5=0) == E                                 # empty box
    assert _add(s, a8=10) == E                                # plane stride < ny*nz
    with pytest.raises(ValueError):
        _lib.check(_add(s, a10=40, a11=20))


def test_slab_kernels_have_no_scratch_and_no_spills():
    import kernel_meta
    if not os.path.isdir(kernel_meta.LLVM):
        pytest.skip('no ROCm LLVM tools at %s' % kernel_meta.LLVM)
    obj = os.path.join(kernel_meta.CSRC, 'adi_source.o')
    assert os.path.exists(obj), 'run `python -m adi_thermal_fields_amd.build` first'
    ks = {k['short']: k for k in kernel_meta.object_kernels(obj)}
    for name in ('adi::k_source_add_r0', 'adi::k_source_lines0_long_slab', 'adi::k_source_lines0_slab<4, 32>',
                 'adi::k_source_lines0_slab<8, 32>', 'adi::k_source_lines0_slab<16, 32>', 'adi::k_source_lines0_slab<16, 64>'):
        k = ks[name]
        assert not k['scratch'] and not k.get('vgpr_spill_count', 0) and not k.get('sgpr_spill_count', 0), k


def _stepper(source, engine_cls=None):
    from cpu_engine import CpuEngine
    comm = dist_slab.LocalComm.make(1)[0]
    shape = (8, 6, 5)
    return dist_slab.SlabStepper(np.ones(shape, bool), 1e-4, orc.Material(7800.0, 500.0, 30.0), orc.Params(1e-3, 0.5), 300.0,
                                 robin_h=20.0, comm=comm, engine=(engine_cls or CpuEngine)(), source=source)


def _src():
    return hip.GoldakSource(800.0, 0.8, 3e-4, 2.5e-4, 3e-4, 6e-4, origin=(4e-4, 3e-4, 5e-4), velocity=0.1, travel_axis=0)


def test_stepper_source_contract_on_the_reference_engine():
    with pytest.raises(NotImplementedError):
        _stepper(_src())
    with pytest.raises(TypeError):
        _stepper(object())
    with pytest.raises(TypeError):
        _stepper(np.zeros((8, 6, 5)))                         # a field is not a moving source
    st = _stepper(None)
    assert st.source is None
    with pytest.raises(NotImplementedError):
        st.set_source(_src())
    st.set_source(None)                                       # detaching is always allowed


def test_step_needs_the_start_time_with_a_source():
    from cpu_engine import CpuEngine

    class SourceEngine(CpuEngine):                            # the methods exist; step() must refuse before it calls any
        def source_set(self, *a):
            raise AssertionError('called')
        source_lines0 = source_add_r0 = source_set

    st = _stepper(_src(), SourceEngine)
    T0 = np.full((8, 6, 5), 300.0)
    with pytest.raises(ValueError, match='start time'):
        st.step(T0)
    st.set_source(None)
    st.step(T0)                                               # without a source t is not needed


def test_support_test_on_the_host():
    """_source_meets: the kernels' extent along axis 0, widened by one plane; an 8-plane slab starting at global plane 16"""
    from cpu_engine import CpuEngine

    class SourceEngine(CpuEngine):
        def source_set(self, *a):
            pass
        source_lines0 = source_add_r0 = source_set
    st = _stepper(None, SourceEngine)
    dx, R = 1e-4, np.sqrt(40.0 / 3.0)
    s = hip.GoldakSource(800.0, 0.8, 3e-4, 2.5e-4, 3e-4, 6e-4, origin=(0.0, 3e-4, 5e-4), velocity=0.0, travel_axis=1)
    half = R * 3e-4                                           # transverse half-extent along axis 0
    for c0, want in [(20 * dx, True), (16 * dx - half - 0.49 * dx, True), (16 * dx - half - 3.0 * dx, False),
                     (24 * dx + half + 0.49 * dx, True), (24 * dx + half + 3.0 * dx, False)]:
        s.origin = (c0, 3e-4, 5e-4)
        assert st._source_meets(s, 0.0, 1e-3, 16) is want, (c0 / dx, want)
