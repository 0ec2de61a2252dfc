"""CPU: the moving heat source of the cylindrical step (include/adi_hip.h, "Moving heat source of the cylindrical step") --
the host evaluator's normalisation, split, cut and motion, the argument checks of CylGoldakSource and of the C ABI (all made
before any HIP call), the block layout, the kernels' register footprint and the spiral driver on the oracle."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from adi_thermal_fields_amd import _lib  # noqa: E402
import adi_thermal_fields_amd.adi3d_hip_cyl as hipcyl  # noqa: E402

P, ETA = 1500.0, 0.8
A, B, CF, CR = 2e-3, 1.5e-3, 2e-3, 4e-3
RC, Z0 = 0.06, 0.02


def _src(**kw):
    args = dict(f_f=0.6, r_c=RC, phi0=0.0, omega=0.0, z0=Z0, v_z=0.0, depth='z')
    args.update(kw)
    return hipcyl.CylGoldakSource(P, ETA, A, B, CF, CR, **args)


def _mesh(n_r=160, n_phi=240, n_z=160):
    """cell centres and volumes r dr dphi dz of a box in (r, phi, z) around the support (centre at phi = 0, z = Z0): the
    support reaches sqrt(40/3) * 4 mm = 14.6 mm; the angle and the height are split at the centre by cell faces"""
    h = 0.016
    r = RC - h + (np.arange(n_r) + 0.5) * (2 * h / n_r)
    dphi = 2 * 0.28 / n_phi
    phi = -0.28 + (np.arange(n_phi) + 0.5) * dphi
    z = Z0 - h + (np.arange(n_z) + 0.5) * (2 * h / n_z)
    R, PH, Z = np.meshgrid(r, phi, z, indexing='ij')
    V = R * (2 * h / n_r) * dphi * (2 * h / n_z)
    return R, PH, Z, V


def test_integrates_to_two_eta_p_and_eta_p_on_the_half_space():
    R, PH, Z, V = _mesh()
    for depth in ('z', 'r'):
        q = _src(depth=depth).q(R, PH, Z, 0.0)
        tot = float((q * V).sum())
        assert abs(tot - 2 * ETA * P) <= 2e-3 * 2 * ETA * P, (depth, tot)
    # half-space on one side of the centre plane normal to the depth axis, on a Cartesian mesh in the centre's frame (x along
    # the tangent, y along the radius, z along the axis) whose cell faces lie on that plane
    n, h = 120, 0.016
    c = -h + (np.arange(n) + 0.5) * (2 * h / n)
    X, Y, Zc = np.meshgrid(c, c, c, indexing='ij')
    dv = (2 * h / n) ** 3
    r, phi = np.hypot(RC + Y, X), np.arctan2(X, RC + Y)
    for depth, up in (('z', Zc > 0), ('r', Y > 0)):
        q = _src(depth=depth).q(r, phi, Z0 + Zc, 0.0)
        assert abs(float(q.sum()) * dv - 2 * ETA * P) <= 2e-3 * 2 * ETA * P, depth
        hs = float(q[up].sum()) * dv
        assert abs(hs - ETA * P) <= 2e-3 * ETA * P, (depth, hs)


def test_front_rear_split_is_f_f_to_f_r():
    R, PH, Z, V = _mesh()
    for omega, ff in ((3.0, 0.6), (-3.0, 0.6), (0.0, 1.2)):
        s = _src(omega=omega, f_f=ff)
        q = s.q(R, PH, Z, 0.0)
        xi = (-1.0 if omega < 0 else 1.0) * R * np.sin(PH)
        front = float((q * V)[xi >= 0].sum())
        rear = float((q * V)[xi < 0].sum())
        assert abs(front / (ETA * P) - ff) <= 2e-3, (omega, front)
        assert abs(rear / (ETA * P) - (2.0 - ff)) <= 2e-3, (omega, rear)


def test_peak_value_and_exact_zero_past_the_cut():
    s = _src()
    amp = 6.0 * math.sqrt(3.0) * 0.6 * ETA * P / (A * B * CF * math.pi ** 1.5)
    assert s.q(RC, 0.0, Z0, 0.0) == pytest.approx(amp, rel=1e-15)
    # along the axial direction E = 3 zeta^2 / b^2: zero exactly past E = 40, positive inside
    zc = math.sqrt(40.0 / 3.0) * B
    inside, outside = s.q(RC, 0.0, Z0 + 0.999 * zc, 0.0), s.q(RC, 0.0, Z0 + 1.001 * zc, 0.0)
    assert inside > 0.0 and outside == 0.0
    # the same for a point far round the ring and for the radial direction
    assert s.q(RC, math.pi, Z0, 0.0) == 0.0
    rr = math.sqrt(40.0 / 3.0) * A
    assert s.q(RC + 0.999 * rr, 0.0, Z0, 0.0) > 0.0 and s.q(RC + 1.001 * rr, 0.0, Z0, 0.0) == 0.0


def test_centre_moves_as_defined():
    s = _src(phi0=0.3, omega=-2.5, z0=0.01, v_z=1e-3)
    for t in (0.0, 0.4, 3.7):
        rc, phic, zc = s.center(t)
        assert (rc, phic, zc) == (RC, 0.3 + (-2.5) * t, 0.01 + 1e-3 * t)
        peak = s.q(RC, phic, zc, t)
        assert peak == pytest.approx(s.q(RC, 0.3, 0.01, 0.0), rel=1e-14)
        # omega < 0: the front is towards decreasing phi, so just behind in phi is the (longer, weaker) front... the rear
        ahead, behind = s.q(RC, phic - 1e-3, zc, t), s.q(RC, phic + 1e-3, zc, t)
        f_front = math.exp(-3 * (RC * math.sin(1e-3)) ** 2 / CF ** 2) * 0.6 / CF
        f_rear = math.exp(-3 * (RC * math.sin(1e-3)) ** 2 / CR ** 2) * 1.4 / CR
        assert ahead / behind == pytest.approx(f_front / f_rear, rel=1e-9)


def test_support_across_phi_zero_equals_the_rotated_support():
    g = hipcyl.GridCyl(24, 96, 40, 1e-3, 2 * math.pi / 96, 1e-3, 0.06, R_in=0.04)
    m = 17
    for omega, depth in ((0.0, 'z'), (4.0, 'r'), (-4.0, 'z')):
        t = 0.3
        s0 = _src(phi0=-omega * t, omega=omega, r_c=0.05, depth=depth)          # at t: straddles phi = 0 (cells 95 and 0)
        s1 = _src(phi0=-omega * t + m * g.dphi, omega=omega, r_c=0.05, depth=depth)
        q0, q1 = s0.sample(g, t), s1.sample(g, t)
        assert q0.max() > 0 and q0[:, 0].max() > 0 and q0[:, -1].max() > 0
        np.testing.assert_allclose(np.roll(q0, m, axis=1), q1, rtol=0, atol=1e-12 * q0.max())


def test_sample_respects_the_active_mask():
    g = hipcyl.GridCyl(24, 96, 40, 1e-3, 2 * math.pi / 96, 1e-3, 0.06, R_in=0.04)
    s = _src(r_c=0.05)
    act = np.zeros(g.shape, bool)
    act[:, :, :20] = True
    q = s.sample(g, 0.0, act)
    assert np.array_equal(q[~act], np.zeros(int((~act).sum())))
    np.testing.assert_array_equal(q[act], s.sample(g, 0.0)[act])


BAD = [dict(power=-1.0), dict(eta=1.5), dict(eta=-0.1), dict(a=0.0), dict(b=-1e-3), dict(c_f=0.0), dict(c_r=0.0),
       dict(f_f=0.0), dict(f_f=2.0), dict(r_c=-1e-3), dict(phi0=float('nan')), dict(omega=float('inf')),
       dict(z0=float('nan')), dict(v_z=float('inf'))]
MSG = {'power': 'power < 0', 'eta': 'eta outside', 'a': 'non-positive length', 'b': 'non-positive length',
       'c_f': 'non-positive length', 'c_r': 'non-positive length', 'f_f': 'f_f outside', 'r_c': 'r_c < 0',
       'phi0': 'non-finite', 'omega': 'non-finite', 'z0': 'non-finite', 'v_z': 'non-finite'}


def _c_source(**kw):
    v = dict(power=P, eta=ETA, a=A, b=B, c_f=CF, c_r=CR, f_f=0.6, r_c=RC, phi0=0.0, omega=0.0, z0=Z0, v_z=0.0, depth=0)
    v.update(kw)
    return _lib.CylHeatSource(v['power'], v['eta'], v['a'], v['b'], v['c_f'], v['c_r'], v['f_f'], v['r_c'], v['phi0'],
                              v['omega'], v['z0'], v['v_z'], v['depth'], 0)


@pytest.mark.parametrize('bad', BAD, ids=lambda d: '%s=%r' % next(iter(d.items())))
def test_bad_parameters_are_rejected_in_python_and_by_the_abi(bad):
    (name, val), = bad.items()
    kw = dict(power=P, eta=ETA, a=A, b=B, c_f=CF, c_r=CR)
    pos = {k: kw.pop(k) if k in kw else None for k in ('power', 'eta', 'a', 'b', 'c_f', 'c_r')}
    if name in pos:
        pos[name] = val
    extra = {} if name in pos else {name: val}
    args = dict(f_f=0.6, r_c=RC, z0=Z0)
    args.update(extra)
    with pytest.raises(ValueError, match=re.escape(MSG[name])):
        hipcyl.CylGoldakSource(pos['power'], pos['eta'], pos['a'], pos['b'], pos['c_f'], pos['c_r'], **args)
    h = _c_source(**{name: val})
    fake = ctypes.c_void_p(256)          # never dereferenced: the source is checked first
    with pytest.raises(ValueError, match=re.escape(MSG[name])):
        _lib.check(_lib.lib.adi_cyl_source_set(fake, ctypes.byref(h), 0.0, 1e-3, 0, None))
    with pytest.raises(ValueError, match=re.escape(MSG[name])):
        _lib.check(_lib.lib.adi_cyl_source_sample(ctypes.byref(h), 4, 8, 8, 0, 0.0, 1e-3, 0.1, 1e-3, 0.0, None, fake, None))


def test_bad_depth_and_other_abi_arguments():
    with pytest.raises(ValueError, match='depth'):
        _src(depth='x')
    with pytest.raises(ValueError, match='depth'):
        _lib.check(_lib.lib.adi_cyl_source_set(ctypes.c_void_p(256), ctypes.byref(_c_source(depth=2)), 0.0, 1e-3, 0, None))
    good = _c_source()
    with pytest.raises(ValueError, match='null block'):
        _lib.check(_lib.lib.adi_cyl_source_set(None, ctypes.byref(good), 0.0, 1e-3, 0, None))
    with pytest.raises(ValueError, match='bad t0 / dt / n'):
        _lib.check(_lib.lib.adi_cyl_source_set(ctypes.c_void_p(256), ctypes.byref(good), 0.0, 0.0, 0, None))
    with pytest.raises(ValueError, match='bad t0 / dt / n'):
        _lib.check(_lib.lib.adi_cyl_source_set(ctypes.c_void_p(256), ctypes.byref(good), 0.0, 1e-3, -1, None))
    with pytest.raises(ValueError, match='null source'):
        _lib.check(_lib.lib.adi_cyl_source_set(ctypes.c_void_p(256), None, 0.0, 1e-3, 0, None))
    fake = ctypes.c_void_p(256)
    with pytest.raises(ValueError, match='bad r_in / dr / dphi / dz'):
        _lib.check(_lib.lib.adi_cyl_source_sample(ctypes.byref(good), 4, 8, 8, 0, 0.0, 0.0, 0.1, 1e-3, 0.0, None, fake, None))
    with pytest.raises(ValueError, match='plane_stride'):
        _lib.check(_lib.lib.adi_cyl_source_sample(ctypes.byref(good), 4, 8, 8, 10, 0.0, 1e-3, 0.1, 1e-3, 0.0, None, fake, None))
    with pytest.raises(ValueError, match='null output'):
        _lib.check(_lib.lib.adi_cyl_source_sample(ctypes.byref(good), 4, 8, 8, 0, 0.0, 1e-3, 0.1, 1e-3, 0.0, None, None, None))
    with pytest.raises(ValueError, match='null argument'):
        _lib.check(_lib.lib.adi_cyl_step_src(None, fake, fake, ctypes.c_void_p(512), None, 0.0, 0.0, None))
    with pytest.raises(ValueError, match='bad argument'):
        _lib.check(_lib.lib.adi_cyl_sweep_src(None, 0, fake, fake, fake, None, 0.0, 0.0, None))


def test_step_with_a_source_needs_t():
    g = hipcyl.GridCyl(4, 8, 8, 1e-3, 2 * math.pi / 8, 1e-3, 4e-3)
    args = (np.zeros(g.shape), g, hipcyl.Material(7800.0, 500.0, 30.0), hipcyl.Params(0.01, 1.0), hipcyl.RobinR(0.0, 0.0),
            hipcyl.ZBC())
    with pytest.raises(ValueError, match='t .* is required'):
        hipcyl.adi_step(*args, S=_src(r_c=2e-3))
    with pytest.raises(ValueError, match='t .* is required'):
        hipcyl.adi_step_masked(*args, np.ones(g.shape, bool), S=_src(r_c=2e-3))
    with pytest.raises(TypeError):
        hipcyl.StagedCylStepper(g, args[2], args[3], args[4], args[5], source=np.zeros(g.shape))


def test_block_layout_matches_the_header():
    with open(os.path.join(ROOT, 'include', 'adi_hip.h')) as f:
        hdr = f.read()
    body = re.search(r'typedef struct adi_cyl_heat_source \{(.*?)\} adi_cyl_heat_source;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body)
    names = []
    for line in body.split(';'):
        line = re.sub(r'/\*.*?\*/', '', line).strip()
        if line:
            names += [n.strip() for n in line.split(None, 1)[1].split(',')]
    assert names == [n for n, _ in _lib.CylHeatSource._fields_]
    assert ctypes.sizeof(_lib.CylHeatSource) == 104
    # source, t0, dt, counter: 128 bytes, the counter at the Cartesian block's offset (adi_source_tick serves both)
    assert ctypes.sizeof(_lib.CylHeatSource) + 3 * 8 == _lib.SOURCE_BLOCK_BYTES
    assert ctypes.sizeof(_lib.HeatSource) + 2 * 8 == ctypes.sizeof(_lib.CylHeatSource) + 2 * 8 == 120
    assert '#define ADI_CYL_DEPTH_Z 0' in hdr and '#define ADI_CYL_DEPTH_R 1' in hdr
    assert _lib.CYL_DEPTHS == {'z': 0, 'r': 1}


def test_new_kernels_have_no_scratch_and_no_spills():
    import kernel_meta
    if not os.path.isdir(kernel_meta.LLVM):
        pytest.skip('no ROCm LLVM tools at %s' % kernel_meta.LLVM)
    obj = os.path.join(kernel_meta.CSRC, 'adi_cyl.o')
    assert os.path.exists(obj), 'run `python -m adi_thermal_fields_amd.build` first'
    ks = {k['short']: k for k in kernel_meta.object_kernels(obj)}
    new = ['adi::k_cyl_r_fast_src<8>', 'adi::k_cyl_r_fast_src<16>', 'adi::k_cyl_z_fast_tick<16>', 'adi::k_cyl_source_sample',
           'adi::k_cyl_source_set'] + ['adi::k_cyl_strided_src<%d>' % m for m in (2, 4, 8, 16)] + \
          ['adi::k_cyl_contig_tick<%d, %s>' % (m, v) for m in (2, 4, 8, 16) for v in ('false', 'true')]
    for n in new:
        assert n in ks, n
        k = ks[n]
        assert k['scratch'] == 0 and k.get('vgpr_spill_count', 0) == 0, (n, k)
    for m in (8, 16):   # built for 1024 threads: at most 128 VGPRs, as the plain FAST r kernel
        k = ks['adi::k_cyl_r_fast_src<%d>' % m]
        assert k['vgpr_count'] <= 128 and k['max_flat_workgroup_size'] == 1024, k


def test_spiral_driver_on_the_oracle_reproduces_the_reference():
    """waam.run_spiral_deposition with the NumPy oracle (host arrays) against tests/golden/cyl_spiral_annulus.npz"""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from helpers import golden, rel_linf
    from oracle import cyl_oracle as cyl
    from adi_thermal_fields_amd import waam
    g = golden('cyl', 'spiral_annulus')
    k, rho, cp, Tinf, Tdep, R_in, wall, h_side, h_end, z_back, layer_h, n_layers, nphi, tau, nr = g['params']
    grid, fields, masks = waam.run_spiral_deposition(cyl, g['times'], dict(rho=rho, cp=cp, k=k), Tinf, Tdep, R_in, wall,
                                                     h_side, h_end, z_back, layer_h, int(n_layers), tau, int(nr), int(nphi))
    for i in range(len(g['times'])):
        assert np.array_equal(masks[i], g['active'][i]), i
        assert rel_linf(fields[i], g['fields'][i]) <= 1e-10, i


def test_ring_source_sits_on_the_nozzle():
    from adi_thermal_fields_amd import waam
    s = waam.ring_source(_src(depth='r', f_f=0.7), 0.05, 0.01, 0.013, 2.0)
    assert isinstance(s, hipcyl.CylGoldakSource)
    assert (s.r_c, s.phi0, s.omega, s.z0, s.v_z, s.depth, s.f_f) == (0.055, 0.0, math.pi, 0.013, 0.0, 'r', 0.7)
    assert (s.power, s.eta, s.a, s.b, s.c_f, s.c_r) == (P, ETA, A, B, CF, CR)
