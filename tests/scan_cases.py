"""Shared fixtures of the scan-path tests (test_scan_path_cpu.py, test_scan_path_gpu.py): shapes, paths, the time-quadrature
reference of the step-averaged source, its closed-form energy and the oracle step with the source folded into the axis-0 pack."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

RHO, CP, K = 7800.0, 500.0, 30.0
KAPPA = K / (RHO * CP)
DX = 1e-4
DT = 0.5 * DX * DX / KAPPA                   # the step of the moving-source tests (test_heat_source_gpu.py)

# the double ellipsoid of the Goldak tests; SMALL: a support of a few cells, for the small grids of the box tests
SHAPE = dict(eta=0.8, a=3e-4, b=2.5e-4, c_f=3e-4, c_r=6e-4, f_f=0.6)
SMALL = dict(eta=0.8, a=1.2e-4, b=1.2e-4, c_f=1.2e-4, c_r=1.8e-4, f_f=0.7)


class HostGrid:
    """what ScanPath.sample_step reads of a grid, without a device"""

    def __init__(self, shape, dx, mask=None):
        self.nx, self.ny, self.nz = shape
        self.dx = dx
        self.mask = np.ones(shape, dtype=bool) if mask is None else mask

    @property
    def shape(self):
        return (self.nx, self.ny, self.nz)


def rel_linf(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def axes_of(depth_axis):
    return (1 if depth_axis == 0 else 0), (1 if depth_axis == 2 else 2)


def point(depth_axis, u, v, z):
    """the point with in-plane coordinates (u, v) and depth coordinate z"""
    p = [0.0, 0.0, 0.0]
    au, av = axes_of(depth_axis)
    p[au], p[av], p[depth_axis] = u, v, z
    return tuple(p)


def continuous(shape):
    """the same shape with f_f chosen so that the source is continuous across xi = 0 (f_f / c_f = f_r / c_r)"""
    s = dict(shape)
    s['f_f'] = 2.0 * s['c_f'] / (s['c_f'] + s['c_r'])
    return s


def quadrature_step(path, grid, t, dt, npts=200):
    """the step-averaged source by Gauss-Legendre quadrature in time of the instantaneous double ellipsoid (GoldakSource's q in
    the frame of each leg), `npts` points on every piece of a segment inside [t, t + dt]; independent of ScanPath.q_step"""
    xs, ws = np.polynomial.legendre.leggauss(npts)
    x = [(np.arange(n, dtype=np.float64) + 0.5) * grid.dx for n in (grid.nx, grid.ny, grid.nz)]
    X = (x[0][:, None, None], x[1][None, :, None], x[2][None, None, :])
    au, av = axes_of(path.depth_axis)
    tab = path.table()
    out = np.zeros((grid.nx, grid.ny, grid.nz))
    for k in range(tab.shape[0]):
        tb, p, d, vel, P = tab[k, 0], tab[k, 1:4], tab[k, 4:6], tab[k, 6], tab[k, 7]
        te = tab[k + 1, 0] if k + 1 < tab.shape[0] else path.t_end
        tau0, tau1 = max(t, tb), min(t + dt, te)
        if P <= 0 or tau1 <= tau0:
            continue
        ou, ov, z = X[au] - p[au], X[av] - p[av], X[path.depth_axis] - p[path.depth_axis]
        xi0 = ou * d[0] + ov * d[1]
        y = ov * d[0] - ou * d[1]
        Et = 3.0 * y * y / path.a ** 2 + 3.0 * z * z / path.b ** 2
        for xq, wq in zip(xs, ws):
            tq = 0.5 * (tau0 + tau1) + 0.5 * (tau1 - tau0) * xq
            xi = xi0 - vel * (tq - tb)
            f = np.where(xi >= 0, path.f_f, 2.0 - path.f_f)
            c = np.where(xi >= 0, path.c_f, path.c_r)
            q = 6.0 * np.sqrt(3.0) * f * path.eta * P / (path.a * path.b * c * np.pi ** 1.5) * np.exp(-(3.0 * xi * xi / c ** 2 + Et))
            out += (0.5 * (tau1 - tau0) * wq / dt) * q
    return np.where(grid.mask, out, 0.0)


def closed_form_energy(path, t, dt):
    """sum_k 2 eta P_k (tau1 - tau0) over the pieces inside [t, t + dt], from the segment table"""
    tab = path.table()
    e = 0.0
    for k in range(tab.shape[0]):
        te = tab[k + 1, 0] if k + 1 < tab.shape[0] else path.t_end
        w = min(t + dt, te) - max(t, tab[k, 0])
        if w > 0 and tab[k, 7] > 0:
            e += 2.0 * path.eta * tab[k, 7] * w
    return e


def leg_path(hip, shape, lo, angle_deg, length, speed, depth_axis=2, power=800.0, t_start=0.0, **kw):
    """one leg of `length` from the point `lo` = (u, v, z) along the in-plane direction at angle_deg from +u"""
    s = dict(shape)
    s.update(kw)
    a = np.radians(angle_deg)
    c, sn = np.cos(a), np.sin(a)
    if angle_deg % 90 == 0:
        c, sn = float(round(c)), float(round(sn))
    path = hip.ScanPath(power=power, depth_axis=depth_axis, start=point(depth_axis, *lo), t_start=t_start, **s)
    return path.line_to(point(depth_axis, lo[0] + length * c, lo[1] + length * sn, lo[2]), speed)


def tour_path(hip, shape, org, step, speed, depth_axis=2, power=800.0, t_start=0.0):
    """a leg along +u, a 90 degree corner, a leg along +v, a jump back, a dwell with power, a leg along -u: `org` = (u, v, z),
    legs of length `step`"""
    u, v, z = org
    P = lambda a, b: point(depth_axis, a, b, z)
    path = hip.ScanPath(power=power, depth_axis=depth_axis, start=P(u, v), t_start=t_start, **shape)
    path.line_to(P(u + step, v), speed)
    path.line_to(P(u + step, v + step), speed)
    path.line_to(P(u + 0.5 * step, v + 0.5 * step), 4.0 * speed, power=0.0)
    path.dwell(0.5 * step / speed, power=0.5 * power)
    path.line_to(P(u - 0.5 * step, v + 0.5 * step), speed)
    return path


def make_case(shape, dx=DX, **kw):
    """the mask, Dirichlet, Robin and Neumann mix of the Goldak tests, the hole under the path included"""
    from test_heat_source_gpu import make_case as mc
    return mc(shape, dx, **kw)


def setup(hip, orc, shape, dx=DX, dt=DT, **case):
    mask, kw, T0 = make_case(shape, dx, **case)
    g, go = hip.Grid3D(*shape, dx, mask), orc.Grid3D(*shape, dx, mask)
    mat, mato = hip.Material(RHO, CP, K), orc.Material(RHO, CP, K)
    prm, prmo = hip.Params(dt, 0.5), orc.Params(dt, 0.5)
    packs = hip.precompute_coeff_packs_unified(g, mat, **kw)
    return g, go, mat, mato, prm, prmo, packs, kw, T0


def oracle_step(orc, T, grid, mat, prm, kw, q, Tinf=300.0):
    """one oracle step with the source field q folded into the axis-0 pack's qflux: R0 += dt*q/(rho cp) on free rows"""
    packs = orc.precompute_coeff_packs_unified(grid, mat, **kw)
    packs[0].qflux = packs[0].qflux + q / (RHO * CP)
    return orc.adi_step_numba_coeff(T, grid, mat, prm, packs, Tinf=Tinf)
