"""tests/cyl_ref_ld.py -- TEST INFRASTRUCTURE.  Extended-precision (np.longdouble) restatement of the cylindrical
backward-Euler step, written from the equations in the docstrings of oracle/cyl_oracle.py (adi3d_cyl_phi_v3.py:155-350 and
the void-clamping wrapper quick_spiral_deposition_gif_v5.py:31-70).  It shares no code with oracle/cyl_oracle.py and does
not use numpy.fft: it is the reference the float64 oracle itself is measured against (tests/test_cyl_ref_cpu.py) and the
reference of the time-step sweep of tests/test_cyl_switches_gpu.py, where alpha*dt/dr^2 runs from 1e-13 to 1e6 and the phi
factor alpha*dt/(r^2 dphi^2) to 3e9.

One step:  R0 = Tn + dt S/(rho cp);  r lines:  a_i x_{i-1} + b_i x_i + c_i x_{i+1} = R0_i;  phi lines, per radius:
(1 + 2 fac_i) x_j - fac_i (x_{j-1} + x_{j+1}) = d_j, periodic, fac_0 = 0 exactly;  z lines with the closures of build_coeff_z.

Every operator here is  I + (a weighted graph Laplacian) + (non-negative Robin terms): a row is
    (e_i + p_i + q_i) x_i - p_i x_{i-1} - q_i x_{i+1} = d_i,      p_i, q_i >= 0,  e_i >= 1  (its "excess").
Thomas on that form needs no subtraction: with the pivot  P_i = s_i + q_i,
    s_0 = e_0,   s_i = e_i + p_i s_{i-1} / P_{i-1},   d'_i = d_i + p_i d'_{i-1} / P_{i-1},   x_i = (d'_i + q_i x_{i+1}) / P_i
only adds and multiplies positive numbers (the fields are temperatures > 0), so the result keeps the full relative precision
of the format at any alpha*dt/h^2 -- the textbook form  P_i = b_i - a_i c_{i-1} / P_{i-1}  cancels ~log10(f) digits.

The periodic phi system (n >= 3) is solved directly by eliminating the last unknown x_m, m = n - 1: rows 0 .. m-1 form an
ordinary tridiagonal T of the same kind (rows 0 and m-1 have excess 1 + f: their coupling to x_m), and with
    T y = d[0:m],   T q = f (e_0 + e_{m-1}),   T g = 1     (so that q = 1 - g, because T 1 = 1 + f (e_0 + e_{m-1}))
the last row gives  x_m (1 + f (g_0 + g_{m-1})) = d_m + f (y_0 + y_{m-1})  and  x[0:m] = y + x_m q: again no subtraction (the
Schur complement 1 + 2f - f (q_0 + q_{m-1}) is evaluated through g).  n = 2: both neighbours of a cell are the same cell,
(1 + 2f) x_0 - 2f x_1 = d_0, solved in closed form x_0 = (d_0 + 2f (d_0 + d_1)) / (1 + 4f).  n = 1: a copy.
"""
import numpy as np

LD = np.longdouble


def _ld(x):
    return np.asarray(x, dtype=LD)


def thomas_excess(p, q, e, d):
    """Rows along the LAST axis of d; p, q, e broadcast against d (p[..., 0] and q[..., -1] are ignored).  See the module
    docstring: subtraction-free Thomas for (e + p + q) x_i - p x_{i-1} - q x_{i+1} = d."""
    d = _ld(d)
    n = d.shape[-1]
    shape = d.shape
    p = np.broadcast_to(_ld(p), shape); q = np.broadcast_to(_ld(q), shape); e = np.broadcast_to(_ld(e), shape)
    P = np.empty(shape, LD); dp = np.empty(shape, LD); x = np.empty(shape, LD)
    qq = lambda i: q[..., i] if i < n - 1 else LD(0)
    s = e[..., 0]
    P[..., 0] = s + qq(0)
    dp[..., 0] = d[..., 0]
    for i in range(1, n):
        w = p[..., i] / P[..., i - 1]
        s = e[..., i] + w * s
        P[..., i] = s + qq(i)
        dp[..., i] = d[..., i] + w * dp[..., i - 1]
    x[..., n - 1] = dp[..., n - 1] / P[..., n - 1]
    for i in range(n - 2, -1, -1):
        x[..., i] = (dp[..., i] + q[..., i] * x[..., i + 1]) / P[..., i]
    return x


def _geometry(grid):
    nr = grid.nr
    dr = LD(grid.dr)
    r = LD(getattr(grid, 'R_in', 0.0)) + (np.arange(nr, dtype=LD) + LD(0.5)) * dr
    return r, dr


def solve_r(R0, grid, mat, dt, robin_r):
    """build_coeff_r with theta = 1: a_i = -F r_{i-1/2}/(r_i dr^2), c_i = -F r_{i+1/2}/(r_i dr^2), b_i = 1 - (a_i + c_i),
    F = alpha dt; a_0 = 0; the outer row has c = 0 and, for h != 0, the Robin term
    F r_{N+1/2} (h/k) / (r_N dr) on the diagonal and times T_inf on the right-hand side."""
    nr = grid.nr
    assert nr >= 2, "cyl_ref_ld restates grids of at least two radii (for nr = 1 the reference's outer row replaces the axis row)"
    r, dr = _geometry(grid)
    F = LD(mat.k) / (LD(mat.rho) * LD(mat.cp)) * LD(dt)
    tiny = LD(1e-15)
    r_i = np.maximum(r, tiny)
    p = F * (np.maximum(r - LD(0.5) * dr, tiny) / (r_i * dr * dr))
    q = F * ((r + LD(0.5) * dr) / (r_i * dr * dr))
    e = np.ones(nr, LD)
    p[0] = 0
    q[-1] = 0
    d = np.array(np.moveaxis(_ld(R0), 0, -1))               # (nphi, nz, nr)
    h = LD(robin_r.h)
    if h != 0:
        rob = F * ((r[-1] + LD(0.5) * dr) * (h / LD(mat.k))) / (r_i[-1] * dr)
        e[-1] = e[-1] + rob
        d[..., -1] = d[..., -1] + rob * LD(robin_r.T_inf)
    return np.moveaxis(thomas_excess(p, q, e, d), -1, 0)


def solve_phi(T, grid, mat, dt):
    nr, n, nz = T.shape
    T = _ld(T)
    if n == 1:
        return T.copy()
    r, _ = _geometry(grid)
    dphi = LD(grid.dphi)
    f = LD(mat.k) / (LD(mat.rho) * LD(mat.cp)) * LD(dt) / (r * r * dphi * dphi)
    f[0] = 0                                                 # phi_solve_spectral: the loop starts at ir = 1
    d = np.array(np.moveaxis(T, 1, -1))                      # (nr, nz, nphi)
    fb = f[:, None]                                          # broadcast over z
    if n == 2:
        sm = d[..., 0] + d[..., 1]
        x = np.empty_like(d)
        for j in (0, 1):
            x[..., j] = (d[..., j] + 2 * fb * sm) / (1 + 4 * fb)
        return np.moveaxis(x, -1, 1)
    m = n - 1
    fm = np.broadcast_to(fb[..., None], (nr, nz, m))
    e = np.ones((nr, 1, m), LD)
    e[:, 0, 0] += f; e[:, 0, m - 1] += f
    e = np.broadcast_to(e, (nr, nz, m))
    y = thomas_excess(fm, fm, e, d[..., :m])
    # the two table solves do not depend on z
    f1 = f[:, None]
    fm1 = np.broadcast_to(f1, (nr, m))
    e1 = np.ones((nr, m), LD); e1[:, 0] += f; e1[:, m - 1] += f
    rhs_q = np.zeros((nr, m), LD); rhs_q[:, 0] += f; rhs_q[:, m - 1] += f
    q = thomas_excess(fm1, fm1, e1, rhs_q)
    g = thomas_excess(fm1, fm1, e1, np.ones((nr, m), LD))
    S = 1 + f * (g[:, 0] + g[:, m - 1])                      # Schur complement of x_m
    xm = (d[..., m] + fb * (y[..., 0] + y[..., m - 1])) / S[:, None]
    x = np.empty_like(d)
    x[..., :m] = y + xm[..., None] * q[:, None, :]
    x[..., m] = xm
    return np.moveaxis(x, -1, 1)


def solve_z(T, grid, mat, dt, zbc):
    """build_coeff_z with theta = 1, f = alpha dt/dz^2: interior (-f, 1+2f, -f); neumann0 end: diagonal 1 + f; robin end:
    diagonal 1 + f (1 + beta dz), right-hand side + alpha dt (beta/dz) T_inf, beta = h/k; dirichlet end: identity row with the
    right-hand side replaced by the end temperature."""
    nz = grid.nz
    assert nz >= 2, "cyl_ref_ld restates grids of at least two cells along z (for nz = 1 the top closure replaces the bottom one)"
    d = np.array(_ld(T))
    dz = LD(grid.dz)
    ad = LD(mat.k) / (LD(mat.rho) * LD(mat.cp)) * LD(dt)
    f = ad / (dz * dz)
    p = np.full(nz, f, LD); q = np.full(nz, f, LD); e = np.ones(nz, LD)
    p[0] = 0; q[-1] = 0

    def end(i, kind, h, T_inf, T_dir):
        if kind == 'neumann0':
            return
        if kind == 'dirichlet':
            p[i] = 0; q[i] = 0; e[i] = 1
            d[..., i] = LD(T_dir)
        elif kind == 'robin':
            beta = LD(h) / LD(mat.k)
            e[i] = e[i] + f * (beta * dz)
            d[..., i] = d[..., i] + ad * (beta / dz) * LD(T_inf)
        else:
            raise ValueError("unknown z closure %r" % (kind,))
    end(0, zbc.kind_bot, zbc.h_bot, zbc.T_inf_bot, zbc.T_bot)
    end(nz - 1, zbc.kind_top, zbc.h_top, zbc.T_inf_top, zbc.T_top)
    return thomas_excess(p, q, e, d)


def adi_step(Tn, grid, mat, prm, robin_r, zbc, S=None):
    """one backward-Euler step r -> phi -> z in np.longdouble; returns a longdouble array (nr, nphi, nz)"""
    dt = prm.dt
    R0 = _ld(Tn)
    if S is not None:
        R0 = R0 + LD(dt) * (_ld(S) / (LD(mat.rho) * LD(mat.cp)))
    return solve_z(solve_phi(solve_r(R0, grid, mat, dt, robin_r), grid, mat, dt), grid, mat, dt, zbc)


def adi_step_masked(Tn, grid, mat, prm, robin_outer, zbc, active, robin_inner=None, robin_void=None):
    """void cells at robin_void.T_inf before and after the step, inactive cells of the axis row at robin_inner.T_inf after it"""
    robin_inner = robin_inner or robin_outer
    robin_void = robin_void or robin_outer
    active = np.asarray(active, dtype=bool)
    T = np.array(_ld(Tn))
    T[~active] = LD(robin_void.T_inf)
    T = adi_step(T, grid, mat, prm, robin_outer, zbc)
    T[~active] = LD(robin_void.T_inf)
    T[0][~active[0]] = LD(robin_inner.T_inf)
    return T


def residual(x, d, grid, mat, dt):
    """max |A_phi x - d| / max |d| of the periodic phi system, evaluated row by row in longdouble (a check of solve_phi that
    does not go through its elimination)"""
    x = _ld(x); d = _ld(d)
    r, _ = _geometry(grid)
    f = LD(mat.k) / (LD(mat.rho) * LD(mat.cp)) * LD(dt) / (r * r * LD(grid.dphi) ** 2)
    f[0] = 0
    fb = f[:, None, None]
    res = x + fb * ((x - np.roll(x, 1, axis=1)) + (x - np.roll(x, -1, axis=1))) - d
    return float(np.max(np.abs(res)) / np.max(np.abs(d)))
