// adi_matlaw_dev.hpp -- the arithmetic of a material law k(T), cp(T) (include/adi_hip.h, "Temperature-dependent conductivity and
// heat capacity"), written once for the three kernels of adi_matlaw.hip and for the host constants of their launches.
// The law is adi_material_law itself, taken by value.  Piece m of its tables is anchored at knot x[m]; on it a table value is
//     V(t) = V[m] + (y[m] + hs[m]*e)*e,   e = t - x[m]          (hs: half the slope; the last piece has slope 0)
// and below the first knot the piece anchored at x[0] with slope 0.  The piece is found by selects over the knots, so no lane
// indexes the kernel arguments and nothing goes to scratch.  Every function: IEEE fp64, one operation per statement, no
// contraction -- MaterialLaw (phase.py) performs the same operations in NumPy.
#pragma once
#include <math.h>

#include "adi_cart_host.hpp"

namespace adi {

typedef adi_material_law MatLaw;

__host__ __device__ __forceinline__ double mat_fwd(double t, double xa, double y, double hs, double Va)
{
#pragma clang fp contract(off)
    const double e = t - xa;
    const double a1 = hs * e;
    const double a2 = y + a1;
    const double a3 = a2 * e;
    return Va + a3;
}

// t with V(t) = V: e = 2 dV / (y + sqrt(y*y + s2*dV)), s2 twice the slope -- no cancellation, and dV / y where the slope is 0
__host__ __device__ __forceinline__ double mat_inv(double V, double xa, double y, double s2, double Va)
{
#pragma clang fp contract(off)
    const double dV = V - Va;
    const double b1 = y * y;
    const double b2 = s2 * dV;
    const double b3 = b1 + b2;
    const double r = sqrt(b3);
    const double den = y + r;
    const double num = dV + dV;
    const double e = num / den;
    return xa + e;
}

// Theta(t)
__host__ __device__ __forceinline__ double mat_theta(const MatLaw &w, double t)
{
    double xa = w.x[0], y = w.kq[0], hs = 0.0, Va = w.theta[0];
    for (int m = 0; m < w.n_knots; ++m)
        if (t >= w.x[m]) { xa = w.x[m]; y = w.kq[m]; hs = w.hks[m]; Va = w.theta[m]; }
    return mat_fwd(t, xa, y, hs, Va);
}

// k(t) / k_ref
__host__ __device__ __forceinline__ double mat_kq(const MatLaw &w, double t)
{
#pragma clang fp contract(off)
    double xa = w.x[0], y = w.kq[0], hs = 0.0;
    for (int m = 0; m < w.n_knots; ++m)
        if (t >= w.x[m]) { xa = w.x[m]; y = w.kq[m]; hs = w.hks[m]; }
    const double e = t - xa;
    const double s = hs + hs;
    const double a1 = s * e;
    return y + a1;
}

// Theta(t) and H(t) from the one piece that holds t
__device__ __forceinline__ void mat_theta_enthalpy(const MatLaw &w, double t, double &th, double &H)
{
    double xa = w.x[0], ky = w.kq[0], khs = 0.0, kV = w.theta[0], cy = w.c_lo, chs = 0.0, cV = w.H[0];
    for (int m = 0; m < w.n_knots; ++m)
        if (t >= w.x[m]) {
            xa = w.x[m];
            ky = w.kq[m]; khs = w.hks[m]; kV = w.theta[m];
            cy = w.c[m]; chs = w.hcs[m]; cV = w.H[m];
        }
    th = mat_fwd(t, xa, ky, khs, kV);
    H = mat_fwd(t, xa, cy, chs, cV);
}

__device__ __forceinline__ double mat_theta_inv(const MatLaw &w, double V)
{
    double xa = w.x[0], y = w.kq[0], s2 = 0.0, Va = w.theta[0];
    for (int m = 0; m < w.n_knots; ++m)
        if (V >= w.theta[m]) { xa = w.x[m]; y = w.kq[m]; s2 = w.ks2[m]; Va = w.theta[m]; }
    return mat_inv(V, xa, y, s2, Va);
}

__device__ __forceinline__ double mat_enthalpy_inv(const MatLaw &w, double V)
{
    double xa = w.x[0], y = w.c_lo, s2 = 0.0, Va = w.H[0];
    for (int m = 0; m < w.n_knots; ++m)
        if (V >= w.H[m]) { xa = w.x[m]; y = w.c[m]; s2 = w.cs2[m]; Va = w.H[m]; }
    return mat_inv(V, xa, y, s2, Va);
}

// ADI_OK, or the first rule of the header the law breaks
inline int check_matlaw(const char *who, const adi_material_law &s)
{
    const int n = s.n_knots;
    ADI_REQUIRE(n >= 2 && n <= ADI_MATLAW_MAX_KNOTS, "%s: a material law has 2 to %d knots, not %d", who, ADI_MATLAW_MAX_KNOTS, n);
    ADI_REQUIRE(isfinite(s.k_ref) && s.k_ref > 0.0 && isfinite(s.cp_ref) && s.cp_ref > 0.0 && isfinite(s.c_lo) && s.c_lo > 0.0,
                "%s: k_ref, cp_ref and c_lo must be finite and > 0", who);
    for (int m = 0; m < n; ++m) {
        ADI_REQUIRE(isfinite(s.x[m]) && isfinite(s.kq[m]) && isfinite(s.hks[m]) && isfinite(s.ks2[m]) && isfinite(s.theta[m]) &&
                        isfinite(s.c[m]) && isfinite(s.hcs[m]) && isfinite(s.cs2[m]) && isfinite(s.H[m]),
                    "%s: material law not finite at knot %d", who, m);
        ADI_REQUIRE(s.kq[m] > 0.0 && s.c[m] > 0.0, "%s: k and cp must be > 0 (knot %d)", who, m);
        ADI_REQUIRE(m == 0 || (s.x[m] > s.x[m - 1] && s.theta[m] > s.theta[m - 1] && s.H[m] > s.H[m - 1]),
                    "%s: knots, Theta or H do not increase at knot %d", who, m);
        // (the radicand of the inverse stays > 0 up to the next knot)
        ADI_REQUIRE(m == 0 || (s.kq[m - 1] * s.kq[m - 1] + s.ks2[m - 1] * (s.theta[m] - s.theta[m - 1]) > 0.0 &&
                               s.c[m - 1] * s.c[m - 1] + s.cs2[m - 1] * (s.H[m] - s.H[m - 1]) > 0.0),
                    "%s: slopes and integrals of the material law disagree on the interval below knot %d", who, m);
    }
    ADI_REQUIRE(s.hks[n - 1] == 0.0 && s.ks2[n - 1] == 0.0 && s.hcs[n - 1] == 0.0 && s.cs2[n - 1] == 0.0,
                "%s: the last piece of a material law has slope 0", who);
    return ADI_OK;
}

}  // namespace adi
