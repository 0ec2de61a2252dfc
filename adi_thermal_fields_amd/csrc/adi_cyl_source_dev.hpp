// adi_cyl_source_dev.hpp -- device evaluator of the cylindrical step's moving heat source (include/adi_hip.h, "Moving heat
// source of the cylindrical step"), included by adi_cyl.hip only.
// The r sweep's load adds dt*q/(rho cp) to R0, q evaluated in registers: no source field, the step's traffic is unchanged.
#pragma once
#include <cstddef>

#include "adi_goldak_dev.hpp"

namespace adi {

struct CylSrcBlock {
    adi_cyl_heat_source s;
    double t0, dt;
    unsigned long long n;
};
static_assert(sizeof(CylSrcBlock) == ADI_SOURCE_BLOCK_BYTES, "cylindrical source block layout");
static_assert(offsetof(CylSrcBlock, n) == 120, "the counter sits where the Cartesian block keeps it (adi_source_tick)");

struct CylGeo {
    double r_in, dr, dphi, dz;
    int nz;
};

constexpr double kCylTwoPi = 6.283185307179586;

// what one launch needs of the source at time t (uniform over the grid), and per line the angle's sin / cos and the axial term
struct CylSrcEval {
    double rc, phic, zc, sgn, amp_f, amp_r, cf, cr, lrad, lax;
    double sn, cs, ez;
};

__device__ inline void cyl_src_init(const adi_cyl_heat_source &s, double t, CylSrcEval &e)
{
#pragma clang fp contract(off)
    e.rc = s.r_c;
    e.phic = s.phi0 + s.omega * t;
    e.zc = s.z0 + s.v_z * t;
    e.sgn = s.omega < 0.0 ? -1.0 : 1.0;
    e.amp_f = goldak_amp(s.f_f, s.eta, s.power, s.a, s.b, s.c_f);
    e.amp_r = goldak_amp(2.0 - s.f_f, s.eta, s.power, s.a, s.b, s.c_r);
    e.cf = s.c_f; e.cr = s.c_r;
    e.lrad = s.depth == ADI_CYL_DEPTH_Z ? s.a : s.b;   // length of the radial offset rho
    e.lax = s.depth == ADI_CYL_DEPTH_Z ? s.b : s.a;    // length of the axial offset zeta
}

// t_n + dt/2 of the block
__device__ inline double cyl_src_tmid(const CylSrcBlock &B) { return goldak_tmid(B.t0, B.dt, B.n); }

// Whether the cells of the lines [l0, l1] of one radius plane (line = j*nz + k) can meet the support; uniform over a tile.
// Axially: the z range of the lines (all of it when they cross a phi boundary) against z_c +- R*lax.  In the plane: the
// support lies in the disc of radius reach = R*max(c_f, c_r, lrad) about (r_c, phi_c), whose points all lie within
// asin(reach/r_c) of phi_c (every angle when reach >= r_c).  R = sqrt(E_CUT/3); a relative slack of 1e-6 keeps rounding on
// the safe side.
__device__ inline bool cyl_src_tile(const CylSrcEval &e, long l0, long l1, const CylGeo &G)
{
    const double R = sqrt(ADI_SOURCE_E_CUT / 3.0) * (1.0 + 1e-6);
    const unsigned nz = (unsigned)G.nz, j0 = (unsigned)l0 / nz, j1 = (unsigned)l1 / nz;   // (a plane is < 2^31 lines)
    const double zlo = j0 == j1 ? ((double)((unsigned)l0 - j0 * nz) + 0.5) * G.dz : 0.5 * G.dz;
    const double zhi = j0 == j1 ? ((double)((unsigned)l1 - j1 * nz) + 0.5) * G.dz : ((double)nz - 0.5) * G.dz;
    const double hz = R * e.lax;
    if (zhi < e.zc - hz || zlo > e.zc + hz) return false;
    const double reach = R * fmax(fmax(e.cf, e.cr), e.lrad);
    if (reach >= e.rc) return true;
    const double half = asin(reach / e.rc) * (1.0 + 1e-6) + 1e-12;
    const double plo = ((double)j0 + 0.5) * G.dphi, span = (double)(j1 - j0) * G.dphi;
    const double x = e.phic - plo;
    const double u = x - kCylTwoPi * floor(x * (1.0 / kCylTwoPi));   // phi_c - phi_lo in [0, 2 pi) (up to rounding)
    if (u <= span) return true;
    return fmin(u - span, kCylTwoPi - u) <= half;   // (u rounded past 2 pi or below 0 only shrinks a distance)
}

// per line (j, k): false when the axial term alone puts every cell of the line outside the support
__device__ inline bool cyl_src_line(CylSrcEval &e, long line, const CylGeo &G)
{
#pragma clang fp contract(off)
    const unsigned j = (unsigned)line / (unsigned)G.nz, k = (unsigned)line - j * (unsigned)G.nz;
    e.ez = goldak_eterm(((double)k + 0.5) * G.dz - e.zc, e.lax);
    if (!(e.ez <= ADI_SOURCE_E_CUT)) return false;
    sincos(((double)j + 0.5) * G.dphi - e.phic, &e.sn, &e.cs);
    return true;
}

// q at radius r of the current line; exp only where the exponent passes the cut
__device__ inline double cyl_src_q(const CylSrcEval &e, double r)
{
#pragma clang fp contract(off)
    const double xi = e.sgn * (r * e.sn);
    const double rho = r * e.cs - e.rc;
    const bool front = xi >= 0.0;
    const double E = (goldak_eterm(xi, front ? e.cf : e.cr) + goldak_eterm(rho, e.lrad)) + e.ez;
    if (!(E <= ADI_SOURCE_E_CUT)) return 0.0;
    return (front ? e.amp_f : e.amp_r) * exp(-E);
}
__device__ inline double cyl_src_row(const CylSrcEval &e, const CylGeo &G, int i)
{
#pragma clang fp contract(off)
    return cyl_src_q(e, G.r_in + ((double)i + 0.5) * G.dr);   // GridCyl.r
}

}  // namespace adi
