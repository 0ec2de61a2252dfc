// adi_cyl_plan.hpp -- every table and scalar a plan of the cylindrical step holds, built on the host: plain arithmetic, no
// HIP call, so adi_cyl_plan_tables shows a CPU test exactly what adi_cyl_plan_create_annular uploads.  Included by
// adi_cyl.hip only.  The builders follow adi3d_cyl_phi_v3.py operation for operation (BE branch: theta = 1); `tad` is
// theta*alpha*dt, which the reference forms first in each of them.
#pragma once
#include <math.h>
#include <stddef.h>

#include <vector>

#include "../../include/adi_hip.h"

namespace adi {

// layout of the r FAST tables: per segment RF_STRIDE doubles, arrays of RF_MAXM - 1 rows (CylRSegView, adi_cyl_dev.hpp)
constexpr int RF_MAXM = ADI_CYL_RF_MAXM;
constexpr int RF_STRIDE = 4 * (RF_MAXM - 1) + 10 + 13;
static_assert(RF_STRIDE == ADI_CYL_RF_STRIDE, "r FAST table layout (include/adi_hip.h)");

struct CylTables {
    std::vector<double> ar, br, cr;        // [nr] r operator
    double r_add_last;                     // Robin increment of the last row's right-hand side
    std::vector<double> pf, zt, smden;     // [nr] phi factors, [nr * nphi] Sherman-Morrison vectors, [nr] 1 / (1 + v.z)
    double z[ADI_CYL_ZCLOSURE_LEN];        // f b0 bN aN c0 add0 addN T0 TN dir0 dirN: the members of CylZ in order
    int r_M, r_nseg, phi_M;                // rows per thread of the FAST kernels (0: not available for this axis length)
    std::vector<double> rfac;              // [r_nseg][RF_STRIDE]
};

// build_coeff_r, adi3d_cyl_phi_v3.py:155-202
inline void cyl_build_r(int nr, double dr, double r_in, double tad, double k, double robin_h, double robin_Tinf, CylTables &T)
{
    std::vector<double> &ar = T.ar, &br = T.br, &cr = T.cr;
    std::vector<double> r_i(nr), r_imh(nr), r_iph(nr);
    ar.assign(nr, 0.0); br.assign(nr, 0.0); cr.assign(nr, 0.0);
    for (int i = 0; i < nr; ++i) {
        const double r = r_in + ((double)i + 0.5) * dr;       // GridCyl.r, :38 (+ the inner radius of an annular grid)
        r_i[i] = fmax(r, 1e-15);
        r_imh[i] = fmax(r - 0.5 * dr, 1e-15);
        r_iph[i] = r + 0.5 * dr;
    }
    const double fac = tad;
    for (int i = 1; i < nr - 1; ++i) {
        const double ai = -fac * (r_imh[i] / (r_i[i] * dr * dr));
        const double ci = -fac * (r_iph[i] / (r_i[i] * dr * dr));
        ar[i] = ai; cr[i] = ci; br[i] = 1.0 - (ai + ci);
    }
    const double c0 = -fac * (r_iph[0] / (r_i[0] * dr * dr));
    ar[0] = 0.0; br[0] = 1.0 - c0; cr[0] = c0;
    const int N = nr - 1;
    const double aN = -fac * (r_imh[N] / (r_i[N] * dr * dr));
    double bN = 1.0 + fac * (r_imh[N] / (r_i[N] * dr * dr));
    T.r_add_last = 0.0;
    if (robin_h != 0.0) {
        bN += fac * (r_iph[N] * (robin_h / k)) / (r_i[N] * dr);
        T.r_add_last = fac * (r_iph[N] * (robin_h / k)) / (r_i[N] * dr) * robin_Tinf;
    }
    // the reference writes the outer row last, so for nr == 1 it overrides the axis row (:187-190)
    ar[N] = aN; br[N] = bN; cr[N] = 0.0;
    if (nr == 1) ar[0] = 0.0;  // a[0] multiplies nothing in thomas_batch
}

// phi: fac_i and the Sherman-Morrison vectors; phi_solve_spectral, :302-329.  The circulant (-f, 1+2f, -f) is the
// tridiagonal A' with diagonal (2 b0, b0, ..., b0 + f^2/b0), b0 = 1 + 2f, plus u v^T; zt = A'^-1 u, smden = 1 / (1 + v.zt)
inline void cyl_build_phi(int nr, int nphi, double dr, double dphi, double r_in, double tad, CylTables &T)
{
    std::vector<double> &pf = T.pf, &zt = T.zt, &smden = T.smden;
    pf.assign(nr, 0.0); zt.assign((size_t)nr * nphi, 0.0); smden.assign(nr, 1.0);
    for (int i = 1; i < nr; ++i) {
        const double r = r_in + ((double)i + 0.5) * dr;
        pf[i] = tad / (r * r * dphi * dphi);
    }
    if (nphi <= 2) return;
    std::vector<double> cpv(nphi), dpv(nphi);
    for (int i = 0; i < nr; ++i) {
        const double f = pf[i], b0 = 1.0 + 2.0 * f;
        // A' z = u,  u = (gamma, 0, ..., 0, alpha_c) with gamma = -b0, alpha_c = -f
        const int n = nphi;
        auto bb = [&](int j) { return j == 0 ? 2.0 * b0 : (j == n - 1 ? b0 + f * f / b0 : b0); };
        auto uu = [&](int j) { return j == 0 ? -b0 : (j == n - 1 ? -f : 0.0); };
        cpv[0] = (-f) / bb(0);
        dpv[0] = uu(0) / bb(0);
        for (int j = 1; j < n; ++j) {
            const double den = bb(j) - (-f) * cpv[j - 1];
            cpv[j] = (j < n - 1 ? -f : 0.0) / den;
            dpv[j] = (uu(j) - (-f) * dpv[j - 1]) / den;
        }
        double *z = &zt[(size_t)i * n];
        z[n - 1] = dpv[n - 1];
        for (int j = n - 2; j >= 0; --j) z[j] = dpv[j] - cpv[j] * z[j + 1];
        smden[i] = 1.0 / (1.0 + z[0] + (f / b0) * z[n - 1]);
    }
}

// z closure: build_coeff_z, :255-298
inline void cyl_build_z(double dz, double tad, double k, int kind_bot, int kind_top, double h_bot, double h_top,
                        double Tinf_bot, double Tinf_top, double T_bot, double T_top, double (&z)[ADI_CYL_ZCLOSURE_LEN])
{
    const double f = tad / (dz * dz);
    double b0, bN, aN = -f, c0 = -f, add0 = 0.0, addN = 0.0, dir0 = 0.0, dirN = 0.0;
    if (kind_bot == ADI_ZBC_NEUMANN0) { b0 = 1.0 + f; }
    else if (kind_bot == ADI_ZBC_DIRICHLET) { b0 = 1.0; c0 = 0.0; dir0 = 1.0; }
    else { const double beta = h_bot / k; b0 = 1.0 + f * (1.0 + beta * dz); add0 = tad * (beta / dz) * Tinf_bot; }
    if (kind_top == ADI_ZBC_NEUMANN0) { bN = 1.0 + f; }
    else if (kind_top == ADI_ZBC_DIRICHLET) { bN = 1.0; aN = 0.0; dirN = 1.0; }
    else { const double beta = h_top / k; bN = 1.0 + f * (1.0 + beta * dz); addN = tad * (beta / dz) * Tinf_top; }
    const double v[ADI_CYL_ZCLOSURE_LEN] = {f, b0, bN, aN, c0, add0, addN, T_bot, T_top, dir0, dirN};
    for (int i = 0; i < ADI_CYL_ZCLOSURE_LEN; ++i) z[i] = v[i];
}

// which FAST kernels an axis length allows.  phi: 16 rows per thread where the line allows it: the in-wave PCR over the
// separators costs the same per separator whatever the segment length (measured on 128 x 256 x 512: 87 us with 8 rows, 59 us
// with 16, 32-line tiles)
inline void cyl_pick_fast(int nr, int nphi, CylTables &T)
{
    auto pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
    T.phi_M = 0;
    if (nphi >= 128 && nphi % 16 == 0 && pow2(nphi / 16) && nphi / 16 <= 32) T.phi_M = 16;
    else if (nphi >= 64 && nphi % 8 == 0 && pow2(nphi / 8) && nphi / 8 <= 32) T.phi_M = 8;
    T.r_M = 0;
    if (nr >= 64 && nr % 8 == 0 && pow2(nr / 8) && nr / 8 <= 16) T.r_M = 8;
    else if (nr >= 64 && nr % 16 == 0 && pow2(nr / 16) && nr / 16 <= 16) T.r_M = 16;
    T.r_nseg = T.r_M ? nr / T.r_M : 0;
}

// r FAST form: the factorisation of every segment of the (line-independent) r operator -- condense<M>, reduced_row and
// pcr_solve of adi_core.hpp on the coefficients alone, with plain divisions and no fused multiply-add (the kernels only
// propagate right-hand sides through these numbers; their bits are part of the result)
inline void cyl_build_r_fast(CylTables &T)
{
    T.rfac.clear();
    const int M = T.r_M, nseg = T.r_nseg;
    if (!M) return;
    const int MI = M - 1;
    std::vector<double> &rfac = T.rfac;
    rfac.assign((size_t)nseg * RF_STRIDE, 0.0);
    std::vector<double> ra(nseg), rb(nseg), rc(nseg), aFv(nseg), cFv(nseg), aLv(nseg), cLv(nseg);
    for (int sgi = 0; sgi < nseg; ++sgi) {          // condense<M> of adi_core.hpp on the coefficients alone
        double *t = &rfac[(size_t)sgi * RF_STRIDE];
        const double *a = &T.ar[sgi * M], *b = &T.br[sgi * M], *c = &T.cr[sgi * M];
        double *wf = t, *wb = t + (RF_MAXM - 1), *ipv = t + 2 * (RF_MAXM - 1), *cv = t + 3 * (RF_MAXM - 1);
        double *sc = t + 4 * (RF_MAXM - 1);
        double e = 1.0;
        ipv[0] = 1.0 / b[0];
        for (int r = 1; r < MI; ++r) {
            wf[r] = a[r] * ipv[r - 1];
            ipv[r] = 1.0 / (b[r] - wf[r] * c[r - 1]);
            e = -wf[r] * e;
        }
        for (int r = 0; r < MI; ++r) cv[r] = c[r];
        double jp = 1.0 / b[MI - 1], f2 = 1.0;
        for (int r = MI - 2; r >= 0; --r) {
            wb[r] = c[r] * jp;
            jp = 1.0 / (b[r] - wb[r] * a[r + 1]);
            f2 = -wb[r] * f2;
        }
        sc[0] = ipv[MI - 1]; sc[1] = jp;
        aFv[sgi] = a[0] * jp; cFv[sgi] = c[MI - 1] * (f2 * jp);
        aLv[sgi] = a[0] * (e * ipv[MI - 1]); cLv[sgi] = c[MI - 1] * ipv[MI - 1];
        sc[2] = aFv[sgi]; sc[3] = cFv[sgi]; sc[4] = aLv[sgi]; sc[5] = cLv[sgi];
        sc[6] = a[0]; sc[7] = a[MI]; sc[8] = c[MI]; sc[9] = b[MI];
    }
    for (int sgi = 0; sgi < nseg; ++sgi) {          // reduced_row, matrix part
        const double *sc = &rfac[(size_t)sgi * RF_STRIDE + 4 * (RF_MAXM - 1)];
        const double aS = sc[7], cS = sc[8], bS = sc[9];
        const double aFn = sgi + 1 < nseg ? aFv[sgi + 1] : 0.0, cFn = sgi + 1 < nseg ? cFv[sgi + 1] : 0.0;
        ra[sgi] = -aS * aLv[sgi];
        rb[sgi] = bS - aS * cLv[sgi] - cS * aFn;
        rc[sgi] = -cS * cFn;
    }
    int lev = 0;
    for (int dl = 1; dl < nseg; dl <<= 1, ++lev) {  // pcr_solve, matrix part: the multipliers of every level
        std::vector<double> na(nseg), nb(nseg), nc(nseg);
        for (int i = 0; i < nseg; ++i) {
            const bool hl = i - dl >= 0, hh = i + dl < nseg;
            const double k1 = hl ? ra[i] / rb[i - dl] : 0.0, k2 = hh ? rc[i] / rb[i + dl] : 0.0;
            double *pk = &rfac[(size_t)i * RF_STRIDE + 4 * (RF_MAXM - 1) + 10];
            pk[lev] = k1; pk[6 + lev] = k2;
            nb[i] = rb[i] - (hl ? k1 * rc[i - dl] : 0.0) - (hh ? k2 * ra[i + dl] : 0.0);
            na[i] = hl ? -k1 * ra[i - dl] : 0.0;
            nc[i] = hh ? -k2 * rc[i + dl] : 0.0;
        }
        ra = na; rb = nb; rc = nc;
    }
    for (int i = 0; i < nseg; ++i) rfac[(size_t)i * RF_STRIDE + 4 * (RF_MAXM - 1) + 10 + 12] = 1.0 / rb[i];
}

// all of it, for a grid and physics already validated (adi_cyl.hip, cyl_plan_check)
inline void cyl_build_tables(int nr, int nphi, double dr, double dphi, double dz, double r_in, double rho, double cp,
                             double k, double dt, double robin_h, double robin_Tinf, int kind_bot, int kind_top, double h_bot,
                             double h_top, double Tinf_bot, double Tinf_top, double T_bot, double T_top, CylTables &T)
{
    const double alpha = k / (rho * cp);  // Material.alpha, :48-50
    const double theta = 1.0;             // BE branch calls the builders with theta = 1.0 (:341, :348)
    const double tad = theta * alpha * dt;
    cyl_build_r(nr, dr, r_in, tad, k, robin_h, robin_Tinf, T);
    cyl_build_phi(nr, nphi, dr, dphi, r_in, tad, T);
    cyl_build_z(dz, tad, k, kind_bot, kind_top, h_bot, h_top, Tinf_bot, Tinf_top, T_bot, T_top, T.z);
    cyl_pick_fast(nr, nphi, T);
    cyl_build_r_fast(T);
}

}  // namespace adi
