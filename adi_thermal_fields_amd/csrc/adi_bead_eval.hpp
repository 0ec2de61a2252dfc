// adi_bead_eval.hpp -- THE evaluator of the bead a scan path lays during a step (include/adi_hip.h, "Bead deposition along a
// scan path"), written once for the host and the device: deposition.PathDeposit.reference operation for operation, fp64, no
// contraction.  The path is the segment table of adi_scan_eval.hpp, whose pieces, window and axes it reuses; every segment
// index used as an address lies in [0, K).
// Host-only code may include this header without the HIP runtime (the stand-alone programs of a sanitizer build do).
#pragma once
#include "adi_scan_eval.hpp"

namespace adi {

// the piece (ta, tb) of segment k inside [t, t1] if the segment DEPOSITS: power > 0 (scan_piece) and speed > 0 -- jumps, idle
// dwells and dwells with power lay nothing
ADI_SCAN_HD bool bead_piece(const double *tab, int K, double t_end, int k, double t, double t1, double &ta, double &tb)
{
#pragma clang fp contract(off)
    double w;
    if (!(tab[(long)k * kScanCols + 6] > 0.0)) return false;
    return scan_piece(tab, K, t_end, k, t, t1, ta, tb, w);
}

// the point x lies in the bead of the piece (ta, tb) of the segment s: within width/2 of the path travelled (round ends), at
// most `cap` below the path's depth coordinate, never above it
ADI_SCAN_HD bool bead_inside(const adi_bead_shape &b, const double *s, double ta, double tb, double x0, double x1, double x2)
{
#pragma clang fp contract(off)
    const int da = b.depth_axis, au = scan_axis_u(da), av = scan_axis_v(da);
    const double o0 = x0 - s[1], o1 = x1 - s[2], o2 = x2 - s[3];
    const double ou = scan_pick3(o0, o1, o2, au), ov = scan_pick3(o0, o1, o2, av), z = scan_pick3(o0, o1, o2, da);
    const double d0 = s[4], d1 = s[5], vel = s[6];
    const double xi0 = ou * d0 + ov * d1;
    const double y = ov * d0 - ou * d1;
    const double sa = vel * ta;
    const double sb = vel * tb;
    const double lo = xi0 > sa ? xi0 : sa;
    const double xc = lo < sb ? lo : sb;
    const double e = xi0 - xc;
    const double r2 = e * e + y * y;
    const double half = 0.5 * b.width;
    const double h2 = half * half;
    const double cap = b.profile == 0 ? b.height : b.height * (1.0 - r2 / h2);
    return r2 <= h2 && z <= 0.0 && -z <= cap;
}

// ... of any piece of the step [t, t1] in the segments [k0, k1) (0 <= k0, k1 <= K: the range of scan_window)
ADI_SCAN_HD bool bead_inside_step(const adi_bead_shape &b, const double *tab, int K, double t_end, int k0, int k1, double t,
                                  double t1, double x0, double x1, double x2)
{
#pragma clang fp contract(off)
    for (int k = k0; k < k1 && k < K; ++k) {
        double ta, tb;
        if (bead_piece(tab, K, t_end, k, t, t1, ta, tb) && bead_inside(b, tab + (long)k * kScanCols, ta, tb, x0, x1, x2))
            return true;
    }
    return false;
}

// [lo, hi) of the cells of an axis of n cells whose centres (i + 1/2) dx can lie in [mn, mx]: the floor / ceil rule of
// ScanPath._index_box, clamped as doubles (no int overflow)
ADI_SCAN_HD void bead_axis_range(double mn, double mx, double dx, int n, int &il, int &ih)
{
#pragma clang fp contract(off)
    double lo = floor(mn / dx - 0.5), hi = ceil(mx / dx - 0.5) + 1.0;
    const double nn = (double)n;
    lo = lo > 0.0 ? lo : 0.0; lo = lo < nn ? lo : nn;
    hi = hi > 0.0 ? hi : 0.0; hi = hi < nn ? hi : nn;
    hi = hi > lo ? hi : lo;
    il = (int)lo; ih = (int)hi;
}

// index box of the piece (ta, tb) of segment s on an n[0] x n[1] x n[2] grid, joined to B: width/2 (1 + 1e-9) in the plane
// around both ends of the piece, [p - height (1 + 1e-9), p] in depth
ADI_SCAN_HD void bead_box_join(const adi_bead_shape &b, const double *s, double ta, double tb, const int (&n)[3], double dx,
                               ScanBox &B)
{
#pragma clang fp contract(off)
    const int da = b.depth_axis, au = scan_axis_u(da), av = scan_axis_v(da);
    for (int ax = 0; ax < 3; ++ax) {
        const double p = scan_pick3(s[1], s[2], s[3], ax);
        double mn, mx;
        if (ax == da) {
            mn = p - b.height * (1.0 + 1e-9); mx = p;
        } else {
            const double dir = ax == au ? s[4] : (ax == av ? s[5] : 0.0);
            const double m = (0.5 * b.width) * (1.0 + 1e-9);
            const double ca = p + dir * (s[6] * ta), cb = p + dir * (s[6] * tb);
            mn = (ca < cb ? ca : cb) - m; mx = (ca > cb ? ca : cb) + m;
        }
        int il, ih;
        bead_axis_range(mn, mx, dx, n[ax], il, ih);
        if (il < B.lo[ax]) B.lo[ax] = il;
        if (ih > B.hi[ax]) B.hi[ax] = ih;
    }
}

// the union of the index boxes of the depositing pieces of the step [t, t1] in the segments [k0, k1); -> whether any segment
// deposits in the step.  No such piece, or none that meets the grid, leaves B = [0, 0) on every axis.
ADI_SCAN_HD bool bead_window_box(const adi_bead_shape &b, const double *tab, int K, double t_end, int k0, int k1, double t,
                                 double t1, const int (&n)[3], double dx, ScanBox &B)
{
    bool deposits = false;
    scan_box_clear(B);
    for (int k = k0; k < k1 && k < K; ++k) {
        double ta, tb;
        if (bead_piece(tab, K, t_end, k, t, t1, ta, tb)) {
            deposits = true;
            bead_box_join(b, tab + (long)k * kScanCols, ta, tb, n, dx, B);
        }
    }
    if (scan_box_empty(B))
        for (int a = 0; a < 3; ++a) { B.lo[a] = 0; B.hi[a] = 0; }
    return deposits;
}

// adi_bead_deposit_host's loop over a dense C-order (nx, ny, nz) host array: born = inside, within (NULL: every cell), not
// active (NULL: no cell is)
inline void bead_deposit_host(const adi_bead_shape &b, const double *tab, int K, double t_end, const uint8_t *active,
                              const uint8_t *within, int nx, int ny, int nz, double dx, double t, double dt, uint8_t *born)
{
#pragma clang fp contract(off)
    const double t1 = t + dt;
    int k0, k1;
    scan_window(tab, K, t, t1, k0, k1);
    const int n[3] = {nx, ny, nz};
    ScanBox B;
    bead_window_box(b, tab, K, t_end, k0, k1, t, t1, n, dx, B);
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < ny; ++j)
            for (int k = 0; k < nz; ++k) {
                const long p = ((long)i * ny + j) * nz + k;
                const bool in = i >= B.lo[0] && i < B.hi[0] && j >= B.lo[1] && j < B.hi[1] && k >= B.lo[2] && k < B.hi[2];
                born[p] = (in && (active == nullptr || !active[p]) && (within == nullptr || within[p]) &&
                           bead_inside_step(b, tab, K, t_end, k0, k1, t, t1, (i + 0.5) * dx, (j + 0.5) * dx, (k + 0.5) * dx))
                              ? 1 : 0;
            }
}

}  // namespace adi
