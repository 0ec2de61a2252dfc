// adi_scan_eval.hpp -- THE evaluator of a scan path's step-averaged heat input (include/adi_hip.h, "Scan path"), written
// once for the host and the device: heat_source.ScanPath._piece / _qbar / q_step / _index_box operation for operation, fp64,
// no contraction.  A path is a table of K segments of 8 doubles (t_begin, start point p[3], in-plane unit direction d[2],
// speed, power) and the end time of the last one; every segment index used as an address lies in [0, K).
// Host-only code may include this header without the HIP runtime (the stand-alone programs of a sanitizer build do).
#pragma once
#include <math.h>
#include <stdint.h>

#include "adi_goldak_dev.hpp"

#if defined(__HIPCC__)
#define ADI_SCAN_HD __host__ __device__ inline
#else
#define ADI_SCAN_HD inline
#endif

namespace adi {

constexpr double kScanDeltaMin = 1e-3;     // ScanPath.DELTA_MIN: travel of a piece over min(c_f, c_r) below which Simpson's rule
constexpr int kScanCols = ADI_SCAN_TABLE_COLS;

// in-plane axes (u, v) of a depth axis: the other two in increasing order
ADI_SCAN_HD int scan_axis_u(int da) { return da == 0 ? 1 : 0; }
ADI_SCAN_HD int scan_axis_v(int da) { return da == 2 ? 1 : 2; }

ADI_SCAN_HD double scan_pick3(double v0, double v1, double v2, int a) { return a == 0 ? v0 : (a == 1 ? v1 : v2); }

// end of segment k: the begin of the next one, t_end for the last
ADI_SCAN_HD double scan_t_next(const double *tab, int K, double t_end, int k)
{
    return k + 1 < K ? tab[(long)(k + 1) * kScanCols] : t_end;
}

// ScanPath._piece: the piece of segment k inside [t, t1] as times since the segment's start (ta, tb) and its length w;
// false if it deposits nothing
ADI_SCAN_HD bool scan_piece(const double *tab, int K, double t_end, int k, double t, double t1, double &ta, double &tb,
                            double &w)
{
#pragma clang fp contract(off)
    const double *s = tab + (long)k * kScanCols;
    if (!(s[7] > 0.0)) return false;
    const double tn = scan_t_next(tab, K, t_end, k);
    const double tau0 = t > s[0] ? t : s[0];
    const double tau1 = t1 < tn ? t1 : tn;
    if (!(tau1 > tau0)) return false;
    ta = tau0 - s[0]; tb = tau1 - s[0]; w = tau1 - tau0;
    return true;
}

// ScanPath._qi: the instantaneous double ellipsoid at along-leg offset xi, Et the exponent of the other two axes
ADI_SCAN_HD double scan_qi(const adi_scan_shape &h, double P, double xi, double Et)
{
#pragma clang fp contract(off)
    const bool front = xi >= 0.0;
    const double f = front ? h.f_f : 2.0 - h.f_f;
    const double cl = front ? h.c_f : h.c_r;
    const double amp = goldak_amp(f, h.eta, P, h.a, h.b, cl);
    const double E = goldak_eterm(xi, cl) + Et;
    return amp * exp(-E);
}

// ScanPath._qbar for a piece (ta, tb, w) of the segment s: the time average over a step of length dt at the point x
ADI_SCAN_HD double scan_qbar(const adi_scan_shape &h, const double *s, double ta, double tb, double w, double dt, double x0,
                             double x1, double x2)
{
#pragma clang fp contract(off)
    const int da = h.depth_axis, au = scan_axis_u(da), av = scan_axis_v(da);
    const double o0 = x0 - s[1], o1 = x1 - s[2], o2 = x2 - s[3];
    const double ou = scan_pick3(o0, o1, o2, au), ov = scan_pick3(o0, o1, o2, av), z = scan_pick3(o0, o1, o2, da);
    const double d0 = s[4], d1 = s[5], vel = s[6], P = s[7];
    const double xi0 = ou * d0 + ov * d1;
    const double y = ov * d0 - ou * d1;
    const double xia = xi0 - vel * ta;
    const double xib = xi0 - vel * tb;
    const double Et = goldak_eterm(y, h.a) + goldak_eterm(z, h.b);
    const double R = sqrt(ADI_SOURCE_E_CUT / 3.0);
    if (!(Et <= ADI_SOURCE_E_CUT && xib <= R * h.c_f && xia >= -(R * h.c_r))) return 0.0;
    const double travel = vel * w;
    const double delta = travel / (h.c_f < h.c_r ? h.c_f : h.c_r);
    if (delta >= kScanDeltaMin) {
        const double s3 = sqrt(3.0);
        const double pa = xia > 0.0 ? xia : 0.0, pb = xib > 0.0 ? xib : 0.0;
        const double na = xia < 0.0 ? xia : 0.0, nb = xib < 0.0 ? xib : 0.0;
        const double Ff = erf(s3 * pa / h.c_f) - erf(s3 * pb / h.c_f);
        const double Fr = erf(s3 * na / h.c_r) - erf(s3 * nb / h.c_r);
        const double brace = h.f_f * Ff + (2.0 - h.f_f) * Fr;
        const double amp = (3.0 * h.eta * P) / (M_PI * h.a * h.b * vel * dt);
        return (amp * exp(-Et)) * brace;
    }
    if (travel == 0.0) return (w / dt) * scan_qi(h, P, xia, Et);
    const double xim = xi0 - vel * (0.5 * (ta + tb));
    const double qs = (scan_qi(h, P, xia, Et) + 4.0 * scan_qi(h, P, xim, Et)) + scan_qi(h, P, xib, Et);
    return (w / dt) * (qs / 6.0);
}

// ScanPath.q_step at the point x for the step [t, t1] of length dt: the sum over the segments [k0, k1) in ascending order
// (0 <= k0, k1 <= K: the caller's range holds every segment the step overlaps; the others contribute nothing)
ADI_SCAN_HD double scan_q_step(const adi_scan_shape &h, const double *tab, int K, double t_end, int k0, int k1, double t,
                               double t1, double dt, double x0, double x1, double x2)
{
#pragma clang fp contract(off)
    double q = 0.0;
    for (int k = k0; k < k1 && k < K; ++k) {
        double ta, tb, w;
        if (scan_piece(tab, K, t_end, k, t, t1, ta, tb, w))
            q += scan_qbar(h, tab + (long)k * kScanCols, ta, tb, w, dt, x0, x1, x2);
    }
    return q;
}

// The segments a step [t, t1] can overlap: [k0, k1) with k0 the segment that holds t (0 before the path, K - 1 from t_end
// on) and k1 the first one beginning at or after t1.  A binary search of at most 32 halvings, then k1 by another; every
// index read lies in [0, K).
ADI_SCAN_HD void scan_window(const double *tab, int K, double t, double t1, int &k0, int &k1)
{
    int lo = 0, hi = K;                                    // first k with t_begin[k] > t
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = lo + (hi - lo) / 2;
        if (tab[(long)mid * kScanCols] > t) hi = mid; else lo = mid + 1;
    }
    k0 = lo > 0 ? lo - 1 : 0;
    int a = k0, b = K;                                     // first k >= k0 with t_begin[k] >= t1
    for (int it = 0; it < 32 && a < b; ++it) {
        const int mid = a + (b - a) / 2;
        if (tab[(long)mid * kScanCols] >= t1) b = mid; else a = mid + 1;
    }
    k1 = a > k0 ? a : k0;
    if (k1 > K) k1 = K;
}

// index box [lo, hi) per axis: empty to start a union with
struct ScanBox {
    int lo[3], hi[3];
};
ADI_SCAN_HD void scan_box_clear(ScanBox &B)
{
    for (int a = 0; a < 3; ++a) { B.lo[a] = 0x7fffffff; B.hi[a] = 0; }
}
ADI_SCAN_HD bool scan_box_empty(const ScanBox &B)
{
    return B.lo[0] >= B.hi[0] || B.lo[1] >= B.hi[1] || B.lo[2] >= B.hi[2];
}

// ScanPath._index_box of the piece [ta, tb] (times since the start) of segment s on an n[0] x n[1] x n[2] grid, joined to B:
// the cells whose centres can lie in the support, R hypot(max(c_f, c_r), a) from the centre in the plane and R b in depth
ADI_SCAN_HD void scan_box_join(const adi_scan_shape &h, const double *s, double ta, double tb, const int (&n)[3], double dx,
                               ScanBox &B)
{
#pragma clang fp contract(off)
    const double R = sqrt(ADI_SOURCE_E_CUT / 3.0);
    const int da = h.depth_axis, au = scan_axis_u(da), av = scan_axis_v(da);
    const double cm = h.c_f > h.c_r ? h.c_f : h.c_r;
    for (int ax = 0; ax < 3; ++ax) {
        const double dir = ax == da ? 0.0 : (ax == au ? s[4] : (ax == av ? s[5] : 0.0));
        const double m = (ax == da ? R * h.b : R * hypot(cm, h.a)) * (1.0 + 1e-9);
        const double p = scan_pick3(s[1], s[2], s[3], ax);
        const double ca = p + dir * (s[6] * ta), cb = p + dir * (s[6] * tb);
        const double mn = ca < cb ? ca : cb, mx = ca > cb ? ca : cb;
        double lo = floor((mn - m) / dx - 0.5), hi = ceil((mx + m) / dx - 0.5) + 1.0;
        const double nn = (double)n[ax];
        lo = lo > 0.0 ? lo : 0.0; lo = lo < nn ? lo : nn;             // (clamped as doubles: no int overflow)
        hi = hi > 0.0 ? hi : 0.0; hi = hi < nn ? hi : nn;
        hi = hi > lo ? hi : lo;
        const int il = (int)lo, ih = (int)hi;
        if (il < B.lo[ax]) B.lo[ax] = il;
        if (ih > B.hi[ax]) B.hi[ax] = ih;
    }
}

// the union of the index boxes of the pieces of the step [t, t1] in the segments [k0, k1); an empty window leaves B empty
ADI_SCAN_HD void scan_window_box(const adi_scan_shape &h, const double *tab, int K, double t_end, int k0, int k1, double t,
                                 double t1, const int (&n)[3], double dx, ScanBox &B)
{
    scan_box_clear(B);
    for (int k = k0; k < k1 && k < K; ++k) {
        double ta, tb, w;
        if (scan_piece(tab, K, t_end, k, t, t1, ta, tb, w)) scan_box_join(h, tab + (long)k * kScanCols, ta, tb, n, dx, B);
    }
    if (scan_box_empty(B))
        for (int a = 0; a < 3; ++a) { B.lo[a] = 0; B.hi[a] = 0; }
}

// adi_scan_sample_host's loop: q_step at the cell centres of a dense C-order (nx, ny, nz) host array, 0 off the mask
// (mask NULL: every cell is in)
inline void scan_sample_host(const adi_scan_shape &h, const double *tab, int K, double t_end, const uint8_t *mask, int nx,
                             int ny, int nz, double dx, double t, double dt, double *out)
{
#pragma clang fp contract(off)
    const double t1 = t + dt;
    int k0, k1;
    scan_window(tab, K, t, t1, k0, k1);
    const int n[3] = {nx, ny, nz};
    ScanBox B;
    scan_window_box(h, tab, K, t_end, k0, k1, t, t1, n, dx, B);
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < ny; ++j)
            for (int k = 0; k < nz; ++k) {
                const long p = ((long)i * ny + j) * nz + k;
                const bool in = i >= B.lo[0] && i < B.hi[0] && j >= B.lo[1] && j < B.hi[1] && k >= B.lo[2] && k < B.hi[2];
                out[p] = (in && (mask == nullptr || mask[p]))
                             ? scan_q_step(h, tab, K, t_end, k0, k1, t, t1, dt, (i + 0.5) * dx, (j + 0.5) * dx, (k + 0.5) * dx)
                             : 0.0;
            }
}

// The window of the step [t, t + dt] as a launch carries it: the segment range and the index box, found on the host
struct ScanWindow {
    int k0, k1;
    ScanBox B;
};
inline ScanWindow scan_window_of(const adi_scan_shape &h, const double *tab, int K, double t_end, int nx, int ny, int nz,
                                 double dx, double t, double dt)
{
#pragma clang fp contract(off)
    ScanWindow W;
    const double t1 = t + dt;
    scan_window(tab, K, t, t1, W.k0, W.k1);
    const int n[3] = {nx, ny, nz};
    scan_window_box(h, tab, K, t_end, W.k0, W.k1, t, t1, n, dx, W.B);
    return W;
}

// One cell of the path added to R0 on a grid of several materials: r + (dt * q_step) / C[id], r itself where q_step is 0 (the
// caller then writes nothing).  C: the kMapMaxMat = 8 entries, the id masked as everywhere.
ADI_SCAN_HD bool scan_add_r0_cell(const adi_scan_shape &h, const double *tab, int K, double t_end, int k0, int k1, double t,
                                  double dt, double dx, int i, int j, int k, const double *C, unsigned id, double &r)
{
#pragma clang fp contract(off)
    const double q = scan_q_step(h, tab, K, t_end, k0, k1, t, t + dt, dt, (i + 0.5) * dx, (j + 0.5) * dx, (k + 0.5) * dx);
    if (q == 0.0) return false;
    r = r + (dt * q) / C[id & 7u];
    return true;
}

// adi_matmap_scan_add_r0_host's loop over the window's box of dense C-order (nx, ny, nz) host arrays (mask NULL: every cell)
inline void scan_add_r0_host(const adi_scan_shape &h, const double *tab, int K, double t_end, const ScanWindow &W, double *R0,
                             const uint8_t *mask, const uint8_t *ids, int ny, int nz, double dx, double t, double dt,
                             const double *C)
{
    for (int i = W.B.lo[0]; i < W.B.hi[0]; ++i)
        for (int j = W.B.lo[1]; j < W.B.hi[1]; ++j)
            for (int k = W.B.lo[2]; k < W.B.hi[2]; ++k) {
                const long p = ((long)i * ny + j) * nz + k;
                if (mask != nullptr && !mask[p]) continue;
                double r = R0[p];
                if (scan_add_r0_cell(h, tab, K, t_end, W.k0, W.k1, t, dt, dx, i, j, k, C, ids[p], r)) R0[p] = r;
            }
}

}  // namespace adi
