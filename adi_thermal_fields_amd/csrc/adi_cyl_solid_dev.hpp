// adi_cyl_solid_dev.hpp -- the conditions at the freezing front of the cylindrical step (include/adi_hip.h, "Solidification
// record of the cylindrical step"): the per-cell function, written once for the kernel of adi_cyl_solid.hip and for its host
// twin, the tile geometry, the argument checks and the host loops.
// Conventions of the cylindrical backend (adi_cyl_extras_dev.hpp): fields in the (nr, nphi, nz) layout with z contiguous and
// plane stride sx, `active` an optional byte per cell (NULL: every cell).  NaN in the state means "never froze", whether or not
// the cell was ever active, so there is nothing to seed and a birth needs no call.  A tile is ADI_CYL_SOLID_TILE consecutive
// cells p = j*nz + k of one radius' plane; tile q of radius i has the word i*ntile + q of the hot words.
#pragma once
#include "adi_cyl_extras_dev.hpp"

namespace adi {

constexpr int kCylSolidTile = ADI_CYL_SOLID_TILE;
static_assert(kCylSolidTile == 512, "a workgroup of 256 threads owns two cells per thread");

// what a record takes by value: the level, the clock-independent geometry and the three steps (h, 2h) of the axes whose step
// does not depend on the cell
struct CylSolidScal {
    double T_f, R_in, dr, dphi;
    double h_r, two_h_r, h_z, two_h_z;
};

inline CylSolidScal make_cyl_solid_scal(double T_f, double R_in, double dr, double dphi, double dz)
{
#pragma clang fp contract(off)
    CylSolidScal w;
    w.T_f = T_f; w.R_in = R_in; w.dr = dr; w.dphi = dphi;
    w.h_r = dr; w.two_h_r = 2.0 * dr;
    w.h_z = dz; w.two_h_z = 2.0 * dz;
    return w;
}

__host__ __device__ __forceinline__ long cyl_solid_tiles(const CylBox &g)
{
    return ((long)g.nphi * g.nz + (kCylSolidTile - 1)) / kCylSolidTile;
}

__host__ __device__ __forceinline__ bool cyl_solid_present(const uint8_t *act, long p) { return act == nullptr || act[p] != 0; }

// dF/dx at cell p (centre value f0) from the neighbours at pm (present: lo) and pp (present: hi): central where both are
// present, one-sided where one is, 0 where none is
__host__ __device__ __forceinline__ double cyl_solid_grad(const double *F, long pm, long pp, double f0, bool lo, bool hi, double h,
                                                          double two_h)
{
#pragma clang fp contract(off)
    if (lo && hi) {
        const double d = F[pp] - F[pm];
        return d / two_h;
    }
    if (hi) {
        const double d = F[pp] - f0;
        return d / h;
    }
    if (lo) {
        const double d = f0 - F[pm];
        return d / h;
    }
    return 0.0;
}

// The record of one cell (i, j, k) that freezes in the step a -> b (a > T_f >= b, the cell active) at t_n: the crossing time,
// the cooling rate and the squared gradient at the crossing time, every operation in the order of
// CylSolidificationRecord.record_reference.  Reads up to six neighbours of A, of B and of `active`: i -+ 1 and k -+ 1 inside
// the box, (j -+ 1) mod nphi (none with nphi == 1); a neighbour counts only where `active` holds it.
__host__ __device__ __forceinline__ void cyl_solid_cell(const CylSolidScal &w, const CylBox &g, double tn, double dt,
                                                        const double *A, const double *B, const uint8_t *act, int i, int j, int k,
                                                        double a, double b, double &tc, double &cr, double &g2)
{
#pragma clang fp contract(off)
    const long p = (long)i * g.sx + (long)j * g.nz + k;
    const double den = a - b;
    const double num = a - w.T_f;
    const double fr = num / den;
    const double off = dt * fr;
    tc = tn + off;
    cr = den / dt;
    const double ih = (double)i + 0.5;
    const double ro = ih * w.dr;
    const double r_i = w.R_in + ro;
    const double h_phi = r_i * w.dphi;
    const double two_h_phi = 2.0 * h_phi;
    const int jm = j == 0 ? g.nphi - 1 : j - 1, jp = j == g.nphi - 1 ? 0 : j + 1;
    const long pm[3] = {p - g.sx, p + (long)(jm - j) * g.nz, p - 1};
    const long pp[3] = {p + g.sx, p + (long)(jp - j) * g.nz, p + 1};
    const bool in_lo[3] = {i > 0, g.nphi > 1, k > 0};
    const bool in_hi[3] = {i < g.nr - 1, g.nphi > 1, k < g.nz - 1};
    const double h[3] = {w.h_r, h_phi, w.h_z};
    const double two_h[3] = {w.two_h_r, two_h_phi, w.two_h_z};
    double gr[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const bool lo = in_lo[ax] && cyl_solid_present(act, pm[ax]);
        const bool hi = in_hi[ax] && cyl_solid_present(act, pp[ax]);
        const double gA = cyl_solid_grad(A, pm[ax], pp[ax], a, lo, hi, h[ax], two_h[ax]);
        const double gB = cyl_solid_grad(B, pm[ax], pp[ax], b, lo, hi, h[ax], two_h[ax]);
        const double dg = gB - gA;
        const double sg = fr * dg;
        gr[ax] = gA + sg;
    }
    const double rr = gr[0] * gr[0];
    const double pq = gr[1] * gr[1];
    const double zz = gr[2] * gr[2];
    const double s2 = rr + pq;
    g2 = s2 + zz;
}

// what adi_cyl_solid_record and its host twin refuse
inline int check_cyl_solid_record(const char *who, double T_freeze, double R_in, double dr, double dphi, double dz,
                                  const void *block, const double *T_in, const double *T_out, const double *t_solid,
                                  const double *rate, const double *g2, const int32_t *log, int nr, int nphi, int nz,
                                  long plane_stride, CylBox *g)
{
    ADI_REQUIRE(block && T_in && T_out && t_solid && rate && g2 && log, "%s: null argument", who);
    ADI_REQUIRE(T_in != T_out, "%s: T_out aliases T_in", who);
    ADI_REQUIRE(t_solid != T_in && t_solid != T_out && rate != T_in && rate != T_out && g2 != T_in && g2 != T_out,
                "%s: a state array aliases T", who);
    ADI_REQUIRE(t_solid != rate && t_solid != g2 && rate != g2, "%s: the state arrays alias", who);
    ADI_REQUIRE(isfinite(T_freeze), "%s: T_freeze not finite", who);
    ADI_REQUIRE(isfinite(dr) && dr > 0.0 && isfinite(dphi) && dphi > 0.0 && isfinite(dz) && dz > 0.0,
                "%s: dr, dphi and dz must be positive", who);
    ADI_REQUIRE(isfinite(R_in) && R_in >= 0.0, "%s: R_in must be >= 0", who);
    ADI_REQUIRE(((uintptr_t)log & 7u) == 0 && ((uintptr_t)block & 7u) == 0, "%s: block or log not 8-byte aligned", who);
    return make_cyl_box(who, nr, nphi, nz, plane_stride, g);
}

// what adi_cyl_solid_hot_seed and its host twin refuse
inline int check_cyl_solid_hot_seed(const char *who, double T_freeze, const double *T, const int32_t *hot, int nr, int nphi,
                                    int nz, long plane_stride, CylBox *g)
{
    ADI_REQUIRE(T && hot, "%s: null argument", who);
    ADI_REQUIRE((const void *)T != (const void *)hot, "%s: hot aliases T", who);
    ADI_REQUIRE(isfinite(T_freeze), "%s: T_freeze not finite", who);
    return make_cyl_box(who, nr, nphi, nz, plane_stride, g);
}

// the word of every tile from T: 1 where an active cell of the tile has T > T_f, else 0
inline void cyl_solid_hot_seed_host(double T_f, const CylBox &g, const double *T, const uint8_t *act, int32_t *hot)
{
    const long npl = (long)g.nphi * g.nz, ntile = cyl_solid_tiles(g);
    for (int i = 0; i < g.nr; ++i)
        for (long q = 0; q < ntile; ++q) {
            const long p1 = (q + 1) * kCylSolidTile < npl ? (q + 1) * kCylSolidTile : npl;
            int32_t above = 0;
            for (long pl = q * kCylSolidTile; pl < p1; ++pl) {
                const long p = (long)i * g.sx + pl;
                if (cyl_solid_present(act, p) && T[p] > T_f) above = 1;
            }
            hot[(long)i * ntile + q] = above;
        }
}

// the record over host arrays into the block's log row, tile by tile as the kernel goes (the row accumulates as the kernel's
// atomics do); no tick.  hot (nullable): a tile whose word is clear reads `active` and B only.
inline void cyl_solid_record_host(const CylSolidScal &w, const CylBox &g, const HistBlock &blk, const double *A, const double *B,
                                  double *TS, double *CR, double *G2, int32_t *log, const uint8_t *act, int32_t *hot)
{
    const double tn = cyl_history_tn(blk);
    int32_t *r = log + (blk.slot < blk.capacity ? blk.slot : blk.capacity) * ADI_CYL_HISTORY_LOG_INTS;
    long long sum_i;
    memcpy(&sum_i, r + 8, sizeof(sum_i));
    const long npl = (long)g.nphi * g.nz, ntile = cyl_solid_tiles(g);
    for (int i = 0; i < g.nr; ++i)
        for (long q = 0; q < ntile; ++q) {
            const long p0 = q * kCylSolidTile;
            const long p1 = p0 + kCylSolidTile < npl ? p0 + kCylSolidTile : npl;
            if (hot != nullptr) {
                int32_t *word = hot + (long)i * ntile + q;
                const int32_t was = *word;
                int32_t now = 0;
                for (long pl = p0; pl < p1; ++pl) {
                    const long p = (long)i * g.sx + pl;
                    if (cyl_solid_present(act, p) && B[p] > w.T_f) now = 1;
                }
                if (now != was) *word = now;
                if (was == 0) continue;
            }
            for (long pl = p0; pl < p1; ++pl) {
                const long p = (long)i * g.sx + pl;
                if (!cyl_solid_present(act, p)) continue;
                const double b = B[p];
                if (!(b <= w.T_f)) continue;
                const double a = A[p];
                if (!(a > w.T_f)) continue;
                const int j = (int)(pl / g.nz), k = (int)(pl - (long)j * g.nz);
                double tc, cr, g2;
                cyl_solid_cell(w, g, tn, blk.dt, A, B, act, i, j, k, a, b, tc, cr, g2);
                TS[p] = tc; CR[p] = cr; G2[p] = g2;
                r[0] += 1;
                sum_i += i;
                r[1] = i < r[1] ? i : r[1]; r[2] = j < r[2] ? j : r[2]; r[3] = k < r[3] ? k : r[3];
                r[4] = i > r[4] ? i : r[4]; r[5] = j > r[5] ? j : r[5]; r[6] = k > r[6] ? k : r[6];
            }
        }
    memcpy(r + 8, &sum_i, sizeof(sum_i));
}

}  // namespace adi
