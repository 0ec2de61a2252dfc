// adi_cyl_extras_dev.hpp -- latent heat and thermal history of the cylindrical step (include/adi_hip.h, "Latent heat and
// thermal history of the cylindrical step"): the two per-cell functions, written once for the kernels of adi_cyl_extras.hip
// and for their host twins, the box of a launch and the argument checks both sides share.
// Conventions of the cylindrical backend: fields in the (nr, nphi, nz) layout with z contiguous and plane stride sx, `active`
// an optional byte per cell (NULL: every cell), no flags, no bricks, no state to synchronise.  A NaN in the state (f, T_peak)
// marks a cell that has never been seen active; the first pass that sees it active seeds it from the step's input.
#pragma once
#include <math.h>
#include <string.h>

#include "adi_history_dev.hpp"
#include "adi_phase_dev.hpp"

namespace adi {

constexpr int kCylHistEmptyLo = 0x7fffffff;

__host__ __device__ __forceinline__ double cyl_nan() { return __builtin_bit_cast(double, 0x7ff8000000000000LL); }
__host__ __device__ __forceinline__ bool cyl_same_bits(double a, double b)
{
    return __builtin_bit_cast(long long, a) == __builtin_bit_cast(long long, b);
}
__host__ __device__ __forceinline__ double cyl_clamp01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }

// which of a cell's values a pass has to store
constexpr unsigned kCylStoreT = 1u, kCylStoreF = 2u;
constexpr unsigned kCylStorePeak = 1u, kCylStoreHi = 2u, kCylStoreLo = 4u;

// The latent-heat correction of one active cell off the skipped planes: ts the step's result, fs the liquid fraction the
// step started with (NaN: a newborn; then, with `seed`, f0 = f_eq(tin) is taken and stored even if the cell is then at
// rest).  The operations of PhaseChange.f_eq and PhaseChange.correct, in their order.  -> the values to store as a set of
// kCylStore* bits (a value is stored only where its bits change), tn and fn the values.
__host__ __device__ __forceinline__ unsigned cyl_phase_cell(const PhaseLaw &w, double ts, double fs, bool seed, double tin,
                                                            double &tn, double &fn)
{
#pragma clang fp contract(off)
    unsigned st = 0u;
    if (seed && fs != fs) {
        const double e = tin - w.Ts;
        fs = cyl_clamp01(e / w.dT);
        st = kCylStoreF;
    }
    tn = ts;
    fn = fs;
    const bool rest = (fs == 0.0 && ts <= w.Ts) || (fs == 1.0 && ts >= w.Tl);
    if (rest) return st;
    const double h1 = w.cp * ts;
    const double h2 = w.L * fs;
    const double H = h1 + h2;
    if (H <= w.Hs) {
        tn = H / w.cp;
        fn = 0.0;
    } else if (H >= w.Hl) {
        const double d = H - w.L;
        tn = d / w.cp;
        fn = 1.0;
    } else {
        const double d = H - w.Hs;
        const double q = d / w.cm;
        tn = w.Ts + q;
        const double e = tn - w.Ts;
        fn = cyl_clamp01(e / w.dT);
    }
    if (!cyl_same_bits(tn, ts)) st |= kCylStoreT;
    if (!cyl_same_bits(fn, fs)) st |= kCylStoreF;
    return st;
}

// does the record of an active cell with peak pk need the step's input?  True for a newborn (NaN) and wherever a crossing is
// possible under the precondition A <= T_peak.
__host__ __device__ __forceinline__ bool cyl_history_needs_a(const adi_history_levels &w, double pk) { return !(pk <= w.T_lo); }

// The record of one active cell for the step a -> b at t_n: a newborn (pk NaN) is seeded from a -- its three values are always
// stored, NaN times over whatever the arrays held --, then rules 1 - 3 of the thermal history in their order: a rule that
// fires stores its values.  a is only read where cyl_history_needs_a(pk).  -> kCylStore* bits; peak, thi, tlo the values.
__host__ __device__ __forceinline__ unsigned cyl_history_cell(const adi_history_levels &w, double tn, double dt, double a,
                                                              double b, double pk, double &peak, double &thi, double &tlo)
{
#pragma clang fp contract(off)
    unsigned st = 0u;
    const bool have_a = cyl_history_needs_a(w, pk);
    if (pk != pk) {
        pk = a;
        thi = cyl_nan();
        tlo = cyl_nan();
        st = kCylStorePeak | kCylStoreHi | kCylStoreLo;
    }
    peak = pk;
    if (b > pk) {
        peak = b;
        st |= kCylStorePeak;
    }
    if (have_a) {
        const double den = a - b;
        if (a > w.T_hi && b <= w.T_hi) {
            const double num = a - w.T_hi;
            const double fr = num / den;
            const double off = dt * fr;
            thi = tn + off;
            tlo = cyl_nan();
            st |= kCylStoreHi | kCylStoreLo;
        }
        if (a > w.T_lo && b <= w.T_lo) {
            const double num = a - w.T_lo;
            const double fr = num / den;
            const double off = dt * fr;
            tlo = tn + off;
            st |= kCylStoreLo;
        }
    }
    return st;
}

// t_n of the block's clock, the operations of the Cartesian recorder
__host__ __device__ __forceinline__ double cyl_history_tn(const HistBlock &blk)
{
#pragma clang fp contract(off)
    const double nd = (double)blk.n;
    const double adv = nd * blk.dt;
    return blk.t0 + adv;
}

// the box of a launch: cell (i, j, k) at i*sx + j*nz + k
struct CylBox {
    int nr, nphi, nz;
    long sx;
};

// ADI_OK and the box, or the first rule of the header the extents break
inline int make_cyl_box(const char *who, int nr, int nphi, int nz, long plane_stride, CylBox *g)
{
    ADI_REQUIRE(nr > 0 && nphi > 0 && nz > 0, "%s: bad grid %d x %d x %d", who, nr, nphi, nz);
    ADI_REQUIRE((long)nphi * nz <= 0x7fffffffL, "%s: (nphi, nz) plane too large", who);
    ADI_REQUIRE(nr <= 65535, "%s: more than 65535 radii", who);
    const long sx = plane_stride ? plane_stride : (long)nphi * nz;
    ADI_REQUIRE(sx >= (long)nphi * nz, "%s: plane_stride < nphi*nz", who);
    g->nr = nr; g->nphi = nphi; g->nz = nz; g->sx = sx;
    return ADI_OK;
}

inline int check_cyl_levels(const char *who, const adi_history_levels *w)
{
    ADI_REQUIRE(w != nullptr, "%s: null levels", who);
    ADI_REQUIRE(isfinite(w->T_hi) && isfinite(w->T_lo) && isfinite(w->T_melt), "%s: T_hi, T_lo or T_melt not finite", who);
    ADI_REQUIRE(w->T_hi > w->T_lo, "%s: T_hi must be above T_lo", who);
    return ADI_OK;
}

// what adi_cyl_phase_apply and its host twin refuse
inline int check_cyl_phase_apply(const char *who, const adi_phase_change *law, double cp, const double *T, const double *f,
                                 const double *T_in, const uint8_t *active, int nr, int nphi, int nz, long plane_stride,
                                 PhaseLaw *w, CylBox *g)
{
    ADI_REQUIRE(law && T && f, "%s: null argument", who);
    ADI_REQUIRE(T != f, "%s: f aliases T", who);
    ADI_REQUIRE(T_in == nullptr || (T_in != T && T_in != f), "%s: T_in aliases T or f", who);
    ADI_REQUIRE(active == nullptr || T_in != nullptr, "%s: T_in is required with an active mask (newborn cells are seeded from it)", who);
    if (int rc = make_phase_law(who, *law, cp, w)) return rc;
    return make_cyl_box(who, nr, nphi, nz, plane_stride, g);
}

// what adi_cyl_history_record and its host twin refuse
inline int check_cyl_history_record(const char *who, const adi_history_levels *w, const void *block, const double *T_in,
                                    const double *T_out, const double *peak, const double *t_hi, const double *t_lo,
                                    const int32_t *log, int nr, int nphi, int nz, long plane_stride, CylBox *g)
{
    ADI_REQUIRE(block && T_in && T_out && peak && t_hi && t_lo && log, "%s: null argument", who);
    ADI_REQUIRE(T_in != T_out, "%s: T_out aliases T_in", who);
    ADI_REQUIRE(peak != T_in && peak != T_out && t_hi != T_in && t_hi != T_out && t_lo != T_in && t_lo != T_out,
                "%s: a state array aliases T", who);
    ADI_REQUIRE(peak != t_hi && peak != t_lo && t_hi != t_lo, "%s: the state arrays alias", who);
    ADI_REQUIRE(((uintptr_t)log & 7u) == 0 && ((uintptr_t)block & 7u) == 0, "%s: block or log not 8-byte aligned", who);
    if (int rc = check_cyl_levels(who, w)) return rc;
    return make_cyl_box(who, nr, nphi, nz, plane_stride, g);
}

// the latent-heat pass over host arrays: the loop of the kernel, cell by cell
inline void cyl_phase_apply_host(const PhaseLaw &w, const CylBox &g, double *T, double *F, const double *Tin,
                                 const uint8_t *act, bool skip_k0, bool skip_kN)
{
    for (int i = 0; i < g.nr; ++i)
        for (int j = 0; j < g.nphi; ++j)
            for (int k = 0; k < g.nz; ++k) {
                const long p = (long)i * g.sx + (long)j * g.nz + k;
                if (act != nullptr && act[p] == 0) continue;
                if ((skip_k0 && k == 0) || (skip_kN && k == g.nz - 1)) continue;
                const double fs = F[p];
                const bool seed = Tin != nullptr && fs != fs;
                double tn, fn;
                const unsigned st = cyl_phase_cell(w, T[p], fs, seed, seed ? Tin[p] : 0.0, tn, fn);
                if (st & kCylStoreT) T[p] = tn;
                if (st & kCylStoreF) F[p] = fn;
            }
}

// the record over host arrays into the block's log row (the row accumulates as the kernel's atomics do); no tick
inline void cyl_history_record_host(const adi_history_levels &w, const CylBox &g, const HistBlock &blk, const double *A,
                                    const double *B, double *P, double *THI, double *TLO, int32_t *log, const uint8_t *act)
{
    const double tn = cyl_history_tn(blk);
    int32_t *r = log + (blk.slot < blk.capacity ? blk.slot : blk.capacity) * ADI_CYL_HISTORY_LOG_INTS;
    long long sum_i;
    memcpy(&sum_i, r + 8, sizeof(sum_i));
    for (int i = 0; i < g.nr; ++i)
        for (int j = 0; j < g.nphi; ++j)
            for (int k = 0; k < g.nz; ++k) {
                const long p = (long)i * g.sx + (long)j * g.nz + k;
                if (act != nullptr && act[p] == 0) continue;
                const double b = B[p], pk = P[p];
                const double a = cyl_history_needs_a(w, pk) ? A[p] : 0.0;
                double peak, thi = 0.0, tlo = 0.0;
                const unsigned st = cyl_history_cell(w, tn, blk.dt, a, b, pk, peak, thi, tlo);
                if (st & kCylStorePeak) P[p] = peak;
                if (st & kCylStoreHi) THI[p] = thi;
                if (st & kCylStoreLo) TLO[p] = tlo;
                if (b >= w.T_melt) {
                    r[0] += 1;
                    sum_i += i;
                    r[1] = i < r[1] ? i : r[1]; r[2] = j < r[2] ? j : r[2]; r[3] = k < r[3] ? k : r[3];
                    r[4] = i > r[4] ? i : r[4]; r[5] = j > r[5] ? j : r[5]; r[6] = k > r[6] ? k : r[6];
                }
            }
    memcpy(r + 8, &sum_i, sizeof(sum_i));
}

}  // namespace adi
