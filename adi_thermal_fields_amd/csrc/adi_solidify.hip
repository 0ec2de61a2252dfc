// adi_solidify.hip -- the conditions at the freezing front of the Cartesian step (include/adi_hip.h, "Solidification record"):
// for a cell that drops through T_freeze in the step A -> B, the crossing time, the cooling rate and the squared thermal
// gradient at the crossing time.
//   k_solid_record   every step: t_solid, cooling_rate, g2 of the cells that freeze in it; the brick's word
//   k_solid_seed     NaN on selected in-mask cells and off the mask; the brick's word from T (reset, newborn cells)
// One workgroup of 256 threads per 16 x 16 x 16 brick, with the cell ownership and the load forms of adi_history_dev.hpp; the
// clock is a HistBlock driven by adi_history_set_clock / adi_history_tick.  A cold pass loads B (and flags, where the summary
// does not say all-solid) and nothing else: the brick's word, "some in-mask B of this brick was above T_freeze at the previous
// record", decides whether A is loaded at all.  A freezing cell then loads its own flags byte and up to six neighbours of A
// and of B from global memory, whichever brick they lie in.  That part diverges -- a wave runs it once per freezing cell of
// its fullest lane -- and is accepted: the front is a surface, a few cells of a few bricks.  The thread keeps the freezing
// cells as a 16-bit set and walks it, so no register array is indexed at run time and nothing goes to scratch.  Stores go
// cell by cell; a cell that does not freeze is never written.
#include <math.h>

#include "adi_history_dev.hpp"

namespace adi {

struct SolidScal {
    double T_f, dx, two_dx;
};

__device__ __forceinline__ long solid_word(int bi, int bj, int bk)
{
    return ((long)bi * (long)gridDim.y + bj) * (long)gridDim.x + bk;
}

// dF/dx_a at cell p (centre value f0, element stride st): central where both neighbours are in the mask, one-sided where one
// is, 0 where none is
__device__ __forceinline__ double solid_grad(const double *__restrict__ F, long p, long st, double f0, unsigned lo, unsigned hi,
                                             const SolidScal &w)
{
#pragma clang fp contract(off)
    if (lo && hi) {
        const double d = F[p + st] - F[p - st];
        return d / w.two_dx;
    }
    if (hi) {
        const double d = F[p + st] - f0;
        return d / w.dx;
    }
    if (lo) {
        const double d = f0 - F[p - st];
        return d / w.dx;
    }
    return 0.0;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_solid_record(SolidScal w, const HistBlock *__restrict__ blk,
                                                      const double *__restrict__ A, const double *__restrict__ B,
                                                      double *__restrict__ TS, double *__restrict__ CR,
                                                      double *__restrict__ G2, unsigned *__restrict__ hot,
                                                      const uint8_t *__restrict__ flags,
                                                      const unsigned *__restrict__ bricks, Lay L)
{
#pragma clang fp contract(off)
    const int bk = (int)blockIdx.x, bj = (int)blockIdx.y, bi = (int)blockIdx.z;
    const unsigned tid = threadIdx.x;
    const bool solid = hist_all_solid(bricks, L, bi, bj, bk);
    const long word = solid_word(bi, bj, bk);
    const unsigned was = hot[word];                       // (every thread reads it ahead of the barrier below)
    HistCell c[kHistIter];
    double b[kHistIter][2];
#pragma unroll
    for (int it = 0; it < kHistIter; ++it) {
        c[it] = hist_cell(L, bi, bj, bk, it, tid);
        if (c[it].in) c[it].m = solid ? c[it].in : (hist_mask_pair<VEC>(flags, c[it]) & c[it].in);
    }
#pragma unroll
    for (int it = 0; it < kHistIter; ++it) {
        b[it][0] = 0.0; b[it][1] = 0.0;
        if (c[it].m) hist_load_pair<VEC>(B, c[it], b[it][0], b[it][1]);
    }
    bool above = false;               // an in-mask B of this thread's cells above T_freeze: the brick may freeze next step
#pragma unroll
    for (int it = 0; it < kHistIter; ++it) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if ((c[it].m >> s) & 1u) above = above || b[it][s] > w.T_f;
    }
    const unsigned now = __syncthreads_or(above ? 1 : 0) ? 1u : 0u;
    if (tid == 0u && now != was) hot[word] = now;
    if (was == 0u) return;                                // (uniform over the workgroup)
    unsigned fm = 0u;                                     // bit 2 it + s: that cell freezes in this step
#pragma unroll
    for (int it = 0; it < kHistIter; ++it) {
        double a0 = 0.0, a1 = 0.0;
        if (c[it].m) hist_load_pair<VEC>(A, c[it], a0, a1);
        if ((c[it].m & 1u) && a0 > w.T_f && b[it][0] <= w.T_f) fm |= 1u << (2 * it);
        if ((c[it].m & 2u) && a1 > w.T_f && b[it][1] <= w.T_f) fm |= 2u << (2 * it);
    }
    if (fm == 0u) return;
    const double dt = blk->dt;
    const double nd = (double)blk->n;
    const double adv = nd * dt;
    const double tn = blk->t0 + adv;
    const long st[3] = {L.sx, (long)L.nz, 1L};
    while (fm) {
        const int q = __ffs((int)fm) - 1;
        fm &= fm - 1u;
        const long p = hist_cell(L, bi, bj, bk, q >> 1, tid).p + (q & 1);
        const unsigned fl = flags[p];                     // also in an all-solid brick: the byte knows the box faces
        const double as = A[p], bs = B[p];
        const double den = as - bs;
        const double num = as - w.T_f;
        const double fr = num / den;
        const double off = dt * fr;
        TS[p] = tn + off;
        CR[p] = den / dt;
        double g[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const unsigned lo = (fl >> (1 + 2 * ax)) & 1u, hi = (fl >> (2 + 2 * ax)) & 1u;
            const double gA = solid_grad(A, p, st[ax], as, lo, hi, w);
            const double gB = solid_grad(B, p, st[ax], bs, lo, hi, w);
            const double dg = gB - gA;
            const double sg = fr * dg;
            g[ax] = gA + sg;
        }
        const double xx = g[0] * g[0];
        const double yy = g[1] * g[1];
        const double zz = g[2] * g[2];
        const double s2 = xx + yy;
        G2[p] = s2 + zz;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_solid_seed(double T_f, const double *__restrict__ T, double *__restrict__ TS,
                                                    double *__restrict__ CR, double *__restrict__ G2,
                                                    unsigned *__restrict__ hot, const uint8_t *__restrict__ flags,
                                                    const unsigned *__restrict__ bricks, const uint8_t *__restrict__ sel, Lay L)
{
    const int bk = (int)blockIdx.x, bj = (int)blockIdx.y, bi = (int)blockIdx.z;
    const unsigned tid = threadIdx.x;
    const bool solid = hist_all_solid(bricks, L, bi, bj, bk);
    const double nan = hist_nan();
    bool above = false;               // a seeded in-mask cell above T_freeze
#pragma unroll 2
    for (int it = 0; it < kHistIter; ++it) {
        HistCell c = hist_cell(L, bi, bj, bk, it, tid);
        if (!c.in) continue;
        c.m = solid ? c.in : (hist_mask_pair<VEC>(flags, c) & c.in);
        double t0 = 0.0, t1 = 0.0;
        if (c.m) hist_load_pair<VEC>(T, c, t0, t1);
        for (int s = 0; s < 2; ++s) {
            if (!((c.in >> s) & 1u)) continue;
            const long p = c.p + s;
            if (!((c.m >> s) & 1u)) {
                TS[p] = nan; CR[p] = nan; G2[p] = nan;
            } else if (sel == nullptr || sel[p] != 0) {
                TS[p] = nan; CR[p] = nan; G2[p] = nan;
                above = above || (s ? t1 : t0) > T_f;
            }
        }
    }
    if (__syncthreads_or(above ? 1 : 0) && tid == 0u) hot[solid_word(bi, bj, bk)] = 1u;   // (what was set stays set)
}

}  // namespace adi

using namespace adi;

extern "C" {

int adi_solid_record(double T_freeze, double dx, const void *d_block, const double *d_T_in, const double *d_T_out,
                     double *d_t_solid, double *d_rate, double *d_g2, uint32_t *d_hot, const uint8_t *d_flags,
                     const uint32_t *d_bricks, int nx, int ny, int nz, long plane_stride, void *stream)
{
    ADI_REQUIRE(d_block && d_T_in && d_T_out && d_t_solid && d_rate && d_g2 && d_hot && d_flags,
                "adi_solid_record: null argument");
    ADI_REQUIRE(d_T_in != d_T_out, "adi_solid_record: d_T_out aliases d_T_in");
    ADI_REQUIRE(d_t_solid != d_T_in && d_t_solid != d_T_out && d_rate != d_T_in && d_rate != d_T_out && d_g2 != d_T_in &&
                d_g2 != d_T_out, "adi_solid_record: a state array aliases T");
    ADI_REQUIRE(d_t_solid != d_rate && d_t_solid != d_g2 && d_rate != d_g2, "adi_solid_record: the state arrays alias");
    ADI_REQUIRE(isfinite(T_freeze), "adi_solid_record: T_freeze not finite");
    ADI_REQUIRE(isfinite(dx) && dx > 0.0, "adi_solid_record: dx must be positive");
    HistLaunch g;
    if (int rc = make_hist_launch("adi_solid_record", nx, ny, nz, plane_stride, &g)) return rc;
    const SolidScal w = {T_freeze, dx, 2.0 * dx};
    const HistBlock *blk = (const HistBlock *)d_block;
    if (pair_vec(g.L, d_flags, d_T_in, d_T_out))
        hipLaunchKernelGGL(k_solid_record<true>, g.grid, dim3(256), 0, as_stream(stream), w, blk, d_T_in, d_T_out, d_t_solid,
                           d_rate, d_g2, (unsigned *)d_hot, d_flags, (const unsigned *)d_bricks, g.L);
    else
        hipLaunchKernelGGL(k_solid_record<false>, g.grid, dim3(256), 0, as_stream(stream), w, blk, d_T_in, d_T_out, d_t_solid,
                           d_rate, d_g2, (unsigned *)d_hot, d_flags, (const unsigned *)d_bricks, g.L);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_solid_seed(double T_freeze, const double *d_T, double *d_t_solid, double *d_rate, double *d_g2, uint32_t *d_hot,
                   const uint8_t *d_flags, const uint32_t *d_bricks, const uint8_t *d_sel, int nx, int ny, int nz,
                   long plane_stride, void *stream)
{
    ADI_REQUIRE(d_T && d_t_solid && d_rate && d_g2 && d_hot && d_flags, "adi_solid_seed: null argument");
    ADI_REQUIRE(d_t_solid != d_T && d_rate != d_T && d_g2 != d_T, "adi_solid_seed: a state array aliases T");
    ADI_REQUIRE(d_t_solid != d_rate && d_t_solid != d_g2 && d_rate != d_g2, "adi_solid_seed: the state arrays alias");
    ADI_REQUIRE(isfinite(T_freeze), "adi_solid_seed: T_freeze not finite");
    HistLaunch g;
    if (int rc = make_hist_launch("adi_solid_seed", nx, ny, nz, plane_stride, &g)) return rc;
    if (pair_vec(g.L, d_flags, d_T))
        hipLaunchKernelGGL(k_solid_seed<true>, g.grid, dim3(256), 0, as_stream(stream), T_freeze, d_T, d_t_solid, d_rate, d_g2,
                           (unsigned *)d_hot, d_flags, (const unsigned *)d_bricks, d_sel, g.L);
    else
        hipLaunchKernelGGL(k_solid_seed<false>, g.grid, dim3(256), 0, as_stream(stream), T_freeze, d_T, d_t_solid, d_rate, d_g2,
                           (unsigned *)d_hot, d_flags, (const unsigned *)d_bricks, d_sel, g.L);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // extern "C"
