// adi_history.hip -- thermal history of the Cartesian step (include/adi_hip.h, "Thermal history"): after a step A -> B the
// peak temperature, the times of the last downward crossings of two levels and the melt pool of the step are recorded.
//   k_history_record   every step: T_peak, t_hi, t_lo in place, one row of the log
//   k_history_seed     T_peak = T, times NaN on selected in-mask cells, NaN off the mask (reset, newborn cells)
//   k_history_clock, k_history_tick, k_history_reset_log   the device block (t0, dt, n, slot, capacity) and the log rows
// One workgroup of 256 threads per 16 x 16 x 16 brick of the flags summary, with the cell ownership and the load forms of
// adi_history_dev.hpp (shared with adi_solidify.hip).  The loads of a thread are issued
// together ahead of the arithmetic; stores go cell by cell (8 bytes) so that a cell no rule touches is never written.  The
// crossing rules only ever store t_hi and t_lo, so neither is loaded.  The pool of a brick is three words per thread (the
// count, the set of local i and j, the set of local k), OR- / add-reduced over the wave by shuffles and over the four waves
// through LDS; one thread of a brick that holds pool cells issues seven integer atomics.  No existing kernel changes.
#include <math.h>

#include "adi_history_dev.hpp"

namespace adi {

constexpr int kHistEmptyLo = 0x7fffffff;

template <bool VEC>
__global__ __launch_bounds__(256) void k_history_record(adi_history_levels w, const HistBlock *__restrict__ blk,
                                                        const double *__restrict__ A, const double *__restrict__ B,
                                                        double *__restrict__ P, double *__restrict__ THI,
                                                        double *__restrict__ TLO, int *__restrict__ log,
                                                        const uint8_t *__restrict__ flags,
                                                        const unsigned *__restrict__ bricks, Lay L)
{
#pragma clang fp contract(off)
    __shared__ unsigned red[4][3];
    const int bk = (int)blockIdx.x, bj = (int)blockIdx.y, bi = (int)blockIdx.z;
    const unsigned tid = threadIdx.x;
    const bool solid = hist_all_solid(bricks, L, bi, bj, bk);
    HistCell c[kHistIter];
    double b[kHistIter][2], pk[kHistIter][2];
    // the loads of the brick, issued together: flags (only where the flags summary does not say all-solid), then B and
    // T_peak (only where a cell of the pair is in the mask)
#pragma unroll
    for (int it = 0; it < kHistIter; ++it) {
        c[it] = hist_cell(L, bi, bj, bk, it, tid);
        if (c[it].in) c[it].m = solid ? c[it].in : (hist_mask_pair<VEC>(flags, c[it]) & c[it].in);
    }
#pragma unroll
    for (int it = 0; it < kHistIter; ++it) {
        b[it][0] = 0.0; b[it][1] = 0.0; pk[it][0] = 0.0; pk[it][1] = 0.0;
        if (c[it].m) {
            hist_load_pair<VEC>(B, c[it], b[it][0], b[it][1]);
            hist_load_pair<VEC>(P, c[it], pk[it][0], pk[it][1]);
        }
    }
    bool hot = false;                 // an old peak of this thread's cells above T_lo: the brick may hold a crossing
    unsigned cnt = 0u, mij = 0u, mk = 0u;   // pool cells; bit il | bit 16 + jl; bit kl of the local coordinates among them
#pragma unroll
    for (int it = 0; it < kHistIter; ++it) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if ((c[it].m >> s) & 1u) {
                const double bs = b[it][s], ps = pk[it][s];
                if (bs > ps) P[c[it].p + s] = bs;
                hot = hot || ps > w.T_lo;
                if (bs >= w.T_melt) {
                    cnt += 1u;
                    mij |= (1u << (2 * it + (int)(tid >> 7))) | (0x10000u << ((tid >> 3) & 15u));
                    mk |= 1u << (2u * (tid & 7u) + (unsigned)s);
                }
            }
        }
    }
    if (__syncthreads_or(hot ? 1 : 0)) {                    // (uniform over the workgroup)
        const double dt = blk->dt;
        const double nd = (double)blk->n;
        const double adv = nd * dt;
        const double tn = blk->t0 + adv;
        double a[kHistIter][2];
#pragma unroll
        for (int it = 0; it < kHistIter; ++it) {
            a[it][0] = 0.0; a[it][1] = 0.0;
            if (c[it].m) hist_load_pair<VEC>(A, c[it], a[it][0], a[it][1]);
        }
#pragma unroll
        for (int it = 0; it < kHistIter; ++it) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if ((c[it].m >> s) & 1u) {
                    const double as = a[it][s], bs = b[it][s];
                    const double den = as - bs;
                    if (as > w.T_hi && bs <= w.T_hi) {
                        const double num = as - w.T_hi;
                        const double fr = num / den;
                        const double off = dt * fr;
                        THI[c[it].p + s] = tn + off;
                        TLO[c[it].p + s] = hist_nan();
                    }
                    if (as > w.T_lo && bs <= w.T_lo) {
                        const double num = as - w.T_lo;
                        const double fr = num / den;
                        const double off = dt * fr;
                        TLO[c[it].p + s] = tn + off;
                    }
                }
            }
        }
    }
    if (__syncthreads_or(cnt != 0u ? 1 : 0)) {
        cnt = wave_add(cnt);
        mij = wave_or(mij);
        mk = wave_or(mk);
        if ((tid & 63u) == 0u) {
            red[tid >> 6][0] = cnt; red[tid >> 6][1] = mij; red[tid >> 6][2] = mk;
        }
        __syncthreads();
        if (tid == 0u) {
            cnt = red[0][0] + red[1][0] + red[2][0] + red[3][0];
            mij = red[0][1] | red[1][1] | red[2][1] | red[3][1];
            mk = red[0][2] | red[1][2] | red[2][2] | red[3][2];
            const unsigned mi = mij & 0xffffu, mj = mij >> 16;
            const long long slot = blk->slot, cap = blk->capacity;
            int *r = log + (slot < cap ? slot : cap) * ADI_HISTORY_LOG_INTS;
            const int i0 = bi * kBrick, j0 = bj * kBrick, k0 = bk * kBrick;
            atomicAdd(r, (int)cnt);
            atomicMin(r + 1, i0 + __ffs((int)mi) - 1);
            atomicMin(r + 2, j0 + __ffs((int)mj) - 1);
            atomicMin(r + 3, k0 + __ffs((int)mk) - 1);
            atomicMax(r + 4, i0 + 31 - __clz((int)mi));
            atomicMax(r + 5, j0 + 31 - __clz((int)mj));
            atomicMax(r + 6, k0 + 31 - __clz((int)mk));
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_history_seed(const double *__restrict__ T, double *__restrict__ P,
                                                      double *__restrict__ THI, double *__restrict__ TLO,
                                                      const uint8_t *__restrict__ flags, const unsigned *__restrict__ bricks,
                                                      const uint8_t *__restrict__ sel, Lay L)
{
    const int bk = (int)blockIdx.x, bj = (int)blockIdx.y, bi = (int)blockIdx.z;
    const unsigned tid = threadIdx.x;
    const bool solid = hist_all_solid(bricks, L, bi, bj, bk);
    const double nan = hist_nan();
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
                P[p] = nan; THI[p] = nan; TLO[p] = nan;
            } else if (sel == nullptr || sel[p] != 0) {
                P[p] = s ? t1 : t0; THI[p] = nan; TLO[p] = nan;
            }
        }
    }
}

__global__ void k_history_clock(HistBlock *blk, double t0, double dt) { blk->t0 = t0; blk->dt = dt; blk->n = 0; }
__global__ void k_history_tick(HistBlock *blk) { blk->n += 1; blk->slot += 1; }

// rows [0, capacity] of the log empty, one thread per row; the first thread also rewinds the block
__global__ __launch_bounds__(256) void k_history_reset_log(HistBlock *blk, int *__restrict__ log, long long capacity)
{
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row == 0) { blk->n = 0; blk->slot = 0; blk->capacity = capacity; }
    if (row > capacity) return;
    int *r = log + row * ADI_HISTORY_LOG_INTS;
    r[0] = 0;
    r[1] = kHistEmptyLo; r[2] = kHistEmptyLo; r[3] = kHistEmptyLo;
    r[4] = -1; r[5] = -1; r[6] = -1;
    r[7] = 0;
}

}  // namespace adi

using namespace adi;

extern "C" {

int adi_history_record(const adi_history_levels *h_levels, const void *d_block, const double *d_T_in, const double *d_T_out,
                       double *d_peak, double *d_t_hi, double *d_t_lo, int32_t *d_log, const uint8_t *d_flags,
                       const uint32_t *d_bricks, int nx, int ny, int nz, long plane_stride, void *stream)
{
    ADI_REQUIRE(h_levels && d_block && d_T_in && d_T_out && d_peak && d_t_hi && d_t_lo && d_log && d_flags,
                "adi_history_record: null argument");
    ADI_REQUIRE(d_T_in != d_T_out, "adi_history_record: d_T_out aliases d_T_in");
    ADI_REQUIRE(d_peak != d_T_in && d_peak != d_T_out && d_t_hi != d_T_in && d_t_hi != d_T_out && d_t_lo != d_T_in &&
                d_t_lo != d_T_out, "adi_history_record: a state array aliases T");
    ADI_REQUIRE(d_peak != d_t_hi && d_peak != d_t_lo && d_t_hi != d_t_lo, "adi_history_record: the state arrays alias");
    ADI_REQUIRE(isfinite(h_levels->T_hi) && isfinite(h_levels->T_lo) && isfinite(h_levels->T_melt),
                "adi_history_record: T_hi, T_lo or T_melt not finite");
    ADI_REQUIRE(h_levels->T_hi > h_levels->T_lo, "adi_history_record: T_hi must be above T_lo");
    HistLaunch g;
    if (int rc = make_hist_launch("adi_history_record", nx, ny, nz, plane_stride, &g)) return rc;
    const HistBlock *blk = (const HistBlock *)d_block;
    if (pair_vec(g.L, d_flags, d_T_in, d_T_out, d_peak))
        hipLaunchKernelGGL(k_history_record<true>, g.grid, dim3(256), 0, as_stream(stream), *h_levels, blk, d_T_in, d_T_out,
                           d_peak, d_t_hi, d_t_lo, (int *)d_log, d_flags, (const unsigned *)d_bricks, g.L);
    else
        hipLaunchKernelGGL(k_history_record<false>, g.grid, dim3(256), 0, as_stream(stream), *h_levels, blk, d_T_in, d_T_out,
                           d_peak, d_t_hi, d_t_lo, (int *)d_log, d_flags, (const unsigned *)d_bricks, g.L);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_history_set_clock(void *d_block, double t0, double dt, void *stream)
{
    ADI_REQUIRE(d_block, "adi_history_set_clock: null block");
    ADI_REQUIRE(isfinite(t0) && isfinite(dt) && dt > 0.0, "adi_history_set_clock: bad t0 / dt");
    hipLaunchKernelGGL(k_history_clock, dim3(1), dim3(1), 0, as_stream(stream), (HistBlock *)d_block, t0, dt);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_history_tick(void *d_block, void *stream)
{
    ADI_REQUIRE(d_block, "adi_history_tick: null block");
    hipLaunchKernelGGL(k_history_tick, dim3(1), dim3(1), 0, as_stream(stream), (HistBlock *)d_block);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_history_seed(const double *d_T, double *d_peak, double *d_t_hi, double *d_t_lo, const uint8_t *d_flags,
                     const uint32_t *d_bricks, const uint8_t *d_sel, int nx, int ny, int nz, long plane_stride,
                     void *stream)
{
    ADI_REQUIRE(d_T && d_peak && d_t_hi && d_t_lo && d_flags, "adi_history_seed: null argument");
    ADI_REQUIRE(d_peak != d_T && d_t_hi != d_T && d_t_lo != d_T, "adi_history_seed: a state array aliases T");
    ADI_REQUIRE(d_peak != d_t_hi && d_peak != d_t_lo && d_t_hi != d_t_lo, "adi_history_seed: the state arrays alias");
    HistLaunch g;
    if (int rc = make_hist_launch("adi_history_seed", nx, ny, nz, plane_stride, &g)) return rc;
    if (pair_vec(g.L, d_flags, d_T))
        hipLaunchKernelGGL(k_history_seed<true>, g.grid, dim3(256), 0, as_stream(stream), d_T, d_peak, d_t_hi, d_t_lo, d_flags,
                           (const unsigned *)d_bricks, d_sel, g.L);
    else
        hipLaunchKernelGGL(k_history_seed<false>, g.grid, dim3(256), 0, as_stream(stream), d_T, d_peak, d_t_hi, d_t_lo, d_flags,
                           (const unsigned *)d_bricks, d_sel, g.L);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_history_reset_log(void *d_block, int32_t *d_log, long capacity, void *stream)
{
    ADI_REQUIRE(d_block && d_log, "adi_history_reset_log: null argument");
    ADI_REQUIRE(capacity >= 1 && capacity < (1L << 31), "adi_history_reset_log: capacity %ld is not in [1, 2^31)", capacity);
    const unsigned nb = (unsigned)((capacity + 1 + 255) / 256);
    hipLaunchKernelGGL(k_history_reset_log, dim3(nb), dim3(256), 0, as_stream(stream), (HistBlock *)d_block, (int *)d_log,
                       (long long)capacity);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // extern "C"
