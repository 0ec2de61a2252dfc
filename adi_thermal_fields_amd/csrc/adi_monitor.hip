// adi_monitor.hip -- the field monitor of the Cartesian step (include/adi_hip.h, "Field monitor"): after a step, the value of
// the final field at up to 256 probe cells and, over the in-mask cells of up to 8 index boxes, the count, the extrema and the
// sums of T, of w[id]*T and of a second field -- one row of a device log per recorded step.
//   k_monitor_reduce      one workgroup of 256 threads per 16 x 16 x 16 brick of the brick box that meets a region, with the
//                         cell ownership and the load forms of adi_history_dev.hpp: flags (unless the summary says all-solid), T
//                         of in-mask pairs once for all regions, ids and the second field only when present; one partial per
//                         region the brick meets
//   k_monitor_finish      one workgroup: the partials of each region in their defined order, the probes, the row
//   k_monitor_reset_log   every word of the log NaN, the block rewound
// The order of every sum is written down in the header and in FieldMonitor.record_reference; nothing here may depart from it.
// Sums travel over the wave by xor-butterfly (every lane ends with the same bits, the addition being commutative) and over the
// four waves through LDS in wave order.  The extrema are taken on integer keys that order the finite doubles with
// -0.0 < +0.0, so they depend on no order at all.  No floating-point atomics, no atomics at all: every (region, brick) record
// of the partial buffer is rewritten by every record launch, since the launch box covers every region's brick box.
#include <math.h>

#include "adi_monitor_dev.hpp"

namespace adi {

constexpr long long kMonKeyMax = 0x7fffffffffffffffLL;

// the finite doubles in their order, -0.0 below +0.0, as signed 64-bit integers; its own inverse
__device__ __forceinline__ long long mon_key(long long bits) { return bits ^ ((bits >> 63) & kMonKeyMax); }

__device__ __forceinline__ long long shfl_xor_ll(long long v, int o)
{
    const int lo = __shfl_xor((int)(v & 0xffffffffLL), o), hi = __shfl_xor((int)(v >> 32), o);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}
__device__ __forceinline__ double wave_sum(double v)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int o = 1; o <= 32; o <<= 1) v = v + __longlong_as_double(shfl_xor_ll(__double_as_longlong(v), o));
    return v;
}
__device__ __forceinline__ long long wave_min_ll(long long v)
{
#pragma unroll
    for (int o = 1; o <= 32; o <<= 1) { const long long u = shfl_xor_ll(v, o); v = u < v ? u : v; }
    return v;
}
__device__ __forceinline__ long long wave_max_ll(long long v)
{
#pragma unroll
    for (int o = 1; o <= 32; o <<= 1) { const long long u = shfl_xor_ll(v, o); v = u > v ? u : v; }
    return v;
}

template <bool VEC>
__device__ __forceinline__ unsigned mon_id_pair(const uint8_t *__restrict__ ids, const HistCell &c)
{
    if (VEC) return *reinterpret_cast<const unsigned short *>(ids + c.p);
    unsigned v = ids[c.p];
    if (c.in & 2u) v |= (unsigned)ids[c.p + 1] << 8;
    return v;
}

struct MonShared {
    double s[kMonRegions][4][3];
    long long k[kMonRegions][4][2];
    unsigned c[kMonRegions][4];
};

template <bool VEC, bool HAS_W, bool HAS_X>
__global__ __launch_bounds__(256) void k_monitor_reduce(MonRegions R, MonWeights W, const double *__restrict__ T,
                                                        const double *__restrict__ X, const uint8_t *__restrict__ ids,
                                                        const uint8_t *__restrict__ flags,
                                                        const unsigned *__restrict__ bricks, long long *__restrict__ partial,
                                                        Lay L, int ob0, int ob1, int ob2)
{
#pragma clang fp contract(off)
    __shared__ MonShared red;
    __shared__ double wt[ADI_MATMAP_MAX];
    const int bk = (int)blockIdx.x + ob2, bj = (int)blockIdx.y + ob1, bi = (int)blockIdx.z + ob0;
    const unsigned tid = threadIdx.x;
    unsigned meet = 0u;                                   // bit r: this brick lies in the brick box of region r (uniform)
    for (int r = 0; r < R.n; ++r) {
        const bool in = bi >= R.blo[r][0] && bi < R.blo[r][0] + R.bn[r][0] && bj >= R.blo[r][1] &&
                        bj < R.blo[r][1] + R.bn[r][1] && bk >= R.blo[r][2] && bk < R.blo[r][2] + R.bn[r][2];
        meet |= (in ? 1u : 0u) << r;
    }
    if (meet == 0u) return;
    if (HAS_W && tid == 0u) {
#pragma unroll
        for (int q = 0; q < ADI_MATMAP_MAX; ++q) wt[q] = W.w[q];
    }
    const bool solid = hist_all_solid(bricks, L, bi, bj, bk);
    HistCell c[kHistIter];
    double t[kHistIter][2], x[kHistIter][2], wT[kHistIter][2];
    unsigned idp[kHistIter];
#pragma unroll
    for (int it = 0; it < kHistIter; ++it) {
        c[it] = hist_cell(L, bi, bj, bk, it, tid);
        if (c[it].in) c[it].m = solid ? c[it].in : (hist_mask_pair<VEC>(flags, c[it]) & c[it].in);
    }
#pragma unroll
    for (int it = 0; it < kHistIter; ++it) {
        t[it][0] = 0.0; t[it][1] = 0.0; x[it][0] = 0.0; x[it][1] = 0.0; idp[it] = 0u;
        if (c[it].m) {
            hist_load_pair<VEC>(T, c[it], t[it][0], t[it][1]);
            if (HAS_W) idp[it] = mon_id_pair<VEC>(ids, c[it]);
            if (HAS_X) hist_load_pair<VEC>(X, c[it], x[it][0], x[it][1]);
        }
    }
    if (HAS_W) {
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kHistIter; ++it) {
            const double w0 = wt[idp[it] & 7u], w1 = wt[(idp[it] >> 8) & 7u];
            wT[it][0] = w0 * t[it][0];
            wT[it][1] = w1 * t[it][1];
        }
    }
    const int j = bj * kBrick + (int)((tid >> 3) & 15u), k0 = bk * kBrick + 2 * (int)(tid & 7u), ih = (int)(tid >> 7);
    for (int r = 0; r < R.n; ++r) {
        if (!((meet >> r) & 1u)) continue;                // (uniform)
        const int lo0 = R.lo[r][0], hi0 = R.hi[r][0];
        const bool jok = j >= R.lo[r][1] && j < R.hi[r][1];
        const bool ok0 = jok && k0 >= R.lo[r][2] && k0 < R.hi[r][2];
        const bool ok1 = jok && k0 + 1 >= R.lo[r][2] && k0 + 1 < R.hi[r][2];
        double sT = 0.0, sW = 0.0, sX = 0.0;
        long long kmin = kMonKeyMax, kmax = -kMonKeyMax - 1;
        unsigned cnt = 0u;
#pragma unroll
        for (int it = 0; it < kHistIter; ++it) {
            const int i = bi * kBrick + 2 * it + ih;
            const bool iok = i >= lo0 && i < hi0;
            const bool in0 = iok && ok0 && (c[it].m & 1u) != 0u, in1 = iok && ok1 && (c[it].m & 2u) != 0u;
            {
                const double a0 = in0 ? t[it][0] : 0.0, a1 = in1 ? t[it][1] : 0.0;
                const double pr = a0 + a1;
                sT = it == 0 ? pr : sT + pr;
            }
            if (HAS_W) {
                const double a0 = in0 ? wT[it][0] : 0.0, a1 = in1 ? wT[it][1] : 0.0;
                const double pr = a0 + a1;
                sW = it == 0 ? pr : sW + pr;
            }
            if (HAS_X) {
                const double a0 = in0 ? x[it][0] : 0.0, a1 = in1 ? x[it][1] : 0.0;
                const double pr = a0 + a1;
                sX = it == 0 ? pr : sX + pr;
            }
            if (in0) {
                const long long key = mon_key(__double_as_longlong(t[it][0]));
                kmin = key < kmin ? key : kmin; kmax = key > kmax ? key : kmax; cnt += 1u;
            }
            if (in1) {
                const long long key = mon_key(__double_as_longlong(t[it][1]));
                kmin = key < kmin ? key : kmin; kmax = key > kmax ? key : kmax; cnt += 1u;
            }
        }
        sT = wave_sum(sT);
        if (HAS_W) sW = wave_sum(sW);
        if (HAS_X) sX = wave_sum(sX);
        kmin = wave_min_ll(kmin);
        kmax = wave_max_ll(kmax);
        cnt = wave_add(cnt);
        if ((tid & 63u) == 0u) {
            const unsigned wv = tid >> 6;
            red.s[r][wv][0] = sT; red.s[r][wv][1] = sW; red.s[r][wv][2] = sX;
            red.k[r][wv][0] = kmin; red.k[r][wv][1] = kmax;
            red.c[r][wv] = cnt;
        }
    }
    __syncthreads();
    if (tid != 0u) return;
    for (int r = 0; r < R.n; ++r) {
        if (!((meet >> r) & 1u)) continue;
        const long nb = (long)R.bn[r][0] * R.bn[r][1] * R.bn[r][2];
        const long n = ((long)(bi - R.blo[r][0]) * R.bn[r][1] + (bj - R.blo[r][1])) * R.bn[r][2] + (bk - R.blo[r][2]);
        long long *o = partial + kMonWords * R.off[r] + n;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if ((q == 1 && !HAS_W) || (q == 2 && !HAS_X)) continue;
            const double s01 = red.s[r][0][q] + red.s[r][1][q];
            const double s012 = s01 + red.s[r][2][q];
            o[q * nb] = __double_as_longlong(s012 + red.s[r][3][q]);
        }
        long long kmin = red.k[r][0][0], kmax = red.k[r][0][1];
        unsigned cnt = red.c[r][0];
#pragma unroll
        for (int wv = 1; wv < 4; ++wv) {
            kmin = red.k[r][wv][0] < kmin ? red.k[r][wv][0] : kmin;
            kmax = red.k[r][wv][1] > kmax ? red.k[r][wv][1] : kmax;
            cnt += red.c[r][wv];
        }
        o[3 * nb] = kmin; o[4 * nb] = kmax; o[5 * nb] = (long long)cnt;
    }
}

__global__ __launch_bounds__(256) void k_monitor_finish(MonRegions R, const HistBlock *__restrict__ blk,
                                                        const long long *__restrict__ partial, const double *__restrict__ T,
                                                        const uint8_t *__restrict__ flags, const int *__restrict__ probes,
                                                        int nprobe, double *__restrict__ log, long long capacity,
                                                        long row_words, Lay L, int has_w, int has_x)
{
#pragma clang fp contract(off)
    __shared__ MonShared red;
    __shared__ long long cells[kMonRegions][4];
    const unsigned tid = threadIdx.x;
    long long cap = blk->capacity;
    cap = (cap >= 1 && cap < capacity) ? cap : capacity;  // (the log was sized for `capacity`: never a row beyond it)
    long long slot = blk->slot;
    slot = slot < 0 ? 0 : slot;
    double *__restrict__ row = log + (slot < cap ? slot : cap) * row_words;
    if ((int)tid < nprobe) {
        const int i = probes[3 * tid], j = probes[3 * tid + 1], k = probes[3 * tid + 2];
        double v = hist_nan();
        if (i >= 0 && i < L.nx && j >= 0 && j < L.ny && k >= 0 && k < L.nz) {
            const long p = (long)i * L.sx + (long)j * L.nz + k;
            if (flags[p] & 1u) v = T[p];
        }
        row[tid] = v;
    }
    for (int r = 0; r < R.n; ++r) {
        const long nb = (long)R.bn[r][0] * R.bn[r][1] * R.bn[r][2];
        const long long *p = partial + kMonWords * R.off[r];
        double sT = 0.0, sW = 0.0, sX = 0.0;
        long long kmin = kMonKeyMax, kmax = -kMonKeyMax - 1, cnt = 0;
        for (long n = tid; n < nb; n += 256) {
            sT = sT + __longlong_as_double(p[n]);
            if (has_w) sW = sW + __longlong_as_double(p[nb + n]);
            if (has_x) sX = sX + __longlong_as_double(p[2 * nb + n]);
            const long long a = p[3 * nb + n], b = p[4 * nb + n];
            kmin = a < kmin ? a : kmin; kmax = b > kmax ? b : kmax;
            cnt += p[5 * nb + n];
        }
        sT = wave_sum(sT);
        sW = wave_sum(sW);
        sX = wave_sum(sX);
        kmin = wave_min_ll(kmin);
        kmax = wave_max_ll(kmax);
#pragma unroll
        for (int o = 1; o <= 32; o <<= 1) cnt += shfl_xor_ll(cnt, o);
        if ((tid & 63u) == 0u) {
            const unsigned wv = tid >> 6;
            red.s[r][wv][0] = sT; red.s[r][wv][1] = sW; red.s[r][wv][2] = sX;
            red.k[r][wv][0] = kmin; red.k[r][wv][1] = kmax;
            cells[r][wv] = cnt;
        }
    }
    __syncthreads();
    if (tid != 0u) return;
    for (int r = 0; r < R.n; ++r) {
        double *o = row + nprobe + ADI_MONITOR_REGION_WORDS * r;
        long long kmin = red.k[r][0][0], kmax = red.k[r][0][1], cnt = cells[r][0];
#pragma unroll
        for (int wv = 1; wv < 4; ++wv) {
            kmin = red.k[r][wv][0] < kmin ? red.k[r][wv][0] : kmin;
            kmax = red.k[r][wv][1] > kmax ? red.k[r][wv][1] : kmax;
            cnt += cells[r][wv];
        }
        o[0] = __longlong_as_double(cnt);
        o[1] = cnt ? __longlong_as_double(mon_key(kmin)) : hist_nan();
        o[2] = cnt ? __longlong_as_double(mon_key(kmax)) : hist_nan();
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double s01 = red.s[r][0][q] + red.s[r][1][q];
            const double s012 = s01 + red.s[r][2][q];
            o[3 + q] = s012 + red.s[r][3][q];
        }
    }
}

// one thread per word of the rows [0, capacity]; the first thread also rewinds the block
__global__ __launch_bounds__(256) void k_monitor_reset_log(HistBlock *blk, double *__restrict__ log, long long capacity,
                                                           long long words)
{
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w == 0) { blk->n = 0; blk->slot = 0; blk->capacity = capacity; }
    if (w < words) log[w] = hist_nan();
}

template <bool VEC>
static void launch_reduce(bool has_w, bool has_x, dim3 grid, hipStream_t st, const MonRegions &R, const MonWeights &W,
                          const double *T, const double *X, const uint8_t *ids, const uint8_t *flags, const unsigned *bricks,
                          long long *partial, const Lay &L, const int *ob)
{
    by_bool(has_w, [&](auto hw) {
        by_bool(has_x, [&](auto hx) {
            hipLaunchKernelGGL((k_monitor_reduce<VEC, decltype(hw)::value, decltype(hx)::value>), grid, dim3(256), 0, st, R, W, T,
                               X, ids, flags, bricks, partial, L, ob[0], ob[1], ob[2]);
            return 0;
        });
        return 0;
    });
}

}  // namespace adi

using namespace adi;

extern "C" {

int adi_monitor_record(const void *d_block, const double *d_T, const double *d_extra, const uint8_t *d_ids,
                       const uint8_t *d_flags, const uint32_t *d_bricks, int nx, int ny, int nz, long plane_stride, int nreg,
                       const int *h_regions, int nprobe, const int *h_probes, const int *d_probes, int nmat,
                       const double *h_weights, double *d_partial, long partial_words, double *d_log, long capacity,
                       void *stream)
{
    ADI_REQUIRE(d_block && d_T && d_flags && d_partial && d_log, "adi_monitor_record: null argument");
    ADI_REQUIRE(nprobe <= 0 || d_probes, "adi_monitor_record: null argument");
    ADI_REQUIRE((const void *)d_log != (const void *)d_T && (const void *)d_partial != (const void *)d_T,
                "adi_monitor_record: the log or the partial buffer aliases T");
    ADI_REQUIRE(d_extra == nullptr || ((const void *)d_log != (const void *)d_extra &&
                                       (const void *)d_partial != (const void *)d_extra),
                "adi_monitor_record: the log or the partial buffer aliases the extra field");
    ADI_REQUIRE(d_log != d_partial, "adi_monitor_record: the log aliases the partial buffer");
    MonWeights W;
    for (int q = 0; q < ADI_MATMAP_MAX; ++q) W.w[q] = 0.0;
    if (d_ids != nullptr) {
        ADI_REQUIRE(h_weights != nullptr, "adi_monitor_record: ids without weights");
        ADI_REQUIRE(nmat >= 1 && nmat <= ADI_MATMAP_MAX, "adi_monitor_record: %d materials (1 to %d)", nmat, ADI_MATMAP_MAX);
        for (int q = 0; q < nmat; ++q) {
            ADI_REQUIRE(isfinite(h_weights[q]), "adi_monitor_record: weight %d is not finite", q);
            W.w[q] = h_weights[q];
        }
    }
    MonPlan P;
    if (int rc = monitor_plan(nx, ny, nz, plane_stride, nreg, h_regions, nprobe, h_probes, partial_words, capacity, &P))
        return rc;
    const dim3 grid((unsigned)P.box_n[2], (unsigned)P.box_n[1], (unsigned)P.box_n[0]);
    const bool vec = pair_vec(P.L, d_flags, d_T, d_extra) && ((uintptr_t)d_ids & 1) == 0;
    if (vec)
        launch_reduce<true>(d_ids != nullptr, d_extra != nullptr, grid, as_stream(stream), P.R, W, d_T, d_extra, d_ids, d_flags,
                            (const unsigned *)d_bricks, (long long *)d_partial, P.L, P.box_lo);
    else
        launch_reduce<false>(d_ids != nullptr, d_extra != nullptr, grid, as_stream(stream), P.R, W, d_T, d_extra, d_ids, d_flags,
                             (const unsigned *)d_bricks, (long long *)d_partial, P.L, P.box_lo);
    ADI_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_monitor_finish, dim3(1), dim3(256), 0, as_stream(stream), P.R, (const HistBlock *)d_block,
                       (const long long *)d_partial, d_T, d_flags, d_probes, nprobe, d_log, (long long)capacity, P.row_words, P.L,
                       d_ids != nullptr ? 1 : 0, d_extra != nullptr ? 1 : 0);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_monitor_reset_log(void *d_block, double *d_log, long capacity, long row_words, void *stream)
{
    ADI_REQUIRE(d_block && d_log, "adi_monitor_reset_log: null argument");
    ADI_REQUIRE(capacity >= 1 && capacity < (1L << 31), "adi_monitor_reset_log: capacity %ld is not in [1, 2^31)", capacity);
    ADI_REQUIRE(row_words >= ADI_MONITOR_REGION_WORDS &&
                row_words <= ADI_MONITOR_MAX_PROBES + ADI_MONITOR_REGION_WORDS * ADI_MONITOR_MAX_REGIONS,
                "adi_monitor_reset_log: a row of %ld words", row_words);
    const long long words = (long long)(capacity + 1) * row_words;
    ADI_REQUIRE((words + 255) / 256 < (1LL << 31), "adi_monitor_reset_log: a log of %lld words is too large", words);
    hipLaunchKernelGGL(k_monitor_reset_log, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, as_stream(stream),
                       (HistBlock *)d_block, d_log, (long long)capacity, words);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // extern "C"
