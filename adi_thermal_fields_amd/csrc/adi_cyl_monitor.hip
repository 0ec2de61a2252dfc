// adi_cyl_monitor.hip -- the field monitor of the cylindrical step (include/adi_hip.h, "Field monitor of the cylindrical step"):
// after a step, the value of the final field at up to 256 probe cells and, over the active cells of up to 8 index boxes whose
// phi range may wrap the seam, the count, the sum of the radial index, the extrema and the sums of T, r T, a second field and
// r times it -- one row of a device log per recorded step.
//   k_cyl_monitor_chunks   the launch geometry of adi_cyl_extras.hip: blockIdx.y a radius, 256 threads one chunk of 256 pairs of
//                          the (phi, z) plane, one 16-byte load per pair where nz, the plane stride and the alignment allow it,
//                          two 8-byte loads with the same arithmetic otherwise; `active` first, T and the second field only by
//                          threads that hold an active cell; one record per region the chunk can meet
//   k_cyl_monitor_planes   one workgroup per (region, radius): the chunk records of the plane in their defined order -> S_i
//   k_cyl_monitor_finish   one workgroup: thread r adds the S_i of region r in increasing i (r_i S_i formed first for the
//                          weighted sums), every thread below nprobe reads a probe; the row at the block's slot
//   k_cyl_monitor_reset_log   every word of the log NaN, the block rewound
// Only the radii and chunks a region meets are launched.  The order of every sum is written down in the header and in
// CylFieldMonitor.record_reference; nothing here may depart from it.  Sums travel over the wave by xor-butterfly and over the
// four waves through LDS in wave order; the extrema are taken on integer keys, so they depend on no order.  No atomics: every
// record a later kernel reads is rewritten by every record launch.  Plain loads and stores, contraction off.
#include "adi_cyl_monitor_dev.hpp"

namespace adi {

__device__ __forceinline__ long long cm_shfl_xor_ll(long long v, int o)
{
    const int lo = __shfl_xor((int)(v & 0xffffffffLL), o), hi = __shfl_xor((int)(v >> 32), o);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}
__device__ __forceinline__ double cm_wave_sum(double v)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int o = 1; o <= 32; o <<= 1) v = v + __longlong_as_double(cm_shfl_xor_ll(__double_as_longlong(v), o));
    return v;
}
__device__ __forceinline__ long long cm_wave_min(long long v)
{
#pragma unroll
    for (int o = 1; o <= 32; o <<= 1) { const long long u = cm_shfl_xor_ll(v, o); v = u < v ? u : v; }
    return v;
}
__device__ __forceinline__ long long cm_wave_max(long long v)
{
#pragma unroll
    for (int o = 1; o <= 32; o <<= 1) { const long long u = cm_shfl_xor_ll(v, o); v = u > v ? u : v; }
    return v;
}

struct CylMonShared {
    double s[kCylMonRegions][4][2];
    long long k[kCylMonRegions][4][2];
    long long c[kCylMonRegions][4];
};

// ((w0 + w1) + w2) + w3 of quantity q of region r
__device__ __forceinline__ double cm_waves(const CylMonShared &red, int r, int q)
{
#pragma clang fp contract(off)
    const double s01 = red.s[r][0][q] + red.s[r][1][q];
    const double s012 = s01 + red.s[r][2][q];
    return s012 + red.s[r][3][q];
}

// the record of (region r, record n of np): SoA over the five words
__device__ __forceinline__ void cm_store(long long *__restrict__ o, long np, long n, const CylMonShared &red, int r, bool has_x)
{
    o[n] = __double_as_longlong(cm_waves(red, r, 0));
    o[np + n] = __double_as_longlong(has_x ? cm_waves(red, r, 1) : 0.0);
    long long kmin = red.k[r][0][0], kmax = red.k[r][0][1], cnt = red.c[r][0];
#pragma unroll
    for (int wv = 1; wv < 4; ++wv) {
        kmin = red.k[r][wv][0] < kmin ? red.k[r][wv][0] : kmin;
        kmax = red.k[r][wv][1] > kmax ? red.k[r][wv][1] : kmax;
        cnt += red.c[r][wv];
    }
    o[2 * np + n] = kmin; o[3 * np + n] = kmax; o[4 * np + n] = cnt;
}

template <bool VEC, bool HAS_X>
__global__ __launch_bounds__(256) void k_cyl_monitor_chunks(CylMonRegions R, const double *__restrict__ T,
                                                            const double *__restrict__ X, const uint8_t *__restrict__ act,
                                                            long long *__restrict__ partial, CylBox g, unsigned per_line,
                                                            unsigned per_plane, unsigned nchunk, int ilo, int clo)
{
#pragma clang fp contract(off)
    __shared__ CylMonShared red;
    const unsigned tid = threadIdx.x;
    const int c = (int)blockIdx.x + clo, i = (int)blockIdx.y + ilo;
    unsigned meet = 0u;                                   // bit r: region r holds radius i and can meet chunk c (uniform)
    for (int r = 0; r < R.n; ++r) meet |= ((i >= R.i0[r] && i < R.i1[r] && cyl_mon_meets(R, r, c)) ? 1u : 0u) << r;
    if (meet == 0u) return;
    const CylMonPair pr = cyl_mon_pair((unsigned)c * 256u + tid, per_line, per_plane, g.nz);
    const long p = (long)i * g.sx + (long)pr.j * g.nz + pr.k;
    unsigned m = pr.in;
    if (act != nullptr && pr.in) {
        if (VEC) {
            const unsigned v = *reinterpret_cast<const unsigned short *>(act + p);
            m = ((v & 0xffu) ? 1u : 0u) | ((v >> 8) ? 2u : 0u);
        } else {
            m = act[p] != 0 ? 1u : 0u;
            if ((pr.in & 2u) && act[p + 1] != 0) m |= 2u;
        }
    }
    double t0 = 0.0, t1 = 0.0, x0 = 0.0, x1 = 0.0;
    if (m) {
        if (VEC) {
            const double2 v = *reinterpret_cast<const double2 *>(T + p);
            t0 = v.x; t1 = v.y;
            if (HAS_X) { const double2 w = *reinterpret_cast<const double2 *>(X + p); x0 = w.x; x1 = w.y; }
        } else {
            t0 = T[p];
            if (pr.in & 2u) t1 = T[p + 1];
            if (HAS_X) { x0 = X[p]; if (pr.in & 2u) x1 = X[p + 1]; }
        }
    }
    for (int r = 0; r < R.n; ++r) {
        if (!((meet >> r) & 1u)) continue;                // (uniform)
        const unsigned inc = cyl_mon_member(R, r, g.nphi, pr.j, pr.k, m);
        const CylMonTerm e = cyl_mon_term(inc, t0, t1, HAS_X, x0, x1);
        const double sT = cm_wave_sum(e.sT);
        double sX = 0.0;
        if (HAS_X) sX = cm_wave_sum(e.sX);
        const long long kmin = cm_wave_min(e.kmin), kmax = cm_wave_max(e.kmax);
        const unsigned cnt = wave_add(e.cnt);
        if ((tid & 63u) == 0u) {
            const unsigned wv = tid >> 6;
            red.s[r][wv][0] = sT; red.s[r][wv][1] = sX;
            red.k[r][wv][0] = kmin; red.k[r][wv][1] = kmax;
            red.c[r][wv] = (long long)cnt;
        }
    }
    __syncthreads();
    if (tid != 0u) return;
    for (int r = 0; r < R.n; ++r) {
        if (!((meet >> r) & 1u)) continue;
        const long np = (long)(R.i1[r] - R.i0[r]) * nchunk;
        cm_store(partial + kCylMonWords * R.off[r], np, (long)(i - R.i0[r]) * nchunk + c, red, r, HAS_X);
    }
}

// blockIdx.y the region, blockIdx.x the radius of the region: thread t adds the chunk records t, t + 256, ... from +0.0
__global__ __launch_bounds__(256) void k_cyl_monitor_planes(CylMonRegions R, long long *__restrict__ partial, long chunk_records,
                                                            unsigned nchunk, int has_x)
{
#pragma clang fp contract(off)
    __shared__ CylMonShared red;
    const unsigned tid = threadIdx.x;
    const int r = (int)blockIdx.y, ii = (int)blockIdx.x;
    const int ni = R.i1[r] - R.i0[r];
    if (ii >= ni) return;
    const long np = (long)ni * nchunk;
    const long long *p = partial + kCylMonWords * R.off[r] + (long)ii * nchunk;
    double sT = 0.0, sX = 0.0;
    long long kmin = kCylMonKeyMax, kmax = -kCylMonKeyMax - 1, cnt = 0;
    for (unsigned n = tid; n < nchunk; n += 256u) {
        if (!cyl_mon_meets(R, r, (int)n)) continue;       // (never written: +0.0, which keeps the bits of a sum that is never -0.0)
        sT = sT + __longlong_as_double(p[n]);
        if (has_x) sX = sX + __longlong_as_double(p[np + n]);
        const long long a = p[2 * np + n], b = p[3 * np + n];
        kmin = a < kmin ? a : kmin; kmax = b > kmax ? b : kmax;
        cnt += p[4 * np + n];
    }
    sT = cm_wave_sum(sT);
    sX = cm_wave_sum(sX);
    kmin = cm_wave_min(kmin);
    kmax = cm_wave_max(kmax);
#pragma unroll
    for (int o = 1; o <= 32; o <<= 1) cnt += cm_shfl_xor_ll(cnt, o);
    if ((tid & 63u) == 0u) {
        const unsigned wv = tid >> 6;
        red.s[0][wv][0] = sT; red.s[0][wv][1] = sX;
        red.k[0][wv][0] = kmin; red.k[0][wv][1] = kmax;
        red.c[0][wv] = cnt;
    }
    __syncthreads();
    if (tid != 0u) return;
    cm_store(partial + kCylMonWords * chunk_records + kCylMonWords * R.poff[r], ni, ii, red, 0, has_x != 0);
}

__global__ __launch_bounds__(256) void k_cyl_monitor_finish(CylMonRegions R, const HistBlock *__restrict__ blk,
                                                            const long long *__restrict__ planes, const double *__restrict__ T,
                                                            const uint8_t *__restrict__ act, const int *__restrict__ probes,
                                                            int nprobe, double *__restrict__ log, long long capacity,
                                                            long row_words, CylBox g, double r_in, double dr)
{
#pragma clang fp contract(off)
    const unsigned tid = threadIdx.x;
    long long cap = blk->capacity;
    cap = (cap >= 1 && cap < capacity) ? cap : capacity;  // (the log was sized for `capacity`: never a row beyond it)
    long long slot = blk->slot;
    slot = slot < 0 ? 0 : slot;
    double *__restrict__ row = log + (slot < cap ? slot : cap) * row_words;
    if ((int)tid < nprobe) {
        const int i = probes[3 * tid], j = probes[3 * tid + 1], k = probes[3 * tid + 2];
        double v = cyl_nan();
        if (i >= 0 && i < g.nr && j >= 0 && j < g.nphi && k >= 0 && k < g.nz) {
            const long p = (long)i * g.sx + (long)j * g.nz + k;
            if (act == nullptr || act[p] != 0) v = T[p];
        }
        row[tid] = v;
    }
    if ((int)tid >= R.n) return;
    const int r = (int)tid, ni = R.i1[r] - R.i0[r];
    const long long *p = planes + kCylMonWords * R.poff[r];
    CylMonTotal tot;
    cyl_mon_total_init(tot);
    for (int ii = 0; ii < ni; ++ii)
        cyl_mon_total_add(tot, r_in, dr, R.i0[r] + ii, __longlong_as_double(p[ii]), __longlong_as_double(p[ni + ii]),
                          p[2 * ni + ii], p[3 * ni + ii], p[4 * ni + ii]);
    cyl_mon_total_store(tot, row + nprobe + ADI_CYL_MONITOR_REGION_WORDS * r);
}

// one thread per word of the rows [0, capacity]; the first thread also rewinds the block
__global__ __launch_bounds__(256) void k_cyl_monitor_reset_log(HistBlock *blk, double *__restrict__ log, long long capacity,
                                                               long long words)
{
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w == 0) { blk->n = 0; blk->slot = 0; blk->capacity = capacity; }
    if (w < words) log[w] = cyl_nan();
}

static int check_cyl_monitor_arrays(const char *who, const void *block, const double *T, const double *extra, const double *log)
{
    ADI_REQUIRE(block && T && log, "%s: null argument", who);
    ADI_REQUIRE(((uintptr_t)log & 7u) == 0 && ((uintptr_t)block & 7u) == 0, "%s: block or log not 8-byte aligned", who);
    ADI_REQUIRE((const void *)log != (const void *)T && (extra == nullptr || (const void *)log != (const void *)extra),
                "%s: the log aliases T or the extra field", who);
    return ADI_OK;
}

}  // namespace adi

using namespace adi;

extern "C" {

int adi_cyl_monitor_record(const void *d_block, const double *d_T, const double *d_extra, const uint8_t *d_active, int nr,
                           int nphi, int nz, long plane_stride, double r_in, double dr, int nreg, const int *h_regions,
                           int nprobe, const int *h_probes, const int *d_probes, double *d_partial, long partial_words,
                           double *d_log, long capacity, void *stream)
{
    const char *who = "adi_cyl_monitor_record";
    if (int rc = check_cyl_monitor_arrays(who, d_block, d_T, d_extra, d_log)) return rc;
    ADI_REQUIRE(d_partial != nullptr && (nprobe <= 0 || d_probes != nullptr), "%s: null argument", who);
    ADI_REQUIRE((const void *)d_partial != (const void *)d_T && (const void *)d_partial != (const void *)d_extra &&
                d_partial != d_log, "%s: the partial buffer aliases T, the extra field or the log", who);
    CylMonPlan P;
    if (int rc = cyl_monitor_plan(who, nr, nphi, nz, plane_stride, r_in, dr, nreg, h_regions, nprobe, h_probes, capacity, &P))
        return rc;
    const long need = cyl_monitor_words(P.chunk_records, P.plane_records);
    ADI_REQUIRE(partial_words >= need, "%s: %ld words of partials, %ld needed", who, partial_words, need);
    ADI_REQUIRE(P.nc <= 0x7fffffff && P.ni <= 65535, "%s: launch box too large", who);
    hipStream_t st = as_stream(stream);
    long long *partial = (long long *)d_partial;
    const dim3 grid((unsigned)P.nc, (unsigned)P.ni);
    // 16-byte access: even nz and plane stride (a pair then never straddles a row and starts at an even offset), arrays aligned
    const bool vec = P.g.nz % 2 == 0 && P.g.sx % 2 == 0 && (((uintptr_t)d_T | (uintptr_t)d_extra) & 15u) == 0 &&
                     ((uintptr_t)d_active & 1u) == 0;
    by_bool(vec, [&](auto v) {
        by_bool(d_extra != nullptr, [&](auto hx) {
            hipLaunchKernelGGL((k_cyl_monitor_chunks<decltype(v)::value, decltype(hx)::value>), grid, dim3(256), 0, st, P.R, d_T,
                               d_extra, d_active, partial, P.g, P.per_line, P.per_plane, P.nchunk, P.ilo, P.clo);
            return 0;
        });
        return 0;
    });
    ADI_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_cyl_monitor_planes, dim3((unsigned)P.max_ni, (unsigned)nreg), dim3(256), 0, st, P.R, partial,
                       P.chunk_records, P.nchunk, d_extra != nullptr ? 1 : 0);
    ADI_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_cyl_monitor_finish, dim3(1), dim3(256), 0, st, P.R, (const HistBlock *)d_block,
                       (const long long *)(partial + kCylMonWords * P.chunk_records), d_T, d_active, d_probes, nprobe, d_log,
                       (long long)capacity, P.row_words, P.g, r_in, dr);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_cyl_monitor_record_host(const void *h_block, const double *h_T, const double *h_extra, const uint8_t *h_active, int nr,
                                int nphi, int nz, long plane_stride, double r_in, double dr, int nreg, const int *h_regions,
                                int nprobe, const int *h_probes, double *h_log, long capacity)
{
    const char *who = "adi_cyl_monitor_record_host";
    if (int rc = check_cyl_monitor_arrays(who, h_block, h_T, h_extra, h_log)) return rc;
    CylMonPlan P;
    if (int rc = cyl_monitor_plan(who, nr, nphi, nz, plane_stride, r_in, dr, nreg, h_regions, nprobe, h_probes, capacity, &P))
        return rc;
    HistBlock blk;
    memcpy(&blk, h_block, sizeof(blk));
    long long cap = (blk.capacity >= 1 && blk.capacity < capacity) ? blk.capacity : capacity;
    const long long slot = blk.slot < 0 ? 0 : blk.slot;
    cyl_monitor_record_host(P, r_in, dr, h_T, h_extra, h_active, nprobe, h_probes, h_log + (slot < cap ? slot : cap) * P.row_words);
    return ADI_OK;
}

int adi_cyl_monitor_reset_log(void *d_block, double *d_log, long capacity, long row_words, void *stream)
{
    ADI_REQUIRE(d_block && d_log, "adi_cyl_monitor_reset_log: null argument");
    ADI_REQUIRE(capacity >= 1 && capacity < (1L << 31), "adi_cyl_monitor_reset_log: capacity %ld is not in [1, 2^31)", capacity);
    ADI_REQUIRE(row_words >= ADI_CYL_MONITOR_REGION_WORDS &&
                row_words <= ADI_MONITOR_MAX_PROBES + ADI_CYL_MONITOR_REGION_WORDS * ADI_MONITOR_MAX_REGIONS,
                "adi_cyl_monitor_reset_log: a row of %ld words", row_words);
    const long long words = (long long)(capacity + 1) * row_words;
    ADI_REQUIRE((words + 255) / 256 < (1LL << 31), "adi_cyl_monitor_reset_log: a log of %lld words is too large", words);
    hipLaunchKernelGGL(k_cyl_monitor_reset_log, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, as_stream(stream),
                       (HistBlock *)d_block, d_log, (long long)capacity, words);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // extern "C"
