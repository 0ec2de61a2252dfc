// adi_cyl_extras.hip -- latent heat and thermal history of the cylindrical step (include/adi_hip.h, "Latent heat and thermal
// history of the cylindrical step"): the two passes that follow the three sweeps of adi_cyl.hip, in that backend's conventions.
//   k_cyl_phase_apply      every step: T and f in place, newborn cells seeded from the step's input
//   k_cyl_history_record   every step: T_peak, t_hi, t_lo in place, one row of the log
//   k_cyl_phase_seed, k_cyl_history_seed, k_cyl_history_reset_log   construction, reset, outside edits
// Layout (nr, nphi, nz), z contiguous: blockIdx.y is the radius index, the threads of blockIdx.x walk the (phi, z) plane, one
// thread per PAIR of z-cells with 16-byte loads where nz and the plane stride are even and the arrays 16-byte aligned (W = 2),
// one thread per cell otherwise (W = 1) -- the choice k_cyl_contig's launcher makes.  The unconditional loads of a thread
// (active, T, f / active, B, T_peak) are issued together ahead of the arithmetic; the step's input is loaded only by threads
// that hold a cell which needs it (a newborn; a peak above T_lo).  Stores go cell by cell (8 bytes): T and f only where their
// bits change, the history's values where a rule fires (a newborn's three values always), so a cold region writes nothing.  The pool row of a workgroup is reduced over the wave by shuffles and over the
// four waves through LDS; one thread then issues at most eight integer atomics.  256 threads, no scratch, plain loads and
// stores (the cache policy of adi_cyl.hip: the fields of the loop live in the Infinity Cache).  No existing kernel changes.
// The per-cell functions, the argument checks and the host twins' loops are in adi_cyl_extras_dev.hpp.
#include "adi_cyl_extras_dev.hpp"

namespace adi {

template <int W>
__device__ __forceinline__ void cyl_load(const double *a, long p, double (&v)[W])
{
    if constexpr (W == 2) {
        const double2 x = *reinterpret_cast<const double2 *>(a + p);
        v[0] = x.x; v[1] = x.y;
    } else {
        v[0] = a[p];
    }
}

// bit s: cell s of the thread is active (act == nullptr: every cell)
template <int W>
__device__ __forceinline__ unsigned cyl_load_active(const uint8_t *act, long p)
{
    if (act == nullptr) return (1u << W) - 1u;
    if constexpr (W == 2) {
        const unsigned v = *reinterpret_cast<const unsigned short *>(act + p);
        return ((v & 0xffu) ? 1u : 0u) | ((v >> 8) ? 2u : 0u);
    } else {
        return act[p] != 0 ? 1u : 0u;
    }
}

// the thread's first cell: q-th group of W cells of the plane of radius blockIdx.y
struct CylCell {
    long p;
    int j, k;
    bool in;
};
template <int W>
__device__ __forceinline__ CylCell cyl_cell(const CylBox &g, unsigned per_line, unsigned per_plane)
{
    const unsigned q = blockIdx.x * 256u + threadIdx.x;
    CylCell c;
    c.in = q < per_plane;
    const unsigned j = c.in ? q / per_line : 0u;
    c.j = (int)j;
    c.k = c.in ? (int)(q - j * per_line) * W : 0;
    c.p = (long)blockIdx.y * g.sx + (long)c.j * g.nz + c.k;
    return c;
}

template <int W>
__global__ __launch_bounds__(256) void k_cyl_phase_apply(PhaseLaw w, double *__restrict__ T, double *__restrict__ F,
                                                         const double *__restrict__ Tin, const uint8_t *__restrict__ act,
                                                         CylBox g, unsigned per_line, unsigned per_plane, int skip0, int skipN)
{
#pragma clang fp contract(off)
    const CylCell c = cyl_cell<W>(g, per_line, per_plane);
    if (!c.in) return;
    double t[W], f[W], a[W];
    unsigned m = cyl_load_active<W>(act, c.p);
    cyl_load<W>(T, c.p, t);
    cyl_load<W>(F, c.p, f);
    if (skip0 && c.k == 0) m &= ~1u;
    if (skipN && c.k + W == g.nz) m &= ~(1u << (W - 1));
    bool newborn = false;
#pragma unroll
    for (int s = 0; s < W; ++s) {
        a[s] = 0.0;
        newborn = newborn || (((m >> s) & 1u) && f[s] != f[s]);
    }
    if (Tin != nullptr && newborn) cyl_load<W>(Tin, c.p, a);
#pragma unroll
    for (int s = 0; s < W; ++s) {
        if ((m >> s) & 1u) {
            double tn, fn;
            const unsigned st = cyl_phase_cell(w, t[s], f[s], Tin != nullptr, a[s], tn, fn);
            if (st & kCylStoreT) T[c.p + s] = tn;
            if (st & kCylStoreF) F[c.p + s] = fn;
        }
    }
}

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

template <int W>
__global__ __launch_bounds__(256) void k_cyl_history_record(adi_history_levels w, const HistBlock *__restrict__ blk,
                                                            const double *__restrict__ A, const double *__restrict__ B,
                                                            double *__restrict__ P, double *__restrict__ THI,
                                                            double *__restrict__ TLO, int *__restrict__ log,
                                                            const uint8_t *__restrict__ act, CylBox g, unsigned per_line,
                                                            unsigned per_plane)
{
#pragma clang fp contract(off)
    __shared__ int red[4][5];
    const unsigned tid = threadIdx.x;
    const CylCell c = cyl_cell<W>(g, per_line, per_plane);
    double a[W], b[W], pk[W];
    unsigned m = 0u;
#pragma unroll
    for (int s = 0; s < W; ++s) { a[s] = 0.0; b[s] = 0.0; pk[s] = 0.0; }
    if (c.in) {
        m = cyl_load_active<W>(act, c.p);
        cyl_load<W>(B, c.p, b);
        cyl_load<W>(P, c.p, pk);
    }
    bool need = false;
#pragma unroll
    for (int s = 0; s < W; ++s) need = need || (((m >> s) & 1u) && cyl_history_needs_a(w, pk[s]));
    if (need) cyl_load<W>(A, c.p, a);
    int cnt = 0, jlo = kCylHistEmptyLo, jhi = -1, klo = kCylHistEmptyLo, khi = -1;
    if (m) {
        const HistBlock clk = *blk;
        const double tn = cyl_history_tn(clk);
#pragma unroll
        for (int s = 0; s < W; ++s) {
            if ((m >> s) & 1u) {
                double peak, thi = 0.0, tlo = 0.0;
                const unsigned st = cyl_history_cell(w, tn, clk.dt, a[s], b[s], pk[s], peak, thi, tlo);
                if (st & kCylStorePeak) P[c.p + s] = peak;
                if (st & kCylStoreHi) THI[c.p + s] = thi;
                if (st & kCylStoreLo) TLO[c.p + s] = tlo;
                if (b[s] >= w.T_melt) {
                    cnt += 1;
                    jlo = c.j; jhi = c.j;
                    klo = min(klo, c.k + s); khi = c.k + s;
                }
            }
        }
    }
    if (__syncthreads_or(cnt != 0 ? 1 : 0)) {                // (uniform over the workgroup)
        cnt = (int)wave_add((unsigned)cnt);
        jlo = wave_min(jlo); klo = wave_min(klo);
        jhi = wave_max(jhi); khi = wave_max(khi);
        if ((tid & 63u) == 0u) {
            int *r = red[tid >> 6];
            r[0] = cnt; r[1] = jlo; r[2] = klo; r[3] = jhi; r[4] = khi;
        }
        __syncthreads();
        if (tid == 0u) {
            cnt = red[0][0] + red[1][0] + red[2][0] + red[3][0];
            jlo = min(min(red[0][1], red[1][1]), min(red[2][1], red[3][1]));
            klo = min(min(red[0][2], red[1][2]), min(red[2][2], red[3][2]));
            jhi = max(max(red[0][3], red[1][3]), max(red[2][3], red[3][3]));
            khi = max(max(red[0][4], red[1][4]), max(red[2][4], red[3][4]));
            const int i = (int)blockIdx.y;                   // one radius per workgroup: lo_i = hi_i = i, sum_i = i * cells
            const long long slot = blk->slot, cap = blk->capacity;
            int *r = log + (slot < cap ? slot : cap) * ADI_CYL_HISTORY_LOG_INTS;
            atomicAdd(r, cnt);
            atomicMin(r + 1, i);
            atomicMin(r + 2, jlo);
            atomicMin(r + 3, klo);
            atomicMax(r + 4, i);
            atomicMax(r + 5, jhi);
            atomicMax(r + 6, khi);
            if (i != 0) atomicAdd(reinterpret_cast<unsigned long long *>(r + 8), (unsigned long long)i * (unsigned long long)cnt);
        }
    }
}

// f = f_eq(T) on the active cells sel selects, NaN on inactive cells; one thread per cell
__global__ __launch_bounds__(256) void k_cyl_phase_seed(PhaseLaw w, const double *__restrict__ T, double *__restrict__ F,
                                                        const uint8_t *__restrict__ act, const uint8_t *__restrict__ sel,
                                                        CylBox g, unsigned per_line, unsigned per_plane)
{
#pragma clang fp contract(off)
    const CylCell c = cyl_cell<1>(g, per_line, per_plane);
    if (!c.in) return;
    if (act != nullptr && act[c.p] == 0) {
        F[c.p] = cyl_nan();
    } else if (sel == nullptr || sel[c.p] != 0) {
        const double e = T[c.p] - w.Ts;
        F[c.p] = cyl_clamp01(e / w.dT);
    }
}

// T_peak = T, times NaN on the active cells sel selects, all three NaN on inactive cells; one thread per cell
__global__ __launch_bounds__(256) void k_cyl_history_seed(const double *__restrict__ T, double *__restrict__ P,
                                                          double *__restrict__ THI, double *__restrict__ TLO,
                                                          const uint8_t *__restrict__ act, const uint8_t *__restrict__ sel,
                                                          CylBox g, unsigned per_line, unsigned per_plane)
{
    const CylCell c = cyl_cell<1>(g, per_line, per_plane);
    if (!c.in) return;
    const double nan = cyl_nan();
    if (act != nullptr && act[c.p] == 0) {
        P[c.p] = nan; THI[c.p] = nan; TLO[c.p] = nan;
    } else if (sel == nullptr || sel[c.p] != 0) {
        P[c.p] = T[c.p]; THI[c.p] = nan; TLO[c.p] = nan;
    }
}

// rows [0, capacity] of the log empty, one thread per row; the first thread also rewinds the block
__global__ __launch_bounds__(256) void k_cyl_history_reset_log(HistBlock *blk, int *__restrict__ log, long long capacity)
{
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row == 0) { blk->n = 0; blk->slot = 0; blk->capacity = capacity; }
    if (row > capacity) return;
    int *r = log + row * ADI_CYL_HISTORY_LOG_INTS;
    r[0] = 0;
    r[1] = kCylHistEmptyLo; r[2] = kCylHistEmptyLo; r[3] = kCylHistEmptyLo;
    r[4] = -1; r[5] = -1; r[6] = -1;
    r[7] = 0; r[8] = 0; r[9] = 0; r[10] = 0; r[11] = 0;
}

// the launch geometry of a box for W cells per thread
struct CylExtrasLaunch {
    unsigned per_line, per_plane;
    dim3 grid;
};
static CylExtrasLaunch cyl_extras_launch(const CylBox &g, int W)
{
    CylExtrasLaunch l;
    l.per_line = (unsigned)(g.nz / W);
    l.per_plane = l.per_line * (unsigned)g.nphi;
    l.grid = dim3((l.per_plane + 255u) / 256u, (unsigned)g.nr);
    return l;
}

// 16-byte access: even nz and plane stride (a pair then never straddles a row and starts at an even offset), arrays aligned
template <class... P>
static bool cyl_pair_vec(const CylBox &g, const uint8_t *act, const P *...arrays)
{
    const uintptr_t bits = (... | (uintptr_t)arrays);
    return g.nz % 2 == 0 && g.sx % 2 == 0 && (bits & 15u) == 0 && ((uintptr_t)act & 1u) == 0;
}

}  // namespace adi

using namespace adi;

extern "C" {

int adi_cyl_phase_apply(const adi_phase_change *h_law, double cp, double *d_T, double *d_f, const double *d_T_in,
                        const uint8_t *d_active, int skip_k0, int skip_kN, int nr, int nphi, int nz, long plane_stride,
                        void *stream)
{
    PhaseLaw w;
    CylBox g;
    if (int rc = check_cyl_phase_apply("adi_cyl_phase_apply", h_law, cp, d_T, d_f, d_T_in, d_active, nr, nphi, nz, plane_stride,
                                       &w, &g))
        return rc;
    if (cyl_pair_vec(g, d_active, d_T, d_f, d_T_in)) {
        const CylExtrasLaunch l = cyl_extras_launch(g, 2);
        hipLaunchKernelGGL(k_cyl_phase_apply<2>, l.grid, dim3(256), 0, as_stream(stream), w, d_T, d_f, d_T_in, d_active, g,
                           l.per_line, l.per_plane, skip_k0 != 0, skip_kN != 0);
    } else {
        const CylExtrasLaunch l = cyl_extras_launch(g, 1);
        hipLaunchKernelGGL(k_cyl_phase_apply<1>, l.grid, dim3(256), 0, as_stream(stream), w, d_T, d_f, d_T_in, d_active, g,
                           l.per_line, l.per_plane, skip_k0 != 0, skip_kN != 0);
    }
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_cyl_phase_apply_host(const adi_phase_change *h_law, double cp, double *h_T, double *h_f, const double *h_T_in,
                             const uint8_t *h_active, int skip_k0, int skip_kN, int nr, int nphi, int nz, long plane_stride)
{
    PhaseLaw w;
    CylBox g;
    if (int rc = check_cyl_phase_apply("adi_cyl_phase_apply_host", h_law, cp, h_T, h_f, h_T_in, h_active, nr, nphi, nz,
                                       plane_stride, &w, &g))
        return rc;
    cyl_phase_apply_host(w, g, h_T, h_f, h_T_in, h_active, skip_k0 != 0, skip_kN != 0);
    return ADI_OK;
}

int adi_cyl_phase_seed(const adi_phase_change *h_law, const double *d_T, double *d_f, const uint8_t *d_active,
                       const uint8_t *d_sel, int nr, int nphi, int nz, long plane_stride, void *stream)
{
    ADI_REQUIRE(h_law && d_T && d_f, "adi_cyl_phase_seed: null argument");
    ADI_REQUIRE(d_T != d_f, "adi_cyl_phase_seed: d_f aliases d_T");
    PhaseLaw w;
    if (int rc = make_phase_law("adi_cyl_phase_seed", *h_law, 1.0, &w)) return rc;
    CylBox g;
    if (int rc = make_cyl_box("adi_cyl_phase_seed", nr, nphi, nz, plane_stride, &g)) return rc;
    const CylExtrasLaunch l = cyl_extras_launch(g, 1);
    hipLaunchKernelGGL(k_cyl_phase_seed, l.grid, dim3(256), 0, as_stream(stream), w, d_T, d_f, d_active, d_sel, g, l.per_line,
                       l.per_plane);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_cyl_history_record(const adi_history_levels *h_levels, const void *d_block, const double *d_T_in,
                           const double *d_T_out, double *d_peak, double *d_t_hi, double *d_t_lo, int32_t *d_log,
                           const uint8_t *d_active, int nr, int nphi, int nz, long plane_stride, void *stream)
{
    CylBox g;
    if (int rc = check_cyl_history_record("adi_cyl_history_record", h_levels, d_block, d_T_in, d_T_out, d_peak, d_t_hi, d_t_lo,
                                          d_log, nr, nphi, nz, plane_stride, &g))
        return rc;
    const HistBlock *blk = (const HistBlock *)d_block;
    if (cyl_pair_vec(g, d_active, d_T_in, d_T_out, (const double *)d_peak)) {
        const CylExtrasLaunch l = cyl_extras_launch(g, 2);
        hipLaunchKernelGGL(k_cyl_history_record<2>, l.grid, dim3(256), 0, as_stream(stream), *h_levels, blk, d_T_in, d_T_out,
                           d_peak, d_t_hi, d_t_lo, (int *)d_log, d_active, g, l.per_line, l.per_plane);
    } else {
        const CylExtrasLaunch l = cyl_extras_launch(g, 1);
        hipLaunchKernelGGL(k_cyl_history_record<1>, l.grid, dim3(256), 0, as_stream(stream), *h_levels, blk, d_T_in, d_T_out,
                           d_peak, d_t_hi, d_t_lo, (int *)d_log, d_active, g, l.per_line, l.per_plane);
    }
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_cyl_history_record_host(const adi_history_levels *h_levels, const void *h_block, const double *h_T_in,
                                const double *h_T_out, double *h_peak, double *h_t_hi, double *h_t_lo, int32_t *h_log,
                                const uint8_t *h_active, int nr, int nphi, int nz, long plane_stride)
{
    CylBox g;
    if (int rc = check_cyl_history_record("adi_cyl_history_record_host", h_levels, h_block, h_T_in, h_T_out, h_peak, h_t_hi,
                                          h_t_lo, h_log, nr, nphi, nz, plane_stride, &g))
        return rc;
    HistBlock blk;
    memcpy(&blk, h_block, sizeof(blk));
    ADI_REQUIRE(blk.slot >= 0 && blk.capacity >= 1 && isfinite(blk.t0) && isfinite(blk.dt),
                "adi_cyl_history_record_host: bad block");
    cyl_history_record_host(*h_levels, g, blk, h_T_in, h_T_out, h_peak, h_t_hi, h_t_lo, h_log, h_active);
    return ADI_OK;
}

int adi_cyl_history_seed(const double *d_T, double *d_peak, double *d_t_hi, double *d_t_lo, const uint8_t *d_active,
                         const uint8_t *d_sel, int nr, int nphi, int nz, long plane_stride, void *stream)
{
    ADI_REQUIRE(d_T && d_peak && d_t_hi && d_t_lo, "adi_cyl_history_seed: null argument");
    ADI_REQUIRE(d_peak != d_T && d_t_hi != d_T && d_t_lo != d_T, "adi_cyl_history_seed: a state array aliases T");
    ADI_REQUIRE(d_peak != d_t_hi && d_peak != d_t_lo && d_t_hi != d_t_lo, "adi_cyl_history_seed: the state arrays alias");
    CylBox g;
    if (int rc = make_cyl_box("adi_cyl_history_seed", nr, nphi, nz, plane_stride, &g)) return rc;
    const CylExtrasLaunch l = cyl_extras_launch(g, 1);
    hipLaunchKernelGGL(k_cyl_history_seed, l.grid, dim3(256), 0, as_stream(stream), d_T, d_peak, d_t_hi, d_t_lo, d_active,
                       d_sel, g, l.per_line, l.per_plane);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_cyl_history_reset_log(void *d_block, int32_t *d_log, long capacity, void *stream)
{
    ADI_REQUIRE(d_block && d_log, "adi_cyl_history_reset_log: null argument");
    ADI_REQUIRE(capacity >= 1 && capacity < (1L << 31), "adi_cyl_history_reset_log: capacity %ld is not in [1, 2^31)", capacity);
    const unsigned nb = (unsigned)((capacity + 1 + 255) / 256);
    hipLaunchKernelGGL(k_cyl_history_reset_log, dim3(nb), dim3(256), 0, as_stream(stream), (HistBlock *)d_block, (int *)d_log,
                       (long long)capacity);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // extern "C"
