// adi_cyl_solid.hip -- the conditions at the freezing front of the cylindrical step (include/adi_hip.h, "Solidification record
// of the cylindrical step"): for a cell that drops through T_freeze in the step A -> B, the crossing time, the cooling rate and
// the squared thermal gradient at the crossing time; per step one row of the front's log; per tile one hot word.
//   k_cyl_solid_record     every step: t_solid, cooling_rate, g2 of the cells that freeze in it, the front row, the tile's word
//   k_cyl_solid_hot_seed   the word of every tile from a field
// Layout (nr, nphi, nz), z contiguous: blockIdx.y is the radius index, the workgroup blockIdx.x of 256 threads owns the tile of
// the 512 consecutive cells p = j*nz + k in [512 q, 512 q + 512) of that radius' plane, thread t the cells 512 q + 2 t and the
// next one -- whatever the load form.  Loads are 16 bytes under cyl_pair_vec (even nz and plane stride, aligned arrays) and 8
// bytes otherwise.  `active` and B are loaded unconditionally and together; A only by a thread one of whose active cells has
// B <= T_f (exact: only such a cell can freeze); the up to six neighbours of A, B and `active` only by a thread that holds a
// freezing cell, from global memory, whichever tile they lie in.  That part diverges and is accepted: the front is a surface.
// Stores only where a cell freezes (3 x 8 bytes).  A workgroup whose hot word is clear stops after `active` and B.  The front
// row is reduced over the wave by shuffles and over the four waves through LDS, entered only when some cell of the tile froze;
// one thread then issues at most eight integer atomics.  No scratch, plain loads and stores.
// The per-cell function, the argument checks and the host twins' loops are in adi_cyl_solid_dev.hpp.
#include "adi_cyl_solid_dev.hpp"

namespace adi {

// the thread's two cells pl, pl + 1 of the plane as values v[0], v[1]; a cell past the plane reads 0
template <bool VEC>
__device__ __forceinline__ void solid_load(const double *__restrict__ a, long base, long pl, long npl, double (&v)[2])
{
    if constexpr (VEC) {                                  // (npl is even: the pair is inside the plane or outside it)
        const double2 x = *reinterpret_cast<const double2 *>(a + base + pl);
        v[0] = x.x; v[1] = x.y;
    } else {
        v[0] = a[base + pl];
        v[1] = pl + 1 < npl ? a[base + pl + 1] : 0.0;
    }
}

// bit s: cell pl + s is inside the plane and active (act == nullptr: every cell)
template <bool VEC>
__device__ __forceinline__ unsigned solid_load_active(const uint8_t *__restrict__ act, long base, long pl, long npl)
{
    const unsigned in = pl + 1 < npl ? 3u : 1u;
    if (act == nullptr) return in;
    if constexpr (VEC) {
        const unsigned v = *reinterpret_cast<const unsigned short *>(act + base + pl);
        return ((v & 0xffu) ? 1u : 0u) | ((v >> 8) ? 2u : 0u);
    } else {
        unsigned m = act[base + pl] != 0 ? 1u : 0u;
        if (in & 2u) m |= act[base + pl + 1] != 0 ? 2u : 0u;
        return m;
    }
}

__device__ __forceinline__ int solid_wave_min(int v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int solid_wave_max(int v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_cyl_solid_record(CylSolidScal w, const HistBlock *__restrict__ blk,
                                                          const double *__restrict__ A, const double *__restrict__ B,
                                                          double *__restrict__ TS, double *__restrict__ CR,
                                                          double *__restrict__ G2, int *__restrict__ log,
                                                          const uint8_t *__restrict__ act, int *__restrict__ hot, CylBox g, long npl)
{
#pragma clang fp contract(off)
    __shared__ int red[4][5];
    const unsigned tid = threadIdx.x;
    const int i = (int)blockIdx.y;
    const long base = (long)i * g.sx;
    const long pl = (long)blockIdx.x * kCylSolidTile + 2 * (long)tid;
    const long word = (long)i * (long)gridDim.x + blockIdx.x;
    const int was = hot != nullptr ? hot[word] : 1;       // (every thread reads it ahead of the barrier below)
    unsigned m = 0u;
    double a[2] = {0.0, 0.0}, b[2] = {0.0, 0.0};
    if (pl < npl) {
        m = solid_load_active<VEC>(act, base, pl, npl);
        solid_load<VEC>(B, base, pl, npl, b);
    }
    const bool cold0 = !(m & 1u) || !(b[0] <= w.T_f), cold1 = !(m & 2u) || !(b[1] <= w.T_f);
    if (hot != nullptr) {
        const bool above = ((m & 1u) && b[0] > w.T_f) || ((m & 2u) && b[1] > w.T_f);
        const int now = __syncthreads_or(above ? 1 : 0) ? 1 : 0;
        if (tid == 0u && now != was) hot[word] = now;
        if (was == 0) return;                             // (uniform over the workgroup)
    }
    if (!(cold0 && cold1)) solid_load<VEC>(A, base, pl, npl, a);
    const unsigned fm = ((!cold0 && a[0] > w.T_f) ? 1u : 0u) | ((!cold1 && a[1] > w.T_f) ? 2u : 0u);
    int cnt = 0, jlo = kCylHistEmptyLo, jhi = -1, klo = kCylHistEmptyLo, khi = -1;
    if (fm) {
        const HistBlock clk = *blk;
        const double tn = cyl_history_tn(clk);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if ((fm >> s) & 1u) {
                const unsigned ps = (unsigned)(pl + s);   // (< 2^31: make_cyl_box)
                const int j = (int)(ps / (unsigned)g.nz), k = (int)(ps - (unsigned)j * (unsigned)g.nz);
                double tc, cr, g2;
                cyl_solid_cell(w, g, tn, clk.dt, A, B, act, i, j, k, a[s], b[s], tc, cr, g2);
                const long p = base + pl + s;
                TS[p] = tc; CR[p] = cr; G2[p] = g2;
                cnt += 1;
                jlo = min(jlo, j); jhi = max(jhi, j);
                klo = min(klo, k); khi = max(khi, k);
            }
        }
    }
    if (__syncthreads_or(cnt != 0 ? 1 : 0)) {             // (uniform over the workgroup)
        cnt = (int)wave_add((unsigned)cnt);
        jlo = solid_wave_min(jlo); klo = solid_wave_min(klo);
        jhi = solid_wave_max(jhi); khi = solid_wave_max(khi);
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
            const long long slot = blk->slot, cap = blk->capacity;   // one radius per workgroup: lo_i = hi_i = i
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

template <bool VEC>
__global__ __launch_bounds__(256) void k_cyl_solid_hot_seed(double T_f, const double *__restrict__ T,
                                                            const uint8_t *__restrict__ act, int *__restrict__ hot, CylBox g,
                                                            long npl)
{
    const unsigned tid = threadIdx.x;
    const long base = (long)blockIdx.y * g.sx;
    const long pl = (long)blockIdx.x * kCylSolidTile + 2 * (long)tid;
    unsigned m = 0u;
    double t[2] = {0.0, 0.0};
    if (pl < npl) {
        m = solid_load_active<VEC>(act, base, pl, npl);
        solid_load<VEC>(T, base, pl, npl, t);
    }
    const bool above = ((m & 1u) && t[0] > T_f) || ((m & 2u) && t[1] > T_f);
    const int now = __syncthreads_or(above ? 1 : 0) ? 1 : 0;
    if (tid == 0u) hot[(long)blockIdx.y * (long)gridDim.x + blockIdx.x] = now;
}

// 16-byte access: the conditions of cyl_pair_vec (adi_cyl_extras.hip) -- even nz and plane stride (the plane then holds an even
// number of cells and a pair starts at an even offset), arrays 16-byte aligned, `active` 2-byte aligned
template <class... P>
static bool solid_pair_vec(const CylBox &g, const uint8_t *act, const P *...arrays)
{
    const uintptr_t bits = (... | (uintptr_t)arrays);
    return g.nz % 2 == 0 && g.sx % 2 == 0 && (bits & 15u) == 0 && ((uintptr_t)act & 1u) == 0;
}

static dim3 solid_grid(const CylBox &g) { return dim3((unsigned)cyl_solid_tiles(g), (unsigned)g.nr); }

}  // namespace adi

using namespace adi;

extern "C" {

int adi_cyl_solid_record(double T_freeze, double R_in, double dr, double dphi, double dz, const void *d_block,
                         const double *d_T_in, const double *d_T_out, double *d_t_solid, double *d_rate, double *d_g2,
                         int32_t *d_log, const uint8_t *d_active, int32_t *d_hot, int nr, int nphi, int nz, long plane_stride,
                         void *stream)
{
    CylBox g;
    if (int rc = check_cyl_solid_record("adi_cyl_solid_record", T_freeze, R_in, dr, dphi, dz, d_block, d_T_in, d_T_out, d_t_solid,
                                        d_rate, d_g2, d_log, nr, nphi, nz, plane_stride, &g))
        return rc;
    const CylSolidScal w = make_cyl_solid_scal(T_freeze, R_in, dr, dphi, dz);
    const HistBlock *blk = (const HistBlock *)d_block;
    const long npl = (long)g.nphi * g.nz;
    if (solid_pair_vec(g, d_active, d_T_in, d_T_out))
        hipLaunchKernelGGL(k_cyl_solid_record<true>, solid_grid(g), dim3(256), 0, as_stream(stream), w, blk, d_T_in, d_T_out,
                           d_t_solid, d_rate, d_g2, (int *)d_log, d_active, (int *)d_hot, g, npl);
    else
        hipLaunchKernelGGL(k_cyl_solid_record<false>, solid_grid(g), dim3(256), 0, as_stream(stream), w, blk, d_T_in, d_T_out,
                           d_t_solid, d_rate, d_g2, (int *)d_log, d_active, (int *)d_hot, g, npl);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_cyl_solid_record_host(double T_freeze, double R_in, double dr, double dphi, double dz, const void *h_block,
                              const double *h_T_in, const double *h_T_out, double *h_t_solid, double *h_rate, double *h_g2,
                              int32_t *h_log, const uint8_t *h_active, int32_t *h_hot, int nr, int nphi, int nz,
                              long plane_stride)
{
    CylBox g;
    if (int rc = check_cyl_solid_record("adi_cyl_solid_record_host", T_freeze, R_in, dr, dphi, dz, h_block, h_T_in, h_T_out,
                                        h_t_solid, h_rate, h_g2, h_log, nr, nphi, nz, plane_stride, &g))
        return rc;
    HistBlock blk;
    memcpy(&blk, h_block, sizeof(blk));
    ADI_REQUIRE(blk.slot >= 0 && blk.capacity >= 1 && isfinite(blk.t0) && isfinite(blk.dt),
                "adi_cyl_solid_record_host: bad block");
    cyl_solid_record_host(make_cyl_solid_scal(T_freeze, R_in, dr, dphi, dz), g, blk, h_T_in, h_T_out, h_t_solid, h_rate, h_g2,
                          h_log, h_active, h_hot);
    return ADI_OK;
}

int adi_cyl_solid_hot_seed(double T_freeze, const double *d_T, const uint8_t *d_active, int32_t *d_hot, int nr, int nphi, int nz,
                           long plane_stride, void *stream)
{
    CylBox g;
    if (int rc = check_cyl_solid_hot_seed("adi_cyl_solid_hot_seed", T_freeze, d_T, d_hot, nr, nphi, nz, plane_stride, &g))
        return rc;
    const long npl = (long)g.nphi * g.nz;
    if (solid_pair_vec(g, d_active, d_T))
        hipLaunchKernelGGL(k_cyl_solid_hot_seed<true>, solid_grid(g), dim3(256), 0, as_stream(stream), T_freeze, d_T, d_active,
                           (int *)d_hot, g, npl);
    else
        hipLaunchKernelGGL(k_cyl_solid_hot_seed<false>, solid_grid(g), dim3(256), 0, as_stream(stream), T_freeze, d_T, d_active,
                           (int *)d_hot, g, npl);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_cyl_solid_hot_seed_host(double T_freeze, const double *h_T, const uint8_t *h_active, int32_t *h_hot, int nr, int nphi,
                                int nz, long plane_stride)
{
    CylBox g;
    if (int rc = check_cyl_solid_hot_seed("adi_cyl_solid_hot_seed_host", T_freeze, h_T, h_hot, nr, nphi, nz, plane_stride, &g))
        return rc;
    cyl_solid_hot_seed_host(T_freeze, g, h_T, h_active, h_hot);
    return ADI_OK;
}

}  // extern "C"
