// adi_cyl_dev.hpp -- device code of the cylindrical step, included by adi_cyl.hip only (one translation unit: adi_cyl.o
// holds every kernel of the backend).  The general kernels (k_cyl_strided, k_cyl_contig), the FAST forms (k_cyl_phi_fast,
// k_cyl_z_fast, k_cyl_r_fast), their *_src / *_tick instantiations for the moving source, k_copy and the source's own two
// kernels.  The cache-policy macros (ADI_STORE_AUX, ADI_LOAD_NT_CONTIG, ADI_CYL_NT) are set by the including unit.
#pragma once
#include "adi_cart_dev.hpp"
#include "adi_cyl_plan.hpp"
#include "adi_cyl_source_dev.hpp"

namespace adi {

struct CylZ {
    double f, b0, bN, aN, c0, add0, addN, T0, TN;
    int dir0, dirN;
};

// ---- r sweep / phi sweep: strided kernel with table-driven rows ---------------------------------
// MODE 0: r sweep (axis 0).  MODE 1: phi sweep (axis 1, periodic, Sherman-Morrison).
// SRC (MODE 0 only): the moving source of the block blk added in the load (k_cyl_strided_src)
template <int M, int MODE, bool SRC>
__device__ __forceinline__ void cyl_strided_body(
    const double *in, double *out, int n, long stride, int n_inner, long outer_stride,
    int Lp, int LINES, int tiles_inner, long ntiles,
    const double *__restrict__ ta, const double *__restrict__ tb, const double *__restrict__ tc, double add_last,
    const double *__restrict__ S, double s_scale, const uint8_t *__restrict__ active_mask, double T_void,
    const double *__restrict__ fac, const double *__restrict__ zt, const double *__restrict__ smden,
    const CylSrcBlock *__restrict__ blk, const CylGeo &G)
{
    extern __shared__ __align__(16) double sm[];
    const int tid = threadIdx.x;
    const long tile = xcd_chunk_tile(blockIdx.x, ntiles);
    const long to = (long)((unsigned)tile / (unsigned)tiles_inner);   // block-uniform, < 2^31 tiles
    const int ti = (int)(tile - to * tiles_inner);
    const int kk = tid & (LINES - 1), sg = tid >> (__ffs(LINES) - 1);   // LINES is a power of two
    const int kcol = ti * LINES + kk;
    const bool active = kcol < n_inner;
    const long base = to * outer_stride + kcol;
    const int r0 = sg * M;

    double a[M], b[M], c[M], d[M];
    CylSrcEval E;
    bool src_on = false;
    if constexpr (SRC) {   // (tile-uniform test first: a tile the support cannot reach evaluates nothing)
        cyl_src_init(blk->s, cyl_src_tmid(*blk), E);
        const long l0 = (long)ti * LINES, l1 = min(l0 + LINES, (long)n_inner) - 1;
        src_on = cyl_src_tile(E, l0, l1, G) && active && cyl_src_line(E, kcol, G);
    }
    double f = 0.0, b0 = 1.0;
    if (MODE == 1) {
        f = fac[to];
        b0 = 1.0 + 2.0 * f;
    }
#pragma unroll
    for (int r = 0; r < M; ++r) {
        const int row = r0 + r;
        const bool ok = active && row < n;
        const long p = base + (long)row * stride;
        double v = ok ? in[p] : 0.0;
        if (MODE == 0) {
            if (active_mask != nullptr && ok && active_mask[p] == 0) v = T_void;  // T_work[void] = ambient, :56-57
            if constexpr (SRC)                                                  // R0 = Tn + dt*q/(rho cp), active cells
                if (src_on && ok && !(active_mask != nullptr && active_mask[p] == 0)) v = v + s_scale * cyl_src_row(E, G, row);
            if (S != nullptr && ok) v = v + s_scale * S[p];                    // R0 = Tn + dt*(S/(rho cp)), :339
            a[r] = (row < n) ? ta[row] : 0.0;
            b[r] = (row < n) ? tb[row] : 1.0;
            c[r] = (row < n) ? tc[row] : 0.0;
            if (row == n - 1) v = v + add_last;                                // rhs_r[:, -1] += ..., :201
        } else {
            const bool inr = row < n;
            if (n == 2) {  // both neighbours are the same cell
                a[r] = (inr && row == 1) ? -2.0 * f : 0.0;
                c[r] = (inr && row == 0) ? -2.0 * f : 0.0;
                b[r] = inr ? b0 : 1.0;
            } else {
                a[r] = (inr && row > 0) ? -f : 0.0;
                c[r] = (inr && row < n - 1) ? -f : 0.0;
                // Sherman-Morrison split with gamma = -b0: b'_0 = 2 b0, b'_{n-1} = b0 + f^2 / b0
                b[r] = !inr ? 1.0 : (row == 0 ? 2.0 * b0 : (row == n - 1 ? b0 + f * f / b0 : b0));
            }
        }
        d[r] = v;
    }

    double ip[M - 1];
    Cond k;
    condense<M>(a, b, c, d, ip, k);

    const int ld = Lp + 1;
    const int plane = LINES * ld;
    double *sX1 = sm, *sX2 = sm + plane, *sCS = sm + 2 * plane, *sX4 = sm + 3 * plane;
    double *sGF = sm + 4 * plane, *sAF = sm + 5 * plane, *sCF = sm + 6 * plane, *sXS = sm + 7 * plane;
    {
        const int w = kk * ld + sg;
        const double aS = a[M - 1];
        sX1[w] = -aS * k.aL;
        sX2[w] = __builtin_fma(-aS, k.cL, b[M - 1]);
        sCS[w] = c[M - 1];
        sX4[w] = __builtin_fma(-aS, k.gL, d[M - 1]);
        sGF[w] = k.gF;
        sAF[w] = k.aF;
        sCF[w] = k.cF;
    }
    __syncthreads();
    {
        const int pl = tid >> (__ffs(Lp) - 1), ps = tid & (Lp - 1);   // Lp is a power of two
        const int w = pl * ld + ps;
        const double cS = sCS[w];
        const bool hasn = ps < Lp - 1;
        const double gFn = hasn ? sGF[w + 1] : 0.0, aFn = hasn ? sAF[w + 1] : 0.0, cFn = hasn ? sCF[w + 1] : 0.0;
        const double ra = sX1[w];
        const double rb = __builtin_fma(-cS, aFn, sX2[w]);
        const double rc = -cS * cFn;
        const double rd = __builtin_fma(-cS, gFn, sX4[w]);
        sXS[w] = pcr_solve(ra, rb, rc, rd, ps, Lp);
    }
    __syncthreads();
    const double xS = sXS[kk * ld + sg];
    const double xL = (sg > 0) ? sXS[kk * ld + sg - 1] : 0.0;
    double x[M];
    back_solve<M>(a, c, d, ip, xL, xS, x);

    if (MODE == 1 && n > 2) {
        // x = y - z * (v.y) / (1 + v.z),  v = (1, 0, ..., 0, beta/gamma) with beta/gamma = f / b0
        double *sY0 = sm, *sYN = sm + LINES;  // the condensation arrays are dead after the second barrier
#pragma unroll
        for (int r = 0; r < M; ++r) {
            if (r0 + r == 0) sY0[kk] = x[r];
            if (r0 + r == n - 1) sYN[kk] = x[r];
        }
        __syncthreads();
        const double mu = (sY0[kk] + (f / b0) * sYN[kk]) * smden[to];
        const double *z = zt + to * (long)n;
#pragma unroll
        for (int r = 0; r < M; ++r)
            if (r0 + r < n) x[r] = __builtin_fma(-mu, z[r0 + r], x[r]);
    }
#pragma unroll
    for (int r = 0; r < M; ++r)
        if (active && (r0 + r) < n) {
#if ADI_CYL_NT
            __builtin_nontemporal_store(x[r], out + base + (long)(r0 + r) * stride);   // written once, whole 128-byte pieces
#else
            out[base + (long)(r0 + r) * stride] = x[r];
#endif
        }
}

template <int M, int MODE>
__global__ __launch_bounds__(M <= 8 ? 1024 : 512) void k_cyl_strided(
    const double *in, double *out, int n, long stride, int n_inner, long outer_stride,
    int Lp, int LINES, int tiles_inner, long ntiles,
    const double *__restrict__ ta, const double *__restrict__ tb, const double *__restrict__ tc, double add_last,
    const double *__restrict__ S, double s_scale, const uint8_t *__restrict__ active_mask, double T_void,
    const double *__restrict__ fac, const double *__restrict__ zt, const double *__restrict__ smden)
{
    cyl_strided_body<M, MODE, false>(in, out, n, stride, n_inner, outer_stride, Lp, LINES, tiles_inner, ntiles, ta, tb, tc,
                                     add_last, S, s_scale, active_mask, T_void, fac, zt, smden, nullptr, CylGeo{});
}

// the r sweep (MODE 0) with the moving source of the block
template <int M>
__global__ __launch_bounds__(M <= 8 ? 1024 : 512) void k_cyl_strided_src(
    const double *in, double *out, int n, long stride, int n_inner, int Lp, int LINES, int tiles_inner, long ntiles,
    const double *__restrict__ ta, const double *__restrict__ tb, const double *__restrict__ tc, double add_last,
    double s_scale, const uint8_t *__restrict__ active_mask, double T_void, const CylSrcBlock *__restrict__ blk, CylGeo G)
{
    cyl_strided_body<M, 0, true>(in, out, n, stride, n_inner, 0, Lp, LINES, tiles_inner, ntiles, ta, tb, tc, add_last,
                                 nullptr, s_scale, active_mask, T_void, nullptr, nullptr, nullptr, blk, G);
}

// ---- z sweep: contiguous kernel, constant coefficients with end closures -----------------------
// TICK: the first thread of block 0 advances the source block's counter (k_cyl_contig_tick: the step's last kernel; every
// reader of the counter -- the r sweep -- has finished before it starts)
template <int M, bool VEC, bool TICK>
__device__ __forceinline__ void cyl_contig_body(const double *in, double *out,
                                                long nlines, int n, int Lp, CylZ z,
                                                const uint8_t *__restrict__ active_mask, double T_void,
                                                double T_inner, long lines_per_r0, long sx, unsigned long long *tick)
{
    if constexpr (TICK)
        if (blockIdx.x == 0 && threadIdx.x == 0) *tick = *tick + 1ull;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lw = 64 >> (__ffs(Lp) - 1);
    const int li = lane & (Lp - 1);
    const unsigned line = (blockIdx.x * (blockDim.x >> 6) + wave) * (unsigned)lw + ((unsigned)lane >> (__ffs(Lp) - 1));
    const bool active = line < (unsigned long)nlines;
    const int r0 = li * M;
    const unsigned pi = line / (unsigned)lines_per_r0;   // radius index; lines_per_r0 = nphi
    const long base = (long)pi * sx + (long)(line - pi * (unsigned)lines_per_r0) * n + r0;

    double a[M], b[M], c[M], d[M];
    if (VEC) {
        if (active && r0 < n) {
            const double2 *q = reinterpret_cast<const double2 *>(in + base);
#pragma unroll
            for (int i = 0; i < M / 2; ++i) {
                const double2 t = q[i];
                d[2 * i] = t.x;
                d[2 * i + 1] = t.y;
            }
        } else {
#pragma unroll
            for (int r = 0; r < M; ++r) d[r] = 0.0;
        }
    } else {
#pragma unroll
        for (int r = 0; r < M; ++r) d[r] = (active && r0 + r < n) ? in[base + r] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < M; ++r) {
        const int row = r0 + r;
        const bool inr = row < n;
        double av = inr ? -z.f : 0.0, bv = inr ? 1.0 + 2.0 * z.f : 1.0, cv = inr ? -z.f : 0.0;
        if (row == 0) {                 // bottom closure, adi3d_cyl_phi_v3.py:271-283
            av = 0.0; bv = z.b0; cv = z.c0;
            d[r] = z.dir0 ? z.T0 : d[r] + z.add0;
        }
        if (row == n - 1) {             // top closure, :285-296 (applied last, as in the reference, when n == 1)
            av = (n == 1) ? 0.0 : z.aN; bv = z.bN; cv = 0.0;
            d[r] = z.dirN ? z.TN : d[r] + z.addN;
        }
        a[r] = av; b[r] = bv; c[r] = cv;
    }
    double ip[M - 1];
    Cond k;
    condense<M>(a, b, c, d, ip, k);
    const double gFn = __shfl_down(k.gF, 1, Lp), aFn = __shfl_down(k.aF, 1, Lp), cFn = __shfl_down(k.cF, 1, Lp);
    double ra, rb, rc, rd;
    reduced_row(a[M - 1], b[M - 1], c[M - 1], d[M - 1], k, gFn, aFn, cFn, ra, rb, rc, rd);
    const double xS = pcr_solve(ra, rb, rc, rd, li, Lp);
    double xL = __shfl_up(xS, 1, Lp);
    if (li == 0) xL = 0.0;
    double x[M];
    back_solve<M>(a, c, d, ip, xL, xS, x);

    if (active_mask != nullptr && active) {   // Tnp1[void] = ambient_void; Tnp1[0, ~active[0]] = ambient_inner (:61-68)
        const bool axis_row = line < lines_per_r0;
#pragma unroll
        for (int r = 0; r < M; ++r)
            if (r0 + r < n && active_mask[base + r] == 0) x[r] = axis_row ? T_inner : T_void;
    }
    if (VEC) {
        if (active && r0 < n) {
            double2 *q = reinterpret_cast<double2 *>(out + base);
#pragma unroll
            for (int i = 0; i < M / 2; ++i) q[i] = make_double2(x[2 * i], x[2 * i + 1]);
        }
    } else {
#pragma unroll
        for (int r = 0; r < M; ++r)
            if (active && r0 + r < n) out[base + r] = x[r];
    }
}

template <int M, bool VEC>
__global__ __launch_bounds__(256) void k_cyl_contig(const double *in, double *out,
                                                   long nlines, int n, int Lp, CylZ z,
                                                   const uint8_t *__restrict__ active_mask, double T_void,
                                                   double T_inner, long lines_per_r0, long sx)
{
    cyl_contig_body<M, VEC, false>(in, out, nlines, n, Lp, z, active_mask, T_void, T_inner, lines_per_r0, sx, nullptr);
}
template <int M, bool VEC>
__global__ __launch_bounds__(256) void k_cyl_contig_tick(const double *in, double *out,
                                                        long nlines, int n, int Lp, CylZ z,
                                                        const uint8_t *__restrict__ active_mask, double T_void,
                                                        double T_inner, long lines_per_r0, long sx, unsigned long long *tick)
{
    cyl_contig_body<M, VEC, true>(in, out, nlines, n, Lp, z, active_mask, T_void, T_inner, lines_per_r0, sx, tick);
}

// ---- FAST forms ------------------------------------------------------------------------------------------------
// The three operators of the BE step have coefficients that do not depend on the data and hardly on the position:
//   phi  (-f_i, 1+2f_i, -f_i) along the line, f_i by radius      -> the uniform-interior model of adi_core.hpp with one
//        UniC per radius (block-uniform: a tile lies in one radius plane), rows 0 / n-1 carry the Sherman-Morrison split
//   z    (-f, 1+2f, -f) everywhere, closures in rows 0 / n-1    -> the same model, one UniC per plan
//   r    a_i, b_i, c_i by radius index, the same for every line -> the whole factorisation of every segment (pivots,
//        multipliers, the six condensation numbers and the PCR multipliers of the separator system) is data-independent:
//        computed once on the host, the kernel only propagates right-hand sides
// No reciprocal is left in any of the three kernels; 50-60 VGPRs; every input read once, every output written once.

// phi sweep: tile = LINES adjacent z-lines x all nphi rows of one radius plane
template <int M>
__global__ __launch_bounds__(1024) void k_cyl_phi_fast(
    const double *in, double *out, int n, long stride, int n_inner, long outer_stride,
    int Lp, int LINES, int tiles_inner, long ntiles, const UniC<M> *__restrict__ utab,
    const double *__restrict__ fac, const double *__restrict__ zt, const double *__restrict__ smden)
{
    extern __shared__ __align__(16) double sm[];
    const int tid = threadIdx.x;
    const long tile = xcd_chunk_tile(blockIdx.x, ntiles);
    const long to = (long)((unsigned)tile / (unsigned)tiles_inner);   // radius index: block-uniform
    const int ti = (int)(tile - to * tiles_inner);
    const int kk = tid & (LINES - 1), sg = tid >> (__ffs(LINES) - 1);
    const int kcol = ti * LINES + kk;                                 // (host: n_inner % LINES == 0, Lp * M == n)
    const long base = to * outer_stride + kcol;
    const int r0 = sg * M;
    const UniC<M> U = utab[to];                                       // scalar loads: one radius per tile
    const double f = fac[to], b0 = 1.0 + 2.0 * f;

    double d[M];
#if ADI_LOAD_PRIO
    __builtin_amdgcn_s_setprio(ADI_LOAD_PRIO);
#endif
#pragma unroll
    for (int r = 0; r < M; ++r) d[r] = in[base + (long)(r0 + r) * stride];
#if ADI_LOAD_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
    // Sherman-Morrison split with gamma = -b0 (see k_cyl_strided): b'_0 = 2 b0, b'_{n-1} = b0 + f^2 / b0
    const bool firstseg = r0 == 0, lastseg = r0 + M == n;
    const double a0 = firstseg ? 0.0 : U.s, bf = firstseg ? 2.0 * b0 : U.bu;
    const double aS = U.s, bS = lastseg ? b0 + f * f / b0 : U.bu, cS = lastseg ? 0.0 : U.s;
    Cond k;
    double kappa;
    condense_uniform<M>(U, a0, bf, d, k, kappa);
    double xL, xS;
    tile_separators(sm, tid, kk, sg, Lp, LINES, aS, bS, cS, d[M - 1], k, xL, xS);
    back_solve_uniform<M>(U, a0, kappa, d, xL, xS);
    // x = y - z * (v.y) / (1 + v.z),  v = (1, 0, ..., 0, beta/gamma) with beta/gamma = f / b0
    double *sY0 = sm, *sYN = sm + LINES;      // (the separator arrays are dead: every thread has read its xS / xL...
    __syncthreads();                          //  ...once all of them have passed this barrier)
    if (firstseg) sY0[kk] = d[0];
    if (lastseg) sYN[kk] = d[M - 1];
    __syncthreads();
    const double mu = (sY0[kk] + (f / b0) * sYN[kk]) * smden[to];
    const double *z = zt + to * (long)n + r0;
#pragma unroll
    for (int r = 0; r < M; ++r) {
        const double x = __builtin_fma(-mu, z[r], d[r]);
#if ADI_CYL_NT
        __builtin_nontemporal_store(x, out + base + (long)(r0 + r) * stride);
#else
        out[base + (long)(r0 + r) * stride] = x;
#endif
    }
}

// z sweep: one wave = 64/Lp lines, lane li owns rows [li*M, li*M+M); coalesced loads / stores through a wave-private
// LDS strip (adi_cart_dev.hpp, coal_load).  Closures without a Dirichlet end (neumann0 / robin): row 0 and row n-1
// differ from the uniform row in their diagonal and right-hand side only.
template <int M, bool TICK>
__device__ __forceinline__ void cyl_z_fast_body(const double *in, double *out, long nlines,
                                                int n, int Lp, CylZ z, UniC<M> U,
                                                const uint8_t *__restrict__ active_mask, double T_void, double T_inner,
                                                long lines_per_r0, long sx, unsigned long long *tick)
{
    if constexpr (TICK)    // (cyl_contig_body)
        if (blockIdx.x == 0 && threadIdx.x == 0) *tick = *tick + 1ull;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ __align__(16) double strips[4 * 32 * (M + 2)];
    double *strip = strips + wave * 32 * (M + 2);
    const int sh = __ffs(Lp) - 1;
    const int lw = 64 >> sh;
    const int li = lane & (Lp - 1);
    const unsigned line = (blockIdx.x * (blockDim.x >> 6) + wave) * (unsigned)lw + ((unsigned)lane >> sh);
    if ((long)(blockIdx.x * (blockDim.x >> 6) + wave) * lw >= nlines) return;       // (host: nlines % lw == 0)
    const int r0 = li * M;
    const unsigned pi = line / (unsigned)lines_per_r0;               // radius index; lines_per_r0 = nphi (host: % lw == 0)
    const long base = (long)pi * sx + (long)(line - pi * (unsigned)lines_per_r0) * n + r0;
    const long wbase = __shfl(base, 0);                              // the wave's 64*M doubles are contiguous from lane 0's
    double d[M];
#if ADI_LOAD_PRIO
    __builtin_amdgcn_s_setprio(ADI_LOAD_PRIO);
#endif
    coal_load<M>(in + wbase, strip, lane, d);
#if ADI_LOAD_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
    const bool firstseg = li == 0, lastseg = r0 + M == n;
    const double a0 = firstseg ? 0.0 : U.s, bf = firstseg ? z.b0 : U.bu;
    if (firstseg) d[0] = d[0] + z.add0;                              // bottom closure, adi3d_cyl_phi_v3.py:271-283
    const double aS = lastseg ? z.aN : U.s, bS = lastseg ? z.bN : U.bu, cS = lastseg ? 0.0 : U.s;
    if (lastseg) d[M - 1] = d[M - 1] + z.addN;                       // top closure, :285-296
    Cond k;
    double kappa;
    condense_uniform<M>(U, a0, bf, d, k, kappa);
    const double gFn = __shfl_down(k.gF, 1, Lp), aFn = __shfl_down(k.aF, 1, Lp), cFn = __shfl_down(k.cF, 1, Lp);
    double ra, rb, rc, rd;
    reduced_row(aS, bS, cS, d[M - 1], k, gFn, aFn, cFn, ra, rb, rc, rd);
    const double xS = pcr_solve(ra, rb, rc, rd, li, Lp);
    double xL = __shfl_up(xS, 1, Lp);
    if (li == 0) xL = 0.0;
    back_solve_uniform<M>(U, a0, kappa, d, xL, xS);
    if (active_mask != nullptr) {   // Tnp1[void] = ambient_void; Tnp1[0, ~active[0]] = ambient_inner (:61-68)
        const bool axis_row = line < lines_per_r0;
#pragma unroll
        for (int r = 0; r < M; ++r)
            if (active_mask[base + r] == 0) d[r] = axis_row ? T_inner : T_void;
    }
    coal_store<M>(out + wbase, strip, lane, d);
}

template <int M>
__global__ __launch_bounds__(256) void k_cyl_z_fast(const double *in, double *out, long nlines,
                                                   int n, int Lp, CylZ z, UniC<M> U,
                                                   const uint8_t *__restrict__ active_mask, double T_void, double T_inner,
                                                   long lines_per_r0, long sx)
{
    cyl_z_fast_body<M, false>(in, out, nlines, n, Lp, z, U, active_mask, T_void, T_inner, lines_per_r0, sx, nullptr);
}
template <int M>
__global__ __launch_bounds__(256) void k_cyl_z_fast_tick(const double *in, double *out, long nlines,
                                                        int n, int Lp, CylZ z, UniC<M> U,
                                                        const uint8_t *__restrict__ active_mask, double T_void,
                                                        double T_inner, long lines_per_r0, long sx, unsigned long long *tick)
{
    cyl_z_fast_body<M, true>(in, out, nlines, n, Lp, z, U, active_mask, T_void, T_inner, lines_per_r0, sx, tick);
}

// r sweep.  Per segment (M rows, row M-1 = separator) the host stores (cyl_build_r_fast, adi_cyl_plan.hpp), RF_STRIDE
// doubles each:
//   wf[M-1]  forward multipliers  a_r * ip_{r-1}  (wf[0] unused)      wb[M-1] backward multipliers c_r * jp_{r+1}
//   ip[M-1]  inverse pivots of the top-down factorisation             cr[M-1] the c_r of the interior rows
//   ipl, jpf the last / first inverse pivot of the two eliminations   aF, cF, aL, cL the matrix part of the condensation
//   a0       a of the segment's first row                             aS, cS   separator couplings
//   pk1[6], pk2[6], pinv  the PCR multipliers of this separator's row of the (line-independent) separator system
struct CylRSegView {
    const double *p;
    __device__ __forceinline__ double wf(int r) const { return p[r]; }
    __device__ __forceinline__ double wb(int r) const { return p[(RF_MAXM - 1) + r]; }
    __device__ __forceinline__ double ip(int r) const { return p[2 * (RF_MAXM - 1) + r]; }
    __device__ __forceinline__ double cr(int r) const { return p[3 * (RF_MAXM - 1) + r]; }
    __device__ __forceinline__ double sc(int i) const { return p[4 * (RF_MAXM - 1) + i]; }     // ipl jpf aF cF aL cL a0 aS cS bS
    __device__ __forceinline__ double pk(int i) const { return p[4 * (RF_MAXM - 1) + 10 + i]; }
};

// tile = 64 adjacent lines (one wave = one segment of 64 lines: the tables are wave-uniform -> scalar loads) x all
// segments; 512-byte row pieces
// SRC: the moving source of the block blk added in the load (k_cyl_r_fast_src)
template <int M, bool SRC>
__device__ __forceinline__ void cyl_r_fast_body(
    const double *in, double *out, int n, long stride, int n_inner, int nseg, int Lp,
    long ntiles, const double *__restrict__ rfac, double add_last, const double *__restrict__ S, double s_scale,
    const uint8_t *__restrict__ active_mask, double T_void, const CylSrcBlock *__restrict__ blk, const CylGeo &G)
{
    extern __shared__ __align__(16) double sm[];          // 2 x [Lp][64] separator right-hand sides + [Lp][64] first-row data
    constexpr int MI = M - 1;
    const int tid = threadIdx.x;
    const int kk = tid & 63;
    const int sg = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long tile = xcd_chunk_tile(blockIdx.x, ntiles);
    const long base = tile * 64 + kk;                     // (host: n_inner % 64 == 0)
    const int r0 = sg * M;
    CylRSegView T;
    T.p = rfac + (size_t)sg * RF_STRIDE;
    double d[M];
    CylSrcEval E;
    bool src_on = false;
    if constexpr (SRC) {   // (the tile's 64 lines first: a tile the support cannot reach evaluates nothing)
        cyl_src_init(blk->s, cyl_src_tmid(*blk), E);
        src_on = cyl_src_tile(E, tile * 64, tile * 64 + 63, G) && cyl_src_line(E, base, G);
    }
#if ADI_LOAD_PRIO
    __builtin_amdgcn_s_setprio(ADI_LOAD_PRIO);
#endif
#pragma unroll
    for (int r = 0; r < M; ++r) {
        const long p = base + (long)(r0 + r) * stride;
        double v = in[p];
        if (active_mask != nullptr && active_mask[p] == 0) v = T_void;        // T_work[void] = ambient, :56-57
        if constexpr (SRC)                                                    // R0 = Tn + dt*q/(rho cp), active cells
            if (src_on && !(active_mask != nullptr && active_mask[p] == 0)) v = v + s_scale * cyl_src_row(E, G, r0 + r);
        if (S != nullptr) v = v + s_scale * S[p];                            // R0 = Tn + dt*(S/(rho cp)), :339
        d[r] = v;
    }
#if ADI_LOAD_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
    if (r0 + M == n) d[M - 1] = d[M - 1] + add_last;                          // rhs_r[:, -1] += ..., :201
    // condensation of the right-hand side (the two recurrences of condense<M>, pivots from the table)
    double y = d[0], zb = d[MI - 1];
#pragma unroll
    for (int r = 1; r < MI; ++r) y = __builtin_fma(-T.wf(r), y, d[r]);
#pragma unroll
    for (int r = MI - 2; r >= 0; --r) zb = __builtin_fma(-T.wb(r), zb, d[r]);
    const double gL = y * T.sc(0), gF = zb * T.sc(1);
    // separator row: rd = dS - aS*gL - cS*gF(next segment); the matrix part of the row and of the whole PCR is tabulated
    double *sG = sm + 2 * Lp * 64;                        // gF of every segment, for the segment before it
    sG[sg * 64 + kk] = gF;
    __syncthreads();
    double rd = __builtin_fma(-T.sc(7), gL, d[M - 1]);
    if (sg + 1 < nseg) rd = __builtin_fma(-T.sc(8), sG[(sg + 1) * 64 + kk], rd);
    // PCR over the nseg separators of a line (the lanes of a line sit in different WAVES here: through LDS, one barrier
    // per level; log2(Lp) <= 6 levels).  rd_i <- rd_i - k1_i rd_{i-dl} - k2_i rd_{i+dl}
    int lev = 0;
    for (int dl = 1; dl < Lp; dl <<= 1, ++lev) {
        double *cur = sm + (lev & 1) * (Lp * 64);         // two buffers in turn: one barrier per level
        cur[sg * 64 + kk] = rd;
        __syncthreads();
        const double lo = (sg - dl >= 0) ? cur[(sg - dl) * 64 + kk] : 0.0;
        const double hi = (sg + dl < nseg) ? cur[(sg + dl) * 64 + kk] : 0.0;
        rd = __builtin_fma(-T.pk(6 + lev), hi, __builtin_fma(-T.pk(lev), lo, rd));
    }
    const double xS = rd * T.pk(12);
    sG[sg * 64 + kk] = xS;                                // (sG was last read before the first PCR barrier)
    __syncthreads();
    const double xL = (sg > 0) ? sG[(sg - 1) * 64 + kk] : 0.0;
    // back-substitution of the interior rows (back_solve<M> with tabulated pivots)
    d[0] = __builtin_fma(-T.sc(6), xL, d[0]);
#pragma unroll
    for (int r = 1; r < MI; ++r) d[r] = __builtin_fma(-T.wf(r), d[r - 1], d[r]);
    d[MI - 1] = __builtin_fma(-T.cr(MI - 1), xS, d[MI - 1]) * T.ip(MI - 1);
#pragma unroll
    for (int r = MI - 2; r >= 0; --r) d[r] = __builtin_fma(-T.cr(r), d[r + 1], d[r]) * T.ip(r);
    d[M - 1] = xS;
#pragma unroll
    for (int r = 0; r < M; ++r) {
#if ADI_CYL_NT
        __builtin_nontemporal_store(d[r], out + base + (long)(r0 + r) * stride);
#else
        out[base + (long)(r0 + r) * stride] = d[r];
#endif
    }
}

template <int M>
__global__ __launch_bounds__(1024) void k_cyl_r_fast(
    const double *in, double *out, int n, long stride, int n_inner, int nseg, int Lp,
    long ntiles, const double *__restrict__ rfac, double add_last, const double *__restrict__ S, double s_scale,
    const uint8_t *__restrict__ active_mask, double T_void)
{
    cyl_r_fast_body<M, false>(in, out, n, stride, n_inner, nseg, Lp, ntiles, rfac, add_last, S, s_scale, active_mask, T_void,
                              nullptr, CylGeo{});
}
template <int M>
__global__ __launch_bounds__(1024) void k_cyl_r_fast_src(
    const double *in, double *out, int n, long stride, int n_inner, int nseg, int Lp,
    long ntiles, const double *__restrict__ rfac, double add_last, double s_scale,
    const uint8_t *__restrict__ active_mask, double T_void, const CylSrcBlock *__restrict__ blk, CylGeo G)
{
    cyl_r_fast_body<M, true>(in, out, n, stride, n_inner, nseg, Lp, ntiles, rfac, add_last, nullptr, s_scale, active_mask,
                             T_void, blk, G);
}

// elementwise pass used when a sweep degenerates (nphi == 1) or the grid is too long for the fast path
__global__ __launch_bounds__(256) void k_copy(const double *in, double *out, size_t n)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) out[p] = in[p];
}

// q at every cell centre at time t (0 on inactive cells): the field form of the source, and what the tests compare with
__global__ __launch_bounds__(256) void k_cyl_source_sample(adi_cyl_heat_source s, CylGeo G, int nr, int nphi, long sx,
                                                           double t, const uint8_t *__restrict__ active, double *__restrict__ out)
{
    const long plane = (long)nphi * G.nz;
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= plane * nr) return;
    const int i = (int)(q / plane);
    const long line = q - (long)i * plane;
    const long p = (long)i * sx + line;
    CylSrcEval e;
    cyl_src_init(s, t, e);
    const bool on = (active == nullptr || active[p] != 0) && cyl_src_line(e, line, G);
    out[p] = on ? cyl_src_row(e, G, i) : 0.0;
}

__global__ void k_cyl_source_set(CylSrcBlock *blk, CylSrcBlock v) { *blk = v; }

}  // namespace adi
