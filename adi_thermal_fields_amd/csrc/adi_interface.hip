// adi_interface.hip -- K5c / K5d: the interface side of the slab decomposition along memory axis 0, between pass A
// (adi_condense.hip, or the zero-boundary solve of the deferred forms) and pass B / the corrected axis-1 sweep:
//   k_interface, k_interface_uniform, k_interface_pair     the reduced system of the two-pass forms and of `deferred_exact`
//   k_interface_deferred, k_interface_deferred_lines       the 2 x 2 systems per boundary of the deferred forms
//   k_deferred_lines_apply                                 the flagged lines' own weights applied in memory
//   k_deferred_exact_setup, k_deferred_exact_coef          the deferred form without decay: plan constants, per-step coefficients
// and the two entries that build the uniform line's weights on the host (adi_axis0_weights.hpp) and upload them.
// One thread per line everywhere; no counterpart in the reference (single process).
#include <vector>

#include "adi_axis0_weights.hpp"
#include "adi_cart_host.hpp"

namespace adi {

// K5c: interface solve.  cond_all: [nranks][6][nlines] (all-gathered).  For this rank, merge the slabs below
// and above it, solve the 2x2 system for its own first/last unknown and emit the neighbours' boundary
// values: xlo = last unknown of the slab below, xhi = first unknown of the slab above.
__global__ __launch_bounds__(256) void k_interface(const double *__restrict__ cond_all, int nranks, int rank,
                                                   long nlines, double *__restrict__ xlo, double *__restrict__ xhi)
{
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= nlines) return;
    auto ld = [&](int r) {
        const double *q = cond_all + (long)r * 6 * nlines + id;
        Cond k;
        k.gF = q[0]; k.aF = q[nlines]; k.cF = q[2 * nlines]; k.gL = q[3 * nlines]; k.aL = q[4 * nlines];
        k.cL = q[5 * nlines];
        return k;
    };
    const Cond C = ld(rank);
    Cond P = {0, 0, 0, 0, 0, 0}, S = {0, 0, 0, 0, 0, 0};   // empty neighbours: decoupled zeros
    if (rank > 0) {
        P = ld(0);
        for (int r = 1; r < rank; ++r) P = merge_cond(P, ld(r));
    }
    if (rank < nranks - 1) {
        S = ld(nranks - 1);
        for (int r = nranks - 2; r > rank; --r) S = merge_cond(ld(r), S);
    }
    // unknowns f = x_first(C), l = x_last(C);  x_last(P) = P.gL - P.cL f ;  x_first(S) = S.gF - S.aF l
    //   f = C.gF - C.aF (P.gL - P.cL f) - C.cF (S.gF - S.aF l)
    //   l = C.gL - C.aL (P.gL - P.cL f) - C.cL (S.gF - S.aF l)
    const double m00 = 1.0 - C.aF * P.cL, m01 = -C.cF * S.aF;
    const double m10 = -C.aL * P.cL, m11 = 1.0 - C.cL * S.aF;
    const double r0 = C.gF - C.aF * P.gL - C.cF * S.gF;
    const double r1 = C.gL - C.aL * P.gL - C.cL * S.gF;
    const double idet = 1.0 / (m00 * m11 - m01 * m10);
    const double f = (r0 * m11 - m01 * r1) * idet;
    const double l = (m00 * r1 - m10 * r0) * idet;
    xlo[id] = P.gL - P.cL * f;
    xhi[id] = S.gF - S.aF * l;
}

// The same solve for the deferred form without decay: only the right-hand sides (gF, gL) = (plane 0, plane n-1 of x0) are
// gathered every step, g_all [nranks][2][nlines]; the matrix entries are constants of the plan -- per line on the first and
// the last rank (their global end rows: mat_all [nranks][4][nlines] = aF, cF, aL, cL, gathered once), the same two numbers
// (-w0, -wn) for every line of a middle rank (scal_all [nranks][2]).  A third of the per-step payload and of this kernel's reads.
__global__ __launch_bounds__(256) void k_interface_uniform(const double *__restrict__ g_all, const double *__restrict__ mat_all,
                                                           const double *__restrict__ scal_all, int nranks, int rank,
                                                           long nlines, double *__restrict__ xlo, double *__restrict__ xhi)
{
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= nlines) return;
    auto ld = [&](int r) {
        const double *g = g_all + (long)r * 2 * nlines + id;
        Cond k;
        k.gF = g[0]; k.gL = g[nlines];
        if (r == 0 || r == nranks - 1) {
            const double *m = mat_all + (long)r * 4 * nlines + id;
            k.aF = m[0]; k.cF = m[nlines]; k.aL = m[2 * nlines]; k.cL = m[3 * nlines];
        } else {
            const double w0 = scal_all[2 * r], wn = scal_all[2 * r + 1];
            k.aF = -w0; k.cF = -wn; k.aL = -wn; k.cL = -w0;
        }
        return k;
    };
    const Cond C = ld(rank);
    Cond P = {0, 0, 0, 0, 0, 0}, S = {0, 0, 0, 0, 0, 0};
    if (rank > 0) {
        P = ld(0);
        for (int r = 1; r < rank; ++r) P = merge_cond(P, ld(r));
    }
    if (rank < nranks - 1) {
        S = ld(nranks - 1);
        for (int r = nranks - 2; r > rank; --r) S = merge_cond(ld(r), S);
    }
    const double m00 = 1.0 - C.aF * P.cL, m01 = -C.cF * S.aF;      // (as in k_interface)
    const double m10 = -C.aL * P.cL, m11 = 1.0 - C.cL * S.aF;
    const double r0 = C.gF - C.aF * P.gL - C.cF * S.gF;
    const double r1 = C.gL - C.aL * P.gL - C.cL * S.gF;
    const double idet = 1.0 / (m00 * m11 - m01 * m10);
    const double f = (r0 * m11 - m01 * r1) * idet;
    const double l = (m00 * r1 - m10 * r0) * idet;
    xlo[id] = P.gL - P.cL * f;
    xhi[id] = S.gF - S.aF * l;
}

// Neighbour-only form of the interface system, valid when the far-side couplings of the boundary windows
// (aL of the window that ends a slab, cF of the window that starts one) have decayed below rounding:
//   x_last(r)    = gL  - cL  * x_first(r+1)        (window = last rows of slab r)
//   x_first(r+1) = gF' - aF' * x_last(r)           (window = first rows of slab r+1)
// my_lo / my_hi: [6][nlines] condensations of this slab's first / last window; prev_hi: rows (gL,aL,cL) of the
// slab below; next_lo: rows (gF,aF) of the slab above.  NULL neighbour -> 0.
__global__ __launch_bounds__(256) void k_interface_pair(const double *__restrict__ my_lo, const double *__restrict__ my_hi,
                                                        const double *__restrict__ prev_hi, const double *__restrict__ next_lo,
                                                        long nlines, double *__restrict__ xlo, double *__restrict__ xhi)
{
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= nlines) return;
    double lo = 0.0, hi = 0.0;
    if (prev_hi) {
        const double gLp = prev_hi[id], cLp = prev_hi[2 * nlines + id];
        const double gF = my_lo[id], aF = my_lo[nlines + id];
        lo = (gLp - cLp * gF) / (1.0 - cLp * aF);
    }
    if (next_lo) {
        const double gFn = next_lo[id], aFn = next_lo[nlines + id];
        const double gL = my_hi[3 * nlines + id], cL = my_hi[5 * nlines + id];
        hi = (gFn - aFn * gL) / (1.0 - aFn * cL);
    }
    xlo[id] = lo;
    xhi[id] = hi;
}

// ------------------------------------------------------------------------------------------------
// K5c: interface values of the DEFERRED form.  Every rank has solved its part of every sharded-axis line with zero
// boundary values: x0.  By linearity the solution of the whole line is, inside the slab,
//     x[i] = x0[i] + xlo * w[i] + xhi * w[n-1-i],     w = theta*gamma * tridiag(-tg, 1+2tg, -tg)^-1 e_0,
// with xlo / xhi the unknowns adjacent to the slab on the neighbouring ranks.  Where w has decayed below rounding
// across a slab (the caller checks it, as for adi_interface_pair) the interface system splits into one 2 x 2 system per
// boundary: with L the last unknown of the slab below, F the first unknown of this slab and om = w[0],
//     L = x0_last(below) + om * F,    F = x0_first(mine) + om * L.
// first / last: planes 0 and n-1 of this rank's x0; prev_last / next_first: the adjacent planes of the neighbours' x0
// (null: no neighbour).  ulo = L of the boundary below, uhi = F of the boundary above; 0 where there is no neighbour.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_interface_deferred(const double *__restrict__ first, const double *__restrict__ last,
                                                            const double *__restrict__ prev_last,
                                                            const double *__restrict__ next_first, double om, double idet,
                                                            long nlines, double *__restrict__ ulo, double *__restrict__ uhi)
{
    const long l = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= nlines) return;
    double lo = 0.0, hi = 0.0;
    if (prev_last != nullptr) {
        const double gL = prev_last[l];
        const double F = __builtin_fma(om, gL, first[l]) * idet;
        lo = __builtin_fma(om, F, gL);
    }
    if (next_first != nullptr) hi = __builtin_fma(om, last[l], next_first[l]) * idet;
    ulo[l] = lo;
    uhi[l] = hi;
}

// The same for lines that are NOT uniform (curved solids, voids, Dirichlet cells): every line has its own decaying
// homogeneous solutions, computed once per plan by two ordinary axis-0 sweeps with zero right-hand sides and unit boundary
// values.  om_*: their value in the plane next to the interface -- om_lo_own / om_hi_own of this rank's lines, om_hi_prev /
// om_lo_next received from the neighbours at plan time.  Per line and boundary a 2 x 2 system, as above with two weights.
__global__ __launch_bounds__(256) void k_interface_deferred_lines(
    const double *__restrict__ first, const double *__restrict__ last, const double *__restrict__ prev_last,
    const double *__restrict__ next_first, const double *__restrict__ om_lo_own, const double *__restrict__ om_hi_prev,
    const double *__restrict__ om_hi_own, const double *__restrict__ om_lo_next, long nlines, double *__restrict__ ulo,
    double *__restrict__ uhi, const uint8_t *__restrict__ uni_lo, const uint8_t *__restrict__ uni_hi,
    double *__restrict__ ulo_uni, double *__restrict__ uhi_uni)
{
    const long l = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= nlines) return;
    double lo = 0.0, hi = 0.0;
    if (prev_last != nullptr) {
        const double gL = prev_last[l], wl = om_lo_own[l], wh = om_hi_prev[l];
        const double F = __builtin_fma(wl, gL, first[l]) / (1.0 - wl * wh);     // this rank's first unknown
        lo = __builtin_fma(wh, F, gL);                                          // the neighbour's last one: what w_lo multiplies
    }
    if (next_first != nullptr) {
        const double wh = om_hi_own[l], wl = om_lo_next[l];
        hi = __builtin_fma(wl, last[l], next_first[l]) / (1.0 - wl * wh);       // the neighbour's first unknown
    }
    ulo[l] = lo;
    uhi[l] = hi;
    // the same values on the lines whose rows within reach of the interface are uniform (they take the scalar weights inside
    // the axis-1 sweep); the others get their own weights from k_deferred_lines_apply, or none (lines outside the mask)
    if (ulo_uni != nullptr) ulo_uni[l] = (uni_lo != nullptr && uni_lo[l] != 0) ? lo : 0.0;
    if (uhi_uni != nullptr) uhi_uni[l] = (uni_hi != nullptr && uni_hi[l] != 0) ? hi : 0.0;
}

// x[i][cell[q]] += wc[r][q] * u[cell[q]]: the rank-one update of the flagged lines of one side of the slab (the lines that
// cross a void, the surface or a Dirichlet cell within reach of the interface).  Thread = one flagged line, blockIdx.y strides
// the K rows; consecutive q are mostly consecutive cells (runs along the contiguous axis), the compact weights are read
// coalesced.  The same fma as corr_apply: a line gives the same bits whichever way its correction is applied.
__global__ __launch_bounds__(256) void k_deferred_lines_apply(double *__restrict__ x, int nx, long sx, const int *__restrict__ cells,
                                                              long nflag, const double *__restrict__ wc, int K,
                                                              const double *__restrict__ u, int from_hi,
                                                              const int *__restrict__ nrows)
{
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nflag) return;
    const long cell = cells[q];
    const double uu = u[cell];
    const int Kq = (nrows != nullptr && nrows[q] < K) ? nrows[q] : K;     // rows beyond carry exact zeros: not read
    for (int r = blockIdx.y; r < Kq; r += gridDim.y) {
        // a flagged line's weights are exact zeros beyond its first row outside the mask (identity rows cut the coupling): a
        // line through a cavity 150 planes from the interface carries 150 weights, not K; x + 0 * u = x is skipped unread
        const double w = wc[(long)r * nflag + q];
        if (w != 0.0) {
            const long i = from_hi ? (long)(nx - 1 - r) : (long)r;
            double *p = x + i * sx + cell;
            *p = __builtin_fma(w, uu, *p);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// K5d: the deferred form WITHOUT decay (thin slabs, strong scaling).  x = x0 + xlo * psi_lo + xhi * psi_hi still holds;
// what changes is that (1) the interface system couples all ranks -- the all-gather + k_interface of the `exact` form, fed
// with gF = x0_first, gL = x0_last (planes of x0) and the matrix entries below -- and (2) on the first / last rank the
// homogeneous solutions feel the global end row, whose diagonal differs from the uniform one by delta = dt * coeff - tg
// (a line start / end with its Robin coefficient).  Sherman-Morrison on the uniform matrix U (p0 = w0 / tg = (U^-1)_00,
// pn = wn / tg = (U^-1)_0,n-1), kappa = delta / (1 + delta p0):
//     first rank (row 0 modified):   psi_hi[i] = w[n-1-i] - kappa pn w[i]      (no psi_lo: nothing below)
//     last rank (row n-1 modified):  psi_lo[i] = w[i] - kappa pn w[n-1-i]      (no psi_hi)
// so the correction keeps the form  c_lo * w[i] + c_hi * w[n-1-i]  that adi_sweep_corrected applies, with per-line c_lo / c_hi.
// k_deferred_exact_setup: once per plan -- matrix entries mat [4][nlines] = (aF, cF, aL, cL) of this rank and kappa * pn per
// line and end (0 where the end row is an ordinary interior row).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_deferred_exact_setup(const uint8_t *__restrict__ flags_first,
                                                              const uint8_t *__restrict__ flags_last,
                                                              const double *__restrict__ coeff_first,
                                                              const double *__restrict__ coeff_last, double tg, double dt,
                                                              double w0, double wn, long nlines, double *__restrict__ mat,
                                                              double *__restrict__ kap)
{
    const long l = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= nlines) return;
    const bool has_lo = (flags_first[l] & 2u) != 0, has_hi = (flags_last[l] & 4u) != 0;   // the line continues below / above
    const double p0 = w0 / tg, pn = wn / tg;
    double aF = 0.0, cF = 0.0, aL = 0.0, cL = 0.0, klo = 0.0, khi = 0.0;
    if (has_lo && has_hi) {                       // a middle rank: psi_lo = w, psi_hi = reversed w
        aF = -w0; cF = -wn; aL = -wn; cL = -w0;
    } else if (has_hi) {                          // first rank: row 0 is the global line start
        const double delta = dt * coeff_first[l] - tg;
        const double kappa = delta / (1.0 + delta * p0);
        klo = kappa * pn;                         // psi_hi = rev(w) - klo * w
        cF = -(wn - klo * w0);
        cL = -(w0 - klo * wn);
    } else if (has_lo) {                          // last rank: row n-1 is the global line end
        const double delta = dt * coeff_last[l] - tg;
        const double kappa = delta / (1.0 + delta * p0);
        khi = kappa * pn;                         // psi_lo = w - khi * rev(w)
        aF = -(w0 - khi * wn);
        aL = -(wn - khi * w0);
    }
    mat[l] = aF; mat[nlines + l] = cF; mat[2 * nlines + l] = aL; mat[3 * nlines + l] = cL;
    kap[l] = klo; kap[nlines + l] = khi;
}

// per step, after the interface solve: the coefficients of w[i] and w[n-1-i] in the correction of every line
__global__ __launch_bounds__(256) void k_deferred_exact_coef(const double *__restrict__ xlo, const double *__restrict__ xhi,
                                                             const double *__restrict__ kap, long nlines,
                                                             double *__restrict__ clo, double *__restrict__ chi)
{
    const long l = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= nlines) return;
    const double lo = xlo[l], hi = xhi[l];        // (0 where there is no neighbour: k_interface)
    clo[l] = __builtin_fma(-kap[l], hi, lo);            // first rank: xlo = 0, c_lo = -klo * xhi
    chi[l] = __builtin_fma(-kap[nlines + l], lo, hi);   // last rank:  xhi = 0, c_hi = -khi * xlo
}

// weights built on the host (adi_axis0_weights.hpp) to the device; synchronises: they live on the caller's stack frame
static int upload_weights(const std::vector<double> &w, double *d_w, hipStream_t st)
{
    ADI_HIP_TRY(hipMemcpyAsync(d_w, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice, st));
    ADI_HIP_TRY(hipStreamSynchronize(st));
    return ADI_OK;
}

}  // namespace adi

using namespace adi;

extern "C" {

int adi_axis0_weights_host(int n, double theta, double gam, int kind, double tol, double *h_w, int *h_reach)
{
    ADI_REQUIRE(n >= 2 && h_w && h_reach && tol >= 0.0, "adi_axis0_weights_host: bad argument");
    ADI_REQUIRE(kind == ADI_AXIS0_WEIGHTS_DOTS || kind == ADI_AXIS0_WEIGHTS_DEFERRED, "adi_axis0_weights_host: bad kind %d", kind);
    axis0_weights(n, theta, gam, kind == ADI_AXIS0_WEIGHTS_DEFERRED, h_w, tol, h_reach);
    return ADI_OK;
}

int adi_axis0_dots_setup(int n, double theta, double gam, double *d_weights, void *stream)
{
    ADI_REQUIRE(n >= 2 && d_weights, "adi_axis0_dots_setup: bad argument");
    std::vector<double> u(n);      // first column of tridiag(-tg, 1+2tg, -tg)^-1
    axis0_weights(n, theta, gam, false, u.data());
    return upload_weights(u, d_weights, as_stream(stream));
}

int adi_axis0_deferred_setup(int n, double theta, double gam, double tol, double *d_w, double *h_omega, int *h_reach,
                             void *stream)
{
    ADI_REQUIRE(n >= 2 && d_w && h_omega && h_reach && tol >= 0.0, "adi_axis0_deferred_setup: bad argument");
    // w = tg * tridiag(-tg, 1+2tg, -tg)^-1 e_0 (n x n); the closure of the far end does not matter where w has decayed
    // there, which is the condition the caller tests (*h_reach < n)
    std::vector<double> w(n);
    axis0_weights(n, theta, gam, true, w.data(), tol, h_reach);
    *h_omega = w[0];
    return upload_weights(w, d_w, as_stream(stream));
}

int adi_interface_solve(const double *d_cond_all, int nranks, int rank, long nlines, double *d_xlo, double *d_xhi,
                        void *stream)
{
    ADI_REQUIRE(d_cond_all && d_xlo && d_xhi && nranks >= 1 && rank >= 0 && rank < nranks && nlines > 0,
                "adi_interface_solve: bad argument");
    hipLaunchKernelGGL(k_interface, dim3((unsigned)((nlines + 255) / 256)), dim3(256), 0, as_stream(stream), d_cond_all,
                       nranks, rank, nlines, d_xlo, d_xhi);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_interface_pair(const double *d_my_lo, const double *d_my_hi, const double *d_prev_hi, const double *d_next_lo,
                       long nlines, double *d_xlo, double *d_xhi, void *stream)
{
    ADI_REQUIRE(d_xlo && d_xhi && nlines > 0, "adi_interface_pair: bad argument");
    ADI_REQUIRE((!d_prev_hi || d_my_lo) && (!d_next_lo || d_my_hi), "adi_interface_pair: missing own window");
    hipLaunchKernelGGL(k_interface_pair, dim3((unsigned)((nlines + 255) / 256)), dim3(256), 0, as_stream(stream), d_my_lo,
                       d_my_hi, d_prev_hi, d_next_lo, nlines, d_xlo, d_xhi);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_interface_deferred(const double *d_first, const double *d_last, const double *d_prev_last,
                           const double *d_next_first, double omega, long nlines, double *d_ulo, double *d_uhi,
                           void *stream)
{
    ADI_REQUIRE(d_ulo && d_uhi && nlines > 0, "adi_interface_deferred: bad argument");
    ADI_REQUIRE((!d_prev_last || d_first) && (!d_next_first || d_last), "adi_interface_deferred: missing own plane");
    ADI_REQUIRE(omega >= 0.0 && omega < 1.0, "adi_interface_deferred: omega = %g is not a decaying weight", omega);
    const double idet = 1.0 / (1.0 - omega * omega);
    hipLaunchKernelGGL(k_interface_deferred, dim3((unsigned)((nlines + 255) / 256)), dim3(256), 0, as_stream(stream),
                       d_first, d_last, d_prev_last, d_next_first, omega, idet, nlines, d_ulo, d_uhi);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}
int adi_interface_deferred_lines(const double *d_first, const double *d_last, const double *d_prev_last,
                                 const double *d_next_first, const double *d_om_lo_own, const double *d_om_hi_prev,
                                 const double *d_om_hi_own, const double *d_om_lo_next, long nlines, double *d_ulo,
                                 double *d_uhi, const uint8_t *d_uni_lo, const uint8_t *d_uni_hi, double *d_ulo_uni,
                                 double *d_uhi_uni, void *stream)
{
    ADI_REQUIRE(d_first && d_last && d_ulo && d_uhi && nlines > 0, "adi_interface_deferred_lines: bad argument");
    ADI_REQUIRE(!d_prev_last || (d_om_lo_own && d_om_hi_prev), "adi_interface_deferred_lines: lower boundary without its weights");
    ADI_REQUIRE(!d_next_first || (d_om_hi_own && d_om_lo_next), "adi_interface_deferred_lines: upper boundary without its weights");
    hipLaunchKernelGGL(k_interface_deferred_lines, dim3((unsigned)((nlines + 255) / 256)), dim3(256), 0, as_stream(stream),
                       d_first, d_last, d_prev_last, d_next_first, d_om_lo_own, d_om_hi_prev, d_om_hi_own, d_om_lo_next,
                       nlines, d_ulo, d_uhi, d_uni_lo, d_uni_hi, d_ulo_uni, d_uhi_uni);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_deferred_lines_apply(double *d_x, int nx, long plane_stride, long plane_cells, const int *d_cells, long nflag,
                             const double *d_wc, int K, const double *d_u, int from_high_end, const int *d_nrows, void *stream)
{
    ADI_REQUIRE(d_x && d_u && nx > 0 && plane_cells > 0 && plane_stride >= plane_cells && K >= 0 && K <= nx && nflag >= 0,
                "adi_deferred_lines_apply: bad argument");
    if (nflag == 0 || K == 0) return ADI_OK;
    ADI_REQUIRE(d_cells && d_wc, "adi_deferred_lines_apply: flagged lines without their cells / weights");
    const unsigned gy = (unsigned)(K < 64 ? K : 64);
    hipLaunchKernelGGL(k_deferred_lines_apply, dim3((unsigned)((nflag + 255) / 256), gy), dim3(256), 0, as_stream(stream), d_x, nx,
                       plane_stride, d_cells, nflag, d_wc, K, d_u, from_high_end, d_nrows);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_deferred_exact_setup(const uint8_t *d_flags_first, const uint8_t *d_flags_last, const double *d_coeff_first,
                             const double *d_coeff_last, double theta, double gam, double dt, double w0, double wn,
                             long nlines, double *d_mat, double *d_kap, void *stream)
{
    ADI_REQUIRE(d_flags_first && d_flags_last && d_coeff_first && d_coeff_last && d_mat && d_kap && nlines > 0,
                "adi_deferred_exact_setup: bad argument");
    ADI_REQUIRE(theta * gam > 0.0 && w0 > 0.0, "adi_deferred_exact_setup: needs theta*gam > 0");
    hipLaunchKernelGGL(k_deferred_exact_setup, dim3((unsigned)((nlines + 255) / 256)), dim3(256), 0, as_stream(stream),
                       d_flags_first, d_flags_last, d_coeff_first, d_coeff_last, theta * gam, dt, w0, wn, nlines, d_mat, d_kap);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_interface_solve_uniform(const double *d_g_all, const double *d_mat_all, const double *d_scal_all, int nranks, int rank,
                                long nlines, double *d_xlo, double *d_xhi, void *stream)
{
    ADI_REQUIRE(d_g_all && d_mat_all && d_scal_all && d_xlo && d_xhi && nranks >= 2 && rank >= 0 && rank < nranks && nlines > 0,
                "adi_interface_solve_uniform: bad argument");
    hipLaunchKernelGGL(k_interface_uniform, dim3((unsigned)((nlines + 255) / 256)), dim3(256), 0, as_stream(stream), d_g_all,
                       d_mat_all, d_scal_all, nranks, rank, nlines, d_xlo, d_xhi);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_deferred_exact_coef(const double *d_xlo, const double *d_xhi, const double *d_kap, long nlines, double *d_clo,
                            double *d_chi, void *stream)
{
    ADI_REQUIRE(d_xlo && d_xhi && d_kap && d_clo && d_chi && nlines > 0, "adi_deferred_exact_coef: bad argument");
    hipLaunchKernelGGL(k_deferred_exact_coef, dim3((unsigned)((nlines + 255) / 256)), dim3(256), 0, as_stream(stream), d_xlo,
                       d_xhi, d_kap, nlines, d_clo, d_chi);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}
}  // extern "C"
