// adi_explicit.hip -- K1, the explicit stage (hand-written HIP for gfx950, HBM-bound):
//   k_explicit_v5     the masked 7-point explicit stage -> R0 (lap1D_x/y/z + R0, adi3d_numba_coeff.py:240-288, :298),
//                     2.5-D marching form; <.., DOTS>: pass A of the slab decomposition folded in (partial dot products
//                     that adi_axis0_dots_finish, adi_condense.hip, turns into the six numbers of a line)
//   k_explicit_cell   the same, one thread per cell (odd nz, unaligned views)
// The flag / coefficient builders and the byte kernels of a layer birth are in adi_fields.hip.
#include "adi_cart_host.hpp"
#include "adi_cell_dev.hpp"

namespace adi {

template <int JT, bool DOTS = false>
__global__ __launch_bounds__(256) void k_explicit_v5(const double *__restrict__ T, const uint8_t *__restrict__ flags,
                                                     double *__restrict__ R0, Lay L, double invdx2, double f,
                                                     int jslab, int ktiles, int ichunk, long ntiles, int i_begin,
                                                     int i_end, const double *__restrict__ wu = nullptr,
                                                     double *__restrict__ part = nullptr, int i_org = 0, int n_line = 0,
                                                     int nt = 1)
{
#pragma clang fp contract(off)
    const int nx = L.nx, ny = L.ny, nz = L.nz;
    const long tile = xcd_chunk_tile(blockIdx.x, ntiles);
    // tile order: [slab][i-chunk][j-tile in slab][k-tile]
    const int jt_per_slab = (jslab + JT - 1) / JT;
    const int nchunk = (i_end - i_begin + ichunk - 1) / ichunk;
    const long per_chunk = (long)jt_per_slab * ktiles;
    const long per_slab = per_chunk * nchunk;
    const unsigned t32 = (unsigned)tile, pch = (unsigned)per_chunk, psl = (unsigned)per_slab;
    const int slab = (int)(t32 / psl);
    unsigned rem = t32 - (unsigned)slab * psl;
    const int ic = (int)(rem / pch);
    rem -= (unsigned)ic * pch;
    const int jt = (int)(rem / (unsigned)ktiles), kt = (int)(rem - (unsigned)jt * (unsigned)ktiles);
    const int j0 = slab * jslab + jt * JT;
    int jend = j0 + JT;
    if (jend > (slab + 1) * jslab) jend = (slab + 1) * jslab;
    if (jend > ny) jend = ny;
    if (j0 >= jend) return;
    const int i0 = i_begin + ic * ichunk;
    const int i1 = (i0 + ichunk < i_end) ? i0 + ichunk : i_end;
    const int k0 = kt * 512 + 2 * (int)threadIdx.x;
    const bool kin = k0 < nz;
    const int lane = threadIdx.x & 63;
    const long sx = L.sx, sy = nz;
    const double2 zero2 = make_double2(0.0, 0.0);
    const long pbase = (long)j0 * sy + k0;
    // lane 0 / lane 63 fetch the value just outside the wave's k range (one load per row)
    const bool edge = kin && ((lane == 0 && k0 > 0) || (lane == 63 && k0 + 2 < nz));
    const long eoff = (lane == 0) ? -1 : 2;
    const bool up = kin && j0 > 0, dn = kin && jend < ny;

    double2 tm[JT], tc[JT], tp[JT], tq[JT];
    unsigned fl[JT], fln[JT];
    double ke[JT], ken[JT];
    double2 hm = zero2, hp = zero2, hmn = zero2, hpn = zero2;
    auto load_plane = [&](int i, double2 (&dst)[JT]) {
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            dst[r] = zero2;
            if (kin && j0 + r < jend && i >= 0 && i < nx)
                dst[r] = *reinterpret_cast<const double2 *>(T + (long)i * sx + pbase + (long)r * sy);
        }
    };
    auto load_meta = [&](int i, unsigned (&F)[JT], double (&E)[JT], double2 &HM, double2 &HP) {
        const long p = (long)i * sx + pbase;
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            F[r] = 0; E[r] = 0.0;
            if (kin && j0 + r < jend) F[r] = *reinterpret_cast<const uint16_t *>(flags + p + (long)r * sy);
            if (edge && j0 + r < jend) E[r] = T[p + (long)r * sy + eoff];
        }
        HM = zero2; HP = zero2;
        if (up) HM = *reinterpret_cast<const double2 *>(T + p - sy);
        if (dn) HP = *reinterpret_cast<const double2 *>(T + p + (long)(jend - j0) * sy);
    };
    load_plane(i0 - 1, tm);
    load_plane(i0, tc);
    load_plane(i0 + 1, tp);
    load_meta(i0, fl, ke, hm, hp);
    double2 su[DOTS ? JT : 1], sv[DOTS ? JT : 1];
    if (DOTS) {
#pragma unroll
        for (int r = 0; r < JT; ++r) { su[r] = zero2; sv[r] = zero2; }
    }
    // DOTS: lines start at plane i_org and have n_line rows; this launch covers whole chunks of them
    for (int i = i0; i < i1; ++i) {
        const long p = (long)i * sx + pbase;
        const bool more = i + 1 < i1;
        double wa = 0.0, wb = 0.0;
        if (DOTS) { wa = wu[i - i_org]; wb = wu[n_line - 1 - (i - i_org)]; }          // block-uniform: scalar loads
        if (more) {
            load_plane(i + 2, tq);
            load_meta(i + 1, fln, ken, hmn, hpn);
        }
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            const bool rin = j0 + r < jend;
            const long q = p + (long)r * sy;
            double kl = __shfl_up(tc[r].y, 1), kr = __shfl_down(tc[r].x, 1);
            if (lane == 0) kl = ke[r];
            if (lane == 63) kr = ke[r];
            const double2 jm = (r == 0) ? hm : tc[r > 0 ? r - 1 : 0];
            const double2 jp = (j0 + r + 1 == jend) ? hp : tc[r + 1 < JT ? r + 1 : JT - 1];
            const unsigned f0 = fl[r] & 0xffu, f1 = fl[r] >> 8;
            double r0v, r1v;
            {
                double L0 = 0.0, L1 = 0.0, L2 = 0.0;
                if (f0 & 1u) {
                    L0 = lap_axis(f0 & 2u, f0 & 4u, tm[r].x, tp[r].x, tc[r].x, invdx2);
                    L1 = lap_axis(f0 & 8u, f0 & 16u, jm.x, jp.x, tc[r].x, invdx2);
                    L2 = lap_axis(f0 & 32u, f0 & 64u, kl, tc[r].y, tc[r].x, invdx2);
                }
                r0v = tc[r].x + f * ((L0 + L1) + L2);
            }
            {
                double L0 = 0.0, L1 = 0.0, L2 = 0.0;
                if (f1 & 1u) {
                    L0 = lap_axis(f1 & 2u, f1 & 4u, tm[r].y, tp[r].y, tc[r].y, invdx2);
                    L1 = lap_axis(f1 & 8u, f1 & 16u, jm.y, jp.y, tc[r].y, invdx2);
                    L2 = lap_axis(f1 & 32u, f1 & 64u, tc[r].x, kr, tc[r].y, invdx2);
                }
                r1v = tc[r].y + f * ((L0 + L1) + L2);
            }
            if (kin && rin) st_stream2(reinterpret_cast<double2 *>(R0 + q), make_double2(r0v, r1v), nt != 0);
            if (DOTS) {
                su[r].x = __builtin_fma(wa, r0v, su[r].x); su[r].y = __builtin_fma(wa, r1v, su[r].y);
                sv[r].x = __builtin_fma(wb, r0v, sv[r].x); sv[r].y = __builtin_fma(wb, r1v, sv[r].y);
            }
        }
#pragma unroll
        for (int r = 0; r < JT; ++r) {
            tm[r] = tc[r]; tc[r] = tp[r]; tp[r] = tq[r];
            fl[r] = fln[r]; ke[r] = ken[r];
        }
        hm = hmn; hp = hpn;
    }
    if (DOTS) {
        const long nlines = (long)ny * nz;
        double *pu = part + (long)((i_begin - i_org) / ichunk + ic) * 2 * nlines, *pv = pu + nlines;   // global chunk id
#pragma unroll
        for (int r = 0; r < JT; ++r)
            if (kin && j0 + r < jend) {
                const long line = (long)(j0 + r) * nz + k0;
                *reinterpret_cast<double2 *>(pu + line) = su[r];
                *reinterpret_cast<double2 *>(pv + line) = sv[r];
            }
    }
}

// generic form (odd nz or unaligned views): one cell per thread
__global__ __launch_bounds__(256) void k_explicit_cell(const double *__restrict__ T, const uint8_t *__restrict__ flags,
                                                  double *__restrict__ R0, Lay L, double invdx2, double f, int i_begin,
                                                  int i_end)
{
#pragma clang fp contract(off)
    int i, j, k;
    long p;
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x + (long)i_begin * L.ny * L.nz;
    if (q >= (long)i_end * L.ny * L.nz) return;
    if (!cell_of(q, L, i, j, k, p)) return;
    unsigned fl;
    R0[p] = explicit_cell(T, flags, p, L, invdx2, f, fl, [] {});
}

// The marching kernel on the planes [i_begin, i_end), in chunks of ichunk planes per block.  part != nullptr: with the partial
// dot products of pass A (weights wu; the lines are the planes [i_org, i_org + n_line)).
static void launch_marching(const double *d_T, const uint8_t *d_flags, double *d_R0, const Lay &L, double invdx2, double f,
                            int i_begin, int i_end, int ichunk, const double *wu, double *part, int i_org, int n_line,
                            hipStream_t st)
{
    const int jslab = (L.ny + 7) / 8;
    const int nslab = (L.ny + jslab - 1) / jslab;
    const int ktiles = (L.nz + 511) / 512;
    const int nchunk = (i_end - i_begin + ichunk - 1) / ichunk;
    const long ntiles = (long)nslab * nchunk * ((jslab + 1) / 2) * ktiles;
    const auto kernel = part != nullptr ? k_explicit_v5<2, true> : k_explicit_v5<2, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)ntiles), dim3(256), 0, st, d_T, d_flags, d_R0, L, invdx2, f, jslab, ktiles, ichunk,
                       ntiles, i_begin, i_end, wu, part, i_org, n_line, store_policy_nt(L.nx, L.sx));
}

}  // namespace adi

using namespace adi;

extern "C" {

int adi_explicit_rhs_planes(const double *d_T, const uint8_t *d_flags, int nx, int ny, int nz, long plane_stride,
                            double dx, double dt, double kappa, double theta, double *d_R0, int i_begin, int i_end,
                            void *stream)
{
    ADI_REQUIRE(d_T && d_flags && d_R0, "adi_explicit_rhs: null argument");
    ADI_REQUIRE(d_T != d_R0, "adi_explicit_rhs: output aliases input");
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    if (int rc = check_plane_range("adi_explicit_rhs_planes", i_begin, i_end, nx)) return rc;
    if (i_begin == i_end) return ADI_OK;
    const double invdx2 = 1.0 / (dx * dx);
    const double f = dt * kappa * (1.0 - theta);
    const int np = i_end - i_begin;
    if (pair_vec(L, d_flags, d_T, d_R0)) {
        // planes marched per block: 32 amortises the leading halo plane; short plane ranges (the boundary windows of a
        // slab) get shorter chunks so that the launch still has ~16 chunks' worth of blocks
        launch_marching(d_T, d_flags, d_R0, L, invdx2, f, i_begin, i_end, dots_ichunk(np), nullptr, nullptr, 0, 0,
                        as_stream(stream));
    } else {    // odd nz / unaligned views: one thread per cell
        const long cells = (long)np * ny * nz;
        hipLaunchKernelGGL(k_explicit_cell, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, as_stream(stream), d_T,
                           d_flags, d_R0, L, invdx2, f, i_begin, i_end);
    }
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_explicit_rhs(const double *d_T, const uint8_t *d_flags, int nx, int ny, int nz, long plane_stride, double dx,
                     double dt, double kappa, double theta, double *d_R0, void *stream)
{
    return adi_explicit_rhs_planes(d_T, d_flags, nx, ny, nz, plane_stride, dx, dt, kappa, theta, d_R0, 0, nx, stream);
}

// ---- pass A folded into the explicit stage (slab decomposition) ------------------------------------------------------
int adi_axis0_dots_supported(int nx, int ny, int nz, long plane_stride)
{
    Lay L;
    if (make_lay(nx, ny, nz, plane_stride, &L) != ADI_OK) return 0;
    return (nx >= 2 && pair_vec(L, nullptr)) ? 1 : 0;      // the marching explicit kernel's own conditions
}

int adi_axis0_dots_workspace(int nx, int ny, int nz, size_t *part_bytes, size_t *list_bytes)
{
    ADI_REQUIRE(nx > 0 && ny > 0 && nz > 0 && part_bytes && list_bytes, "adi_axis0_dots_workspace: bad argument");
    *part_bytes = (size_t)dots_nchunk(nx) * 2 * (size_t)ny * nz * sizeof(double);
    *list_bytes = ((size_t)ny * nz + 1) * sizeof(unsigned);
    return ADI_OK;
}

int adi_axis0_dots_ichunk(int n_line) { return dots_ichunk(n_line); }

int adi_explicit_rhs_dots(const double *d_T, const uint8_t *d_flags, int nx, int ny, int nz, long plane_stride,
                          double dx, double dt, double kappa, double theta, double *d_R0, int i_begin, int i_end,
                          int i_org, int n_line, const double *d_weights, double *d_part, void *stream)
{
    ADI_REQUIRE(d_T && d_flags && d_R0 && d_weights && d_part, "adi_explicit_rhs_dots: null argument");
    ADI_REQUIRE(d_T != d_R0, "adi_explicit_rhs_dots: output aliases input");
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    ADI_REQUIRE(i_begin >= 0 && i_end <= nx && i_begin < i_end, "adi_explicit_rhs_dots: bad plane range [%d, %d)", i_begin,
                i_end);
    ADI_REQUIRE(n_line >= 2 && i_org >= 0 && i_org + n_line <= nx && i_begin >= i_org && i_end <= i_org + n_line,
                "adi_explicit_rhs_dots: planes [%d, %d) outside the lines [%d, %d)", i_begin, i_end, i_org, i_org + n_line);
    ADI_REQUIRE(pair_vec(L, d_flags, d_T, d_R0, d_part),
                "adi_explicit_rhs_dots: needs even nz / plane stride and 16-byte aligned fields");
    // chunks of planes are counted from the start of the lines: a launch on part of the planes (interior first, the
    // planes next to the halos once those have landed) covers whole chunks, except at the end of the lines
    const int ichunk = dots_ichunk(n_line);
    ADI_REQUIRE((i_begin - i_org) % ichunk == 0 && ((i_end - i_org) % ichunk == 0 || i_end == i_org + n_line),
                "adi_explicit_rhs_dots: plane range [%d, %d) does not cover whole chunks of %d planes", i_begin, i_end, ichunk);
    launch_marching(d_T, d_flags, d_R0, L, 1.0 / (dx * dx), dt * kappa * (1.0 - theta), i_begin, i_end, ichunk, d_weights,
                    d_part, i_org, n_line, as_stream(stream));
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // extern "C"

