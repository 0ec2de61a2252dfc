// adi_matmap.hip -- the Cartesian step on a grid of several materials (include/adi_hip.h, "Several materials"; DESIGN.md
// section 6l): every cell carries a material id, the coupling of a cell to a neighbour is the pair-table entry
// G[own id][neighbour's id], and each row is divided by its own C = rho cp.  Hand-written HIP for gfx950:
//   k_matmap_build_coeffs   Robin coefficient + Neumann flux fields of the three axes, (h A) / (C_id V) per exposed face
//                           (map_coeffs_cell of adi_matmap_dev.hpp); k_mapcoeffs_planes: the same cells' values on a range of
//                           axis-2 planes only
//   k_matmap_explicit       R0 = T + (1 - theta) sum G[id][id_n] (T_n - T)  [+ dt S / C_id]
//   k_matmap_sweep_contig   sweep along memory axis 2: a line's segments in the lanes of one wave (condense / pcr_solve /
//                           back_solve of adi_core.hpp with per-row off-diagonals), lines of at most kMaxFastLine rows
//   k_matmap_sweep_strided  sweep along memory axes 0 and 1: tiles of adjacent lines, segments of M rows in registers with the
//                           off-diagonals as table indices (TableCoef), separators through LDS; lines of at most kMaxFastLine rows
//   k_matmap_sweep_lines    any axis beyond kMaxFastLine rows: one thread per line, the subtraction-free elimination with c' in
//                           an HBM workspace and d' in the output
// 64-bit element offsets throughout; no kernel here uses scratch (tests/test_matmap_cpu.py reads it from the code object).
#include "adi_matmap_dev.hpp"

namespace adi {

__global__ __launch_bounds__(256) void k_matmap_build_coeffs(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ ids,
                                                             Lay L, double A, MapScal s, MapFaceSpec h, MapFaceSpec q,
                                                             double *__restrict__ c0, double *__restrict__ c1,
                                                             double *__restrict__ c2, double *__restrict__ q0,
                                                             double *__restrict__ q1, double *__restrict__ q2)
{
    __shared__ double sG[kMapMaxMat * kMapMaxMat], sC[kMapMaxMat];
    map_tables_to_lds(s, sG, sC);
    int i, j, k;
    long p;
    if (!cell_of((long)blockIdx.x * blockDim.x + threadIdx.x, L, i, j, k, p)) return;
    map_coeffs_cell(mask, ids, L, A, sC, h, q, i, j, k, p, c0, c1, c2, q0, q1, q2);
}

// The same cells' values on the planes [k0, k1) of axis 2 only (the planes a birth or a deposit touches): one thread per cell of
// the range, nothing outside it is written.  Only the C table goes to LDS.
__global__ __launch_bounds__(256) void k_mapcoeffs_planes(const uint8_t *__restrict__ mask,
                                                                    const uint8_t *__restrict__ ids, Lay L, int k0, int k1,
                                                                    double A, MapScal s, MapFaceSpec h, MapFaceSpec q,
                                                                    double *__restrict__ c0, double *__restrict__ c1,
                                                                    double *__restrict__ c2, double *__restrict__ q0,
                                                                    double *__restrict__ q1, double *__restrict__ q2)
{
    __shared__ double sC[kMapMaxMat];
    {
        const double *kc = s.c;
        if (threadIdx.x < kMapMaxMat) sC[threadIdx.x] = kc[threadIdx.x];
        __syncthreads();
    }
    int i, j, k;
    long p;
    if (!cell_of_k((long)blockIdx.x * blockDim.x + threadIdx.x, L, k0, k1, i, j, k, p)) return;
    map_coeffs_cell(mask, ids, L, A, sC, h, q, i, j, k, p, c0, c1, c2, q0, q1, q2);
}

// Explicit stage: kExplicitCells cells per thread, a block's threads on consecutive cells (the table's way into LDS is paid once
// per 1024 cells); the six neighbours and their ids are read only where the flags byte has them, in the order axis 0 -, 0 +,
// 1 -, 1 +, 2 -, 2 + of the definition (contraction off: the operations of MaterialMap.step_reference).
constexpr int kExplicitCells = 4;
__global__ __launch_bounds__(256) void k_matmap_explicit(const double *__restrict__ T, const double *__restrict__ S,
                                                         const uint8_t *__restrict__ flags, const uint8_t *__restrict__ ids,
                                                         Lay L, MapScal s, double *__restrict__ out)
{
#pragma clang fp contract(off)
    __shared__ double sG[kMapMaxMat * kMapMaxMat], sC[kMapMaxMat];
    map_tables_to_lds(s, sG, sC);
    const long sx = L.sx, sy = L.nz;
    const long q0 = (long)blockIdx.x * (kExplicitCells * 256) + threadIdx.x;
#pragma unroll
    for (int u = 0; u < kExplicitCells; ++u) {
        int i, j, k;
        long p;
        if (!cell_of(q0 + u * 256, L, i, j, k, p)) continue;
        const double t = T[p];
        const unsigned fl = flags[p];
        double r = t;
        if (fl & 1u) {
            const unsigned idi = ids[p] & (kMapMaxMat - 1);
            const double *row = sG + idi * kMapMaxMat;
            double acc = 0.0;
            if (fl & 2u) acc += row[ids[p - sx] & (kMapMaxMat - 1)] * (T[p - sx] - t);
            if (fl & 4u) acc += row[ids[p + sx] & (kMapMaxMat - 1)] * (T[p + sx] - t);
            if (fl & 8u) acc += row[ids[p - sy] & (kMapMaxMat - 1)] * (T[p - sy] - t);
            if (fl & 16u) acc += row[ids[p + sy] & (kMapMaxMat - 1)] * (T[p + sy] - t);
            if (fl & 32u) acc += row[ids[p - 1] & (kMapMaxMat - 1)] * (T[p - 1] - t);
            if (fl & 64u) acc += row[ids[p + 1] & (kMapMaxMat - 1)] * (T[p + 1] - t);
            r = t + s.om * acc;
            if (S != nullptr) r = r + (s.dt * S[p]) / sC[idi];
        }
        out[p] = r;
    }
}

// Sweep along the contiguous axis: Lp = next_pow2(ceil(n / M)) lanes of a wave hold the segments of M rows of one line, 64 / Lp
// lines per wave.  Pack arrays are read only where the definition uses them: coeff / qflux on free cells exposed along the
// axis (adi_matmap_build_coeffs leaves zeros elsewhere), dir_val on Dirichlet cells.
template <int M, bool HAS_DIR, bool HAS_Q>
__global__ __launch_bounds__(256) void k_matmap_sweep_contig(
    const double *__restrict__ in, const uint8_t *__restrict__ flags, const uint8_t *__restrict__ ids,
    const double *__restrict__ coeff, const uint8_t *__restrict__ dmask, const double *__restrict__ dval,
    const double *__restrict__ qf, double *__restrict__ out, Lay L, int Lp, MapScal s)
{
    __shared__ double sG[kMapMaxMat * kMapMaxMat];
    map_tables_to_lds(s, sG, nullptr);
    const int n = L.nz;
    const long nlines = (long)L.nx * L.ny;
    const int lane = threadIdx.x & 63;
    const int sh = __ffs(Lp) - 1;
    const long unit = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int li = lane & (Lp - 1);
    const long line = unit * (64 >> sh) + (lane >> sh);
    const bool active = line < nlines;                  // (no early return: every lane takes part in the shuffles)
    const int r0 = li * M;
    const long pi = active ? line / L.ny : 0;
    const long base = pi * L.sx + (active ? line - pi * L.ny : 0) * (long)n + r0;

    double a[M], b[M], c[M], d[M];
#pragma unroll
    for (int r = 0; r < M; ++r) {
        a[r] = 0.0; c[r] = 0.0; b[r] = 1.0; d[r] = 0.0;   // rows beyond the line / of a lane without a line: identity
        if (active && r0 + r < n) {
            const long p = base + r;
            const unsigned f = flags[p];
            const bool m = f & 1u, lo = (f >> 5) & 1u, hi = (f >> 6) & 1u;
            const bool dir = HAS_DIR && m && dmask[p] != 0;
            const bool fr = m && !dir;
            const double *row = sG + (m ? (ids[p] & (kMapMaxMat - 1)) : 0) * kMapMaxMat;
            const double plo = (fr && lo) ? row[ids[p - 1] & (kMapMaxMat - 1)] : 0.0;
            const double phi = (fr && hi) ? row[ids[p + 1] & (kMapMaxMat - 1)] : 0.0;
            const bool ex = fr && !(lo && hi);
            const double co = ex ? coeff[p] : 0.0;
            const double qv = (HAS_Q && ex) ? qf[p] : 0.0;
            const double dv = dir ? dval[p] : 0.0;
            double e, pp, qq;
            map_row<HAS_DIR, HAS_Q>(m, lo, hi, dir, in[p], co, dv, qv, plo, phi, s.dt, s.Tinf, e, pp, qq, d[r]);
            a[r] = -pp; c[r] = -qq; b[r] = (e + pp) + qq;
        }
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
#pragma unroll
    for (int r = 0; r < M; ++r)
        if (active && r0 + r < n) out[base + r] = x[r];
}

// Sweep along a strided axis (memory axes 0 and 1, lines of at most kMaxFastLine rows): the layout of strided_tile_general.  A
// workgroup owns LINES adjacent lines and all Lp segments of each; thread (sg, kk) keeps the M rows of segment sg of line kk in
// registers, lanes along the contiguous direction (every access coalesced, LINES * 8 bytes per row piece).  The off-diagonals are
// TableCoefs: one byte per row, the value read from the table in LDS.  Only the condensation numbers of a segment travel through
// LDS (tile_separators: line-major regrouping, in-wave PCR) and the separator values back.  Material data: the id byte of every
// row, plus the two neighbours' where the segment ends.  sm: 7 * LINES * (Lp + 1) doubles.
template <int M, bool HAS_DIR, bool HAS_Q>
__global__ __launch_bounds__(M <= 8 ? 1024 : 512) void k_matmap_sweep_strided(
    const double *__restrict__ in, const uint8_t *__restrict__ flags, const uint8_t *__restrict__ ids,
    const double *__restrict__ coeff, const uint8_t *__restrict__ dmask, const double *__restrict__ dval,
    const double *__restrict__ qf, double *__restrict__ out, LineGeom g, int Lp, int LINES, int tiles_inner, long ntiles, MapScal s)
{
    extern __shared__ __align__(16) double sm[];
    __shared__ double sN[kMapMaxMat * kMapMaxMat];       // -theta G[m][n]: the off-diagonals themselves
    for (int t = threadIdx.x; t < kMapMaxMat * kMapMaxMat; t += blockDim.x) sN[t] = -s.g[t];
    __syncthreads();
    const int tid = (int)threadIdx.x;
    const long tile = xcd_chunk_tile(blockIdx.x, ntiles);
    const long to = tile / tiles_inner;
    const int ti = (int)(tile - to * tiles_inner);
    const int kk = tid & (LINES - 1), sg = tid >> (__ffs(LINES) - 1);
    const int kcol = ti * LINES + kk;
    const bool active = kcol < g.n_inner;               // (no early return: every thread meets the barriers of tile_separators)
    const long base = to * g.outer_stride + kcol;
    const int r0 = sg * M;

    TableCoef<M> a, c;
    a.clear(); c.clear(); a.t = sN; c.t = sN;
    double b[M], d[M];
    {
        unsigned f[M], id[M];
#pragma unroll
        for (int r = 0; r < M; ++r) {
            const bool valid = active && r0 + r < g.n;
            const long p = base + (long)(r0 + r) * g.stride;
            f[r] = valid ? flags[p] : 0u;
            id[r] = valid ? (ids[p] & (kMapMaxMat - 1)) : 0u;
        }
        // the ids across the two ends of the segment, where the flags say that neighbour is in the mask
        const unsigned idlo = ((f[0] >> g.lbit) & 1u) ? (ids[base + (long)(r0 - 1) * g.stride] & (kMapMaxMat - 1)) : 0u;
        const unsigned idhi = ((f[M - 1] >> (g.lbit + 1)) & 1u) ? (ids[base + (long)(r0 + M) * g.stride] & (kMapMaxMat - 1)) : 0u;
#pragma unroll
        for (int r = 0; r < M; ++r) {
            b[r] = 1.0; d[r] = 0.0;                       // rows beyond the line / of a lane without a line: identity
            if (active && r0 + r < g.n) {
                const long p = base + (long)(r0 + r) * g.stride;
                const bool m = f[r] & 1u, lo = (f[r] >> g.lbit) & 1u, hi = (f[r] >> (g.lbit + 1)) & 1u;
                const bool dir = HAS_DIR && m && dmask[p] != 0;
                const bool fr = m && !dir;
                const unsigned plo_i = id[r] * kMapMaxMat + (r == 0 ? idlo : id[r > 0 ? r - 1 : 0]);
                const unsigned phi_i = id[r] * kMapMaxMat + (r == M - 1 ? idhi : id[r < M - 1 ? r + 1 : M - 1]);
                const bool ex = fr && !(lo && hi);
                const double co = ex ? coeff[p] : 0.0;
                const double qv = (HAS_Q && ex) ? qf[p] : 0.0;
                const double dv = dir ? dval[p] : 0.0;
                double e, pp, qq;
                map_row<HAS_DIR, HAS_Q>(m, lo, hi, dir, in[p], co, dv, qv, -sN[plo_i], -sN[phi_i], s.dt, s.Tinf, e, pp, qq, d[r]);
                a.set(r, plo_i, fr && lo);
                c.set(r, phi_i, fr && hi);
                b[r] = (e + pp) + qq;
            }
        }
    }
    double ip[M - 1];
    Cond k;
    condense<M>(a, b, c, d, ip, k);
    double xL, xS;
    tile_separators(sm, tid, kk, sg, Lp, LINES, a[M - 1], b[M - 1], c[M - 1], d[M - 1], k, xL, xS);
    double x[M];
    back_solve<M>(a, c, d, ip, xL, xS, x);
#pragma unroll
    for (int r = 0; r < M; ++r)
        if (active && r0 + r < g.n) out[base + (long)(r0 + r) * g.stride] = x[r];
}

// One thread per line.  Forward pass in the excess form (no subtraction: e >= 1, p, q >= 0):
//   w = p_i / P_{i-1},  s_i = e_i + w s_{i-1},  P_i = s_i + q_i,  d'_i = (d_i + w P_{i-1} d'_{i-1}) / P_i,  c'_i = q_i / P_i
// then x_i = d'_i + c'_i x_{i+1}.  c' goes to the workspace wc, d' to `out`, which the backward pass overwrites with x.
// The id of a row's upper neighbour is loaded once and carried to the next two rows.
template <bool HAS_DIR, bool HAS_Q>
__global__ __launch_bounds__(256) void k_matmap_sweep_lines(
    const double *__restrict__ in, const uint8_t *__restrict__ flags, const uint8_t *__restrict__ ids,
    const double *__restrict__ coeff, const uint8_t *__restrict__ dmask, const double *__restrict__ dval,
    const double *__restrict__ qf, double *__restrict__ out, double *__restrict__ wc, LineGeom g, long inner_stride, MapScal s)
{
    __shared__ double sG[kMapMaxMat * kMapMaxMat];
    map_tables_to_lds(s, sG, nullptr);
    const long lid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (lid >= (long)g.n_inner * g.n_outer) return;
    const long o = lid / g.n_inner, kc = lid - o * g.n_inner;
    const long base = o * g.outer_stride + kc * inner_stride;
    const int n = g.n;
    unsigned idprev = 0, idcur = 0;
    bool have = false;                     // idcur already holds this row's id (loaded as the previous row's upper neighbour)
    double sp = 1.0, Pp = 1.0, ydp = 0.0;  // s, P and P * d' of the previous row
    for (int r = 0; r < n; ++r) {
        const long p = base + (long)r * g.stride;
        const unsigned f = flags[p];
        const bool m = f & 1u, lo = (f >> g.lbit) & 1u, hi = (f >> (g.lbit + 1)) & 1u;
        const bool dir = HAS_DIR && m && dmask[p] != 0;
        const bool fr = m && !dir;
        if (m && !have) idcur = ids[p] & (kMapMaxMat - 1);
        unsigned idn = 0;
        if (hi) idn = ids[p + g.stride] & (kMapMaxMat - 1);
        const double *row = sG + idcur * kMapMaxMat;
        const double plo = (fr && lo) ? row[idprev] : 0.0;
        const double phi = (fr && hi) ? row[idn] : 0.0;
        const bool ex = fr && !(lo && hi);
        const double co = ex ? coeff[p] : 0.0;
        const double qv = (HAS_Q && ex) ? qf[p] : 0.0;
        const double dv = dir ? dval[p] : 0.0;
        double e, pp, qq, d;
        map_row<HAS_DIR, HAS_Q>(m, lo, hi, dir, in[p], co, dv, qv, plo, phi, s.dt, s.Tinf, e, pp, qq, d);
        const double w = pp * frcp(Pp);
        const double sc = __builtin_fma(w, sp, e);
        const double P = sc + qq;
        const double yd = __builtin_fma(w, ydp, d);
        const double iP = frcp(P);
        wc[p] = qq * iP;
        out[p] = yd * iP;
        sp = sc; Pp = P; ydp = yd;
        idprev = idcur; idcur = idn; have = hi;
    }
    double x = 0.0;
    for (int r = n - 1; r >= 0; --r) {
        const long p = base + (long)r * g.stride;
        x = __builtin_fma(wc[p], x, out[p]);
        out[p] = x;
    }
}

// adi_matmap_build_coeffs (planes = false: the whole box) and adi_matmap_build_coeffs_planes (the planes [k_begin, k_end) of
// axis 2, not empty and inside the box); `who` names the entry in the error text
static int map_build_coeffs(const char *who, const uint8_t *d_mask, const uint8_t *d_ids, int nx, int ny, int nz,
                            long plane_stride, double dx, int nmat, const double *h_C, const int *h_mode, const double *h_scalar,
                            const double *const *d_h_field, const int *q_mode, const double *q_scalar,
                            const double *const *d_q_field, double *const *d_coeff, double *const *d_qflux, bool planes,
                            int k_begin, int k_end, void *stream)
{
#pragma clang fp contract(off)
    ADI_REQUIRE(d_mask && d_ids && h_C && h_mode && h_scalar && q_mode && q_scalar && d_coeff && d_qflux, "%s: null argument", who);
    ADI_REQUIRE(isfinite(dx) && dx > 0.0, "%s: dx must be finite and > 0", who);
    if (int rc = check_tables(who, nmat, nullptr, h_C)) return rc;
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    if (planes) ADI_REQUIRE(k_begin >= 0 && k_end <= nz && k_begin < k_end, "%s: bad plane range [%d, %d)", who, k_begin, k_end);
    MapFaceSpec h, q;
    if (int rc = make_face_specs(who, h_mode, h_scalar, d_h_field, q_mode, q_scalar, d_q_field, &h, &q)) return rc;
    for (int a = 0; a < 3; ++a) ADI_REQUIRE(d_coeff[a] && d_qflux[a], "%s: null output", who);
    MapScal s = {};
    const double A = dx * dx;
    const double V = dx * dx * dx;
    for (int m = 0; m < kMapMaxMat; ++m) s.c[m] = m < nmat ? h_C[m] * V : 1.0;
    if (planes) {
        const unsigned blocks = (unsigned)(((long)L.nx * L.ny * (k_end - k_begin) + 255) / 256);
        hipLaunchKernelGGL(k_mapcoeffs_planes, dim3(blocks), dim3(256), 0, as_stream(stream), d_mask, d_ids, L, k_begin,
                           k_end, A, s, h, q, d_coeff[0], d_coeff[1], d_coeff[2], d_qflux[0], d_qflux[1], d_qflux[2]);
    } else {
        hipLaunchKernelGGL(k_matmap_build_coeffs, dim3(cell_blocks(L)), dim3(256), 0, as_stream(stream), d_mask, d_ids, L, A, s, h,
                           q, d_coeff[0], d_coeff[1], d_coeff[2], d_qflux[0], d_qflux[1], d_qflux[2]);
    }
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // namespace adi

using namespace adi;

extern "C" {

int adi_matmap_build_coeffs(const uint8_t *d_mask, const uint8_t *d_ids, int nx, int ny, int nz, long plane_stride, double dx,
                            int nmat, const double *h_C, const int *h_mode, const double *h_scalar,
                            const double *const *d_h_field, const int *q_mode, const double *q_scalar,
                            const double *const *d_q_field, double *const *d_coeff, double *const *d_qflux, void *stream)
{
    return map_build_coeffs("adi_matmap_build_coeffs", d_mask, d_ids, nx, ny, nz, plane_stride, dx, nmat, h_C, h_mode, h_scalar,
                            d_h_field, q_mode, q_scalar, d_q_field, d_coeff, d_qflux, false, 0, nz, stream);
}

int adi_matmap_build_coeffs_planes(const uint8_t *d_mask, const uint8_t *d_ids, int nx, int ny, int nz, long plane_stride,
                                   double dx, int nmat, const double *h_C, const int *h_mode, const double *h_scalar,
                                   const double *const *d_h_field, const int *q_mode, const double *q_scalar,
                                   const double *const *d_q_field, double *const *d_coeff, double *const *d_qflux, int k_begin,
                                   int k_end, void *stream)
{
    return map_build_coeffs("adi_matmap_build_coeffs_planes", d_mask, d_ids, nx, ny, nz, plane_stride, dx, nmat, h_C, h_mode,
                            h_scalar, d_h_field, q_mode, q_scalar, d_q_field, d_coeff, d_qflux, true, k_begin, k_end, stream);
}

int adi_matmap_explicit(const double *d_T, const double *d_S, const uint8_t *d_flags, const uint8_t *d_ids, int nx, int ny,
                        int nz, long plane_stride, int nmat, const double *h_G, const double *h_C, double dt, double theta,
                        double *d_out, void *stream)
{
    ADI_REQUIRE(d_T && d_flags && d_ids && h_G && h_C && d_out, "adi_matmap_explicit: null argument");
    ADI_REQUIRE(d_T != d_out, "adi_matmap_explicit: output aliases input");
    ADI_REQUIRE(isfinite(dt) && dt > 0.0 && theta >= 0.0 && theta <= 1.0, "adi_matmap_explicit: bad dt or theta");
    if (int rc = check_tables("adi_matmap_explicit", nmat, h_G, h_C)) return rc;
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    MapScal s = {};
    for (int m = 0; m < nmat; ++m)
        for (int k = 0; k < nmat; ++k) s.g[m * kMapMaxMat + k] = h_G[m * kMapMaxMat + k];
    for (int m = 0; m < kMapMaxMat; ++m) s.c[m] = m < nmat ? h_C[m] : 1.0;
    s.dt = dt;
    s.om = 1.0 - theta;
    const unsigned blocks = (unsigned)(((long)L.nx * L.ny * L.nz + kExplicitCells * 256 - 1) / (kExplicitCells * 256));
    hipLaunchKernelGGL(k_matmap_explicit, dim3(blocks), dim3(256), 0, as_stream(stream), d_T, d_S, d_flags, d_ids, L, s,
                       d_out);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_matmap_workspace_bytes(int axis, int nx, int ny, int nz, long plane_stride, size_t *bytes)
{
    ADI_REQUIRE(axis >= 0 && axis < 3 && bytes, "adi_matmap_workspace_bytes: bad argument");
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    const int nn[3] = {nx, ny, nz};
    *bytes = nn[axis] <= kMaxFastLine ? 0 : (size_t)L.nx * L.sx * sizeof(double);
    return ADI_OK;
}

int adi_matmap_sweep(int axis, int variant, const double *d_in, const uint8_t *d_flags, const uint8_t *d_ids,
                     const double *d_coeff, const uint8_t *d_dir_mask, const double *d_dir_val, const double *d_qflux, int nx,
                     int ny, int nz, long plane_stride, int nmat, const double *h_G, double dt, double theta, double Tinf,
                     double *d_out, void *d_work, size_t work_bytes, void *stream)
{
#pragma clang fp contract(off)
    ADI_REQUIRE(axis >= 0 && axis < 3, "adi_matmap_sweep: bad axis %d", axis);
    bool has_dir, has_q;
    if (int rc = variant_flags(variant, &has_dir, &has_q)) return rc;
    ADI_REQUIRE(d_in && d_flags && d_ids && d_coeff && h_G && d_out, "adi_matmap_sweep: null argument");
    ADI_REQUIRE(d_in != d_out, "adi_matmap_sweep: output aliases input");
    ADI_REQUIRE(!has_dir || (d_dir_mask && d_dir_val), "adi_matmap_sweep: variant needs Dirichlet arrays");
    ADI_REQUIRE(!has_q || d_qflux, "adi_matmap_sweep: variant needs the flux array");
    ADI_REQUIRE(isfinite(dt) && dt > 0.0 && theta >= 0.0 && theta <= 1.0 && isfinite(Tinf), "adi_matmap_sweep: bad dt, theta or Tinf");
    if (int rc = check_tables("adi_matmap_sweep", nmat, h_G, nullptr)) return rc;
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    size_t need = 0;
    if (int rc = adi_matmap_workspace_bytes(axis, nx, ny, nz, plane_stride, &need)) return rc;
    ADI_REQUIRE(need == 0 || (d_work != nullptr && work_bytes >= need),
                "adi_matmap_sweep: this sweep (axis %d) needs a workspace of %zu bytes", axis, need);
    ADI_REQUIRE(d_work != (void *)d_in && d_work != (void *)d_out, "adi_matmap_sweep: the workspace aliases a field");
    MapScal s = {};
    for (int m = 0; m < nmat; ++m)
        for (int k = 0; k < nmat; ++k) s.g[m * kMapMaxMat + k] = theta * h_G[m * kMapMaxMat + k];
    s.dt = dt;
    s.Tinf = Tinf;
    hipStream_t st = as_stream(stream);
    long inner_stride;
    const LineGeom g = line_geom(axis, L, &inner_stride);
    by_variant(has_dir, has_q, [&](auto dir, auto q) {
        if (need == 0 && axis != 2) {
            const int n = g.n;
            by_rows(RowsGeneral(), strided_rows_per_thread(n), [&](auto m) {
                const int Lp = next_pow2((n + m.value - 1) / m.value);
                int lines = 8;                            // 64-byte row pieces, as the plain GENERAL kernel
                while (lines * Lp < 256) lines <<= 1;
                const int tiles_inner = (g.n_inner + lines - 1) / lines;
                const long ntiles = (long)tiles_inner * g.n_outer;
                const size_t lds = (size_t)7 * lines * (Lp + 1) * sizeof(double);
                hipLaunchKernelGGL((k_matmap_sweep_strided<m.value, dir.value, q.value>), dim3((unsigned)ntiles), dim3(lines * Lp),
                                   lds, st, d_in, d_flags, d_ids, d_coeff, d_dir_mask, d_dir_val, d_qflux, d_out, g, Lp, lines,
                                   tiles_inner, ntiles, s);
            });
        } else if (need == 0) {
            const int n = L.nz;
            by_rows(RowsContig(), contig_rows_per_lane(n), [&](auto m) {
                const int Lp = next_pow2((n + m.value - 1) / m.value);
                const long nunits = ((long)L.nx * L.ny + 64 / Lp - 1) / (64 / Lp);
                hipLaunchKernelGGL((k_matmap_sweep_contig<m.value, dir.value, q.value>), dim3((unsigned)((nunits + 3) / 4)),
                                   dim3(256), 0, st, d_in, d_flags, d_ids, d_coeff, d_dir_mask, d_dir_val, d_qflux, d_out, L, Lp, s);
            });
        } else {
            const long nl = (long)g.n_inner * g.n_outer;
            hipLaunchKernelGGL((k_matmap_sweep_lines<dir.value, q.value>), dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, st,
                               d_in, d_flags, d_ids, d_coeff, d_dir_mask, d_dir_val, d_qflux, d_out, (double *)d_work, g,
                               inner_stride, s);
        }
    });
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // extern "C"
