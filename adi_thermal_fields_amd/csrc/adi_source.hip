// adi_source.hip -- volumetric heat source of the Cartesian step (include/adi_hip.h, "Volumetric heat source"):
//   k_source_sample     Goldak's double ellipsoid at the cell centres -> a field (output, the field form, tests)
//   k_explicit_src      the explicit stage with a source FIELD: R0 = T + f*(Lx+Ly+Lz) + dt*S/(rho cp) on in-mask cells
//   k_source_lines0     the moving source by superposition: w = A0^-1 s added to the output of sweep 0 on the axis-0 lines
//                       that can meet the support (one line = SEG segments of M rows, condense / separator solve / back
//                       solve of adi_core.hpp); k_source_lines0_long: the same for lines of more than 1024 rows, one
//                       thread per line with the Thomas factors in a workspace
//   k_source_set, k_source_tick   the device parameter block (source, t0, dt, step counter) a captured graph reads
//   k_source_add_r0     the source added to R0 on the planes of a slab the support can meet (the slab forms whose axis-0 lines
//                       cross ranks without a zero-boundary local solve: dist_slab's 'exact', 'slab', 'window')
//   k_source_lines0_slab, k_source_lines0_long_slab   the lines kernels for one slab of a grid cut along axis 0
//   k_mapsource_add_r0   the source added to R0 on a grid of several materials, each cell divided by the C of its own id
//                       (the step of a MaterialMap takes the source there: its couplings differ from cell to cell, so the
//                       sweep-0 correction of the lines kernels does not apply)
// No existing kernel changes: the correction runs after whichever sweep-0 form (fused or not) the step used.  The slab
// kernels take a plane origin i_org: local plane i of a slab that starts at global plane i_org has its centre at
// (i_org + i + 1/2) dx; the single-domain kernels are the same bodies without it (their arguments and arithmetic as before).
#include <math.h>

#include "adi_cart_host.hpp"
#include "adi_cell_dev.hpp"
#include "adi_goldak_dev.hpp"
#include "adi_matmap_dev.hpp"

namespace adi {

struct SrcBlock {
    adi_heat_source s;
    double t0, dt;
    unsigned long long n;
};
static_assert(sizeof(SrcBlock) == ADI_SOURCE_BLOCK_BYTES, "source block layout");

// centre of the source at time t (metres)
__host__ __device__ inline void src_centre(const adi_heat_source &s, double t, double (&c)[3])
{
#pragma clang fp contract(off)
    const double shift = ((double)s.travel_sign * s.velocity) * t;
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = (a == s.travel_axis) ? s.origin[a] + shift : s.origin[a];   // (no dynamic index)
}

__host__ __device__ inline double pick3(double v0, double v1, double v2, int a) { return a == 0 ? v0 : (a == 1 ? v1 : v2); }

// the half-length L of an axis for offset o (role- and side-dependent), for the exponent term goldak_eterm(o, L)
__host__ __device__ inline double src_len(const adi_heat_source &s, int axis, double o)
{
    if (axis == s.travel_axis) return ((double)s.travel_sign * o >= 0.0) ? s.c_f : s.c_r;
    return axis == s.depth_axis ? s.b : s.a;
}

// q [W/m^3] at the point (x0, x1, x2) for centre c.  Exponent summed in the order travel, transverse, depth (the NumPy
// evaluator of adi3d_hip_coeff.GoldakSource.sample does the same).
__host__ __device__ inline double goldak_q(const adi_heat_source &s, const double (&c)[3], double x0, double x1, double x2)
{
#pragma clang fp contract(off)
    const int ta = s.travel_axis, da = s.depth_axis, tr = 3 - ta - da;
    const double o0 = x0 - c[0], o1 = x1 - c[1], o2 = x2 - c[2];
    const double xi = pick3(o0, o1, o2, ta), y = pick3(o0, o1, o2, tr), z = pick3(o0, o1, o2, da);
    const bool front = (double)s.travel_sign * xi >= 0.0;
    const double f = front ? s.f_f : 2.0 - s.f_f;
    const double cl = front ? s.c_f : s.c_r;
    const double E = (goldak_eterm(xi, cl) + goldak_eterm(y, s.a)) + goldak_eterm(z, s.b);
    if (!(E <= ADI_SOURCE_E_CUT)) return 0.0;
    return goldak_amp(f, s.eta, s.power, s.a, s.b, cl) * exp(-E);
}

// half-extents of the support along `axis` below / above the centre
__host__ __device__ inline void src_extent(const adi_heat_source &s, int axis, double &lo, double &hi)
{
    const double R = sqrt(ADI_SOURCE_E_CUT / 3.0);
    if (axis == s.travel_axis) {
        const double fr = R * s.c_f, re = R * s.c_r;
        lo = s.travel_sign > 0 ? re : fr;
        hi = s.travel_sign > 0 ? fr : re;
    } else {
        lo = hi = R * (axis == s.depth_axis ? s.b : s.a);
    }
}

// lines of the launch box along an axis: every cell centre inside the support, one line of margin each side
inline int src_box_lines(const adi_heat_source &s, int axis, double dx)
{
    double lo, hi;
    src_extent(s, axis, lo, hi);
    return (int)floor((lo + hi) / dx) + 4;
}
// first line of the launch box, never below -2: a box clamped to n + 4 lines (lines0_box) then still reaches line n + 1,
// and an unclamped box that starts lower covers no in-grid line the raised one misses (its lines below 0 are off the grid)
__device__ inline int src_box_first(const adi_heat_source &s, const double (&c)[3], int axis, double dx)
{
    double lo, hi;
    src_extent(s, axis, lo, hi);
    const int first = (int)floor((c[axis] - lo) / dx - 0.5) - 1;
    return first > -2 ? first : -2;
}

// t_n + dt/2 from the block
__device__ inline double src_tmid(const SrcBlock &B) { return goldak_tmid(B.t0, B.dt, B.n); }

__global__ __launch_bounds__(256) void k_source_sample(adi_heat_source s, const uint8_t *__restrict__ flags, Lay L,
                                                       double dx, double t, double *__restrict__ out)
{
#pragma clang fp contract(off)
    const long plane = (long)L.ny * L.nz;
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= plane * L.nx) return;
    const int i = (int)(q / plane);
    const long r = q - (long)i * plane;
    const int j = (int)(r / L.nz), k = (int)(r - (long)j * L.nz);
    const long p = (long)i * L.sx + r;
    double c[3];
    src_centre(s, t, c);
    out[p] = (flags[p] & 1u) ? goldak_q(s, c, (i + 0.5) * dx, (j + 0.5) * dx, (k + 0.5) * dx) : 0.0;
}

// k_explicit_cell (adi_explicit.hip; explicit_cell of adi_cell_dev.hpp is the value both store) with the source field
// added last: R0 = (T + f*((L0 + L1) + L2)) + scale*S
__global__ __launch_bounds__(256) void k_explicit_src(const double *__restrict__ T, const double *__restrict__ S,
                                                      const uint8_t *__restrict__ flags, double *__restrict__ R0, Lay L,
                                                      double invdx2, double f, double scale)
{
#pragma clang fp contract(off)
    const long plane = (long)L.ny * L.nz;
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= plane * L.nx) return;
    const int i = (int)(q / plane);
    const long r = q - (long)i * plane;
    const long p = (long)i * L.sx + r;
    unsigned fl;
    double src = 0.0;
    const double r0 = explicit_cell(T, flags, p, L, invdx2, f, fl, [&] { src = scale * S[p]; });
    R0[p] = (fl & 1u) ? r0 + src : r0;
}

__global__ void k_source_set(SrcBlock *blk, SrcBlock v) { *blk = v; }
__global__ void k_source_tick(SrcBlock *blk) { blk->n += 1ull; }

struct LinesArgs {
    double tg, dt, dx, scale;   // theta*gamma, dt, dx, dt/(rho cp)
    int fconst, sparse;
    double fc0, fc1;            // c-, c+ of the axis-0 faces (fconst)
    int nj, nk;                 // lines of the launch box along axes 1 / 2
};
// the same for one slab of a grid cut along axis 0: local plane i lies at global plane i_org + i
struct LinesArgsSlab : LinesArgs {
    int i_org;
};
// global plane of local plane i: the single-domain kernels keep their arithmetic (and their code) as it was
__device__ inline int lines0_plane(const LinesArgs &, int i) { return i; }
__device__ inline int lines0_plane(const LinesArgsSlab &A, int i) { return A.i_org + i; }

// The axis-0 line (j, k) = (first_j + jb, first_k + kb) of the launch box, placed from the centre at the block's mid-step
// time.  It takes part when it lies in the grid and in the box and its (j, k) offsets alone do not put it outside the
// support (then s = 0 on every row and w = 0: adding the exponent of axis 0 can only make the sum larger).
__device__ inline bool lines0_line(const SrcBlock &B, const Lay &L, const LinesArgs &A, int jb, int kb, double (&c)[3],
                                   int &j, int &k)
{
#pragma clang fp contract(off)
    const adi_heat_source &s = B.s;
    src_centre(s, src_tmid(B), c);
    j = src_box_first(s, c, 1, A.dx) + jb;
    k = src_box_first(s, c, 2, A.dx) + kb;
    if (!(j >= 0 && j < L.ny && k >= 0 && k < L.nz && jb < A.nj && kb < A.nk)) return false;
    const double yj = (j + 0.5) * A.dx, zk = (k + 0.5) * A.dx;
    const double e1 = goldak_eterm(yj - c[1], src_len(s, 1, yj - c[1]));
    const double e2 = goldak_eterm(zk - c[2], src_len(s, 2, zk - c[2]));
    return (e1 + e2) <= ADI_SOURCE_E_CUT;
}

// Row i of A0 w = s on the line at `base` = j*nz + k, assembled as adi_sweep(axis 0) assembles it (assemble_row): b the
// diagonal, lo / hi whether the row couples to its minus / plus neighbour (coefficient -tg), rhs = s.  Off-mask and
// Dirichlet rows are identity rows with s = 0.
template <class AR>
__device__ inline void lines0_row(const adi_heat_source &s, const double (&c)[3], const uint8_t *__restrict__ flags,
                                  const double *__restrict__ coeff, const uint8_t *__restrict__ dirm, const Lay &L,
                                  const AR &A, int i, long base, double yj, double zk, double &b, bool &lo,
                                  bool &hi, double &rhs)
{
#pragma clang fp contract(off)
    b = 1.0; rhs = 0.0; lo = hi = false;
    const long p = (long)i * L.sx + base;
    const unsigned fl = flags[p];
    const bool m = fl & 1u, mL = fl & 2u, mR = fl & 4u;
    const bool fr = m && !(dirm != nullptr && dirm[p]);
    if (!fr) return;
    double co;
    if (A.fconst) {
        co = 0.0;
        if (!mL) co += A.fc0;
        if (!mR) co += A.fc1;
    } else {
        co = (!A.sparse || axis_exposed(fl, 1)) ? coeff[p] : 0.0;
    }
    const double nnb = (double)((int)mL + (int)mR);
    b = 1.0 + A.tg * nnb + A.dt * co;      // assemble_row's diagonal, same operations
    lo = mL; hi = mR;
    rhs = A.scale * goldak_q(s, c, (lines0_plane(A, i) + 0.5) * A.dx, yj, zk);
}

// Lines longer than the in-register limit (nx > kMaxFastLine): one thread per line, Thomas along the line with c' and d'
// in the workspace ([2][nx][lines of the box], lines dense, so the threads of a wave touch adjacent words), then the back
// substitution adds w to U.  Lanes are adjacent lines along k, so every row access of a wave is contiguous.
template <class AR>
__device__ __forceinline__ void lines0_long(const SrcBlock *__restrict__ blk, double *__restrict__ U,
                                            const uint8_t *__restrict__ flags, const double *__restrict__ coeff,
                                            const uint8_t *__restrict__ dirm, const Lay &L, const AR &A,
                                            double *__restrict__ work)
{
#pragma clang fp contract(off)
    const SrcBlock &B = *blk;
    const int kb = (int)(blockIdx.x * blockDim.x + threadIdx.x), jb = (int)blockIdx.y;
    double c[3];
    int j, k;
    if (!lines0_line(B, L, A, jb, kb, c, j, k)) return;
    const long nl = (long)A.nj * A.nk, line = (long)jb * A.nk + kb;
    double *__restrict__ cpw = work + line;
    double *__restrict__ dpw = work + (long)L.nx * nl + line;
    const long base = (long)j * L.nz + k;
    const double yj = (j + 0.5) * A.dx, zk = (k + 0.5) * A.dx;
    double cp = 0.0, dp = 0.0;
    bool any = false;
    for (int i = 0; i < L.nx; ++i) {
        double b, rhs;
        bool lo, hi;
        lines0_row(B.s, c, flags, coeff, dirm, L, A, i, base, yj, zk, b, lo, hi, rhs);
        const double a = lo ? -A.tg : 0.0, cc = hi ? -A.tg : 0.0;
        const double den = b - a * cp;
        cp = cc / den;
        dp = (rhs - a * dp) / den;
        any = any || rhs != 0.0;
        cpw[(long)i * nl] = cp;
        dpw[(long)i * nl] = dp;
    }
    if (!any) return;                      // s = 0 on the whole line: w = 0
    double x = 0.0;
    for (int i = L.nx - 1; i >= 0; --i) {
        x = dpw[(long)i * nl] - cpw[(long)i * nl] * x;
        if (x != 0.0) {
            const long p = (long)i * L.sx + base;
            U[p] = U[p] + x;
        }
    }
}
__global__ __launch_bounds__(256) void k_source_lines0_long(const SrcBlock *__restrict__ blk, double *__restrict__ U,
                                                            const uint8_t *__restrict__ flags,
                                                            const double *__restrict__ coeff,
                                                            const uint8_t *__restrict__ dirm, Lay L, LinesArgs A,
                                                            double *__restrict__ work)
{
    lines0_long(blk, U, flags, coeff, dirm, L, A, work);
}
__global__ __launch_bounds__(256) void k_source_lines0_long_slab(const SrcBlock *__restrict__ blk, double *__restrict__ U,
                                                                 const uint8_t *__restrict__ flags,
                                                                 const double *__restrict__ coeff,
                                                                 const uint8_t *__restrict__ dirm, Lay L, LinesArgsSlab A,
                                                                 double *__restrict__ work)
{
    lines0_long(blk, U, flags, coeff, dirm, L, A, work);
}

// One workgroup = KL adjacent lines along k x SEG segments of M rows; thread (kl, seg) owns rows [seg*M, seg*M + M) of line
// kl, in registers.  Lanes kl of one segment are adjacent in memory, so every row load / store of a wave covers whole
// 128-byte lines of U.  Rows past the end of the line are identity rows with s = 0.
template <int M, int SEG, class AR>
__device__ __forceinline__ void lines0_seg(const SrcBlock *__restrict__ blk, double *__restrict__ U,
                                           const uint8_t *__restrict__ flags, const double *__restrict__ coeff,
                                           const uint8_t *__restrict__ dirm, const Lay &L, const AR &A,
                                           double (&sh)[4][SEG][512 / SEG])
{
#pragma clang fp contract(off)
    constexpr int KL = 512 / SEG;
    const SrcBlock &B = *blk;            // (read in place: a local copy of the block would live in scratch)
    const adi_heat_source &s = B.s;
    const int kl = threadIdx.x % KL, seg = threadIdx.x / KL;
    double c[3];
    int j, k;
    const bool act = lines0_line(B, L, A, (int)blockIdx.y, (int)blockIdx.x * KL + kl, c, j, k);
    if (!__syncthreads_or(act)) return;

    const long base = (long)j * L.nz + k;
    const double yj = (j + 0.5) * A.dx, zk = (k + 0.5) * A.dx;
    double b[M], d[M];
    unsigned am = 0u, cm = 0u;
#pragma unroll
    for (int r = 0; r < M; ++r) {
        const int i = seg * M + r;
        b[r] = 1.0; d[r] = 0.0;
        if (act && i < L.nx) {
            bool lo, hi;
            lines0_row(s, c, flags, coeff, dirm, L, A, i, base, yj, zk, b[r], lo, hi, d[r]);
            am |= (lo ? 1u : 0u) << r;
            cm |= (hi ? 1u : 0u) << r;
        }
    }
    const MaskedCoef av{am, -A.tg}, cv{cm, -A.tg};

    // phase 1: condense the interior block, publish (gF, aF, cF) for the previous segment's reduced row
    double ip[M - 1];
    Cond cd;
    condense<M>(av, b, cv, d, ip, cd);
    sh[0][seg][kl] = cd.gF; sh[1][seg][kl] = cd.aF; sh[2][seg][kl] = cd.cF;
    __syncthreads();
    const bool last = seg == SEG - 1;
    const double gFn = last ? 0.0 : sh[0][seg + 1][kl], aFn = last ? 0.0 : sh[1][seg + 1][kl];
    const double cFn = last ? 0.0 : sh[2][seg + 1][kl];
    double ra, rb, rc, rd;
    reduced_row(av[M - 1], b[M - 1], last ? 0.0 : cv[M - 1], d[M - 1], cd, gFn, aFn, cFn, ra, rb, rc, rd);
    __syncthreads();
    sh[0][seg][kl] = ra; sh[1][seg][kl] = rb; sh[2][seg][kl] = rc; sh[3][seg][kl] = rd;
    __syncthreads();
    // phase 2: the SEG separators of a line, Thomas by the line's segment-0 thread (diagonally dominant Schur complement)
    if (seg == 0) {
        double cp = sh[2][0][kl] / sh[1][0][kl];
        double dp = sh[3][0][kl] / sh[1][0][kl];
        sh[2][0][kl] = cp; sh[3][0][kl] = dp;
        for (int q = 1; q < SEG; ++q) {
            const double aq = sh[0][q][kl];
            const double den = sh[1][q][kl] - aq * cp;
            cp = sh[2][q][kl] / den;
            dp = (sh[3][q][kl] - aq * dp) / den;
            sh[2][q][kl] = cp; sh[3][q][kl] = dp;
        }
        double x = dp;
        sh[3][SEG - 1][kl] = x;
        for (int q = SEG - 2; q >= 0; --q) {
            x = sh[3][q][kl] - sh[2][q][kl] * x;
            sh[3][q][kl] = x;
        }
    }
    __syncthreads();
    // phase 3: the block rows from both separators, added to U
    const double xS = sh[3][seg][kl], xL = seg > 0 ? sh[3][seg - 1][kl] : 0.0;
    double x[M];
    back_solve<M>(av, cv, d, ip, xL, xS, x);
    if (!act) return;
#pragma unroll
    for (int r = 0; r < M; ++r) {
        const int i = seg * M + r;
        if (i < L.nx && x[r] != 0.0) {
            const long p = (long)i * L.sx + base;
            U[p] = U[p] + x[r];
        }
    }
}
template <int M, int SEG>
__global__ __launch_bounds__(512) void k_source_lines0(const SrcBlock *__restrict__ blk, double *__restrict__ U,
                                                       const uint8_t *__restrict__ flags, const double *__restrict__ coeff,
                                                       const uint8_t *__restrict__ dirm, Lay L, LinesArgs A)
{
    __shared__ double sh[4][SEG][512 / SEG];
    lines0_seg<M, SEG>(blk, U, flags, coeff, dirm, L, A, sh);
}
template <int M, int SEG>
__global__ __launch_bounds__(512) void k_source_lines0_slab(const SrcBlock *__restrict__ blk, double *__restrict__ U,
                                                            const uint8_t *__restrict__ flags, const double *__restrict__ coeff,
                                                            const uint8_t *__restrict__ dirm, Lay L, LinesArgsSlab A)
{
    __shared__ double sh[4][SEG][512 / SEG];
    lines0_seg<M, SEG>(blk, U, flags, coeff, dirm, L, A, sh);
}

struct AddArgs {
    double dx, scale;           // dx, dt/(rho cp)
    int i_org, i_begin, i_end;  // global plane of local plane 0; the local planes [i_begin, i_end) to touch
    int n0, nj, nk;             // planes of the launch box along axis 0 (at most i_end - i_begin), lines along axes 1 / 2
};

// The column (j, k) of the launch box that thread kb of line jb owns, and the first local plane i_lo of its walk along axis 0.
// The box is placed from the block's mid-step centre c as lines0_line places it; along axis 0 it starts at the later of its
// first plane and i_begin.  false: a column outside the box or off the grid.
__device__ inline bool add_r0_column(const SrcBlock &B, const Lay &L, const AddArgs &A, int jb, int kb, double (&c)[3], int &j,
                                     int &k, int &i_lo)
{
#pragma clang fp contract(off)
    const adi_heat_source &s = B.s;
    if (kb >= A.nk || jb >= A.nj) return false;
    src_centre(s, src_tmid(B), c);
    j = src_box_first(s, c, 1, A.dx) + jb;
    k = src_box_first(s, c, 2, A.dx) + kb;
    if (!(j >= 0 && j < L.ny && k >= 0 && k < L.nz)) return false;
    const int g0 = src_box_first(s, c, 0, A.dx) - A.i_org;
    i_lo = g0 > A.i_begin ? g0 : A.i_begin;
    return true;
}

// R0 += dt*q(t_n + dt/2)/(rho cp) on the in-mask, non-Dirichlet cells of local planes [i_begin, i_end) inside the launch box,
// one thread per cell of the box (lanes adjacent along k).  Cells of the box outside the support get q = 0 (goldak_q's cut)
// and are not written.
__global__ __launch_bounds__(64) void k_source_add_r0(const SrcBlock *__restrict__ blk, double *__restrict__ R0,
                                                      const uint8_t *__restrict__ flags, const uint8_t *__restrict__ dirm,
                                                      Lay L, AddArgs A)
{
#pragma clang fp contract(off)
    const SrcBlock &B = *blk;            // (read in place, as k_source_lines0 does)
    const adi_heat_source &s = B.s;
    double c[3];
    int j, k, i_lo;
    if (!add_r0_column(B, L, A, (int)blockIdx.y, (int)(blockIdx.x * blockDim.x + threadIdx.x), c, j, k, i_lo)) return;
    const double yj = (j + 0.5) * A.dx, zk = (k + 0.5) * A.dx;
    const long base = (long)j * L.nz + k;
    for (int ib = (int)blockIdx.z; ib < A.n0; ib += (int)gridDim.z) {
        const int i = i_lo + ib;
        if (i >= A.i_end) return;
        const long p = (long)i * L.sx + base;
        if (!(flags[p] & 1u) || (dirm != nullptr && dirm[p])) continue;
        const double q = goldak_q(s, c, ((A.i_org + i) + 0.5) * A.dx, yj, zk);
        if (q != 0.0) R0[p] = R0[p] + A.scale * q;
    }
}

// The same walk on a grid of several materials (include/adi_hip.h, "Several materials"): R0 = R0 + (dt * q) / C[id] on every
// in-mask cell of the box the support reaches -- the operations of k_matmap_explicit's source-field branch, in its order, with
// q evaluated here instead of read from a field.  A.scale = dt; C travels by value and goes through LDS (a lane picks the
// entry of its cell's id).  17 bytes per in-mask cell of the support: flags, id, R0 read and written.
struct MapCTab {
    double c[kMapMaxMat];
};
__global__ __launch_bounds__(64) void k_mapsource_add_r0(const SrcBlock *__restrict__ blk, double *__restrict__ R0,
                                                             const uint8_t *__restrict__ flags, const uint8_t *__restrict__ ids,
                                                             Lay L, AddArgs A, MapCTab C)
{
#pragma clang fp contract(off)
    __shared__ double sC[kMapMaxMat];
    {
        const double *kc = C.c;
        if (threadIdx.x < kMapMaxMat) sC[threadIdx.x] = kc[threadIdx.x];
        __syncthreads();
    }
    const SrcBlock &B = *blk;            // (read in place, as k_source_lines0 does)
    const adi_heat_source &s = B.s;
    double c[3];
    int j, k, i_lo;
    if (!add_r0_column(B, L, A, (int)blockIdx.y, (int)(blockIdx.x * blockDim.x + threadIdx.x), c, j, k, i_lo)) return;
    const double yj = (j + 0.5) * A.dx, zk = (k + 0.5) * A.dx;
    const long base = (long)j * L.nz + k;
    for (int ib = (int)blockIdx.z; ib < A.n0; ib += (int)gridDim.z) {
        const int i = i_lo + ib;
        if (i >= A.i_end) return;
        const long p = (long)i * L.sx + base;
        if (!(flags[p] & 1u)) continue;
        const double q = goldak_q(s, c, (i + 0.5) * A.dx, yj, zk);
        if (q != 0.0) R0[p] = R0[p] + (A.scale * q) / sC[ids[p] & (kMapMaxMat - 1)];
    }
}

static int check_source(const adi_heat_source *h, const char *fn)
{
    ADI_REQUIRE(h != nullptr, "%s: null source", fn);
    const double v[] = {h->power, h->eta, h->a, h->b, h->c_f, h->c_r, h->f_f, h->origin[0], h->origin[1], h->origin[2],
                        h->velocity};
    for (double x : v) ADI_REQUIRE(std::isfinite(x), "%s: non-finite source parameter", fn);
    ADI_REQUIRE(h->power >= 0.0, "%s: power < 0", fn);
    ADI_REQUIRE(h->eta >= 0.0 && h->eta <= 1.0, "%s: eta outside [0, 1]", fn);
    ADI_REQUIRE(h->a > 0.0 && h->b > 0.0 && h->c_f > 0.0 && h->c_r > 0.0, "%s: non-positive length", fn);
    ADI_REQUIRE(h->f_f > 0.0 && h->f_f < 2.0, "%s: f_f outside (0, 2)", fn);
    ADI_REQUIRE(h->velocity >= 0.0, "%s: velocity < 0", fn);
    ADI_REQUIRE(h->travel_axis >= 0 && h->travel_axis < 3 && h->depth_axis >= 0 && h->depth_axis < 3,
                "%s: axis out of range", fn);
    ADI_REQUIRE(h->travel_axis != h->depth_axis, "%s: travel_axis == depth_axis", fn);
    ADI_REQUIRE(h->travel_sign == 1 || h->travel_sign == -1, "%s: travel_sign must be +1 or -1", fn);
    return ADI_OK;
}

// lines of the launch box along axes 1 / 2, at most n + 4 for a support wider than the grid: the box then starts at line
// -2 at the lowest (src_box_first) and so reaches every in-grid line; the lines beyond the grid exit on their own
static void lines0_box(const adi_heat_source &s, int ny, int nz, double dx, int &nj, int &nk)
{
    nj = src_box_lines(s, 1, dx);
    nk = src_box_lines(s, 2, dx);
    if (nj > ny + 4) nj = ny + 4;
    if (nk > nz + 4) nk = nz + 4;
}

// the arguments and the launch grid of the add-R0 kernels for the local planes [i_begin, i_end): the box of the support, at most
// the planes given along axis 0 and lines0_box along axes 1 / 2
static dim3 add_r0_box(const adi_heat_source &s, int ny, int nz, double dx, double scale, int i_org, int i_begin, int i_end,
                       AddArgs &A)
{
    A.dx = dx; A.scale = scale;
    A.i_org = i_org; A.i_begin = i_begin; A.i_end = i_end;
    double lo, hi;
    src_extent(s, 0, lo, hi);
    const double n0 = floor((lo + hi) / dx) + 4.0;          // src_box_lines along axis 0, in double: no int overflow
    A.n0 = n0 < (double)(i_end - i_begin) ? (int)n0 : i_end - i_begin;
    lines0_box(s, ny, nz, dx, A.nj, A.nk);
    const unsigned gz = (unsigned)(A.n0 < 65535 ? A.n0 : 65535);
    return dim3((unsigned)((A.nk + 63) / 64), (unsigned)A.nj, gz);
}

template <int M, int SEG>
static void launch_lines0(dim3 grid, hipStream_t st, const SrcBlock *blk, double *U, const uint8_t *flags,
                          const double *coeff, const uint8_t *dirm, const Lay &L, const LinesArgs &A)
{
    hipLaunchKernelGGL((k_source_lines0<M, SEG>), grid, dim3(512), 0, st, blk, U, flags, coeff, dirm, L, A);
}
template <int M, int SEG>
static void launch_lines0(dim3 grid, hipStream_t st, const SrcBlock *blk, double *U, const uint8_t *flags,
                          const double *coeff, const uint8_t *dirm, const Lay &L, const LinesArgsSlab &A)
{
    hipLaunchKernelGGL((k_source_lines0_slab<M, SEG>), grid, dim3(512), 0, st, blk, U, flags, coeff, dirm, L, A);
}
static void launch_lines0_long(dim3 grid, hipStream_t st, const SrcBlock *blk, double *U, const uint8_t *flags,
                               const double *coeff, const uint8_t *dirm, const Lay &L, const LinesArgs &A, double *work)
{
    hipLaunchKernelGGL(k_source_lines0_long, grid, dim3(64), 0, st, blk, U, flags, coeff, dirm, L, A, work);
}
static void launch_lines0_long(dim3 grid, hipStream_t st, const SrcBlock *blk, double *U, const uint8_t *flags,
                               const double *coeff, const uint8_t *dirm, const Lay &L, const LinesArgsSlab &A, double *work)
{
    hipLaunchKernelGGL(k_source_lines0_long_slab, grid, dim3(64), 0, st, blk, U, flags, coeff, dirm, L, A, work);
}

// the in-register kernel for lines of nx <= kMaxFastLine rows: SEG segments of M rows
template <class AR>
static void launch_lines0_box(int nx, hipStream_t st, const SrcBlock *blk, double *U, const uint8_t *flags,
                              const double *coeff, const uint8_t *dirm, const Lay &L, const AR &A)
{
    const dim3 g16((unsigned)((A.nk + 15) / 16), (unsigned)A.nj), g8((unsigned)((A.nk + 7) / 8), (unsigned)A.nj);
    if (nx <= 128) launch_lines0<4, 32>(g16, st, blk, U, flags, coeff, dirm, L, A);
    else if (nx <= 256) launch_lines0<8, 32>(g16, st, blk, U, flags, coeff, dirm, L, A);
    else if (nx <= 512) launch_lines0<16, 32>(g16, st, blk, U, flags, coeff, dirm, L, A);
    else launch_lines0<16, 64>(g8, st, blk, U, flags, coeff, dirm, L, A);
}

// adi_source_lines0 / adi_source_lines0_slab (fn: the entry point's name for the messages; slab: the kernels that take the
// plane origin -- with slab = false the single-domain kernels, whose arguments and code are those without it)
static int source_lines0(const void *d_block, const adi_heat_source *h_src, double *d_U, const uint8_t *d_flags,
                         const double *d_coeff, const uint8_t *d_dir_mask, int nx, int ny, int nz, long plane_stride,
                         int i_org, int sparse, double dx, double theta, double gam, double dt, double rho, double cp,
                         const double *h_face_consts, void *d_work, size_t work_bytes, void *stream, bool slab,
                         const char *fn)
{
    if (int rc = check_source(h_src, fn)) return rc;
    ADI_REQUIRE(d_block && d_U && d_flags, "%s: null argument", fn);
    const bool fconst = h_face_consts != nullptr && (sparse & 1);
    ADI_REQUIRE(fconst || d_coeff, "%s: no coefficient array and no face constants", fn);
    const double sc[] = {dx, theta, gam, dt, rho, cp};
    for (double x : sc) ADI_REQUIRE(std::isfinite(x), "%s: non-finite scalar", fn);
    ADI_REQUIRE(dx > 0.0 && dt > 0.0 && rho > 0.0 && cp > 0.0 && gam >= 0.0 && theta >= 0.0,
                "%s: bad dx / dt / rho / cp / gam / theta", fn);
    ADI_REQUIRE(i_org >= 0, "%s: plane origin < 0", fn);
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    LinesArgsSlab A;
    A.tg = theta * gam; A.dt = dt; A.dx = dx; A.scale = dt / (rho * cp);
    A.fconst = fconst ? 1 : 0; A.sparse = (sparse & 1) ? 1 : 0;
    A.fc0 = fconst ? h_face_consts[0] : 0.0; A.fc1 = fconst ? h_face_consts[1] : 0.0;
    A.i_org = i_org;
    lines0_box(*h_src, ny, nz, dx, A.nj, A.nk);
    const SrcBlock *blk = (const SrcBlock *)d_block;
    hipStream_t st = as_stream(stream);
    if (nx > kMaxFastLine) {
        const size_t need = 2 * sizeof(double) * (size_t)nx * (size_t)A.nj * (size_t)A.nk;
        ADI_REQUIRE(d_work && work_bytes >= need, "%s: lines of %d rows need %zu bytes of workspace "
                    "(adi_source_workspace_bytes), got %zu", fn, nx, need, d_work ? work_bytes : (size_t)0);
        if (slab) launch_lines0_long(dim3((unsigned)((A.nk + 63) / 64), (unsigned)A.nj), st, blk, d_U, d_flags, d_coeff,
                                     d_dir_mask, L, A, (double *)d_work);
        else launch_lines0_long(dim3((unsigned)((A.nk + 63) / 64), (unsigned)A.nj), st, blk, d_U, d_flags, d_coeff,
                                d_dir_mask, L, (const LinesArgs &)A, (double *)d_work);
    } else if (slab) {
        launch_lines0_box(nx, st, blk, d_U, d_flags, d_coeff, d_dir_mask, L, A);
    } else {
        launch_lines0_box(nx, st, blk, d_U, d_flags, d_coeff, d_dir_mask, L, (const LinesArgs &)A);
    }
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // namespace adi

using namespace adi;

extern "C" {

int adi_source_sample(const adi_heat_source *h_src, const uint8_t *d_flags, int nx, int ny, int nz, long plane_stride,
                      double dx, double t, double *d_out, void *stream)
{
    if (int rc = check_source(h_src, "adi_source_sample")) return rc;
    ADI_REQUIRE(d_flags && d_out, "adi_source_sample: null argument");
    ADI_REQUIRE(std::isfinite(dx) && dx > 0.0 && std::isfinite(t), "adi_source_sample: bad dx / t");
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    const long cells = (long)nx * ny * nz;
    hipLaunchKernelGGL(k_source_sample, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, as_stream(stream), *h_src,
                       d_flags, L, dx, t, d_out);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_source_set(void *d_block, const adi_heat_source *h_src, double t0, double dt, long long n, void *stream)
{
    if (int rc = check_source(h_src, "adi_source_set")) return rc;
    ADI_REQUIRE(d_block, "adi_source_set: null block");
    ADI_REQUIRE(std::isfinite(t0) && std::isfinite(dt) && dt > 0.0 && n >= 0, "adi_source_set: bad t0 / dt / n");
    SrcBlock v;
    v.s = *h_src;
    v.t0 = t0; v.dt = dt; v.n = (unsigned long long)n;
    hipLaunchKernelGGL(k_source_set, dim3(1), dim3(1), 0, as_stream(stream), (SrcBlock *)d_block, v);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_source_tick(void *d_block, void *stream)
{
    ADI_REQUIRE(d_block, "adi_source_tick: null block");
    hipLaunchKernelGGL(k_source_tick, dim3(1), dim3(1), 0, as_stream(stream), (SrcBlock *)d_block);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_source_workspace_bytes(const adi_heat_source *h_src, int nx, int ny, int nz, double dx, size_t *bytes)
{
    if (int rc = check_source(h_src, "adi_source_workspace_bytes")) return rc;
    ADI_REQUIRE(bytes && nx > 0 && ny > 0 && nz > 0 && std::isfinite(dx) && dx > 0.0,
                "adi_source_workspace_bytes: bad argument");
    int nj, nk;
    lines0_box(*h_src, ny, nz, dx, nj, nk);
    *bytes = nx > kMaxFastLine ? 2 * sizeof(double) * (size_t)nx * (size_t)nj * (size_t)nk : 0;
    return ADI_OK;
}

int adi_source_lines0(const void *d_block, const adi_heat_source *h_src, double *d_U, const uint8_t *d_flags,
                      const double *d_coeff, const uint8_t *d_dir_mask, int nx, int ny, int nz, long plane_stride,
                      int sparse, double dx, double theta, double gam, double dt, double rho, double cp,
                      const double *h_face_consts, void *d_work, size_t work_bytes, void *stream)
{
    return source_lines0(d_block, h_src, d_U, d_flags, d_coeff, d_dir_mask, nx, ny, nz, plane_stride, 0, sparse, dx, theta,
                         gam, dt, rho, cp, h_face_consts, d_work, work_bytes, stream, false, "adi_source_lines0");
}

int adi_source_lines0_slab(const void *d_block, const adi_heat_source *h_src, double *d_U, const uint8_t *d_flags,
                           const double *d_coeff, const uint8_t *d_dir_mask, int nx, int ny, int nz, long plane_stride,
                           int i_org, int sparse, double dx, double theta, double gam, double dt, double rho, double cp,
                           const double *h_face_consts, void *d_work, size_t work_bytes, void *stream)
{
    return source_lines0(d_block, h_src, d_U, d_flags, d_coeff, d_dir_mask, nx, ny, nz, plane_stride, i_org, sparse, dx,
                         theta, gam, dt, rho, cp, h_face_consts, d_work, work_bytes, stream, true,
                         "adi_source_lines0_slab");
}

int adi_source_add_r0(const void *d_block, const adi_heat_source *h_src, double *d_R0, const uint8_t *d_flags,
                      const uint8_t *d_dir_mask, int nx, int ny, int nz, long plane_stride, int i_org, int i_begin,
                      int i_end, double dx, double dt, double rho, double cp, void *stream)
{
    if (int rc = check_source(h_src, "adi_source_add_r0")) return rc;
    ADI_REQUIRE(d_block && d_R0 && d_flags, "adi_source_add_r0: null argument");
    const double sc[] = {dx, dt, rho, cp};
    for (double x : sc) ADI_REQUIRE(std::isfinite(x), "adi_source_add_r0: non-finite scalar");
    ADI_REQUIRE(dx > 0.0 && dt > 0.0 && rho > 0.0 && cp > 0.0, "adi_source_add_r0: bad dx / dt / rho / cp");
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    ADI_REQUIRE(i_org >= 0, "adi_source_add_r0: plane origin < 0");
    ADI_REQUIRE(i_begin >= 0 && i_begin <= i_end && i_end <= nx, "adi_source_add_r0: planes [%d, %d) outside [0, %d]",
                i_begin, i_end, nx);
    if (i_begin == i_end) return ADI_OK;
    AddArgs A;
    const dim3 grid = add_r0_box(*h_src, ny, nz, dx, dt / (rho * cp), i_org, i_begin, i_end, A);
    hipLaunchKernelGGL(k_source_add_r0, grid, dim3(64), 0, as_stream(stream), (const SrcBlock *)d_block, d_R0, d_flags,
                       d_dir_mask, L, A);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_matmap_source_add_r0(const void *d_block, const adi_heat_source *h_src, double *d_R0, const uint8_t *d_flags,
                             const uint8_t *d_ids, int nx, int ny, int nz, long plane_stride, double dx, double dt, int nmat,
                             const double *h_C, void *stream)
{
    if (int rc = check_source(h_src, "adi_matmap_source_add_r0")) return rc;
    ADI_REQUIRE(d_block && d_R0 && d_flags && d_ids && h_C, "adi_matmap_source_add_r0: null argument");
    ADI_REQUIRE(std::isfinite(dx) && std::isfinite(dt) && dx > 0.0 && dt > 0.0, "adi_matmap_source_add_r0: bad dx / dt");
    if (int rc = check_tables("adi_matmap_source_add_r0", nmat, nullptr, h_C)) return rc;
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    AddArgs A;
    const dim3 grid = add_r0_box(*h_src, ny, nz, dx, dt, 0, 0, nx, A);
    MapCTab C;
    for (int m = 0; m < kMapMaxMat; ++m) C.c[m] = m < nmat ? h_C[m] : 1.0;
    hipLaunchKernelGGL(k_mapsource_add_r0, grid, dim3(64), 0, as_stream(stream), (const SrcBlock *)d_block, d_R0, d_flags,
                       d_ids, L, A, C);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_explicit_rhs_src(const double *d_T, const double *d_S, const uint8_t *d_flags, int nx, int ny, int nz,
                         long plane_stride, double dx, double dt, double kappa, double theta, double rho, double cp,
                         double *d_R0, void *stream)
{
    ADI_REQUIRE(d_T && d_S && d_flags && d_R0, "adi_explicit_rhs_src: null argument");
    ADI_REQUIRE(d_T != d_R0 && d_S != d_R0, "adi_explicit_rhs_src: output aliases an input");
    const double sc[] = {dx, dt, kappa, theta, rho, cp};
    for (double x : sc) ADI_REQUIRE(std::isfinite(x), "adi_explicit_rhs_src: non-finite scalar");
    ADI_REQUIRE(dx > 0.0 && rho > 0.0 && cp > 0.0, "adi_explicit_rhs_src: bad dx / rho / cp");
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    const long cells = (long)nx * ny * nz;
    hipLaunchKernelGGL(k_explicit_src, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, as_stream(stream), d_T, d_S,
                       d_flags, d_R0, L, 1.0 / (dx * dx), dt * kappa * (1.0 - theta), dt / (rho * cp));
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // extern "C"
