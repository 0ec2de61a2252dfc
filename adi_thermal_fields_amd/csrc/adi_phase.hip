// adi_phase.hip -- latent heat of melting and freezing of the Cartesian step (include/adi_hip.h, "Latent heat"): after the
// three sweeps the enthalpy cp*T + L*f of every in-mask, non-Dirichlet cell is put back on the equilibrium curve.
//   k_phase_apply   every step, T and f in place
//   k_phase_seed    f = f_eq(T) on selected in-mask cells, 0 off the mask (construction, newborn cells)
// One workgroup of 256 threads per 16 x 16 x 16 brick of the flags summary; it owns the brick's cells and the brick's word of
// the phase summary, so nothing is shared between workgroups and no atomic is needed.  Which cells a thread owns and how it
// loads them is in adi_brick_dev.hpp (shared with adi_matlaw.hip).  The loads of a thread are issued together ahead of the
// arithmetic; stores go cell by cell (8 bytes) so that a cell the law leaves alone is never written.  No existing kernel changes.
// The law's record and its host constants are in adi_phase_dev.hpp (shared with adi_matmap_phase.hip).
#include "adi_phase_dev.hpp"

namespace adi {

template <bool VEC>
__global__ __launch_bounds__(256) void k_phase_apply(PhaseLaw w, double *__restrict__ T, double *__restrict__ F,
                                                     const uint8_t *__restrict__ flags, const unsigned *__restrict__ bricks,
                                                     const uint8_t *__restrict__ dir, unsigned *__restrict__ summary, Lay L,
                                                     int nby, int nbz)
{
#pragma clang fp contract(off)
    const int bk = (int)blockIdx.x, bj = (int)blockIdx.y, bi = (int)blockIdx.z;
    const unsigned tid = threadIdx.x;
    unsigned *entry = summary + ((long)bi * nby + bj) * nbz + bk;
    const bool have_f = *entry != 0u;                       // (uniform over the workgroup)
    const bool solid = brick_all_solid(bricks, L, bi, bj, bk);
    PhaseCell c[kPhaseIter];
    double t[kPhaseIter][2], f[kPhaseIter][2];
    // the loads of the brick, issued together: f (only where some f of the brick is non-zero), flags (only where the flags
    // summary does not say all-solid), T (only where a cell of the pair is in the mask)
#pragma unroll
    for (int it = 0; it < kPhaseIter; ++it) {
        c[it] = phase_cell(L, bi, bj, bk, it, tid);
        f[it][0] = 0.0; f[it][1] = 0.0;
        if (have_f && c[it].in) load_pair<VEC>(F, c[it], f[it][0], f[it][1]);
        if (c[it].in) c[it].m = solid ? c[it].in : (load_mask_pair<VEC>(flags, c[it]) & c[it].in);
    }
#pragma unroll
    for (int it = 0; it < kPhaseIter; ++it) {
        t[it][0] = 0.0; t[it][1] = 0.0;
        if (c[it].m) load_pair<VEC>(T, c[it], t[it][0], t[it][1]);
    }
    bool any = false;                                       // a non-zero f in this thread's cells after the pass
#pragma unroll
    for (int it = 0; it < kPhaseIter; ++it) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const double fs = f[it][s], ts = t[it][s];
            double fn = fs;
            if ((c[it].m >> s) & 1u) {
                const bool rest = (fs == 0.0 && ts <= w.Ts) || (fs == 1.0 && ts >= w.Tl);
                if (!rest && (dir == nullptr || dir[c[it].p + s] == 0)) {
                    const double h1 = w.cp * ts;
                    const double h2 = w.L * fs;
                    const double H = h1 + h2;
                    double tn;
                    if (H <= w.Hs) {
                        tn = H / w.cp;
                        fn = 0.0;
                    } else if (H >= w.Hl) {
                        const double d = H - w.L;
                        tn = d / w.cp;
                        fn = 1.0;
                    } else {
                        const double d = H - w.Hs;
                        const double q = d / w.cm;
                        tn = w.Ts + q;
                        const double e = tn - w.Ts;
                        fn = clamp01(e / w.dT);
                    }
                    T[c[it].p + s] = tn;
                    F[c[it].p + s] = fn;
                }
            }
            any = any || fn != 0.0;
        }
    }
    const int nonzero = __syncthreads_or(any ? 1 : 0);
    if (tid == 0 && (have_f || nonzero)) *entry = nonzero ? 1u : 0u;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_phase_seed(PhaseLaw w, const double *__restrict__ T, double *__restrict__ F,
                                                    const uint8_t *__restrict__ flags, const unsigned *__restrict__ bricks,
                                                    const uint8_t *__restrict__ sel, unsigned *__restrict__ summary, Lay L,
                                                    int nby, int nbz)
{
#pragma clang fp contract(off)
    const int bk = (int)blockIdx.x, bj = (int)blockIdx.y, bi = (int)blockIdx.z;
    const unsigned tid = threadIdx.x;
    const bool solid = brick_all_solid(bricks, L, bi, bj, bk);
    bool any = false;
#pragma unroll 2
    for (int it = 0; it < kPhaseIter; ++it) {
        PhaseCell c = phase_cell(L, bi, bj, bk, it, tid);
        if (!c.in) continue;
        c.m = solid ? c.in : (load_mask_pair<VEC>(flags, c) & c.in);
        double t0 = 0.0, t1 = 0.0;
        if (c.m) load_pair<VEC>(T, c, t0, t1);
        for (int s = 0; s < 2; ++s) {
            if (!((c.in >> s) & 1u)) continue;
            const long p = c.p + s;
            double fn;
            if (!((c.m >> s) & 1u)) {
                fn = 0.0;
                F[p] = fn;
            } else if (sel == nullptr || sel[p] != 0) {
                const double e = (s ? t1 : t0) - w.Ts;
                fn = clamp01(e / w.dT);
                F[p] = fn;
            } else {
                fn = F[p];
            }
            any = any || fn != 0.0;
        }
    }
    const int nonzero = __syncthreads_or(any ? 1 : 0);
    if (tid == 0) summary[((long)bi * nby + bj) * nbz + bk] = nonzero ? 1u : 0u;
}

}  // namespace adi

using namespace adi;

extern "C" {

long adi_phase_summary_words(int nx, int ny, int nz)
{
    if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
    const long nbx = (nx + kBrick - 1) / kBrick, nby = (ny + kBrick - 1) / kBrick, nbz = (nz + kBrick - 1) / kBrick;
    return nbx * nby * nbz;
}

int adi_phase_apply(const adi_phase_change *h_law, double cp, double *d_T, double *d_f, const uint8_t *d_flags,
                    const uint32_t *d_bricks, const uint8_t *d_dir_mask, uint32_t *d_summary, int nx, int ny, int nz,
                    long plane_stride, void *stream)
{
    ADI_REQUIRE(h_law && d_T && d_f && d_flags && d_summary, "adi_phase_apply: null argument");
    ADI_REQUIRE(d_T != d_f, "adi_phase_apply: d_f aliases d_T");
    PhaseLaw w;
    if (int rc = make_phase_law("adi_phase_apply", *h_law, cp, &w)) return rc;
    PhaseLaunch g;
    if (int rc = make_phase_launch("adi_phase_apply", nx, ny, nz, plane_stride, &g)) return rc;
    if (pair_vec(g.L, d_flags, d_T, d_f))
        hipLaunchKernelGGL(k_phase_apply<true>, g.grid, dim3(256), 0, as_stream(stream), w, d_T, d_f, d_flags, d_bricks,
                           d_dir_mask, (unsigned *)d_summary, g.L, g.nby, g.nbz);
    else
        hipLaunchKernelGGL(k_phase_apply<false>, g.grid, dim3(256), 0, as_stream(stream), w, d_T, d_f, d_flags, d_bricks,
                           d_dir_mask, (unsigned *)d_summary, g.L, g.nby, g.nbz);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_phase_seed(const adi_phase_change *h_law, const double *d_T, double *d_f, const uint8_t *d_flags,
                   const uint32_t *d_bricks, const uint8_t *d_sel, uint32_t *d_summary, int nx, int ny, int nz,
                   long plane_stride, void *stream)
{
    ADI_REQUIRE(h_law && d_T && d_f && d_flags && d_summary, "adi_phase_seed: null argument");
    ADI_REQUIRE(d_T != d_f, "adi_phase_seed: d_f aliases d_T");
    PhaseLaw w;
    if (int rc = make_phase_law("adi_phase_seed", *h_law, 1.0, &w)) return rc;
    PhaseLaunch g;
    if (int rc = make_phase_launch("adi_phase_seed", nx, ny, nz, plane_stride, &g)) return rc;
    if (pair_vec(g.L, d_flags, d_T, d_f))
        hipLaunchKernelGGL(k_phase_seed<true>, g.grid, dim3(256), 0, as_stream(stream), w, d_T, d_f, d_flags, d_bricks, d_sel,
                           (unsigned *)d_summary, g.L, g.nby, g.nbz);
    else
        hipLaunchKernelGGL(k_phase_seed<false>, g.grid, dim3(256), 0, as_stream(stream), w, d_T, d_f, d_flags, d_bricks, d_sel,
                           (unsigned *)d_summary, g.L, g.nby, g.nbz);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // extern "C"
