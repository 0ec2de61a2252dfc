// adi_matlaw.hip -- temperature-dependent k(T) and cp(T) around the linear Cartesian step (include/adi_hip.h, "Temperature-
// dependent conductivity and heat capacity"): the step runs on the Kirchhoff temperature Theta with the constant material
// (rho, cp_ref, k_ref), and the enthalpy is put back on its curve afterwards.
//   k_matlaw_theta     before the step: theta = Theta(T) on in-mask cells, T bit for bit on every other cell of the box (the
//                      sweeps pass off-mask cells through, so they hand T back there)
//   k_matlaw_recover   after sweep 2: T_new from T_old and theta*, written over theta*
//   k_surface_loss<., MatRatio>   the surface-loss update of adi_surface_loss_dev.hpp with robin_ratio multiplied into every h
// The first two are shaped like k_phase_apply (adi_brick_dev.hpp): one workgroup per 16^3 brick, 16-byte accesses where the rows
// allow it, the flags of all-solid bricks not read.  No existing kernel changes.
#include "adi_brick_dev.hpp"
#include "adi_matlaw_dev.hpp"
#include "adi_surface_loss_dev.hpp"

namespace adi {

template <bool VEC>
__global__ __launch_bounds__(256) void k_matlaw_theta(MatLaw w, const double *__restrict__ T, double *__restrict__ TH,
                                                      const uint8_t *__restrict__ flags, const unsigned *__restrict__ bricks,
                                                      Lay L)
{
#pragma clang fp contract(off)
    const int bk = (int)blockIdx.x, bj = (int)blockIdx.y, bi = (int)blockIdx.z;
    const unsigned tid = threadIdx.x;
    const bool solid = brick_all_solid(bricks, L, bi, bj, bk);
    PhaseCell c[kPhaseIter];
    double t[kPhaseIter][2];
#pragma unroll
    for (int it = 0; it < kPhaseIter; ++it) {
        c[it] = phase_cell(L, bi, bj, bk, it, tid);
        t[it][0] = 0.0; t[it][1] = 0.0;
        if (c[it].in) {
            c[it].m = solid ? c[it].in : (load_mask_pair<VEC>(flags, c[it]) & c[it].in);
            load_pair<VEC>(T, c[it], t[it][0], t[it][1]);
        }
    }
#pragma unroll
    for (int it = 0; it < kPhaseIter; ++it) {
        if (!c[it].in) continue;
        const double v0 = (c[it].m & 1u) ? mat_theta(w, t[it][0]) : t[it][0];
        const double v1 = (c[it].m & 2u) ? mat_theta(w, t[it][1]) : t[it][1];
        if (VEC) {
            *reinterpret_cast<double2 *>(TH + c[it].p) = make_double2(v0, v1);     // (VEC: both cells of a pair are in the box)
        } else {
            TH[c[it].p] = v0;
            if (c[it].in & 2u) TH[c[it].p + 1] = v1;
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_matlaw_recover(MatLaw w, const double *__restrict__ Tn, double *__restrict__ OUT,
                                                        const uint8_t *__restrict__ flags, const unsigned *__restrict__ bricks,
                                                        const uint8_t *__restrict__ dir, Lay L)
{
#pragma clang fp contract(off)
    const int bk = (int)blockIdx.x, bj = (int)blockIdx.y, bi = (int)blockIdx.z;
    const unsigned tid = threadIdx.x;
    const bool solid = brick_all_solid(bricks, L, bi, bj, bk);
    PhaseCell c[kPhaseIter];
    double t[kPhaseIter][2], o[kPhaseIter][2];
#pragma unroll
    for (int it = 0; it < kPhaseIter; ++it) {
        c[it] = phase_cell(L, bi, bj, bk, it, tid);
        if (c[it].in) c[it].m = solid ? c[it].in : (load_mask_pair<VEC>(flags, c[it]) & c[it].in);
    }
#pragma unroll
    for (int it = 0; it < kPhaseIter; ++it) {
        t[it][0] = 0.0; t[it][1] = 0.0; o[it][0] = 0.0; o[it][1] = 0.0;
        if (c[it].m) {
            load_pair<VEC>(Tn, c[it], t[it][0], t[it][1]);
            load_pair<VEC>(OUT, c[it], o[it][0], o[it][1]);
        }
    }
#pragma unroll
    for (int it = 0; it < kPhaseIter; ++it) {
        double v[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            v[s] = o[it][s];
            if (!((c[it].m >> s) & 1u)) continue;
            if (dir != nullptr && dir[c[it].p + s] != 0) {
                v[s] = mat_theta_inv(w, o[it][s]);
                continue;
            }
            double th, H;
            mat_theta_enthalpy(w, t[it][s], th, H);
            const double d = o[it][s] - th;
            const double g = w.cp_ref * d;
            const double Hn = H + g;
            v[s] = d == 0.0 ? t[it][s] : mat_enthalpy_inv(w, Hn);
        }
        if (VEC && c[it].m == 3u) {
            *reinterpret_cast<double2 *>(OUT + c[it].p) = make_double2(v[0], v[1]);
        } else {
            if (c[it].m & 1u) OUT[c[it].p] = v[0];
            if (c[it].m & 2u) OUT[c[it].p + 1] = v[1];
        }
    }
}

// robin_ratio: (t - Tinf) / (Theta(t) - Theta(Tinf)), and 1 / kq(Tinf) where the denominator is 0
struct MatRatio {
    static constexpr bool on = true;
    MatLaw w;
    double Tinf, theta_inf, rinf;
    __device__ __forceinline__ double operator()(double t) const
    {
#pragma clang fp contract(off)
        const double num = t - Tinf;
        const double th = mat_theta(w, t);
        const double den = th - theta_inf;
        return den == 0.0 ? rinf : num / den;
    }
};

}  // namespace adi

using namespace adi;

extern "C" {

int adi_matlaw_theta(const adi_material_law *h_law, const double *d_T, double *d_theta, const uint8_t *d_flags,
                     const uint32_t *d_bricks, int nx, int ny, int nz, long plane_stride, void *stream)
{
    ADI_REQUIRE(h_law && d_T && d_theta && d_flags, "adi_matlaw_theta: null argument");
    ADI_REQUIRE(d_T != d_theta, "adi_matlaw_theta: d_theta aliases d_T");
    if (int rc = check_matlaw("adi_matlaw_theta", *h_law)) return rc;
    PhaseLaunch g;
    if (int rc = make_phase_launch("adi_matlaw_theta", nx, ny, nz, plane_stride, &g)) return rc;
    if (pair_vec(g.L, d_flags, d_T, d_theta))
        hipLaunchKernelGGL(k_matlaw_theta<true>, g.grid, dim3(256), 0, as_stream(stream), *h_law, d_T, d_theta, d_flags,
                           d_bricks, g.L);
    else
        hipLaunchKernelGGL(k_matlaw_theta<false>, g.grid, dim3(256), 0, as_stream(stream), *h_law, d_T, d_theta, d_flags,
                           d_bricks, g.L);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_matlaw_recover(const adi_material_law *h_law, const double *d_T, double *d_out, const uint8_t *d_flags,
                       const uint32_t *d_bricks, const uint8_t *d_dir_mask, int nx, int ny, int nz, long plane_stride,
                       void *stream)
{
    ADI_REQUIRE(h_law && d_T && d_out && d_flags, "adi_matlaw_recover: null argument");
    ADI_REQUIRE(d_T != d_out, "adi_matlaw_recover: d_out aliases d_T");
    if (int rc = check_matlaw("adi_matlaw_recover", *h_law)) return rc;
    PhaseLaunch g;
    if (int rc = make_phase_launch("adi_matlaw_recover", nx, ny, nz, plane_stride, &g)) return rc;
    if (pair_vec(g.L, d_flags, d_T, d_out))
        hipLaunchKernelGGL(k_matlaw_recover<true>, g.grid, dim3(256), 0, as_stream(stream), *h_law, d_T, d_out, d_flags,
                           d_bricks, d_dir_mask, g.L);
    else
        hipLaunchKernelGGL(k_matlaw_recover<false>, g.grid, dim3(256), 0, as_stream(stream), *h_law, d_T, d_out, d_flags,
                           d_bricks, d_dir_mask, g.L);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_matlaw_loss_update(const adi_material_law *h_mat, const adi_surface_loss *h_law, double Tinf, const double *d_T,
                           const uint8_t *d_flags, const uint32_t *d_bricks, int nx, int ny, int nz, long plane_stride, double dx,
                           double rho, double cp, double *const d_coeff[3], int k_begin, int k_end, int full, void *stream)
{
#pragma clang fp contract(off)
    ADI_REQUIRE(h_mat, "adi_matlaw_loss_update: null argument");
    if (int rc = check_matlaw("adi_matlaw_loss_update", *h_mat)) return rc;
    ADI_REQUIRE(isfinite(Tinf), "adi_matlaw_loss_update: Tinf not finite");
    MatRatio r;
    r.w = *h_mat;
    r.Tinf = Tinf;
    r.theta_inf = mat_theta(r.w, Tinf);
    const double q = mat_kq(r.w, Tinf);
    r.rinf = 1.0 / q;
    return launch_surface_loss("adi_matlaw_loss_update", r, h_law, Tinf, d_T, d_flags, d_bricks, nx, ny, nz, plane_stride, dx, rho,
                               cp, d_coeff, k_begin, k_end, full, stream);
}

}  // extern "C"
