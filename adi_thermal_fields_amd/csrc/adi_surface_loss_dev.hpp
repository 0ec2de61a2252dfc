// adi_surface_loss_dev.hpp -- temperature-dependent surface loss of the Cartesian step (include/adi_hip.h, "Temperature-dependent
// surface loss"): the Robin coefficient arrays of the three axes rewritten in place from the field at the start of a step.
//   k_surface_loss<false>   every step: only the in-mask cells exposed along an axis are written, T is loaded only where a
//                           cell has an exposed face, bricks without such a cell are left after one word of the flags summary
//   k_surface_loss<true>    a new pack set / the planes a birth changed: every cell of the planes is written, zeros where
//                           the cell is not exposed along the axis
// One workgroup per 16 x 16 x 16 brick of the flags summary; thread (di, dj) owns the 16 cells of row (i, j) along axis 2 and
// reads their flags bytes in one 16-byte load.  Arithmetic: the law of the header, then (h * A) / Ccell accumulated '-' face
// first -- the expressions of k_build_coeffs (adi_fields.hip) fed with the six h fields, contraction off.  No existing
// kernel changes: the sweeps read the arrays as they read any pack built from per-voxel h.
// A header, because adi_matlaw.hip launches the same kernel with a ratio multiplied into every h (RATIO below).
#pragma once
#include <math.h>

#include "adi_cart_host.hpp"

namespace adi {

// the law as the kernel takes it: products and quotients that do not depend on the cell evaluated once on the host, each
// the very fp64 operation the per-cell expression would perform
struct LossLaw {
    double h[6];
    double eps_sigma[6];      // emissivity[f] * SIGMA
    int tab_on[6];            // the table applies to face f (h[f] or emissivity[f] non-zero, and a table is given)
    double T_offset, Ta, Ta2; // Ta = Tinf + T_offset, Ta2 = Ta * Ta
    int n;                    // knots (0: no table)
    double xp[ADI_SURFACE_LOSS_MAX_KNOTS], fp[ADI_SURFACE_LOSS_MAX_KNOTS];
    double slope[ADI_SURFACE_LOSS_MAX_KNOTS];   // (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]), j < n - 1
};

// piecewise-linear table at t, clamped to the end values (t >= 2 knots); the interval is found by selects, so no per-lane
// index into the kernel arguments is needed
__device__ __forceinline__ double loss_table(const LossLaw &w, double t)
{
#pragma clang fp contract(off)
    double x0 = w.xp[0], f0 = w.fp[0], sl = w.slope[0];
    for (int m = 1; m < w.n - 1; ++m)
        if (t >= w.xp[m]) { x0 = w.xp[m]; f0 = w.fp[m]; sl = w.slope[m]; }
    double tab = f0 + sl * (t - x0);
    if (t < w.xp[0]) tab = w.fp[0];
    if (t >= w.xp[w.n - 1]) tab = w.fp[w.n - 1];
    return tab;
}

// RATIO: what every h is multiplied by ahead of A / Ccell, a function of the cell's temperature (adi_matlaw.hip); NoRatio: nothing,
// the arithmetic of adi_surface_loss_update as it always was
struct NoRatio {
    static constexpr bool on = false;
    __device__ __forceinline__ double operator()(double) const { return 1.0; }
};

template <bool FULL, class RATIO>
__global__ __launch_bounds__(256) void k_surface_loss(LossLaw w, RATIO ratio, const double *__restrict__ T,
                                                      const uint8_t *__restrict__ flags, const unsigned *__restrict__ bricks,
                                                      Lay L, int bnz, int bwx, double A, double Ccell,
                                                      double *__restrict__ c0, double *__restrict__ c1,
                                                      double *__restrict__ c2, int k0, int k1, int bk0, int packed)
{
#pragma clang fp contract(off)
    const int bk = bk0 + (int)blockIdx.x, bj = (int)blockIdx.y, bi = (int)blockIdx.z;
    if (!FULL && bricks != nullptr) {
        // a set brick holds the flags its position implies: exposed faces only on the faces of the box
        const bool inner = bi > 0 && (bi + 1) * kBrick < L.nx && bj > 0 && (bj + 1) * kBrick < L.ny && bk > 0 &&
                           (bk + 1) * kBrick < L.nz;
        if (inner && (bricks[brick_word(bi * kBrick, bj * kBrick, bk * kBrick, bnz, bwx)] & brick_bit(bi * kBrick)) != 0u)
            return;
    }
    const int i = bi * kBrick + (int)(threadIdx.x >> 4), j = bj * kBrick + (int)(threadIdx.x & 15u);
    if (i >= L.nx || j >= L.ny) return;
    const int kb = bk * kBrick;
    const long p0 = (long)i * L.sx + (long)j * L.nz + kb;
    // the 16 flags bytes of the row piece, byte b in bits 8b.. of lo (b < 8) / hi; bytes beyond the row read as 0
    unsigned long long lo = 0, hi = 0;
    if (packed && kb + kBrick <= L.nz) {
        const uint4 v = *reinterpret_cast<const uint4 *>(flags + p0);
        lo = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
        hi = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
    } else {
        for (int b = 0; b < kBrick; ++b) {
            if (kb + b >= L.nz) break;
            const unsigned long long f = flags[p0 + b];
            if (b < 8) lo |= f << (8 * b);
            else hi |= f << (8 * (b - 8));
        }
    }
    if (!FULL && lo == 0 && hi == 0) return;
    const int b_begin = k0 > kb ? k0 - kb : 0, b_end = k1 - kb < kBrick ? k1 - kb : kBrick;   // (k1 <= nz)
#pragma unroll 1
    for (int b = b_begin; b < b_end; ++b) {
        const unsigned fl = (unsigned)((b < 8 ? lo >> (8 * b) : hi >> (8 * (b - 8))) & 0xffull);
        const bool open = (fl & 1u) != 0u && (fl & 0x7eu) != 0x7eu;     // in the mask, a neighbour missing
        const long p = p0 + b;
        if (!open) {
            if (FULL) { c0[p] = 0.0; c1[p] = 0.0; c2[p] = 0.0; }
            continue;
        }
        const double t = T[p];
        const double Tk = t + w.T_offset;
        const double s2 = Tk * Tk + w.Ta2;
        const double s1 = Tk + w.Ta;
        const double tab = w.n > 0 ? loss_table(w, t) : 0.0;
        const double rt = RATIO::on ? ratio(t) : 1.0;
        double co[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            co[a] = 0.0;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int f = 2 * a + s;
                if ((fl & (2u << f)) == 0u) {        // bit 1 + f: the neighbour across face f is in the mask
                    const double rad = (w.eps_sigma[f] * s2) * s1;
                    double hv = (w.h[f] + (w.tab_on[f] ? tab : 0.0)) + rad;
                    if (RATIO::on) hv = hv * rt;
                    co[a] += (hv * A / Ccell);
                }
            }
        }
        if ((fl & 0x06u) != 0x06u) c0[p] = co[0];
        else if (FULL) c0[p] = 0.0;
        if ((fl & 0x18u) != 0x18u) c1[p] = co[1];
        else if (FULL) c1[p] = 0.0;
        if ((fl & 0x60u) != 0x60u) c2[p] = co[2];
        else if (FULL) c2[p] = 0.0;
    }
}

// ADI_OK, or the first rule of the header the law breaks
inline int check_law(const adi_surface_loss &s, double Tinf)
{
    for (int f = 0; f < 6; ++f) {
        ADI_REQUIRE(isfinite(s.h[f]) && s.h[f] >= 0.0, "adi_surface_loss: h < 0 or not finite on face %d", f);
        ADI_REQUIRE(isfinite(s.emissivity[f]) && s.emissivity[f] >= 0.0 && s.emissivity[f] <= 1.0,
                    "adi_surface_loss: emissivity outside [0, 1] on face %d", f);
    }
    ADI_REQUIRE(isfinite(s.T_offset) && isfinite(Tinf), "adi_surface_loss: T_offset or Tinf not finite");
    ADI_REQUIRE(Tinf + s.T_offset > 0.0, "adi_surface_loss: Tinf + T_offset <= 0 (the ambient in kelvin)");
    ADI_REQUIRE(s.n_knots == 0 || (s.n_knots >= 2 && s.n_knots <= ADI_SURFACE_LOSS_MAX_KNOTS),
                "adi_surface_loss: a table has 2 to %d knots, not %d", ADI_SURFACE_LOSS_MAX_KNOTS, s.n_knots);
    for (int m = 0; m < s.n_knots; ++m) {
        ADI_REQUIRE(isfinite(s.knot_T[m]) && isfinite(s.knot_h[m]), "adi_surface_loss: knot %d not finite", m);
        ADI_REQUIRE(m == 0 || s.knot_T[m] > s.knot_T[m - 1], "adi_surface_loss: knots do not increase at knot %d", m);
    }
    return ADI_OK;
}

// the body of adi_surface_loss_update, for it and for adi_matlaw_loss_update (`who` names the entry in error texts)
template <class RATIO>
int launch_surface_loss(const char *who, const RATIO &ratio, const adi_surface_loss *h_law, double Tinf, const double *d_T,
                        const uint8_t *d_flags, const uint32_t *d_bricks, int nx, int ny, int nz, long plane_stride, double dx,
                        double rho, double cp, double *const d_coeff[3], int k_begin, int k_end, int full, void *stream)
{
#pragma clang fp contract(off)
    ADI_REQUIRE(h_law && d_T && d_flags && d_coeff, "%s: null argument", who);
    for (int a = 0; a < 3; ++a) ADI_REQUIRE(d_coeff[a], "%s: null output", who);
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    if (int rc = check_plane_range(who, k_begin, k_end, nz)) return rc;
    ADI_REQUIRE(dx > 0.0 && rho > 0.0 && cp > 0.0, "%s: dx, rho and cp must be > 0", who);
    if (int rc = check_law(*h_law, Tinf)) return rc;
    if (k_begin == k_end) return ADI_OK;
    LossLaw w;
    bool table_used = false;
    for (int f = 0; f < 6; ++f) {
        w.h[f] = h_law->h[f];
        w.eps_sigma[f] = h_law->emissivity[f] * ADI_SURFACE_LOSS_SIGMA;
        w.tab_on[f] = (h_law->n_knots > 0 && (h_law->h[f] != 0.0 || h_law->emissivity[f] != 0.0)) ? 1 : 0;
        table_used = table_used || w.tab_on[f];
    }
    w.T_offset = h_law->T_offset;
    w.Ta = Tinf + h_law->T_offset;
    w.Ta2 = w.Ta * w.Ta;
    w.n = table_used ? h_law->n_knots : 0;
    for (int m = 0; m < ADI_SURFACE_LOSS_MAX_KNOTS; ++m) {
        const bool in = m < h_law->n_knots;
        w.xp[m] = in ? h_law->knot_T[m] : 0.0;
        w.fp[m] = in ? h_law->knot_h[m] : 0.0;
        w.slope[m] = 0.0;
    }
    for (int m = 0; m + 1 < h_law->n_knots; ++m) w.slope[m] = (w.fp[m + 1] - w.fp[m]) / (w.xp[m + 1] - w.xp[m]);
    double A, Ccell;
    cell_constants(dx, rho, cp, &A, &Ccell);
    const int nbx = (nx + kBrick - 1) / kBrick, nby = (ny + kBrick - 1) / kBrick, nbz = (nz + kBrick - 1) / kBrick;
    const int bwx = (nbx + 31) >> 5;
    const int bk0 = k_begin / kBrick, bk1 = (k_end + kBrick - 1) / kBrick;
    ADI_REQUIRE(nby <= 65535 && nbx <= 65535, "%s: box of %d x %d x %d is too large", who, nx, ny, nz);
    // 16-byte flag loads: rows of whole bricks whose first byte is 16-byte aligned
    const int packed = (L.nz % 16 == 0 && L.sx % 16 == 0 && ((uintptr_t)d_flags & 15) == 0) ? 1 : 0;
    const dim3 grid((unsigned)(bk1 - bk0), (unsigned)nby, (unsigned)nbx);
    if (full)
        hipLaunchKernelGGL((k_surface_loss<true, RATIO>), grid, dim3(256), 0, as_stream(stream), w, ratio, d_T, d_flags,
                           d_bricks, L, nbz, bwx, A, Ccell, d_coeff[0], d_coeff[1], d_coeff[2], k_begin, k_end, bk0, packed);
    else
        hipLaunchKernelGGL((k_surface_loss<false, RATIO>), grid, dim3(256), 0, as_stream(stream), w, ratio, d_T, d_flags,
                           d_bricks, L, nbz, bwx, A, Ccell, d_coeff[0], d_coeff[1], d_coeff[2], k_begin, k_end, bk0, packed);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // namespace adi
