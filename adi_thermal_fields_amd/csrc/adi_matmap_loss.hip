// adi_matmap_loss.hip -- temperature-dependent surface loss on a grid of several materials (include/adi_hip.h, "Several
// materials: latent heat and surface loss"): the Robin coefficient arrays of a MaterialMap rewritten in
// place from the field at the start of a step, every exposed cell by the law and the heat capacity of its own material.
//   k_maploss<false>   every step: only the in-mask cells exposed along an axis are written
//   k_maploss<true>    a plane range in full: zeros where a cell is not exposed along the axis
// The structure is k_surface_loss's (adi_surface_loss_dev.hpp): one workgroup per 16 x 16 x 16 brick, thread (di, dj) owns the 16
// cells of row (i, j) along axis 2, reads their flags bytes in one 16-byte load and leaves early on a set inner brick.  The id
// byte and T are loaded only at open cells.  Eight LossLaw records are too large for the kernel arguments: they live, with
// C_m dx^3, in a device table the caller owns (adi_matmap_loss_table fills its host image; nothing in it depends on Tinf), and
// a cell reads the record of its material through the caches.  Ta = Tinf + T_offset and Ta2 = Ta * Ta are evaluated per cell
// from Tinf by value: the two fp64 operations the host performs for k_surface_loss.  Arithmetic: the law of the header, then
// (h * A) / (C_id * V) accumulated '-' face first -- the expressions of k_matmap_build_coeffs fed with the six h fields,
// contraction off.
#include <string.h>

#include "adi_surface_loss_dev.hpp"
#include "adi_matmap_dev.hpp"

namespace adi {

struct MapLossTable {
    LossLaw law[kMapMaxMat];    // Ta and Ta2 are not used: the kernel evaluates them from the launch's Tinf
    double cv[kMapMaxMat];      // C_m * (dx dx dx)
    int nmat, reserved;
};

template <bool FULL>
__global__ __launch_bounds__(256) void k_maploss(const MapLossTable *__restrict__ tab, double Tinf,
                                                     const double *__restrict__ T, const uint8_t *__restrict__ flags,
                                                     const unsigned *__restrict__ bricks, const uint8_t *__restrict__ ids,
                                                     Lay L, int bnz, int bwx, double A, double *__restrict__ c0,
                                                     double *__restrict__ c1, double *__restrict__ c2, int k0, int k1, int bk0,
                                                     int packed)
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
        const unsigned id = ids[p] & (unsigned)(kMapMaxMat - 1);
        const LossLaw &w = tab->law[id];
        const double Ccell = tab->cv[id];
        const double t = T[p];
        const double off = w.T_offset;
        const double Ta = Tinf + off;
        const double Ta2 = Ta * Ta;
        const double Tk = t + off;
        const double s2 = Tk * Tk + Ta2;
        const double s1 = Tk + Ta;
        const double tab_h = w.n > 0 ? loss_table(w, t) : 0.0;
        double co[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            co[a] = 0.0;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int f = 2 * a + s;
                if ((fl & (2u << f)) == 0u) {        // bit 1 + f: the neighbour across face f is in the mask
                    const double rad = (w.eps_sigma[f] * s2) * s1;
                    const double hv = (w.h[f] + (w.tab_on[f] ? tab_h : 0.0)) + rad;
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

}  // namespace adi

using namespace adi;

extern "C" {

size_t adi_matmap_loss_table_bytes(void) { return sizeof(MapLossTable); }

int adi_matmap_loss_table(int nmat, const adi_surface_loss *h_laws, const double *h_C, double dx, void *h_table, size_t bytes)
{
#pragma clang fp contract(off)
    ADI_REQUIRE(h_laws && h_C && h_table, "adi_matmap_loss_table: null argument");
    ADI_REQUIRE(bytes >= sizeof(MapLossTable), "adi_matmap_loss_table: the table needs %zu bytes, not %zu", sizeof(MapLossTable),
                bytes);
    ADI_REQUIRE(nmat >= 1 && nmat <= kMapMaxMat, "adi_matmap_loss_table: %d materials (1 to %d)", nmat, kMapMaxMat);
    ADI_REQUIRE(isfinite(dx) && dx > 0.0, "adi_matmap_loss_table: dx must be finite and > 0");
    MapLossTable t = {};
    const double V = dx * dx * dx;
    for (int m = 0; m < kMapMaxMat; ++m) t.cv[m] = 1.0;
    for (int m = 0; m < nmat; ++m) {
        const adi_surface_loss &s = h_laws[m];
        if (int rc = check_law(s, 1.0 - s.T_offset)) return rc;      // (every rule but the ambient's, which the update checks)
        ADI_REQUIRE(isfinite(h_C[m]) && h_C[m] > 0.0, "adi_matmap_loss_table: C of material %d must be finite and > 0", m);
        LossLaw &w = t.law[m];
        bool table_used = false;
        for (int f = 0; f < 6; ++f) {
            w.h[f] = s.h[f];
            w.eps_sigma[f] = s.emissivity[f] * ADI_SURFACE_LOSS_SIGMA;
            w.tab_on[f] = (s.n_knots > 0 && (s.h[f] != 0.0 || s.emissivity[f] != 0.0)) ? 1 : 0;
            table_used = table_used || w.tab_on[f];
        }
        w.T_offset = s.T_offset;
        w.n = table_used ? s.n_knots : 0;
        for (int k = 0; k < s.n_knots; ++k) { w.xp[k] = s.knot_T[k]; w.fp[k] = s.knot_h[k]; }
        for (int k = 0; k + 1 < s.n_knots; ++k) w.slope[k] = (w.fp[k + 1] - w.fp[k]) / (w.xp[k + 1] - w.xp[k]);
        t.cv[m] = h_C[m] * V;
    }
    t.nmat = nmat;
    memcpy(h_table, &t, sizeof(t));
    return ADI_OK;
}

int adi_matmap_loss_update(const void *d_table, double Tinf, double min_T_offset, const double *d_T, const uint8_t *d_flags,
                           const uint32_t *d_bricks, const uint8_t *d_ids, int nx, int ny, int nz, long plane_stride,
                           double dx, double *const d_coeff[3], int k_begin, int k_end, int full, void *stream)
{
#pragma clang fp contract(off)
    const char *who = "adi_matmap_loss_update";
    ADI_REQUIRE(d_table && d_T && d_flags && d_ids && d_coeff, "%s: null argument", who);
    for (int a = 0; a < 3; ++a) ADI_REQUIRE(d_coeff[a], "%s: null output", who);
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    if (int rc = check_plane_range(who, k_begin, k_end, nz)) return rc;
    ADI_REQUIRE(isfinite(dx) && dx > 0.0, "%s: dx must be finite and > 0", who);
    ADI_REQUIRE(isfinite(Tinf) && isfinite(min_T_offset), "%s: Tinf or T_offset not finite", who);
    ADI_REQUIRE(Tinf + min_T_offset > 0.0, "%s: Tinf + T_offset <= 0 (the ambient in kelvin)", who);
    if (k_begin == k_end) return ADI_OK;
    const double A = dx * dx;
    const int nbx = (nx + kBrick - 1) / kBrick, nby = (ny + kBrick - 1) / kBrick, nbz = (nz + kBrick - 1) / kBrick;
    const int bwx = (nbx + 31) >> 5;
    const int bk0 = k_begin / kBrick, bk1 = (k_end + kBrick - 1) / kBrick;
    ADI_REQUIRE(nby <= 65535 && nbx <= 65535, "%s: box of %d x %d x %d is too large", who, nx, ny, nz);
    // 16-byte flag loads: rows of whole bricks whose first byte is 16-byte aligned
    const int packed = (L.nz % 16 == 0 && L.sx % 16 == 0 && ((uintptr_t)d_flags & 15) == 0) ? 1 : 0;
    const dim3 grid((unsigned)(bk1 - bk0), (unsigned)nby, (unsigned)nbx);
    const MapLossTable *tab = (const MapLossTable *)d_table;
    if (full)
        hipLaunchKernelGGL(k_maploss<true>, grid, dim3(256), 0, as_stream(stream), tab, Tinf, d_T, d_flags, d_bricks, d_ids,
                           L, nbz, bwx, A, d_coeff[0], d_coeff[1], d_coeff[2], k_begin, k_end, bk0, packed);
    else
        hipLaunchKernelGGL(k_maploss<false>, grid, dim3(256), 0, as_stream(stream), tab, Tinf, d_T, d_flags, d_bricks, d_ids,
                           L, nbz, bwx, A, d_coeff[0], d_coeff[1], d_coeff[2], k_begin, k_end, bk0, packed);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // extern "C"
