// adi_matmap_dev.hpp -- device-side pieces of the several-materials step (adi_matmap.hip): the scalars a
// launch carries by value, the row of a sweep whose couplings differ from face to face, the host's check of the tables, the
// pack values of one cell (shared with adi_matmap_transition.hip) and the id bytes of a brick pass's pair of cells.
#pragma once
#include "adi_cart_host.hpp"
#include "adi_cell_dev.hpp"
#include "adi_brick_dev.hpp"

namespace adi {

constexpr int kMapMaxMat = ADI_MATMAP_MAX;   // (a power of two: ids are masked with kMapMaxMat - 1) materials per grid: the pair table is kMapMaxMat x kMapMaxMat doubles

// What a launch of the several-materials kernels carries by value.  g: the pair table, G[m][n] in the explicit stage and
// theta * G[m][n] in the sweeps, row m = the cell's own material (each row is divided by the cell's own C, so g is not
// symmetric).  c: C_m = rho_m cp_m (explicit stage with a source) or C_m dx^3 (coefficient build).
struct MapScal {
    double g[kMapMaxMat * kMapMaxMat];
    double c[kMapMaxMat];
    double dt, Tinf, om;           // om = 1 - theta (explicit stage)
};

// The tables go through LDS: a lane picks the entry of (own id, neighbour's id), an index that differs from lane to lane,
// and an indexed read of a by-value kernel argument would put the whole table into scratch.
__device__ __forceinline__ void map_tables_to_lds(const MapScal &s, double *sG, double *sC)
{
    const double *kg = s.g, *kc = s.c;
    for (int t = threadIdx.x; t < kMapMaxMat * kMapMaxMat; t += blockDim.x) sG[t] = kg[t];
    if (sC != nullptr)
        for (int t = threadIdx.x; t < kMapMaxMat; t += blockDim.x) sC[t] = kc[t];
    __syncthreads();
}

// Off-diagonals of the M rows of a segment for condense / back_solve of adi_core.hpp (any type with operator[]): an
// off-diagonal takes one of the at most 64 values -theta G[m][n] or 0, so a row keeps one byte -- the 6-bit pair index m * 8 + n and
// a coupling bit -- eight rows to a 64-bit word, and the value is read from the table's copy in LDS where it is used: 2 VGPRs per
// off-diagonal of an 8-row segment instead of 16.  t: the LDS table of the NEGATED couplings (the off-diagonals themselves).
template <int M>
struct TableCoef {
    unsigned long long w[(M + 7) / 8];
    const double *t;
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int i = 0; i < (M + 7) / 8; ++i) w[i] = 0ull;
    }
    __device__ __forceinline__ void set(int r, unsigned pair, bool couples)
    {
        w[r >> 3] |= (unsigned long long)((pair & 63u) | (couples ? 64u : 0u)) << (8 * (r & 7));
    }
    __device__ __forceinline__ double operator[](int r) const
    {
        const unsigned b = (unsigned)(w[r >> 3] >> (8 * (r & 7)));
        return (b & 64u) ? t[b & 63u] : 0.0;
    }
};

// One row of the full-length system of a sweep (include/adi_hip.h, "Several materials"):
//   free cell      (e + p + q) x_i - p x_{i-1} - q x_{i+1} = d,  e = 1 + dt coeff,  d = in + dt qflux + dt coeff Tinf
//   Dirichlet cell x = dv          off-mask cell x = in
// plo / phi: theta G[id_i][id_{i-1}] / theta G[id_i][id_{i+1}], used only where that neighbour is in the mask (lo / hi).
// The row is returned in the excess form (e, p, q) the thread-per-line solver eliminates without a subtraction.
template <bool HAS_DIR, bool HAS_Q>
__device__ __forceinline__ void map_row(bool m, bool lo, bool hi, bool dir, double in, double co, double dv, double qv,
                                        double plo, double phi, double dt, double Tinf, double &e, double &p, double &q,
                                        double &d)
{
    const bool fr = HAS_DIR ? (m && !dir) : m;
    const double dc = dt * co;
    p = (fr && lo) ? plo : 0.0;
    q = (fr && hi) ? phi : 0.0;
    e = fr ? (1.0 + dc) : 1.0;
    double rhs = in;
    if (HAS_Q) rhs = rhs + dt * qv;
    rhs = rhs + dc * Tinf;
    d = fr ? rhs : ((HAS_DIR && m) ? dv : in);
}

struct MapFaceSpec {
    int mode[6];
    double scalar[6];
    const double *field[6];
};

// k_build_coeffs (adi_fields.hip) with the cell's own heat capacity: '-' face then '+' face per axis, (h * A) / (C_id * V) with
// IEEE division, contraction off -> bit-identical to MaterialMap.packs_reference.  The six values of the cell (i, j, k) at
// offset p, zeros where it is not exposed: what the coefficient builds (adi_matmap.hip) and the transition pass
// (adi_matmap_transition.hip) store.  Ccell: C_id * V of the cell's own material (not used off the mask).
__device__ __forceinline__ void map_coeffs_cell_c(const uint8_t *__restrict__ mask, const Lay &L, double A, double Ccell,
                                                  const MapFaceSpec &h, const MapFaceSpec &q, int i, int j, int k, long p,
                                                  double *__restrict__ c0, double *__restrict__ c1, double *__restrict__ c2,
                                                  double *__restrict__ q0, double *__restrict__ q1, double *__restrict__ q2)
{
#pragma clang fp contract(off)
    const long st[3] = {L.sx, (long)L.nz, 1};
    const int pos[3] = {i, j, k}, nn[3] = {L.nx, L.ny, L.nz};
    const bool m = mask[p] != 0;
    double co[3] = {0.0, 0.0, 0.0}, qq[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        const int ax = f >> 1;
        const int nbp = pos[ax] + ((f & 1) ? 1 : -1);
        bool exposed = m;
        if (m && nbp >= 0 && nbp < nn[ax]) exposed = mask[p + ((f & 1) ? st[ax] : -st[ax])] == 0;
        if (exposed) {
            if (h.mode[f] != ADI_FACE_NONE) {
                const double hv = (h.mode[f] == ADI_FACE_SCALAR) ? h.scalar[f] : h.field[f][p];
                co[ax] += (hv * A / Ccell);
            }
            if (q.mode[f] != ADI_FACE_NONE) {
                const double qv = (q.mode[f] == ADI_FACE_SCALAR) ? q.scalar[f] : q.field[f][p];
                qq[ax] += (qv * A / Ccell);
            }
        }
    }
    c0[p] = co[0]; c1[p] = co[1]; c2[p] = co[2];
    q0[p] = qq[0]; q1[p] = qq[1]; q2[p] = qq[2];
}

// ... with C read from the id field.  sC: C_m * V in LDS.  An id off the mask is not read.
__device__ __forceinline__ void map_coeffs_cell(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ ids, const Lay &L,
                                                double A, const double *sC, const MapFaceSpec &h, const MapFaceSpec &q, int i, int j,
                                                int k, long p, double *__restrict__ c0, double *__restrict__ c1,
                                                double *__restrict__ c2, double *__restrict__ q0, double *__restrict__ q1,
                                                double *__restrict__ q2)
{
    const double Ccell = mask[p] != 0 ? sC[ids[p] & (kMapMaxMat - 1)] : 1.0;
    map_coeffs_cell_c(mask, L, A, Ccell, h, q, i, j, k, p, c0, c1, c2, q0, q1, q2);
}

// the face specs of a coefficient build as the kernels take them, or the first rule of the header the arguments break
inline int make_face_specs(const char *who, const int *h_mode, const double *h_scalar, const double *const *d_h_field,
                           const int *q_mode, const double *q_scalar, const double *const *d_q_field, MapFaceSpec *h,
                           MapFaceSpec *q)
{
    for (int f = 0; f < 6; ++f) {
        h->mode[f] = h_mode[f]; h->scalar[f] = h_scalar[f]; h->field[f] = d_h_field ? d_h_field[f] : nullptr;
        q->mode[f] = q_mode[f]; q->scalar[f] = q_scalar[f]; q->field[f] = d_q_field ? d_q_field[f] : nullptr;
        ADI_REQUIRE(h->mode[f] >= 0 && h->mode[f] <= 2 && q->mode[f] >= 0 && q->mode[f] <= 2, "%s: bad face mode", who);
        ADI_REQUIRE(h->mode[f] != ADI_FACE_FIELD || h->field[f], "%s: missing h field for face %d", who, f);
        ADI_REQUIRE(q->mode[f] != ADI_FACE_FIELD || q->field[f], "%s: missing q field for face %d", who, f);
    }
    return ADI_OK;
}

// the id bytes of a pair: cell 0 in bits 0-7, cell 1 in bits 8-15 (VEC: one 2-byte load, the id field 2-byte aligned)
template <bool VEC>
__device__ __forceinline__ unsigned load_id_pair(const uint8_t *ids, const PhaseCell &c)
{
    if (VEC) return *reinterpret_cast<const unsigned short *>(ids + c.p);
    unsigned v = ids[c.p];
    if (c.in & 2u) v |= (unsigned)ids[c.p + 1] << 8;
    return v;
}

__device__ __forceinline__ unsigned id_of(unsigned pair, int s) { return (pair >> (8 * s)) & (unsigned)(kMapMaxMat - 1); }

// pair loads (adi_brick_dev.hpp) of the fields a, b and of the flags and id bytes
inline bool map_pair_vec(const Lay &L, const void *flags, const void *ids, const void *a, const void *b)
{
    return pair_vec(L, flags, a, b) && ((uintptr_t)ids & 1) == 0;
}

// nmat and the first nmat x nmat entries of a pair table / nmat entries of a C table
inline int check_tables(const char *who, int nmat, const double *h_G, const double *h_C)
{
    ADI_REQUIRE(nmat >= 1 && nmat <= kMapMaxMat, "%s: %d materials (1 to %d)", who, nmat, kMapMaxMat);
    for (int m = 0; m < nmat; ++m) {
        if (h_C != nullptr) ADI_REQUIRE(isfinite(h_C[m]) && h_C[m] > 0.0, "%s: C of material %d must be finite and > 0", who, m);
        if (h_G != nullptr)
            for (int k = 0; k < nmat; ++k)
                ADI_REQUIRE(isfinite(h_G[m * kMapMaxMat + k]) && h_G[m * kMapMaxMat + k] > 0.0,
                            "%s: pair table entry [%d][%d] must be finite and > 0", who, m, k);
    }
    return ADI_OK;
}

}  // namespace adi
