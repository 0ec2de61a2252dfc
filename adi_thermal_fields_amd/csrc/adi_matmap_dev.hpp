// adi_matmap_dev.hpp -- device-side pieces of the several-materials step (adi_matmap.hip): the scalars a
// launch carries by value, the row of a sweep whose couplings differ from face to face, and the host's check of the tables.
#pragma once
#include "adi_cart_host.hpp"
#include "adi_cell_dev.hpp"

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
