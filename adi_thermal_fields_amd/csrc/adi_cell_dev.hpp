// adi_cell_dev.hpp -- what the one-thread-per-cell kernels of the Cartesian step share (device): the cell index ->
// (i, j, k, memory offset) of a padded-plane layout, over the whole box (cell_of) or over a range of axis-2 planes
// (cell_of_k), and the explicit stage's value of one cell (explicit_cell), which k_explicit_cell (adi_explicit.hip) stores
// and k_explicit_src (adi_source.hip) adds its source to.
#pragma once
#include "adi_cart_dev.hpp"

namespace adi {

// cell index -> (i, j, k, memory offset) for elementwise kernels over a padded-plane layout
__device__ __forceinline__ bool cell_of(long q, const Lay &L, int &i, int &j, int &k, long &p)
{
    const long plane = (long)L.ny * L.nz;
    if (q >= plane * L.nx) return false;
    i = (int)(q / plane);
    const long r = q - (long)i * plane;
    j = (int)(r / L.nz);
    k = (int)(r - (long)j * L.nz);
    p = (long)i * L.sx + r;
    return true;
}

// the same restricted to the planes [k0, k1) of axis 2 (the planes a layer birth touches)
__device__ __forceinline__ bool cell_of_k(long q, const Lay &L, int k0, int k1, int &i, int &j, int &k, long &p)
{
    const int nk = k1 - k0;
    if (q >= (long)L.nx * L.ny * nk) return false;
    const long row = q / nk;
    k = k0 + (int)(q - row * nk);
    i = (int)(row / L.ny);
    j = (int)(row - (long)i * L.ny);
    p = (long)i * L.sx + (long)j * L.nz + k;
    return true;
}

// R0 = T + f*((L0 + L1) + L2) of the cell at offset p, its six neighbours loaded only where the flags byte has them
// (lap1D_x/y/z + R0, adi3d_numba_coeff.py:240-288, :298); fl: the cell's flags byte.  in_mask() runs where the cell is in the
// mask, after the neighbour loads: what a caller loads only there.
template <class F>
__device__ __forceinline__ double explicit_cell(const double *__restrict__ T, const uint8_t *__restrict__ flags, long p,
                                                const Lay &L, double invdx2, double f, unsigned &fl, F in_mask)
{
#pragma clang fp contract(off)
    const long sx = L.sx, sy = L.nz;
    const double t = T[p];
    fl = flags[p];
    double L0 = 0.0, L1 = 0.0, L2 = 0.0;
    if (fl & 1u) {
        L0 = lap_axis(fl & 2u, fl & 4u, (fl & 2u) ? T[p - sx] : 0.0, (fl & 4u) ? T[p + sx] : 0.0, t, invdx2);
        L1 = lap_axis(fl & 8u, fl & 16u, (fl & 8u) ? T[p - sy] : 0.0, (fl & 16u) ? T[p + sy] : 0.0, t, invdx2);
        L2 = lap_axis(fl & 32u, fl & 64u, (fl & 32u) ? T[p - 1] : 0.0, (fl & 64u) ? T[p + 1] : 0.0, t, invdx2);
        in_mask();
    }
    return t + f * ((L0 + L1) + L2);
}

}  // namespace adi
