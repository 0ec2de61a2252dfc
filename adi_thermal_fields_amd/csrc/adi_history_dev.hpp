// adi_history_dev.hpp -- what the recorders of the Cartesian step share (adi_history.hip: peak, cooling time, melt pool;
// adi_solidify.hip: the conditions at the freezing front): the device block of the clock, the cell ownership of a 16 x 16 x 16
// brick with its two load forms, the all-solid test of the flags summary, the wave reductions and the launch geometry.
// One workgroup of 256 threads per brick, with the cell ownership of adi_phase.hip: lane l of a wave owns cells 2(l & 7),
// 2(l & 7) + 1 of row (l >> 3), so one 16-byte load instruction of a wave covers eight whole 128-byte row pieces, and the eight
// loads of a thread cover the 256 rows of the brick.
#pragma once
#include "adi_cart_host.hpp"

namespace adi {

struct HistBlock {
    double t0, dt;
    long long n, slot, capacity;
};
static_assert(sizeof(HistBlock) == ADI_HISTORY_BLOCK_BYTES, "history block layout");

constexpr int kHistIter = 8;      // row groups of a brick per thread: 256 rows / (256 threads / 8 lanes per row)

struct HistCell {
    long p;          // offset of the pair's first cell
    unsigned in;     // bit c: cell c of the pair lies inside the box
    unsigned m;      // bit c: ... and in the mask
};

// 16-byte access needs even row and plane strides and 16-byte aligned arrays (host: `vec`); then a pair never straddles the
// end of a row.  Otherwise cell by cell.
template <bool VEC>
__device__ __forceinline__ void hist_load_pair(const double *a, const HistCell &c, double &v0, double &v1)
{
    if (VEC) {
        const double2 v = *reinterpret_cast<const double2 *>(a + c.p);
        v0 = v.x; v1 = v.y;
    } else {
        v0 = a[c.p];
        v1 = (c.in & 2u) ? a[c.p + 1] : 0.0;
    }
}

template <bool VEC>
__device__ __forceinline__ unsigned hist_mask_pair(const uint8_t *__restrict__ flags, const HistCell &c)
{
    if (VEC) {
        const unsigned v = *reinterpret_cast<const unsigned short *>(flags + c.p);
        return (v & 1u) | ((v >> 7) & 2u);
    }
    unsigned m = flags[c.p] & 1u;
    if (c.in & 2u) m |= (flags[c.p + 1] & 1u) << 1;
    return m;
}

// the pair of cells thread `tid` owns in row group `it` of brick (bi, bj, bk): local (i, j, k) = (2 it + (tid >> 7),
// (tid >> 3) & 15, 2 (tid & 7))
__device__ __forceinline__ HistCell hist_cell(const Lay &L, int bi, int bj, int bk, int it, unsigned tid)
{
    const int row = it * 32 + (int)(tid >> 3);
    const int i = bi * kBrick + (row >> 4), j = bj * kBrick + (row & 15), k = bk * kBrick + 2 * (int)(tid & 7u);
    HistCell c;
    c.p = (long)i * L.sx + (long)j * L.nz + k;
    c.in = (i < L.nx && j < L.ny && k < L.nz) ? ((k + 1 < L.nz) ? 3u : 1u) : 0u;
    c.m = 0u;
    return c;
}

__device__ __forceinline__ bool hist_all_solid(const unsigned *__restrict__ bricks, const Lay &L, int bi, int bj, int bk)
{
    if (bricks == nullptr) return false;
    const int nbx = (L.nx + kBrick - 1) / kBrick, nbz = (L.nz + kBrick - 1) / kBrick;
    return (bricks[brick_word(bi * kBrick, bj * kBrick, bk * kBrick, nbz, (nbx + 31) >> 5)] & brick_bit(bi * kBrick)) != 0u;
}

__device__ __forceinline__ double hist_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

__device__ __forceinline__ unsigned wave_or(unsigned v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned wave_add(unsigned v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

struct HistLaunch {
    Lay L;
    dim3 grid;
};

inline int make_hist_launch(const char *who, int nx, int ny, int nz, long plane_stride, HistLaunch *g)
{
    if (int rc = make_lay(nx, ny, nz, plane_stride, &g->L)) return rc;
    const int nbx = (nx + kBrick - 1) / kBrick, nby = (ny + kBrick - 1) / kBrick, nbz = (nz + kBrick - 1) / kBrick;
    ADI_REQUIRE(nby <= 65535 && nbx <= 65535, "%s: box of %d x %d x %d is too large", who, nx, ny, nz);
    g->grid = dim3((unsigned)nbz, (unsigned)nby, (unsigned)nbx);
    return ADI_OK;
}

}  // namespace adi
