// adi_brick_dev.hpp -- the brick-shaped cell pass that adi_phase.hip and adi_matlaw.hip share: one workgroup of 256 threads per
// 16 x 16 x 16 brick of the flags summary.  A row piece of the brick is 16 doubles = 128 bytes: lane l of a wave owns cells
// 2(l & 7), 2(l & 7) + 1 of row (l >> 3), so one 16-byte load instruction of a wave covers eight whole 128-byte row pieces, and
// the eight loads of a thread cover the 256 rows of the brick.
#pragma once
#include "adi_cart_host.hpp"

namespace adi {

constexpr int kPhaseIter = 8;     // row groups of a brick per thread: 256 rows / (256 threads / 8 lanes per row)

struct PhaseCell {
    long p;          // offset of the pair's first cell
    unsigned in;     // bit c: cell c of the pair lies inside the box
    unsigned m;      // bit c: ... and in the mask
};

// 16-byte access needs even row and plane strides and 16-byte aligned arrays (host: `vec`); then a pair never straddles the
// end of a row (pair_vec, adi_cart_host.hpp).  Otherwise cell by cell.
template <bool VEC>
__device__ __forceinline__ void load_pair(const double *__restrict__ a, const PhaseCell &c, double &v0, double &v1)
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
__device__ __forceinline__ unsigned load_mask_pair(const uint8_t *__restrict__ flags, const PhaseCell &c)
{
    if (VEC) {
        const unsigned v = *reinterpret_cast<const unsigned short *>(flags + c.p);
        return (v & 1u) | ((v >> 7) & 2u);
    }
    unsigned m = flags[c.p] & 1u;
    if (c.in & 2u) m |= (flags[c.p + 1] & 1u) << 1;
    return m;
}

// the pair of cells thread `tid` owns in row group `it` of brick (bi, bj, bk)
__device__ __forceinline__ PhaseCell phase_cell(const Lay &L, int bi, int bj, int bk, int it, unsigned tid)
{
    const int row = it * 32 + (int)(tid >> 3);
    const int i = bi * kBrick + (row >> 4), j = bj * kBrick + (row & 15), k = bk * kBrick + 2 * (int)(tid & 7u);
    PhaseCell c;
    c.p = (long)i * L.sx + (long)j * L.nz + k;
    c.in = (i < L.nx && j < L.ny && k < L.nz) ? ((k + 1 < L.nz) ? 3u : 1u) : 0u;
    c.m = 0u;
    return c;
}

__device__ __forceinline__ bool brick_all_solid(const unsigned *__restrict__ bricks, const Lay &L, int bi, int bj, int bk)
{
    if (bricks == nullptr) return false;
    const int nbx = (L.nx + kBrick - 1) / kBrick, nbz = (L.nz + kBrick - 1) / kBrick;
    return (bricks[brick_word(bi * kBrick, bj * kBrick, bk * kBrick, nbz, (nbx + 31) >> 5)] & brick_bit(bi * kBrick)) != 0u;
}

struct PhaseLaunch {
    Lay L;
    dim3 grid;
    int nby, nbz;
};

inline int make_phase_launch(const char *who, int nx, int ny, int nz, long plane_stride, PhaseLaunch *g)
{
    if (int rc = make_lay(nx, ny, nz, plane_stride, &g->L)) return rc;
    const int nbx = (nx + kBrick - 1) / kBrick;
    g->nby = (ny + kBrick - 1) / kBrick;
    g->nbz = (nz + kBrick - 1) / kBrick;
    ADI_REQUIRE(g->nby <= 65535 && nbx <= 65535, "%s: box of %d x %d x %d is too large", who, nx, ny, nz);
    g->grid = dim3((unsigned)g->nbz, (unsigned)g->nby, (unsigned)nbx);
    return ADI_OK;
}

}  // namespace adi
