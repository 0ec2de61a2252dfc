// adi_voxelize.hip -- solid voxelisation of a closed triangle mesh: voxel (i, j, k) is solid exactly when its centre is
// inside the surface.  A ray along `axis` through every column of voxel centres; each crossing
// toggles the voxels behind it; solid = odd number of toggles.
//
// The toggle grid holds one bit per voxel along the ray plus one "behind the last voxel" bit per column, 32 to a word,
// WORD-MAJOR: word w of column c at w * ncol + c, the columns numbered in the C order of the two axes that are left.  A
// locally flat piece of surface then toggles the same word of neighbouring columns: neighbouring lanes hit neighbouring
// dwords, whatever the ray axis.
//   k_vox_count    one thread per triangle: the 4 x 4 column tiles of its bounding box clipped to the grid; 0 for a
//                  triangle with zero projected area or wholly outside
//   (exclusive scan of the counts by the caller)
//   k_vox_toggle   16 lanes per tile, one lane per column: cover test, depth, first voxel behind it, one atomicXor of one
//                  bit.  XOR commutes: the grid does not depend on the order of arrival, two runs give the same bits.
//   k_vox_prefix   one thread per column: prefix XOR inside each word (shift-XOR ladder), parity carried from word to
//                  word, in place -- bit p of word w becomes "voxel 32 w + p is solid"; the bit behind the last voxel is
//                  the column's leak.  One ballot per wave, one atomic add per workgroup for the leak count.
//   k_vox_expand_*  bits -> the dense uint8 (nx, ny, nz) mask, 16-byte stores: along the ray for axis 2, plane by plane
//                  (16 neighbouring columns x 32 planes per thread) for axes 0 and 1
//   k_vox_majority cell-wise majority of three masks
//
// The cover test and the depth round as the CPU statement of the definition does (tests/voxelize_ref.py, NumPy): every
// product, difference and quotient on its own.  hipcc contracts a*b - c*d to an FMA even under -fno-fast-math, which
// can flip the sign of an edge function that should be zero: contraction is off for this whole translation unit.
#include "adi_common.hpp"

#pragma clang fp contract(off)

namespace adi {

constexpr int kVoxTile = 4;                      // tile side in columns; 16 lanes per tile
constexpr long kVoxMaxThreads = 256L * 0x7fffffffL;

struct VoxGrid {
    double od, ou, ow, dx;      // origin along the ray axis a, along b = (a + 1) % 3, along c = (a + 2) % 3
    int nd, nu, nw;             // extents along a, b, c
    long su, sw;                // column number = iu * su + iw * sw
    long ncol;
    int fast_is_u;              // the axis whose columns are neighbours in memory (sw == 1 or su == 1)
};

// centre of voxel i: origin + (i + 0.5) * dx, in this form everywhere
__device__ inline double vox_centre(double o, int i, double dx) { return o + ((double)i + 0.5) * dx; }

// columns whose centre may lie in [lo, hi]: one column of margin on either side of the estimate, clipped to 0..n-1.
// An empty range (lo > hi in the result) for a triangle outside the grid or with a NaN in it.
__device__ inline void vox_range(double lo, double hi, double o, double dx, int n, int *first, int *last)
{
    const double a = floor((lo - o) / dx - 0.5) - 1.0, b = ceil((hi - o) / dx - 0.5) + 1.0;
    if (!(a <= b) || !(b >= 0.0) || !(a <= (double)(n - 1))) {
        *first = 0;
        *last = -1;
        return;
    }
    *first = a > 0.0 ? (int)a : 0;
    *last = b < (double)(n - 1) ? (int)b : n - 1;
}

struct VoxTri {
    double d0, d1, d2, u0, u1, u2, w0, w1, w2;
    int fu, lu, fw, lw;          // first / last column on either axis
    long tiles_f, tiles;         // tiles along the fast axis, tiles in all
};

__device__ inline VoxTri vox_load(const double *__restrict__ v, int axis, const VoxGrid &g)
{
    const int b = axis == 2 ? 0 : axis + 1, c = axis == 0 ? 2 : axis - 1;
    VoxTri t;
    t.d0 = v[axis]; t.d1 = v[3 + axis]; t.d2 = v[6 + axis];
    t.u0 = v[b]; t.u1 = v[3 + b]; t.u2 = v[6 + b];
    t.w0 = v[c]; t.w1 = v[3 + c]; t.w2 = v[6 + c];
    const double area = (t.u1 - t.u0) * (t.w2 - t.w0) - (t.w1 - t.w0) * (t.u2 - t.u0);
    t.tiles_f = t.tiles = 0;
    t.fu = t.fw = 0;
    t.lu = t.lw = -1;
    if (area == 0.0 || area != area) return t;           // zero projected area covers nothing
    vox_range(fmin(fmin(t.u0, t.u1), t.u2), fmax(fmax(t.u0, t.u1), t.u2), g.ou, g.dx, g.nu, &t.fu, &t.lu);
    vox_range(fmin(fmin(t.w0, t.w1), t.w2), fmax(fmax(t.w0, t.w1), t.w2), g.ow, g.dx, g.nw, &t.fw, &t.lw);
    if (t.lu < t.fu || t.lw < t.fw) return t;
    const long tu = (t.lu - t.fu) / kVoxTile + 1, tw = (t.lw - t.fw) / kVoxTile + 1;
    t.tiles_f = g.fast_is_u ? tu : tw;
    t.tiles = tu * tw;
    return t;
}

__global__ __launch_bounds__(256) void k_vox_count(const double *__restrict__ tri, long ntri, int axis, VoxGrid g,
                                                   long *__restrict__ count)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntri) return;
    count[t] = vox_load(tri + 9 * t, axis, g).tiles;
}

// sign of the edge function of (a -> b) at p, the endpoints taken in lexicographic (u, w) order and the sign flipped
// back, so two triangles that share an edge see the same rounded number.  A zero takes the sign the point would have if
// nudged by (+eps, +eps^2).  0 for a NaN or an edge without length: the triangle then covers nothing.
__device__ inline int vox_side(double au, double aw, double bu, double bw, double pu, double pw)
{
    const bool swap = au > bu || (au == bu && aw > bw);
    if (swap) {
        double t = au; au = bu; bu = t;
        t = aw; aw = bw; bw = t;
    }
    const double du = bu - au, dw = bw - aw;
    const double e = du * (pw - aw) - dw * (pu - au);
    if (e != e) return 0;
    int s = (e > 0.0) - (e < 0.0);
    if (s == 0) s = dw != 0.0 ? (dw < 0.0) - (dw > 0.0) : (du > 0.0) - (du < 0.0);
    return swap ? -s : s;
}

__global__ __launch_bounds__(256) void k_vox_toggle(const double *__restrict__ tri, const long *__restrict__ offset,
                                                    long ntri, long nitem, int axis, VoxGrid g,
                                                    unsigned *__restrict__ words)
{
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long item = gid >> 4;
    const int lane = (int)(gid & 15);
    if (item >= nitem) return;
    // the triangle of this tile: the last t with offset[t] <= item (offset has ntri + 1 entries; triangles without tiles
    // repeat their successor's offset and are stepped over)
    long lo = 0, hi = ntri;
    while (hi - lo > 1) {
        const long mid = lo + ((hi - lo) >> 1);
        if (offset[mid] <= item) lo = mid; else hi = mid;
    }
    const VoxTri t = vox_load(tri + 9 * lo, axis, g);
    const long local = item - offset[lo];
    if (t.tiles_f <= 0 || local >= t.tiles) return;      // cannot happen with the caller's scan; never index past a box
    const int tf = (int)(local % t.tiles_f), ts = (int)(local / t.tiles_f);
    const int lf = lane & (kVoxTile - 1), ls = lane >> 2;
    const int iu = t.fu + kVoxTile * (g.fast_is_u ? tf : ts) + (g.fast_is_u ? lf : ls);
    const int iw = t.fw + kVoxTile * (g.fast_is_u ? ts : tf) + (g.fast_is_u ? ls : lf);
    if (iu > t.lu || iw > t.lw) return;
    const double pu = vox_centre(g.ou, iu, g.dx), pw = vox_centre(g.ow, iw, g.dx);
    const int s0 = vox_side(t.u0, t.w0, t.u1, t.w1, pu, pw);
    const int s1 = vox_side(t.u1, t.w1, t.u2, t.w2, pu, pw);
    const int s2 = vox_side(t.u2, t.w2, t.u0, t.w0, pu, pw);
    if (!((s0 > 0 && s1 > 0 && s2 > 0) || (s0 < 0 && s1 < 0 && s2 < 0))) return;
    const double area = (t.u1 - t.u0) * (t.w2 - t.w0) - (t.w1 - t.w0) * (t.u2 - t.u0);
    const double l1 = ((pu - t.u0) * (t.w2 - t.w0) - (pw - t.w0) * (t.u2 - t.u0)) / area;
    const double l2 = ((t.u1 - t.u0) * (pw - t.w0) - (t.w1 - t.w0) * (pu - t.u0)) / area;
    const double depth = t.d0 + (l1 * (t.d1 - t.d0) + l2 * (t.d2 - t.d0));
    // the first voxel whose centre is >= depth (nd: none, the bit behind the last voxel).  The division only estimates
    // it; comparisons against the centre formula decide, so a rounding in the quotient moves no voxel.
    const double est = ceil((depth - g.od) / g.dx - 0.5);
    int i = est >= 0.0 ? (est < (double)g.nd ? (int)est : g.nd) : (est < 0.0 ? 0 : g.nd);
    while (i > 0 && vox_centre(g.od, i - 1, g.dx) >= depth) --i;
    while (i < g.nd && !(vox_centre(g.od, i, g.dx) >= depth)) ++i;
    const long col = (long)iu * g.su + (long)iw * g.sw;
    atomicXor(words + (long)(i >> 5) * g.ncol + col, 1u << (i & 31));
}

__global__ __launch_bounds__(256) void k_vox_prefix(unsigned *__restrict__ words, long ncol, int nd,
                                                    int *__restrict__ leaks)
{
    __shared__ int wave_leaks[4];
    const long col = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool leak = false;
    if (col < ncol) {
        const int nword = nd / 32 + 1;
        unsigned carry = 0;
        for (int w = 0; w < nword; ++w) {
            unsigned x = words[(long)w * ncol + col];
            x ^= x << 1;
            x ^= x << 2;
            x ^= x << 4;
            x ^= x << 8;
            x ^= x << 16;
            x ^= carry;
            carry = 0u - (x >> 31);
            words[(long)w * ncol + col] = x;
            if (w == nword - 1) leak = ((x >> (nd & 31)) & 1u) != 0;
        }
    }
    const int n = __popcll(__ballot(leak));
    if ((threadIdx.x & 63) == 0) wave_leaks[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = wave_leaks[0] + wave_leaks[1] + wave_leaks[2] + wave_leaks[3];
        if (total) atomicAdd(leaks, total);
    }
}

// bits 0..7 of b -> eight bytes of 0 / 1, bit p in byte p
__device__ inline unsigned long long vox_spread8(unsigned b)
{
    const unsigned long long t = ((unsigned long long)(b & 0xffu) * 0x0101010101010101ULL) & 0x8040201008040201ULL;
    return ((t + 0x7f7f7f7f7f7f7f7fULL) >> 7) & 0x0101010101010101ULL;
}

// ray axis 2: the mask is (ncol, nd) bytes, the ray along the contiguous axis.  One thread per 16 bytes of the flat
// mask, wherever the rows begin: a row length that is no multiple of 16 only means a thread may read two or three words.
__global__ __launch_bounds__(256) void k_vox_expand_ray2(const unsigned *__restrict__ words, long ncol, int nd,
                                                         uint8_t *__restrict__ mask)
{
    const long q0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    const long n = ncol * nd;
    if (q0 >= n) return;
    long col = q0 / nd;
    int k = (int)(q0 - col * nd);
    const int todo = n - q0 < 16 ? (int)(n - q0) : 16;
    if (todo == 16 && k + 16 <= nd && (k & 7) == 0) {           // the whole piece in one column, byte-aligned in its words
        const unsigned x0 = words[(long)(k >> 5) * ncol + col] >> (k & 31);
        const unsigned x1 = words[(long)((k + 8) >> 5) * ncol + col] >> ((k + 8) & 31);
        const unsigned long long a = vox_spread8(x0), b = vox_spread8(x1);
        *reinterpret_cast<uint4 *>(mask + q0) = make_uint4((unsigned)a, (unsigned)(a >> 32), (unsigned)b, (unsigned)(b >> 32));
        return;
    }
    unsigned out[4] = {0u, 0u, 0u, 0u};
    unsigned x = words[(long)(k >> 5) * ncol + col];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        if (t < todo) {
            out[t >> 2] |= ((x >> (k & 31)) & 1u) << (8 * (t & 3));
            if (++k == nd) {
                k = 0;
                ++col;
            }
            if ((k & 31) == 0 && t + 1 < todo) x = words[(long)(k >> 5) * ncol + col];
        }
    }
    if (todo == 16) {
        *reinterpret_cast<uint4 *>(mask + q0) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
        for (int t = 0; t < 16; ++t)
            if (t < todo) mask[q0 + t] = (uint8_t)((out[t >> 2] >> (8 * (t & 3))) & 1u);
    }
}

// ray axes 0 and 1: the mask is (nouter, nd, ninner) bytes and column (o, inner) is number o * ninner + inner.  One thread
// per (word w, o, group of 16 neighbouring columns): 16 words in, up to 32 planes of 16 bytes out.  WIDE: ninner is a
// multiple of 16, so every piece is whole and 16-byte aligned; otherwise byte stores.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_vox_expand_planes(const unsigned *__restrict__ words, long nouter, int nd,
                                                           long ninner, uint8_t *__restrict__ mask)
{
    const long ngroup = (ninner + 15) / 16;
    const int nword = (nd + 31) / 32;                     // the word that holds only the leak bit has no voxel
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= ngroup * nouter * nword) return;
    const long grp = tid % ngroup, rest = tid / ngroup;
    const long o = rest % nouter;
    const int w = (int)(rest / nouter);
    const long inner0 = grp * 16, ncol = nouter * ninner;
    const unsigned *src = words + (long)w * ncol + o * ninner + inner0;
    unsigned x[16];
    if (WIDE) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const uint4 q = reinterpret_cast<const uint4 *>(src)[v];
            x[4 * v] = q.x; x[4 * v + 1] = q.y; x[4 * v + 2] = q.z; x[4 * v + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int t = 0; t < 16; ++t) x[t] = inner0 + t < ninner ? src[t] : 0u;
    }
    const int planes = nd - 32 * w < 32 ? nd - 32 * w : 32;
    uint8_t *dst = mask + (o * nd + 32L * w) * ninner + inner0;
    for (int p = 0; p < planes; ++p, dst += ninner) {
        unsigned out[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            out[t >> 2] |= (x[t] & 1u) << (8 * (t & 3));
            x[t] >>= 1;
        }
        if (WIDE) {
            *reinterpret_cast<uint4 *>(dst) = make_uint4(out[0], out[1], out[2], out[3]);
        } else {
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (inner0 + t < ninner) dst[t] = (uint8_t)((out[t >> 2] >> (8 * (t & 3))) & 1u);
        }
    }
}

template <bool WIDE>
__global__ __launch_bounds__(256) void k_vox_majority(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                                      const uint8_t *__restrict__ c, size_t n, uint8_t *__restrict__ out)
{
    const size_t q = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (q >= n) return;
    if (WIDE && q + 16 <= n) {
        const uint4 x = *reinterpret_cast<const uint4 *>(a + q), y = *reinterpret_cast<const uint4 *>(b + q),
                    z = *reinterpret_cast<const uint4 *>(c + q);
        // masks hold 0 / 1: the majority of three bits, byte by byte
        *reinterpret_cast<uint4 *>(out + q) = make_uint4((x.x & y.x) | (x.x & z.x) | (y.x & z.x), (x.y & y.y) | (x.y & z.y) | (y.y & z.y),
                                                         (x.z & y.z) | (x.z & z.z) | (y.z & z.z), (x.w & y.w) | (x.w & z.w) | (y.w & z.w));
        return;
    }
    for (size_t t = q; t < n && t < q + 16; ++t) out[t] = (uint8_t)(((a[t] != 0) + (b[t] != 0) + (c[t] != 0)) >= 2);
}

inline unsigned vox_blocks(long n) { return (unsigned)((n + 255) / 256); }

// validates the grid arguments and fills g; nullptr origin allowed where no coordinates are needed
inline int vox_grid(const char *who, const double *h_origin, double dx, int nx, int ny, int nz, int axis, bool coords,
                    VoxGrid *g)
{
    ADI_REQUIRE(axis >= 0 && axis <= 2, "%s: ray axis %d outside 0..2", who, axis);
    ADI_REQUIRE(nx > 0 && ny > 0 && nz > 0, "%s: bad grid %d x %d x %d", who, nx, ny, nz);
    if (coords) {
        ADI_REQUIRE(dx > 0.0, "%s: dx must be positive, got %g", who, dx);
        ADI_REQUIRE(h_origin, "%s: null origin", who);
    }
    const int n[3] = {nx, ny, nz};
    const int b = (axis + 1) % 3, c = (axis + 2) % 3;
    g->nd = n[axis];
    g->nu = n[b];
    g->nw = n[c];
    g->dx = dx;
    g->od = coords ? h_origin[axis] : 0.0;
    g->ou = coords ? h_origin[b] : 0.0;
    g->ow = coords ? h_origin[c] : 0.0;
    g->ncol = (long)g->nu * g->nw;
    // columns in the C order of the two remaining axes: (j, k), (i, k), (i, j)
    g->fast_is_u = axis == 1;
    g->su = axis == 1 ? 1 : g->nw;
    g->sw = axis == 1 ? g->nu : 1;
    return ADI_OK;
}

}  // namespace adi

using namespace adi;

extern "C" {

int adi_voxelize_words(int nx, int ny, int nz, int axis, long *words)
{
    VoxGrid g;
    if (int rc = vox_grid("adi_voxelize_words", nullptr, 0.0, nx, ny, nz, axis, false, &g)) return rc;
    ADI_REQUIRE(words, "adi_voxelize_words: null argument");
    *words = (long)(g.nd / 32 + 1) * g.ncol;
    return ADI_OK;
}

int adi_voxelize_count(const double *d_tri, long ntri, const double *h_origin, double dx, int nx, int ny, int nz, int axis,
                       long *d_count, void *stream)
{
    VoxGrid g;
    if (int rc = vox_grid("adi_voxelize_count", h_origin, dx, nx, ny, nz, axis, true, &g)) return rc;
    ADI_REQUIRE(ntri >= 0 && ntri <= kVoxMaxThreads, "adi_voxelize_count: bad triangle count %ld", ntri);
    if (ntri == 0) return ADI_OK;
    ADI_REQUIRE(d_tri && d_count, "adi_voxelize_count: null argument");
    hipLaunchKernelGGL(k_vox_count, dim3(vox_blocks(ntri)), dim3(256), 0, as_stream(stream), d_tri, ntri, axis, g, d_count);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_voxelize_toggle(const double *d_tri, const long *d_offset, long ntri, long nitem, const double *h_origin, double dx,
                        int nx, int ny, int nz, int axis, uint32_t *d_words, void *stream)
{
    VoxGrid g;
    if (int rc = vox_grid("adi_voxelize_toggle", h_origin, dx, nx, ny, nz, axis, true, &g)) return rc;
    ADI_REQUIRE(ntri >= 0 && ntri <= kVoxMaxThreads, "adi_voxelize_toggle: bad triangle count %ld", ntri);
    ADI_REQUIRE(nitem >= 0 && nitem <= kVoxMaxThreads / 16, "adi_voxelize_toggle: bad tile count %ld", nitem);
    ADI_REQUIRE(nitem == 0 || ntri > 0, "adi_voxelize_toggle: %ld tiles without a triangle", nitem);
    if (nitem == 0) return ADI_OK;
    ADI_REQUIRE(d_tri && d_offset && d_words, "adi_voxelize_toggle: null argument");
    hipLaunchKernelGGL(k_vox_toggle, dim3(vox_blocks(nitem * 16)), dim3(256), 0, as_stream(stream), d_tri, d_offset, ntri,
                       nitem, axis, g, d_words);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_voxelize_scan(uint32_t *d_words, int nx, int ny, int nz, int axis, uint8_t *d_mask, int *d_leaks, void *stream)
{
    VoxGrid g;
    if (int rc = vox_grid("adi_voxelize_scan", nullptr, 0.0, nx, ny, nz, axis, false, &g)) return rc;
    ADI_REQUIRE(d_words && d_mask && d_leaks, "adi_voxelize_scan: null argument");
    ADI_REQUIRE(((uintptr_t)d_words & 15) == 0 && ((uintptr_t)d_mask & 15) == 0,
                "adi_voxelize_scan: the toggle grid and the mask must be 16-byte aligned");
    hipLaunchKernelGGL(k_vox_prefix, dim3(vox_blocks(g.ncol)), dim3(256), 0, as_stream(stream), d_words, g.ncol, g.nd, d_leaks);
    ADI_CHECK_LAUNCH();
    if (axis == 2) {
        const long pieces = (g.ncol * g.nd + 15) / 16;
        hipLaunchKernelGGL(k_vox_expand_ray2, dim3(vox_blocks(pieces)), dim3(256), 0, as_stream(stream), d_words, g.ncol, g.nd,
                           d_mask);
    } else {
        const long nouter = axis == 0 ? 1 : nx, ninner = axis == 0 ? (long)ny * nz : nz;
        const long threads = ((ninner + 15) / 16) * nouter * ((g.nd + 31) / 32);
        if (ninner % 16 == 0)
            hipLaunchKernelGGL(k_vox_expand_planes<true>, dim3(vox_blocks(threads)), dim3(256), 0, as_stream(stream), d_words,
                               nouter, g.nd, ninner, d_mask);
        else
            hipLaunchKernelGGL(k_vox_expand_planes<false>, dim3(vox_blocks(threads)), dim3(256), 0, as_stream(stream), d_words,
                               nouter, g.nd, ninner, d_mask);
    }
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_voxelize_majority(const uint8_t *d_m0, const uint8_t *d_m1, const uint8_t *d_m2, size_t n, uint8_t *d_out, void *stream)
{
    ADI_REQUIRE((long)n >= 0 && (long)n <= kVoxMaxThreads, "adi_voxelize_majority: bad cell count %zu", n);
    if (n == 0) return ADI_OK;
    ADI_REQUIRE(d_m0 && d_m1 && d_m2 && d_out, "adi_voxelize_majority: null argument");
    const bool wide = (((uintptr_t)d_m0 | (uintptr_t)d_m1 | (uintptr_t)d_m2 | (uintptr_t)d_out) & 15) == 0;
    const long pieces = (long)((n + 15) / 16);
    if (wide)
        hipLaunchKernelGGL(k_vox_majority<true>, dim3(vox_blocks(pieces)), dim3(256), 0, as_stream(stream), d_m0, d_m1, d_m2, n,
                           d_out);
    else
        hipLaunchKernelGGL(k_vox_majority<false>, dim3(vox_blocks(pieces)), dim3(256), 0, as_stream(stream), d_m0, d_m1, d_m2, n,
                           d_out);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // extern "C"
