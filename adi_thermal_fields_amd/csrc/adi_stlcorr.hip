// adi_stlcorr.hip -- projection of a triangle mesh onto the faces of a voxel mask (voxel_bc_correction.py:53-167,
// STLBoundaryCorrector): the per-voxel Robin coefficient and area-scale fields a curved part needs, built in HBM.
//
// The reference walks triangles, their n x n sub-triangles and a dict of voxels in CPython.  Here every sub-triangle is
// a "slot":
//   k_stl_count      one thread per triangle: n*n slots, or 0 for a triangle at or below area_epsilon
//   (exclusive scan of the counts by the caller)
//   k_stl_bin        one thread per slot: (i, j, lower / upper) decoded from the slot number in the order of
//                    _subdivide_triangle, centroid, voxel -> 64-bit key (the cell's element offset; a sentinel when
//                    the centroid is outside the grid or off-mask) and the sub-triangle's area
//   (stable sort of the keys by the caller)
//   k_stl_accumulate one thread per voxel segment of the sorted keys: sums the segment's entries in slot order into up
//                    to six faces and writes area, area/dx^2 and base*area/dx^2 once per voxel face
//   k_stl_fallback   one thread per cell: exposed faces the mesh missed get the base coefficient and scale 1
// A store pass and a per-destination sum pass, not floating-point atomics: the sums are taken in the reference's order
// (triangle by triangle, sub-triangle by sub-triangle), so the fields do not depend on how the GPU schedules the waves.
//
// The binning arithmetic rounds as NumPy's does -- every product, sum and quotient on its own.  hipcc contracts a*b + c
// to an FMA even under -fno-fast-math, which moves a centroid by an ulp and with it, now and then, a voxel index:
// contraction is off for this whole translation unit.
#include "adi_common.hpp"

#pragma clang fp contract(off)

namespace adi {

constexpr long kStlDropped = ADI_STLCORR_DROPPED;  // key of a slot that lands in no voxel: sorts behind every cell

// n of voxel_bc_correction.py:70-77: ceil of the largest bounding-box extent in voxels, 1 when that is <= 1 (or NaN),
// clamped to [1, max_subdiv]
__device__ inline int stl_subdiv(const double *__restrict__ v, double dx, int max_subdiv)
{
    double span_max = 0.0;
    bool nan = false;                                            // np.min / np.max hand a NaN on: span_max > 1 is False
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double a = v[c], b = v[3 + c], d = v[6 + c];
        const double s = (fmax(fmax(a, b), d) - fmin(fmin(a, b), d)) / dx;
        nan = nan || a != a || b != b || d != d || s != s;
        span_max = c == 0 ? s : fmax(span_max, s);
    }
    if (nan) return 1;
    if (!(span_max > 1.0)) return 1;
    const double n = ceil(span_max);
    return n >= (double)max_subdiv ? max_subdiv : (int)n;
}

__global__ __launch_bounds__(256) void k_stl_count(const double *__restrict__ tri, const double *__restrict__ area,
                                                   long ntri, double dx, int max_subdiv, double area_epsilon,
                                                   long *__restrict__ count)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntri) return;
    long c = 0;
    if (!(area[t] <= area_epsilon)) {
        const long n = stl_subdiv(tri + 9 * t, dx, max_subdiv);
        c = n * n;
    }
    count[t] = c;
}

// bary(i, j) of _subdivide_triangle, one component: c*v0 + a*v1 + b*v2 with a = i/n, b = j/n, c = 1 - a - b
__device__ inline double stl_bary(int i, int j, double fn, double v0, double v1, double v2)
{
    const double a = (double)i / fn, b = (double)j / fn;
    const double c = (1.0 - a) - b;
    return (c * v0 + a * v1) + b * v2;
}

__global__ __launch_bounds__(256) void k_stl_bin(const double *__restrict__ tri, const double *__restrict__ area,
                                                 const long *__restrict__ offset, long ntri, long nslot,
                                                 const uint8_t *__restrict__ mask, int nx, int ny, int nz, long sx, long sy,
                                                 double ox, double oy, double oz, double dx, int max_subdiv,
                                                 long *__restrict__ key, double *__restrict__ sub_area,
                                                 long *__restrict__ slot_tri)
{
    const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslot) return;
    // the triangle of this slot: the last t with offset[t] <= s (offset has ntri + 1 entries, offset[ntri] == nslot;
    // triangles without slots repeat their successor's offset and are stepped over)
    long lo = 0, hi = ntri;
    while (hi - lo > 1) {
        const long mid = lo + ((hi - lo) >> 1);
        if (offset[mid] <= s) lo = mid; else hi = mid;
    }
    const long t = lo;
    const double *v = tri + 9 * t;
    const int n = stl_subdiv(v, dx, max_subdiv);
    const long local = s - offset[t];
    double c[3];
    double a_sub;
    if (n == 1) {
        a_sub = area[t];
#pragma unroll
        for (int d = 0; d < 3; ++d) c[d] = ((v[d] + v[3 + d]) + v[6 + d]) / 3.0;
    } else {
        // row i holds the 2(n - i) - 1 sub-triangles (lower j = 0, upper j = 0, lower j = 1, ...), so i(2n - i) slots
        // precede it: i = n - ceil(sqrt(n*n - local))
        const long r = (long)n * n - local;
        long m = (long)sqrt((double)r);
        while (m * m < r) ++m;
        while ((m - 1) * (m - 1) >= r) --m;
        const int i = n - (int)m;
        const long rem = local - (long)i * (2 * n - i);
        const int j = (int)(rem >> 1);
        const bool upper = (rem & 1) != 0;
        const double fn = (double)n;
        a_sub = area[t] / (double)((long)n * n);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double v0 = v[d], v1 = v[3 + d], v2 = v[6 + d];
            const double p1 = stl_bary(i + 1, j, fn, v0, v1, v2), p2 = stl_bary(i, j + 1, fn, v0, v1, v2);
            // lower (p0, p1, p2), upper (p1, p3, p2): the mean adds them in that order
            const double q = upper ? stl_bary(i + 1, j + 1, fn, v0, v1, v2) : stl_bary(i, j, fn, v0, v1, v2);
            c[d] = (upper ? (p1 + q) + p2 : (q + p1) + p2) / 3.0;
        }
    }
    const double fi = floor((c[0] - ox) / dx), fj = floor((c[1] - oy) / dx), fk = floor((c[2] - oz) / dx);
    long k = kStlDropped;
    if (fi >= 0.0 && fi < (double)nx && fj >= 0.0 && fj < (double)ny && fk >= 0.0 && fk < (double)nz) {
        const long cell = (long)fi * sx + (long)fj * sy + (long)fk;
        if (mask[cell] != 0) k = cell;
    }
    key[s] = k;
    sub_area[s] = a_sub;
    slot_tri[s] = t;
}

struct StlFaces {
    double *area[6], *robin[6], *scale[6];
    double base[6];
};

__global__ __launch_bounds__(256) void k_stl_accumulate(const long *__restrict__ key, const long *__restrict__ order,
                                                        const double *__restrict__ sub_area,
                                                        const long *__restrict__ slot_tri,
                                                        const double *__restrict__ normal, long nslot, double face_area,
                                                        StlFaces f)
{
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nslot) return;
    const long cell = key[p];
    if (cell == kStlDropped || (p > 0 && key[p - 1] == cell)) return;      // the head of a segment does its voxel
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    unsigned seen = 0;
    // a stable sort keeps equal keys in slot order: the order the reference adds them in
    for (long q = p; q < nslot && key[q] == cell; ++q) {
        const long s = order[q];
        const double a = sub_area[s];
        const double *nrm = normal + 3 * slot_tri[s];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const double comp = nrm[ax];
            // _accumulate_face_projection: tol = 1e-12; add_projected_area returns on `area <= 0.0`, so a product that
            // is NaN (a NaN area passes `area <= area_epsilon` too) is added, as the reference adds it
            if (comp > 1e-12) {
                const double w = a * comp;
                if (!(w <= 0.0)) { acc[2 * ax + 1] += w; seen |= 1u << (2 * ax + 1); }
            } else if (comp < -1e-12) {
                const double w = a * (-comp);
                if (!(w <= 0.0)) { acc[2 * ax] += w; seen |= 1u << (2 * ax); }
            }
        }
    }
#pragma unroll
    for (int face = 0; face < 6; ++face) {
        if (!(seen & (1u << face))) continue;
        if (f.area[face]) f.area[face][cell] = acc[face];
        if (f.robin[face]) {                                               // the face is in base_h with a non-zero value
            const double scale = acc[face] / face_area;
            f.robin[face][cell] = 0.0 + f.base[face] * scale;
            f.scale[face][cell] = 0.0 + scale;
        }
    }
}

// build_corrected_fields(fallback_to_base=True), :155-165: exposed_mask(mask, face) & (robin <= 0) -> base, scale 1
__global__ __launch_bounds__(256) void k_stl_fallback(const uint8_t *__restrict__ mask, int nx, int ny, int nz, long sx,
                                                      long sy, int face, double base, double *__restrict__ robin,
                                                      double *__restrict__ scale)
{
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long plane = (long)ny * nz;
    if (q >= plane * nx) return;
    const int i = (int)(q / plane);
    const long r = q - (long)i * plane;
    const int j = (int)(r / nz), k = (int)(r - (long)j * nz);
    const long cell = (long)i * sx + (long)j * sy + k;
    if (mask[cell] == 0) return;
    const int axis = face >> 1, pos = axis == 0 ? i : (axis == 1 ? j : k), n = axis == 0 ? nx : (axis == 1 ? ny : nz);
    const long step = axis == 0 ? sx : (axis == 1 ? sy : 1);
    const bool plus = (face & 1) != 0;
    const bool edge = plus ? pos == n - 1 : pos == 0;
    if (!edge && mask[plus ? cell + step : cell - step] != 0) return;      // the neighbour is solid: not exposed
    if (robin[cell] <= 0.0) {
        robin[cell] = base;
        scale[cell] = 1.0;
    }
}

inline unsigned stl_blocks(long n) { return (unsigned)((n + 255) / 256); }
constexpr long kStlMaxThreads = 256L * 0x7fffffffL;     // one thread per item, 256 per workgroup, 2^31 - 1 workgroups

}  // namespace adi

using namespace adi;

extern "C" {

int adi_stlcorr_count(const double *d_tri, const double *d_area, long ntri, double dx, int max_subdiv,
                      double area_epsilon, long *d_count, void *stream)
{
    ADI_REQUIRE(ntri >= 0 && ntri <= kStlMaxThreads, "adi_stlcorr_count: bad triangle count %ld", ntri);
    ADI_REQUIRE(dx > 0.0, "adi_stlcorr_count: dx must be positive, got %g", dx);
    ADI_REQUIRE(max_subdiv >= 1 && max_subdiv <= ADI_STLCORR_MAX_SUBDIV, "adi_stlcorr_count: max_subdiv %d outside 1..%d",
                max_subdiv, ADI_STLCORR_MAX_SUBDIV);
    ADI_REQUIRE(area_epsilon == area_epsilon, "adi_stlcorr_count: area_epsilon is NaN");
    if (ntri == 0) return ADI_OK;
    ADI_REQUIRE(d_tri && d_area && d_count, "adi_stlcorr_count: null argument");
    hipLaunchKernelGGL(k_stl_count, dim3(stl_blocks(ntri)), dim3(256), 0, as_stream(stream), d_tri, d_area, ntri, dx,
                       max_subdiv, area_epsilon, d_count);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_stlcorr_bin(const double *d_tri, const double *d_area, const long *d_offset, long ntri, long nslot,
                    const uint8_t *d_mask, int nx, int ny, int nz, long stride_x, long stride_y, const double *h_origin,
                    double dx, int max_subdiv, long *d_key, double *d_sub_area, long *d_slot_tri, void *stream)
{
    ADI_REQUIRE(ntri >= 0 && ntri <= kStlMaxThreads, "adi_stlcorr_bin: bad triangle count %ld", ntri);
    ADI_REQUIRE(nslot >= 0 && nslot <= kStlMaxThreads, "adi_stlcorr_bin: bad slot count %ld", nslot);
    ADI_REQUIRE(nslot == 0 || ntri > 0, "adi_stlcorr_bin: %ld slots without a triangle", nslot);
    ADI_REQUIRE(dx > 0.0, "adi_stlcorr_bin: dx must be positive, got %g", dx);
    ADI_REQUIRE(max_subdiv >= 1 && max_subdiv <= ADI_STLCORR_MAX_SUBDIV, "adi_stlcorr_bin: max_subdiv %d outside 1..%d",
                max_subdiv, ADI_STLCORR_MAX_SUBDIV);
    ADI_REQUIRE(nx > 0 && ny > 0 && nz > 0, "adi_stlcorr_bin: bad grid %d x %d x %d", nx, ny, nz);
    ADI_REQUIRE(stride_y >= nz && stride_x >= (long)ny * stride_y, "adi_stlcorr_bin: strides (%ld, %ld) overlap for %d x %d x %d",
                stride_x, stride_y, nx, ny, nz);
    ADI_REQUIRE(h_origin, "adi_stlcorr_bin: null origin");
    if (nslot == 0) return ADI_OK;
    ADI_REQUIRE(d_tri && d_area && d_offset && d_mask && d_key && d_sub_area && d_slot_tri, "adi_stlcorr_bin: null argument");
    hipLaunchKernelGGL(k_stl_bin, dim3(stl_blocks(nslot)), dim3(256), 0, as_stream(stream), d_tri, d_area, d_offset, ntri,
                       nslot, d_mask, nx, ny, nz, stride_x, stride_y, h_origin[0], h_origin[1], h_origin[2], dx, max_subdiv,
                       d_key, d_sub_area, d_slot_tri);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_stlcorr_accumulate(const long *d_key_sorted, const long *d_order, const double *d_sub_area, const long *d_slot_tri,
                           const double *d_normal, long nslot, double dx, const double *h_base, double *const *h_area,
                           double *const *h_robin, double *const *h_scale, void *stream)
{
    ADI_REQUIRE(nslot >= 0 && nslot <= kStlMaxThreads, "adi_stlcorr_accumulate: bad slot count %ld", nslot);
    ADI_REQUIRE(dx > 0.0, "adi_stlcorr_accumulate: dx must be positive, got %g", dx);
    ADI_REQUIRE(h_base && h_area && h_robin && h_scale, "adi_stlcorr_accumulate: null face table");
    StlFaces f;
    for (int face = 0; face < 6; ++face) {
        ADI_REQUIRE((h_robin[face] == nullptr) == (h_scale[face] == nullptr),
                    "adi_stlcorr_accumulate: face %d has one of robin / scale without the other", face);
        f.area[face] = h_area[face];
        f.robin[face] = h_robin[face];
        f.scale[face] = h_scale[face];
        f.base[face] = h_base[face];
    }
    if (nslot == 0) return ADI_OK;
    ADI_REQUIRE(d_key_sorted && d_order && d_sub_area && d_slot_tri && d_normal, "adi_stlcorr_accumulate: null argument");
    hipLaunchKernelGGL(k_stl_accumulate, dim3(stl_blocks(nslot)), dim3(256), 0, as_stream(stream), d_key_sorted, d_order,
                       d_sub_area, d_slot_tri, d_normal, nslot, dx * dx, f);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_stlcorr_fallback(const uint8_t *d_mask, int nx, int ny, int nz, long stride_x, long stride_y, int face, double base,
                         double *d_robin, double *d_scale, void *stream)
{
    ADI_REQUIRE(face >= 0 && face < 6, "bad face");
    ADI_REQUIRE(nx > 0 && ny > 0 && nz > 0, "adi_stlcorr_fallback: bad grid %d x %d x %d", nx, ny, nz);
    ADI_REQUIRE(stride_y >= nz && stride_x >= (long)ny * stride_y,
                "adi_stlcorr_fallback: strides (%ld, %ld) overlap for %d x %d x %d", stride_x, stride_y, nx, ny, nz);
    ADI_REQUIRE(d_mask && d_robin && d_scale, "adi_stlcorr_fallback: null argument");
    const long n = (long)nx * ny * nz;
    ADI_REQUIRE(n <= kStlMaxThreads, "adi_stlcorr_fallback: %ld cells", n);
    hipLaunchKernelGGL(k_stl_fallback, dim3(stl_blocks(n)), dim3(256), 0, as_stream(stream), d_mask, nx, ny, nz, stride_x,
                       stride_y, face, base, d_robin, d_scale);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // extern "C"
