// adi_fields.hip -- K0 and the byte kernels: the fields a step reads, built from the mask (hand-written HIP for gfx950):
//   k_build_flags     the neighbour-flags digest of the mask every step kernel reads
//   k_build_flag_bricks  its summary: one bit per 16^3 brick whose flags bytes are all the ones their positions imply
//   k_build_coeffs    Robin coefficient + Neumann flux fields of the three axes in one pass
//                     (precompute_coeff_packs_unified, adi3d_numba_coeff.py:57-118); adi_face_constants: its per-face scalars
//   k_exposed         exposed_mask (adi3d_numba_coeff.py:38-55);  k_count_exposed: exposed lateral faces per plane
//   k_birth, k_masked_fill, k_mask_or   mask and state updates of a layer birth
#include "adi_cart_host.hpp"
#include "adi_cell_dev.hpp"

namespace adi {

// neighbour flags: bit0 = cell in mask, bit(1 + 2*axis) / bit(2 + 2*axis) = the minus / plus neighbour along
// `axis` exists and is in the mask.  Derived from the mask whenever it changes (the mask "folds into the
// coefficient build on device"); halo planes of a slab decomposition are simply part of the mask array.
__global__ __launch_bounds__(256) void k_build_flags(const uint8_t *__restrict__ mask, Lay L, int k0, int k1,
                                                     uint8_t *__restrict__ flags)
{
    int i, j, k;
    long p;
    if (!cell_of_k((long)blockIdx.x * blockDim.x + threadIdx.x, L, k0, k1, i, j, k, p)) return;
    const long sx = L.sx, sy = L.nz;
    unsigned f = 0;
    if (mask[p]) {
        f = 1u;
        if (i > 0 && mask[p - sx]) f |= 2u;
        if (i + 1 < L.nx && mask[p + sx]) f |= 4u;
        if (j > 0 && mask[p - sy]) f |= 8u;
        if (j + 1 < L.ny && mask[p + sy]) f |= 16u;
        if (k > 0 && mask[p - 1]) f |= 32u;
        if (k + 1 < L.nz && mask[p + 1]) f |= 64u;
    }
    flags[p] = (uint8_t)f;
}

// Flags summary (SweepScal::bricks): the bit of a 16 x 16 x 16 brick is set iff every flags byte of the brick (inside the box
// L) equals pos_flags of its cell -- decided from the flags themselves, so padding, slab halo planes and hand-built flags
// leave their bricks clear.  One workgroup per brick of the axis-2 brick range [bk0, bk1): thread (di, dj) compares the 16
// bytes of row (i, j).  Neighbouring bricks share a word: the bit is set / cleared atomically.
__global__ __launch_bounds__(256) void k_build_flag_bricks(const uint8_t *__restrict__ flags, Lay L, int bk0, int bk1,
                                                           unsigned *__restrict__ bricks)
{
    const int nbx = (L.nx + kBrick - 1) / kBrick, nbz = (L.nz + kBrick - 1) / kBrick, nbr = bk1 - bk0;
    const int bwx = (nbx + 31) >> 5;
    const unsigned b = blockIdx.x;
    const int bi = (int)(b % (unsigned)nbx), bk = bk0 + (int)((b / (unsigned)nbx) % (unsigned)nbr),
              bj = (int)(b / ((unsigned)nbx * (unsigned)nbr));
    const int i = bi * kBrick + (int)(threadIdx.x >> 4), j = bj * kBrick + (int)(threadIdx.x & 15u);
    bool ok = true;
    if (i < L.nx && j < L.ny) {
        const uint8_t *row = flags + (long)i * L.sx + (long)j * L.nz;
#pragma unroll
        for (int dk = 0; dk < kBrick; ++dk) {
            const int k = bk * kBrick + dk;
            if (k < L.nz) ok = ok && row[k] == pos_flags(i, j, k, L.nx, L.ny, L.nz);
        }
    }
    ok = __syncthreads_and(ok);
    if (threadIdx.x == 0) {
        unsigned *w = bricks + brick_word(bi * kBrick, bj * kBrick, bk * kBrick, nbz, bwx);
        const unsigned bit = brick_bit(bi * kBrick);
        if (ok) atomicOr(w, bit);
        else atomicAnd(w, ~bit);
    }
}

// ------------------------------------------------------------------------------------------------
// K0: coefficient build.  Same accumulation order as the reference ('-' face then '+' face per axis,
// (h * A) / Ccell with IEEE division), contraction off -> bit-identical packs.
// ------------------------------------------------------------------------------------------------
struct FaceSpec {
    int mode[6];
    double scalar[6];
    const double *field[6];
};

__global__ __launch_bounds__(256) void k_build_coeffs(const uint8_t *__restrict__ mask, Lay L, int k0, int k1, double A,
                                                      double Ccell, FaceSpec h, FaceSpec q, double *__restrict__ c0,
                                                      double *__restrict__ c1, double *__restrict__ c2,
                                                      double *__restrict__ q0, double *__restrict__ q1,
                                                      double *__restrict__ q2)
{
#pragma clang fp contract(off)
    int i, j, k;
    long p;
    if (!cell_of_k((long)blockIdx.x * blockDim.x + threadIdx.x, L, k0, k1, i, j, k, p)) return;
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

__global__ __launch_bounds__(256) void k_exposed(const uint8_t *__restrict__ mask, Lay L, int face,
                                                 uint8_t *__restrict__ out)
{
    int i, j, k;
    long p;
    if (!cell_of((long)blockIdx.x * blockDim.x + threadIdx.x, L, i, j, k, p)) return;
    const long st[3] = {L.sx, (long)L.nz, 1};
    const int pos[3] = {i, j, k}, nn[3] = {L.nx, L.ny, L.nz};
    const int ax = face >> 1;
    const bool m = mask[p] != 0;
    const int nbp = pos[ax] + ((face & 1) ? 1 : -1);
    bool e = m;
    if (m && nbp >= 0 && nbp < nn[ax]) e = mask[p + ((face & 1) ? st[ax] : -st[ax])] == 0;
    out[p] = e ? 1 : 0;
}

// Exposed lateral faces per plane k of axis 2, from the neighbour-flags digest: an in-mask cell exposes one face for every
// neighbour bit in `bits` that is clear (bits 1..6 = x-, x+, y-, y+, z-, z+; the domain boundary counts as exposed, as in
// exposed_mask).  This is the count loop of quick_compare_layer_birth_robin_v3.py:97-108 for every layer at once.
// Thread t of a block owns plane k = blockIdx.x*256 + t and walks a chunk of (i, j) rows: coalesced along k, one
// 64-bit atomic per thread at the end.
__global__ __launch_bounds__(256) void k_count_exposed(const uint8_t *__restrict__ flags, Lay L, unsigned bits, int rows_per_block,
                                                       unsigned long long *__restrict__ counts)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= L.nz) return;
    const long nrows = (long)L.nx * L.ny;
    const long r0 = (long)blockIdx.y * rows_per_block, r1 = r0 + rows_per_block < nrows ? r0 + rows_per_block : nrows;
    unsigned long long c = 0;
    for (long r = r0; r < r1; ++r) {
        const unsigned i = (unsigned)r / (unsigned)L.ny, j = (unsigned)r - i * (unsigned)L.ny;
        const unsigned f = flags[(long)i * L.sx + (long)j * L.nz + k];
        if (f & 1u) c += __popc(~f & bits & 0x7eu);
    }
    if (c) atomicAdd(&counts[k], c);
}

// A birth in one pass (activate_layer, waam_from_stl_v7_mm.py:487-495): on the planes [k0, k1) of axis 2
//     newborn = full & ~active;   T[newborn] = Ts;   active |= full          and the number of newborn cells is counted.
// Cell q of the (nx*ny) x (k1-k0) box: consecutive threads run along k.
__global__ __launch_bounds__(256) void k_birth(double *__restrict__ T, uint8_t *__restrict__ active,
                                               const uint8_t *__restrict__ full, Lay L, int k0, int k1, double Ts,
                                               unsigned long long *__restrict__ n_new)
{
    const int nk = k1 - k0;
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)L.nx * L.ny * nk;
    unsigned born = 0;
    if (q < total) {
        const long row = q / nk;
        const int k = k0 + (int)(q - row * nk);
        const unsigned i = (unsigned)row / (unsigned)L.ny, j = (unsigned)row - i * (unsigned)L.ny;
        const long p = (long)i * L.sx + (long)j * L.nz + k;
        if (full[p] != 0 && active[p] == 0) { T[p] = Ts; active[p] = 1; born = 1; }
    }
    const unsigned long long b = __ballot(born);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(n_new, (unsigned long long)__popcll(b));
}

__global__ __launch_bounds__(256) void k_masked_fill(double *__restrict__ T, const uint8_t *__restrict__ sel,
                                                     size_t n, double v)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n && sel[p]) T[p] = v;
}

__global__ __launch_bounds__(256) void k_mask_or(uint8_t *__restrict__ dst, const uint8_t *__restrict__ a,
                                                 const uint8_t *__restrict__ b, size_t n)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) dst[p] = (a[p] || b[p]) ? 1 : 0;
}

static unsigned range_blocks(const Lay &L, int k0, int k1) { return (unsigned)(((long)L.nx * L.ny * (k1 - k0) + 255) / 256); }

// the data mode of face f's h and q (`who` names the entry in the error text)
static int check_face_mode(const char *who, int h_mode, int q_mode)
{
    ADI_REQUIRE(h_mode >= 0 && h_mode <= 2 && q_mode >= 0 && q_mode <= 2, "%s: bad face mode", who);
    return ADI_OK;
}

}  // namespace adi

using namespace adi;

extern "C" {

int adi_exposed_mask(const uint8_t *d_mask, int nx, int ny, int nz, long plane_stride, int face, uint8_t *d_exposed,
                     void *stream)
{
    ADI_REQUIRE(face >= 0 && face < 6, "bad face");  // ValueError("bad face"), adi3d_numba_coeff.py:54
    ADI_REQUIRE(d_mask && d_exposed, "adi_exposed_mask: null argument");
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    hipLaunchKernelGGL(k_exposed, dim3(cell_blocks(L)), dim3(256), 0, as_stream(stream), d_mask, L, face, d_exposed);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_count_exposed_faces(const uint8_t *d_flags, int nx, int ny, int nz, long plane_stride, int face_bits,
                            unsigned long long *d_counts, void *stream)
{
    ADI_REQUIRE(d_flags && d_counts, "adi_count_exposed_faces: null argument");
    ADI_REQUIRE(face_bits > 0 && face_bits < 64, "adi_count_exposed_faces: face_bits selects none of the six faces");
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    hipStream_t st = as_stream(stream);
    ADI_HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)nz * sizeof(unsigned long long), st));
    const long nrows = (long)nx * ny;
    const int rows_per_block = nrows > 4096 ? 256 : 16;
    const dim3 grid((unsigned)((nz + 255) / 256), (unsigned)((nrows + rows_per_block - 1) / rows_per_block));
    hipLaunchKernelGGL(k_count_exposed, grid, dim3(256), 0, st, d_flags, L, (unsigned)face_bits << 1, rows_per_block, d_counts);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_birth_planes(double *d_T, uint8_t *d_active, const uint8_t *d_full, int nx, int ny, int nz, long plane_stride,
                     int k_begin, int k_end, double Ts, unsigned long long *d_newborn, void *stream)
{
    ADI_REQUIRE(d_T && d_active && d_full && d_newborn, "adi_birth_planes: null argument");
    ADI_REQUIRE(d_active != d_full, "adi_birth_planes: the active mask aliases the full mask");
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    if (int rc = check_plane_range("adi_birth_planes", k_begin, k_end, nz)) return rc;
    hipStream_t st = as_stream(stream);
    ADI_HIP_TRY(hipMemsetAsync(d_newborn, 0, sizeof(unsigned long long), st));
    if (k_begin == k_end) return ADI_OK;
    const long total = (long)nx * ny * (k_end - k_begin);
    hipLaunchKernelGGL(k_birth, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_T, d_active, d_full, L, k_begin, k_end,
                       Ts, d_newborn);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_build_coeffs_planes(const uint8_t *d_mask, int nx, int ny, int nz, long plane_stride, double dx, double rho,
                            double cp, const int *h_mode, const double *h_scalar, const double *const *d_h_field,
                            const int *q_mode, const double *q_scalar, const double *const *d_q_field,
                            double *const *d_coeff, double *const *d_qflux, int k_begin, int k_end, void *stream)
{
    ADI_REQUIRE(d_mask && h_mode && h_scalar && q_mode && q_scalar && d_coeff && d_qflux, "adi_build_coeffs: null argument");
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    if (int rc = check_plane_range("adi_build_coeffs_planes", k_begin, k_end, nz)) return rc;
    FaceSpec h, q;
    for (int f = 0; f < 6; ++f) {
        h.mode[f] = h_mode[f]; h.scalar[f] = h_scalar[f]; h.field[f] = d_h_field ? d_h_field[f] : nullptr;
        q.mode[f] = q_mode[f]; q.scalar[f] = q_scalar[f]; q.field[f] = d_q_field ? d_q_field[f] : nullptr;
        if (int rc = check_face_mode("adi_build_coeffs", h.mode[f], q.mode[f])) return rc;
        ADI_REQUIRE(h.mode[f] != ADI_FACE_FIELD || h.field[f], "adi_build_coeffs: missing h field for face %d", f);
        ADI_REQUIRE(q.mode[f] != ADI_FACE_FIELD || q.field[f], "adi_build_coeffs: missing q field for face %d", f);
    }
    for (int a = 0; a < 3; ++a) ADI_REQUIRE(d_coeff[a] && d_qflux[a], "adi_build_coeffs: null output");
    if (k_begin == k_end) return ADI_OK;
    double A, Ccell;
    cell_constants(dx, rho, cp, &A, &Ccell);
    hipLaunchKernelGGL(k_build_coeffs, dim3(range_blocks(L, k_begin, k_end)), dim3(256), 0, as_stream(stream), d_mask, L,
                       k_begin, k_end, A, Ccell, h, q, d_coeff[0], d_coeff[1], d_coeff[2], d_qflux[0], d_qflux[1], d_qflux[2]);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_face_constants(double dx, double rho, double cp, const int *h_mode, const double *h_scalar, const int *q_mode,
                       const double *q_scalar, double *h_consts, int *h_valid)
{
#pragma clang fp contract(off)
    ADI_REQUIRE(h_mode && h_scalar && q_mode && q_scalar && h_consts && h_valid, "adi_face_constants: null argument");
    // the very expressions of k_build_coeffs: (h * A) / Ccell, IEEE, no contraction
    double A, Ccell;
    cell_constants(dx, rho, cp, &A, &Ccell);
    for (int a = 0; a < 3; ++a) {
        bool ok = true;
        for (int s = 0; s < 2; ++s) {
            const int f = 2 * a + s;
            if (int rc = check_face_mode("adi_face_constants", h_mode[f], q_mode[f])) return rc;
            ok = ok && h_mode[f] != ADI_FACE_FIELD && q_mode[f] != ADI_FACE_FIELD;
            h_consts[4 * a + s] = (h_mode[f] == ADI_FACE_SCALAR) ? (h_scalar[f] * A / Ccell) : 0.0;
            h_consts[4 * a + 2 + s] = (q_mode[f] == ADI_FACE_SCALAR) ? (q_scalar[f] * A / Ccell) : 0.0;
        }
        h_valid[a] = ok ? 1 : 0;
    }
    return ADI_OK;
}

int adi_build_coeffs(const uint8_t *d_mask, int nx, int ny, int nz, long plane_stride, double dx, double rho,
                     double cp, const int *h_mode, const double *h_scalar, const double *const *d_h_field,
                     const int *q_mode, const double *q_scalar, const double *const *d_q_field,
                     double *const *d_coeff, double *const *d_qflux, void *stream)
{
    return adi_build_coeffs_planes(d_mask, nx, ny, nz, plane_stride, dx, rho, cp, h_mode, h_scalar, d_h_field, q_mode,
                                   q_scalar, d_q_field, d_coeff, d_qflux, 0, nz, stream);
}

int adi_build_nbr_flags_planes(const uint8_t *d_mask, int nx, int ny, int nz, long plane_stride, uint8_t *d_flags,
                               int k_begin, int k_end, void *stream)
{
    ADI_REQUIRE(d_mask && d_flags, "adi_build_nbr_flags: null argument");
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    if (int rc = check_plane_range("adi_build_nbr_flags_planes", k_begin, k_end, nz)) return rc;
    if (k_begin == k_end) return ADI_OK;
    hipLaunchKernelGGL(k_build_flags, dim3(range_blocks(L, k_begin, k_end)), dim3(256), 0, as_stream(stream), d_mask, L, k_begin,
                       k_end, d_flags);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_build_nbr_flags(const uint8_t *d_mask, int nx, int ny, int nz, long plane_stride, uint8_t *d_flags,
                        void *stream)
{
    return adi_build_nbr_flags_planes(d_mask, nx, ny, nz, plane_stride, d_flags, 0, nz, stream);
}

long adi_flag_bricks_words(int nx, int ny, int nz)
{
    if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
    const long nbx = (nx + kBrick - 1) / kBrick, nby = (ny + kBrick - 1) / kBrick, nbz = (nz + kBrick - 1) / kBrick;
    return nby * nbz * ((nbx + 31) / 32);
}

int adi_build_flag_bricks(const uint8_t *d_flags, int nx, int ny, int nz, long plane_stride, uint32_t *d_bricks, int k_begin,
                          int k_end, void *stream)
{
    ADI_REQUIRE(d_flags && d_bricks, "adi_build_flag_bricks: null argument");
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    if (int rc = check_plane_range("adi_build_flag_bricks", k_begin, k_end, nz)) return rc;
    if (k_begin == k_end) return ADI_OK;
    // every brick that holds a plane of the range
    const int bk0 = k_begin / kBrick, bk1 = (k_end + kBrick - 1) / kBrick;
    const long nblocks = (long)((nx + kBrick - 1) / kBrick) * ((ny + kBrick - 1) / kBrick) * (bk1 - bk0);
    ADI_REQUIRE(nblocks < 0x7fffffffL, "adi_build_flag_bricks: box too large");
    hipLaunchKernelGGL(k_build_flag_bricks, dim3((unsigned)nblocks), dim3(256), 0, as_stream(stream), d_flags, L, bk0, bk1,
                       (unsigned *)d_bricks);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_masked_fill(double *d_T, const uint8_t *d_sel, size_t n, double value, void *stream)
{
    ADI_REQUIRE(d_T && d_sel, "adi_masked_fill: null argument");
    if (n == 0) return ADI_OK;
    hipLaunchKernelGGL(k_masked_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), d_T, d_sel, n, value);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_mask_or(uint8_t *d_dst, const uint8_t *d_a, const uint8_t *d_b, size_t n, void *stream)
{
    ADI_REQUIRE(d_dst && d_a && d_b, "adi_mask_or: null argument");
    if (n == 0) return ADI_OK;
    hipLaunchKernelGGL(k_mask_or, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), d_dst, d_a, d_b, n);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // extern "C"
