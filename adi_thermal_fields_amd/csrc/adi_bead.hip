// adi_bead.hip -- the bead a scan path lays during a step (include/adi_hip.h, "Bead deposition along a scan path"):
//   adi_bead_index_box     the index box that holds every cell a step can bear, on the host: no HIP call
//   adi_bead_deposit_host  the evaluator (adi_bead_eval.hpp) on the CPU over host arrays: no HIP call
//   k_bead_deposit         the births of a step on the device: T = Ts and active = 1 on the newborn cells of the launch box,
//                          and their material id where the grid has an id field (adi_bead_deposit_ids)
// The launch box comes from the HOST table inside the entry point and is clipped to the logical box, which lies inside the
// physical one: no argument of the caller is an address range.  K travels by value and bounds every loop over segments.
#include "adi_bead_eval.hpp"
#include "adi_cart_host.hpp"
#include "adi_scan_check.hpp"

namespace adi {

struct BeadPathArg {
    adi_bead_shape b;
    const double *tab;          // K x 8 doubles (device)
    int K, k0, k1;              // the segments [k0, k1) of scan_window for the step, found on the host
    double t_end;
};

// One thread per cell of the launch box B (consecutive threads along axis 2), 64-bit cell indices.  A cell that is active
// already, or outside `within`, is decided before any arithmetic; T and active are written on newborn cells only, and so is
// ids (optional: the id field of a grid of several materials), which gets `id` there.
__global__ __launch_bounds__(256) void k_bead_deposit(BeadPathArg P, ScanBox B, Lay L, double dx, double t, double t1, double Ts,
                                                      double *__restrict__ T, uint8_t *__restrict__ active,
                                                      const uint8_t *__restrict__ within, uint8_t *__restrict__ ids,
                                                      unsigned id, unsigned long long *__restrict__ n_new)
{
#pragma clang fp contract(off)
    const long bj = B.hi[1] - B.lo[1], bk = B.hi[2] - B.lo[2];
    const long total = (long)(B.hi[0] - B.lo[0]) * bj * bk;
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned born = 0;
    if (q < total) {
        const long row = q / bk;
        const int k = B.lo[2] + (int)(q - row * bk);
        const long pl = row / bj;
        const int j = B.lo[1] + (int)(row - pl * bj), i = B.lo[0] + (int)pl;
        const long p = (long)i * L.sx + (long)j * L.nz + k;
        if (active[p] == 0 && (within == nullptr || within[p] != 0) &&
            bead_inside_step(P.b, P.tab, P.K, P.t_end, P.k0, P.k1, t, t1, (i + 0.5) * dx, (j + 0.5) * dx, (k + 0.5) * dx)) {
            T[p] = Ts; active[p] = 1; born = 1;
            if (ids != nullptr) ids[p] = (uint8_t)id;
        }
    }
    const unsigned long long b = __ballot(born);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(n_new, (unsigned long long)__popcll(b));
}

static int check_bead(const adi_bead_shape *b, const char *fn)
{
    ADI_REQUIRE(b != nullptr, "%s: null bead shape", fn);
    ADI_REQUIRE(std::isfinite(b->width) && std::isfinite(b->height), "%s: non-finite bead width / height", fn);
    ADI_REQUIRE(b->width > 0.0 && b->height > 0.0, "%s: non-positive bead width / height", fn);
    ADI_REQUIRE(b->profile == 0 || b->profile == 1, "%s: bead profile must be 0 (box) or 1 (parabola)", fn);
    ADI_REQUIRE(b->depth_axis >= 0 && b->depth_axis < 3, "%s: depth_axis out of range", fn);
    return ADI_OK;
}

// the shape, the host table, the grid and the step
static int check_step(const adi_bead_shape *b, const double *tab, int K, double t_end, int nx, int ny, int nz, double dx,
                      double t, double dt, const char *fn)
{
    if (int rc = check_bead(b, fn)) return rc;
    if (int rc = scan_check_path(K, t_end, fn)) return rc;
    if (int rc = scan_check_rows(tab, K, t_end, fn)) return rc;
    if (int rc = scan_check_grid(nx, ny, nz, dx, fn)) return rc;
    ADI_REQUIRE(std::isfinite(t) && std::isfinite(dt) && dt > 0.0, "%s: bad t / dt (dt must be > 0)", fn);
    return ADI_OK;
}

// the launch box of the step [t, t + dt] on the logical grid and the window of segments; -> whether a segment deposits
static bool step_box(const adi_bead_shape &b, const double *tab, int K, double t_end, int nx, int ny, int nz, double dx,
                     double t, double dt, ScanBox &B, int &k0, int &k1)
{
#pragma clang fp contract(off)
    const double t1 = t + dt;
    scan_window(tab, K, t, t1, k0, k1);
    const int n[3] = {nx, ny, nz};
    return bead_window_box(b, tab, K, t_end, k0, k1, t, t1, n, dx, B);
}

// adi_bead_deposit (d_ids null) and adi_bead_deposit_ids; fn names the entry in the error text
static int bead_deposit(const char *fn, const adi_bead_shape *shape, const double *h_table, const double *d_table, int K,
                        double t_end, double *d_T, uint8_t *d_active, const uint8_t *d_within, uint8_t *d_ids, int id, int lx,
                        int ly, int lz, int nx, int ny, int nz, long plane_stride, double dx, double t, double dt, double Ts,
                        unsigned long long *d_newborn, void *stream)
{
    if (int rc = check_step(shape, h_table, K, t_end, lx, ly, lz, dx, t, dt, fn)) return rc;
    ADI_REQUIRE(std::isfinite(Ts), "%s: non-finite Ts", fn);
    ADI_REQUIRE(d_table && d_T && d_active && d_newborn, "%s: null argument", fn);
    ADI_REQUIRE(d_active != d_within, "%s: the active mask aliases `within`", fn);
    ADI_REQUIRE(lx <= nx && ly <= ny && lz <= nz, "%s: the logical box %d x %d x %d exceeds the physical %d x %d x %d", fn,
                lx, ly, lz, nx, ny, nz);
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    ScanBox B;
    int k0, k1;
    step_box(*shape, h_table, K, t_end, lx, ly, lz, dx, t, dt, B, k0, k1);
    hipStream_t st = as_stream(stream);
    ADI_HIP_TRY(hipMemsetAsync(d_newborn, 0, sizeof(unsigned long long), st));
    if (scan_box_empty(B)) return ADI_OK;
    const long total = (long)(B.hi[0] - B.lo[0]) * (B.hi[1] - B.lo[1]) * (B.hi[2] - B.lo[2]);   // < 2^32: inside the box of L
    const BeadPathArg P{*shape, d_table, K, k0, k1, t_end};
    hipLaunchKernelGGL(k_bead_deposit, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, P, B, L, dx, t, t + dt, Ts, d_T,
                       d_active, d_within, d_ids, (unsigned)id, d_newborn);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // namespace adi

using namespace adi;

extern "C" {

int adi_bead_index_box(const adi_bead_shape *shape, const double *h_table, int K, double t_end, int nx, int ny, int nz,
                       double dx, double t, double dt, int box[6], int *deposits)
{
    if (int rc = check_step(shape, h_table, K, t_end, nx, ny, nz, dx, t, dt, "adi_bead_index_box")) return rc;
    ADI_REQUIRE(box && deposits, "adi_bead_index_box: null output");
    ScanBox B;
    int k0, k1;
    *deposits = step_box(*shape, h_table, K, t_end, nx, ny, nz, dx, t, dt, B, k0, k1) ? 1 : 0;
    for (int a = 0; a < 3; ++a) { box[2 * a] = B.lo[a]; box[2 * a + 1] = B.hi[a]; }
    return ADI_OK;
}

int adi_bead_deposit_host(const adi_bead_shape *shape, const double *h_table, int K, double t_end, const uint8_t *h_active,
                          const uint8_t *h_within, int nx, int ny, int nz, double dx, double t, double dt, uint8_t *h_born)
{
    if (int rc = check_step(shape, h_table, K, t_end, nx, ny, nz, dx, t, dt, "adi_bead_deposit_host")) return rc;
    ADI_REQUIRE(h_born, "adi_bead_deposit_host: null output");
    ADI_REQUIRE(h_born != h_active && h_born != h_within, "adi_bead_deposit_host: the output aliases an input");
    bead_deposit_host(*shape, h_table, K, t_end, h_active, h_within, nx, ny, nz, dx, t, dt, h_born);
    return ADI_OK;
}

int adi_bead_deposit(const adi_bead_shape *shape, const double *h_table, const double *d_table, int K, double t_end, double *d_T,
                     uint8_t *d_active, const uint8_t *d_within, int lx, int ly, int lz, int nx, int ny, int nz,
                     long plane_stride, double dx, double t, double dt, double Ts, unsigned long long *d_newborn, void *stream)
{
    return bead_deposit("adi_bead_deposit", shape, h_table, d_table, K, t_end, d_T, d_active, d_within, nullptr, 0, lx, ly, lz, nx,
                        ny, nz, plane_stride, dx, t, dt, Ts, d_newborn, stream);
}

int adi_bead_deposit_ids(const adi_bead_shape *shape, const double *h_table, const double *d_table, int K, double t_end,
                         double *d_T, uint8_t *d_active, const uint8_t *d_within, uint8_t *d_ids, int id, int lx, int ly, int lz,
                         int nx, int ny, int nz, long plane_stride, double dx, double t, double dt, double Ts,
                         unsigned long long *d_newborn, void *stream)
{
    ADI_REQUIRE(d_ids != nullptr, "adi_bead_deposit_ids: null id field");
    ADI_REQUIRE(id >= 0 && id < ADI_MATMAP_MAX, "adi_bead_deposit_ids: material id %d (0 to %d)", id, ADI_MATMAP_MAX - 1);
    ADI_REQUIRE(d_ids != d_active && d_ids != d_within, "adi_bead_deposit_ids: the id field aliases a mask");
    return bead_deposit("adi_bead_deposit_ids", shape, h_table, d_table, K, t_end, d_T, d_active, d_within, d_ids, id, lx, ly, lz,
                        nx, ny, nz, plane_stride, dx, t, dt, Ts, d_newborn, stream);
}

}  // extern "C"
