// adi_scan.hip -- a scan path of Goldak's double ellipsoid evaluated by the library (include/adi_hip.h, "Scan path"):
//   adi_scan_sample_host   the evaluator (adi_scan_eval.hpp) on the CPU over a host array: no HIP call
//   k_scan_sample          the step-averaged source of a window [t, t + dt] at the cell centres -> a field on the device, for
//                          the field form of the step (adi_explicit_rhs_src)
//   k_mapscan_add_r0       the same source added to the explicit stage's output of a grid of several materials, on the window's
//                          index box only (adi_matmap_scan_add_r0; adi_matmap_scan_add_r0_host is its twin on the CPU)
// K travels by value and bounds every loop over segments; every segment index read lies in [0, K).
#include "adi_cart_host.hpp"
#include "adi_matmap_dev.hpp"
#include "adi_scan_check.hpp"
#include "adi_scan_eval.hpp"

namespace adi {

struct ScanPathArg {
    adi_scan_shape h;
    const double *tab;          // K x 8 doubles (device)
    int K;
    double t_end;
};

__global__ __launch_bounds__(256) void k_scan_sample(ScanPathArg P, const uint8_t *__restrict__ flags, Lay L, double dx,
                                                     double t, double dt, double *__restrict__ out)
{
#pragma clang fp contract(off)
    const long plane = (long)L.ny * L.nz;
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= plane * L.nx) return;
    const int i = (int)(q / plane);
    const long r = q - (long)i * plane;
    const int j = (int)(r / L.nz), k = (int)(r - (long)j * L.nz);
    const long p = (long)i * L.sx + r;
    double v = 0.0;
    if (flags[p] & 1u) {
        const double t1 = t + dt;
        int k0, k1;
        scan_window(P.tab, P.K, t, t1, k0, k1);
        v = scan_q_step(P.h, P.tab, P.K, P.t_end, k0, k1, t, t1, dt, (i + 0.5) * dx, (j + 0.5) * dx, (k + 0.5) * dx);
    }
    out[p] = v;
}

// The path added to the explicit stage's output on a grid of several materials (include/adi_hip.h, "Scan path"): R0 = R0 +
// (dt * q_step) / C[id] on the in-mask cells of the window's index box -- the operations of k_matmap_explicit's source-field
// branch, in its order, with q_step evaluated here instead of read from a field.  One thread per cell of the box, the box
// flattened with axis 2 fastest: the lanes of a wave are adjacent along axis 2, then along axis 1 (a box thinner than a wave
// along axis 2 still fills its waves).  The window -- segment range, box, t, dt -- travels by value, found on the host: the
// bounds of the segment loop are wave-uniform and nothing a previous launch wrote is read but R0, flags and ids.  C travels by
// value and goes through LDS (a lane picks the entry of its cell's id).  17 bytes per in-mask cell of the box: flags, id, R0
// read and written.
struct ScanCTab {
    double c[kMapMaxMat];
};
struct ScanAddArgs {
    int k0, k1;                 // segments the step can overlap
    int lo[3], w[3];            // the box: first cell and extent per axis (every extent >= 1)
    double dx, t, dt;
};
__global__ __launch_bounds__(64) void k_mapscan_add_r0(ScanPathArg P, double *__restrict__ R0, const uint8_t *__restrict__ flags,
                                                       const uint8_t *__restrict__ ids, Lay L, ScanAddArgs A, ScanCTab C)
{
#pragma clang fp contract(off)
    __shared__ double sC[kMapMaxMat];
    {
        const double *kc = C.c;
        if (threadIdx.x < kMapMaxMat) sC[threadIdx.x] = kc[threadIdx.x];
        __syncthreads();
    }
    const long plane = (long)A.w[1] * A.w[2];
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= plane * A.w[0]) return;
    const int ib = (int)(q / plane);
    const long r = q - (long)ib * plane;
    const int jb = (int)(r / A.w[2]), kb = (int)(r - (long)jb * A.w[2]);
    const int i = A.lo[0] + ib, j = A.lo[1] + jb, k = A.lo[2] + kb;
    const long p = (long)i * L.sx + (long)j * L.nz + k;
    if (!(flags[p] & 1u)) return;
    double v = R0[p];
    if (scan_add_r0_cell(P.h, P.tab, P.K, P.t_end, A.k0, A.k1, A.t, A.dt, A.dx, i, j, k, sC, ids[p], v)) R0[p] = v;
}

static int check_shape(const adi_scan_shape *h, const char *fn)
{
    ADI_REQUIRE(h != nullptr, "%s: null shape", fn);
    const double v[] = {h->eta, h->a, h->b, h->c_f, h->c_r, h->f_f};
    for (double x : v) ADI_REQUIRE(std::isfinite(x), "%s: non-finite shape parameter", fn);
    ADI_REQUIRE(h->eta >= 0.0 && h->eta <= 1.0, "%s: eta outside [0, 1]", fn);
    ADI_REQUIRE(h->a > 0.0 && h->b > 0.0 && h->c_f > 0.0 && h->c_r > 0.0, "%s: non-positive length", fn);
    ADI_REQUIRE(h->f_f > 0.0 && h->f_f < 2.0, "%s: f_f outside (0, 2)", fn);
    ADI_REQUIRE(h->depth_axis >= 0 && h->depth_axis < 3, "%s: depth_axis out of range", fn);
    return ADI_OK;
}

// the shape and what can be said of a path without its table
static int check_path(const adi_scan_shape *h, int K, double t_end, const char *fn)
{
    if (int rc = check_shape(h, fn)) return rc;
    return scan_check_path(K, t_end, fn);
}

// ... and the host table (scan_check_rows)
static int check_table(const adi_scan_shape *h, const double *tab, int K, double t_end, const char *fn)
{
    if (int rc = check_path(h, K, t_end, fn)) return rc;
    return scan_check_rows(tab, K, t_end, fn);
}

}  // namespace adi

using namespace adi;

extern "C" {

int adi_scan_sample_host(const adi_scan_shape *h_shape, const double *h_table, int K, double t_end, const uint8_t *h_mask,
                         int nx, int ny, int nz, double dx, double t, double dt, double *h_out)
{
    if (int rc = check_table(h_shape, h_table, K, t_end, "adi_scan_sample_host")) return rc;
    if (int rc = scan_check_grid(nx, ny, nz, dx, "adi_scan_sample_host")) return rc;
    ADI_REQUIRE(h_out, "adi_scan_sample_host: null output");
    ADI_REQUIRE(std::isfinite(t) && std::isfinite(dt) && dt > 0.0, "adi_scan_sample_host: bad t / dt (dt must be > 0)");
    scan_sample_host(*h_shape, h_table, K, t_end, h_mask, nx, ny, nz, dx, t, dt, h_out);
    return ADI_OK;
}

int adi_scan_sample(const adi_scan_shape *h_shape, const double *d_table, int K, double t_end, const uint8_t *d_flags, int nx,
                    int ny, int nz, long plane_stride, double dx, double t, double dt, double *d_out, void *stream)
{
    if (int rc = check_path(h_shape, K, t_end, "adi_scan_sample")) return rc;
    ADI_REQUIRE(d_table && d_flags && d_out, "adi_scan_sample: null argument");
    ADI_REQUIRE(std::isfinite(dx) && dx > 0.0 && std::isfinite(t) && std::isfinite(dt) && dt > 0.0,
                "adi_scan_sample: bad dx / t / dt");
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    const ScanPathArg P{*h_shape, d_table, K, t_end};
    hipLaunchKernelGGL(k_scan_sample, dim3(cell_blocks(L)), dim3(256), 0, as_stream(stream), P, d_flags, L, dx, t, dt, d_out);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

// what the two forms of adi_matmap_scan_add_r0 check alike, and the window of the step
static int mapscan_window(const adi_scan_shape *h_shape, const double *h_table, int K, double t_end, int nx, int ny, int nz,
                          double dx, double t, double dt, int nmat, const double *h_C, int *h_box_out, const char *fn,
                          ScanWindow *W)
{
    if (int rc = check_table(h_shape, h_table, K, t_end, fn)) return rc;
    if (int rc = scan_check_grid(nx, ny, nz, dx, fn)) return rc;
    ADI_REQUIRE(std::isfinite(t) && std::isfinite(dt) && dt > 0.0, "%s: bad t / dt (dt must be > 0)", fn);
    ADI_REQUIRE(h_C, "%s: null argument", fn);
    if (int rc = check_tables(fn, nmat, nullptr, h_C)) return rc;
    *W = scan_window_of(*h_shape, h_table, K, t_end, nx, ny, nz, dx, t, dt);
    const int n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a)
        ADI_REQUIRE(W->B.lo[a] >= 0 && W->B.lo[a] <= W->B.hi[a] && W->B.hi[a] <= n[a], "%s: the window's box leaves the grid", fn);
    if (h_box_out != nullptr)
        for (int a = 0; a < 3; ++a) { h_box_out[2 * a] = W->B.lo[a]; h_box_out[2 * a + 1] = W->B.hi[a]; }
    return ADI_OK;
}

int adi_scan_window_box(const adi_scan_shape *h_shape, const double *h_table, int K, double t_end, int nx, int ny, int nz,
                        double dx, double t, double dt, int *h_seg_out, int *h_box_out)
{
    const char *fn = "adi_scan_window_box";
    ADI_REQUIRE(h_seg_out && h_box_out, "%s: null output", fn);
    const double one = 1.0;
    ScanWindow W;
    if (int rc = mapscan_window(h_shape, h_table, K, t_end, nx, ny, nz, dx, t, dt, 1, &one, h_box_out, fn, &W)) return rc;
    h_seg_out[0] = W.k0; h_seg_out[1] = W.k1;
    return ADI_OK;
}

int adi_matmap_scan_add_r0_host(const adi_scan_shape *h_shape, const double *h_table, int K, double t_end, double *h_R0,
                                const uint8_t *h_mask, const uint8_t *h_ids, int nx, int ny, int nz, double dx, double t,
                                double dt, int nmat, const double *h_C, int *h_box_out)
{
    const char *fn = "adi_matmap_scan_add_r0_host";
    ADI_REQUIRE(h_R0 && h_ids, "%s: null argument", fn);
    ScanWindow W;
    if (int rc = mapscan_window(h_shape, h_table, K, t_end, nx, ny, nz, dx, t, dt, nmat, h_C, h_box_out, fn, &W)) return rc;
    double C[kMapMaxMat];
    for (int m = 0; m < kMapMaxMat; ++m) C[m] = m < nmat ? h_C[m] : 1.0;
    if (!scan_box_empty(W.B)) scan_add_r0_host(*h_shape, h_table, K, t_end, W, h_R0, h_mask, h_ids, ny, nz, dx, t, dt, C);
    return ADI_OK;
}

int adi_matmap_scan_add_r0(const adi_scan_shape *h_shape, const double *h_table, const double *d_table, int K, double t_end,
                           double *d_R0, const uint8_t *d_flags, const uint8_t *d_ids, int nx, int ny, int nz, long plane_stride,
                           double dx, double t, double dt, int nmat, const double *h_C, int *h_box_out, void *stream)
{
    const char *fn = "adi_matmap_scan_add_r0";
    ADI_REQUIRE(d_table && d_R0 && d_flags && d_ids, "%s: null argument", fn);
    ScanWindow W;
    if (int rc = mapscan_window(h_shape, h_table, K, t_end, nx, ny, nz, dx, t, dt, nmat, h_C, h_box_out, fn, &W)) return rc;
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    if (scan_box_empty(W.B)) return ADI_OK;
    ScanAddArgs A;
    A.k0 = W.k0; A.k1 = W.k1;
    for (int a = 0; a < 3; ++a) { A.lo[a] = W.B.lo[a]; A.w[a] = W.B.hi[a] - W.B.lo[a]; }
    A.dx = dx; A.t = t; A.dt = dt;
    ScanCTab C;
    for (int m = 0; m < kMapMaxMat; ++m) C.c[m] = m < nmat ? h_C[m] : 1.0;
    const long cells = (long)A.w[0] * A.w[1] * A.w[2];          // (< 2^32: make_lay's limit on the whole box)
    const ScanPathArg P{*h_shape, d_table, K, t_end};
    hipLaunchKernelGGL(k_mapscan_add_r0, dim3((unsigned)((cells + 63) / 64)), dim3(64), 0, as_stream(stream), P, d_R0, d_flags,
                       d_ids, L, A, C);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // extern "C"
