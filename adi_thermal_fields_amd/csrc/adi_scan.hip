// adi_scan.hip -- a scan path of Goldak's double ellipsoid evaluated by the library (include/adi_hip.h, "Scan path"):
//   adi_scan_sample_host   the evaluator (adi_scan_eval.hpp) on the CPU over a host array: no HIP call
//   k_scan_sample          the step-averaged source of a window [t, t + dt] at the cell centres -> a field on the device, for
//                          the field form of the step (adi_explicit_rhs_src)
// K travels by value and bounds every loop over segments; every segment index read lies in [0, K).
#include "adi_cart_host.hpp"
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

}  // extern "C"
